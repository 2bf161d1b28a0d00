"""The build description (areafunctionsynthesis_amd/build.py): what the digest hashes is what the
compiler reads, an object is rebuilt exactly when something it was built from changed, and a
variant build stays in its own files.  CPU only, and no test here compiles anything: a stand-in
for the compiler writes the files that a compile or link command names."""
import importlib
import os

import pytest

from areafunctionsynthesis_amd import build

FUTURE = 1e9  # seconds added to a file's mtime: newer than every object


def _object(source):
    cmd = build.compile_command(source, objdir=build.OBJ)
    return cmd[cmd.index("-o") + 1]


def _files(root):
    return {os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs}


class Tree:
    """build.py writing under a temporary directory instead of the package, compiling with a
    stand-in whose depfiles name what the include scan finds (test_scan_matches_depfile ties
    the scan to hipcc's own depfiles)."""

    def __init__(self, root, monkeypatch):
        self.root, self.monkeypatch, self.ran, self.fail = str(root), monkeypatch, [], None
        os.makedirs(os.path.join(self.root, "prof"))
        self.redirect()

    def redirect(self):
        for name, value in (("OBJ", os.path.join(self.root, "_obj")), ("HERE", self.root),
                            ("PROF_DIR", os.path.join(self.root, "prof")), ("_run", self.run)):
            self.monkeypatch.setattr(build, name, value)

    def run(self, cmd):
        self.ran.append(cmd)
        src = next((a for a in cmd if a.endswith((".cpp", ".hip"))), None)
        if src and os.path.basename(src) == self.fail:
            raise RuntimeError("stand-in compiler: error in " + src)
        if "-MF" in cmd:  # (the dependency pass)
            with open(cmd[cmd.index("-MF") + 1], "w") as fh:
                fh.write(cmd[cmd.index("-MT") + 1] + ": " + " \\\n  ".join([src] + sorted(build.include_graph(src))) + "\n")
            return
        with open(cmd[cmd.index("-o") + 1], "w") as fh:
            fh.write("stand-in\n")

    def rebuilt(self, **kw):
        """The sources that a build() compiles now, and the libraries it links."""
        del self.ran[:]
        build.build(verbose=False, **kw)
        objs = sorted(os.path.basename(a) for c in self.ran if "-c" in c for a in c if a.endswith((".cpp", ".hip")))
        libs = sorted(os.path.basename(c[c.index("-o") + 1]) for c in self.ran if "-shared" in c)
        return objs, libs

    def newer(self, header):
        """Make one file of the repository look newer than every object."""
        self.monkeypatch.setattr(build, "_mtime", lambda p: os.path.getmtime(p) + (FUTURE if os.path.basename(p) == header else 0))


@pytest.fixture
def tree(tmp_path, monkeypatch):
    t = Tree(tmp_path, monkeypatch)
    assert t.rebuilt() == (sorted(build.SOURCES), ["libafs.so.tmp"])  # (everything is missing)
    return t


def test_default_flags_are_common_plus_per_source():
    for s in build.SOURCES:
        cmd = build.compile_command(s)
        obj = os.path.join(build.OBJ, os.path.splitext(s)[0] + ".o")
        assert cmd[cmd.index("-o") + 1] == obj
        assert cmd[cmd.index("--offload-arch=" + build.ARCH) + 1:] == build.COMMON + build.PER_SOURCE.get(s, [])
        deps = build.deps_command(cmd)  # the same command, preprocessing only, to the object's depfile
        assert "-c" not in deps and "-o" not in deps and deps[-6:] == ["-M", "--cuda-host-only", "-MT", obj, "-MF", obj + ".d"]
        assert deps[:-6] == [a for a in cmd if a not in ("-c", "-o", obj)]
    prof = build.compile_command(build.PROF_SOURCE, ["-DPP_W=64"])
    assert " ".join(build.COMMON + build.PER_SOURCE["tds_tree.hip"]) in " ".join(prof) and prof[-1] == "-DPP_W=64"


@pytest.mark.parametrize("source", build.SOURCES)
def test_scan_matches_depfile(source):
    """kernel_digest's include scan and the rebuild rule see the same files of the repository."""
    path = os.path.join(build.CSRC, source)
    depfile = _object(source) + ".d"
    if not os.path.exists(depfile):
        pytest.skip("no depfiles under _obj/ (this tree received only the library)")
    assert build.include_graph(path) == build.depfile_sources(depfile) - {path}


def test_depfiles_name_the_repository_relative_to_its_root(tree, monkeypatch):
    """A built tree that is copied elsewhere still knows what its objects were built from: the depfiles
    name the repository's files relative to its root, whatever the compiler wrote."""
    depfile = _object("tds_plan.hip") + ".d"
    text = open(depfile).read()
    assert build.ROOT not in text and os.path.join("areafunctionsynthesis_amd", "csrc", "tree_plan.h") in text
    path = os.path.join(build.CSRC, "tds_plan.hip")
    assert build.depfile_sources(depfile) - {path} == build.include_graph(path)
    # the same depfile read from a copy of the tree at another place names the copy's files
    here, there = build.ROOT, os.path.join(tree.root, "moved")
    moved = {os.path.join(there, os.path.relpath(f, here)) for f in build.include_graph(path) | {path}}
    monkeypatch.setattr(build, "ROOT", there)
    assert build.depfile_sources(depfile) == moved
    # a file outside the repository (a system header) keeps its absolute name and is not the repository's
    with open(depfile, "a") as fh:
        fh.write("x.o: /usr/include/stdio.h with\\ space.h\n")
    build.relocatable_depfile(depfile)
    assert "/usr/include/stdio.h" in open(depfile).read() and "with\\ space.h" in open(depfile).read()
    assert build.depfile_sources(depfile) == moved | {os.path.join(there, "with space.h")}


def test_nothing_newer_nothing_stale(tree):
    assert tree.rebuilt() == ([], [])
    assert all(build.stale_reason(build.compile_command(s, objdir=build.OBJ)) is None for s in build.SOURCES)


def test_newer_header_rebuilds_its_includers(tree):
    tree.newer("afs_xcd_order.h")
    assert tree.rebuilt() == (["afs_capi.cpp"], ["libafs.so.tmp"])
    tree.newer("tree_plan.h")
    plan = os.path.join(build.CSRC, "tree_plan.h")
    named = sorted(s for s in build.SOURCES if plan in build.depfile_sources(_object(s) + ".d"))
    assert "tds_plan.hip" in named and "audio_kernels.hip" not in named
    assert tree.rebuilt() == (named, ["libafs.so.tmp"])


def test_changed_tree_flags_rebuild_the_tree_kernel(tree, monkeypatch):
    monkeypatch.setenv("AFS_TREE_FLAGS", "-mllvm -amdgpu-schedule-metric-bias=20")
    try:
        importlib.reload(build)
        tree.redirect()
        assert build.PER_SOURCE["tds_tree.hip"][-2:] == ["-mllvm", "-amdgpu-schedule-metric-bias=20"]
        assert tree.rebuilt() == (["tds_tree.hip"], ["libafs.so.tmp"])
        assert tree.rebuilt() == ([], [])
    finally:
        monkeypatch.delenv("AFS_TREE_FLAGS")
        importlib.reload(build)
    tree.redirect()
    assert tree.rebuilt() == (["tds_tree.hip"], ["libafs.so.tmp"])


def test_missing_depfile_or_object_is_stale(tree):
    os.remove(os.path.join(build.OBJ, "tds_lane.o.d"))
    os.remove(os.path.join(build.OBJ, "afs_comm.o"))
    assert tree.rebuilt() == (["afs_comm.cpp", "tds_lane.hip"], ["libafs.so.tmp"])


def test_force_rebuilds_everything(tree):
    assert tree.rebuilt(force=True) == (sorted(build.SOURCES), ["libafs.so.tmp"])


def test_failed_compile_fails_the_build_and_links_nothing(tree):
    lib = os.path.join(tree.root, "libafs.so")
    os.remove(lib)
    tree.newer("afs_audio.h")
    tree.fail = "audio_kernels.hip"
    with pytest.raises(RuntimeError, match="audio_kernels.hip"):
        tree.rebuilt()
    assert not os.path.exists(lib) and not os.path.exists(lib + ".tmp")
    assert not any("-shared" in c for c in tree.ran)
    tree.fail = None  # the failed object is still stale; the ones that compiled are not
    tree.monkeypatch.setattr(build, "_mtime", os.path.getmtime)
    assert tree.rebuilt() == (["audio_kernels.hip"], ["libafs.so.tmp"])


def test_variant_build_keeps_to_its_own_files(tree):
    before = _files(tree.root)
    objs, libs = tree.rebuilt(tag="nz", flags=["-DAFS_NZ_SET=3"], tree_extra=["-DT=1"], plan_extra=["-DP=1"], profiler=True)
    assert objs == sorted(build.SOURCES + ["phase_prof.hip", "phase_prof.hip"])
    assert libs == ["libafs_nz.so.tmp", "libphase_prof_nz.so.tmp", "libphase_prof_w64_nz.so.tmp"]
    new = {os.path.relpath(f, tree.root) for f in _files(tree.root) - before}
    assert {f for f in new if not f.startswith(os.path.join("_obj", "nz") + os.sep)} == {
        "libafs_nz.so", os.path.join("prof", "libphase_prof_nz.so"), os.path.join("prof", "libphase_prof_w64_nz.so")}
    # the product's command plus the variant's flags, per source
    for cmd in tree.ran:
        if "-c" not in cmd:
            continue
        src = next(a for a in cmd if a.endswith((".cpp", ".hip")))
        name = os.path.basename(src)
        base = build.compile_command(build.PROF_SOURCE if name == "phase_prof.hip" else name)
        flags = lambda c: c[c.index("--offload-arch=" + build.ARCH) + 1:]  # noqa: E731
        extra = {"tds_tree.hip": ["-DT=1"], "phase_prof.hip": ["-DT=1"], "tds_plan.hip": ["-DP=1"]}.get(name, [])
        w64 = ["-DPP_W=64"] if "_w64" in cmd[cmd.index("-o") + 1] else []
        assert flags(cmd) == flags(base) + ["-DAFS_NZ_SET=3"] + extra + w64
    # replacement flags for the tree kernel reach the tree kernel and the profiler alone
    objs, _ = tree.rebuilt(tag="nz", flags=["-DAFS_NZ_SET=3"], tree_extra=["-DT=1"], plan_extra=["-DP=1"], profiler=True,
                           tree_flags=["-fno-signed-zeros"])
    assert objs == ["phase_prof.hip", "phase_prof.hip", "tds_tree.hip"]
    assert all(build.TREE_FLAGS[1] not in c for c in tree.ran)
    # and the default build's objects and library are as they were
    assert tree.rebuilt() == ([], [])
