"""Build libafs.so (HIP, gfx950) in-tree with hipcc: the one description of what the library,
its A/B variants and the phase profiler are compiled from.

Usage: python -m areafunctionsynthesis_amd.build [--force] [--tag TAG] [--flags "..."]
           [--tree-flags "..."] [--tree-extra "..."] [--plan-extra "..."] [--profiler]
The shared library lands next to this file so it travels with the repository snapshot; a tag
gives libafs_TAG.so (loaded with AFS_LIB) from objects of its own under _obj/TAG/.
--profiler also links tools/phase_prof/libphase_prof[_TAG].so and libphase_prof_w64[_TAG].so.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(ROOT, "include")
OBJ = os.path.join(HERE, "_obj")
LIB = os.path.join(HERE, "libafs.so")
ARCH = os.environ.get("AFS_OFFLOAD_ARCH", "gfx950")

SOURCES = ["afs_capi.cpp", "afs_comm.cpp", "afs_tables.cpp", "tds_lane.hip", "tds_tree.hip", "tds_plan.hip",
           "af_kernels.hip", "audio_kernels.hip", "session_kernels.hip", "device_math.hip"]
# The phase profiler (tools/phase_prof): the tree kernel's body with cycle counters, linked with
# the library's own objects of the kernels and their tables.
PROF_DIR = os.path.join(ROOT, "tools", "phase_prof")
PROF_SOURCE = os.path.join(PROF_DIR, "phase_prof.hip")
PROF_SOURCES = ["afs_tables.cpp", "tds_tree.hip", "tds_plan.hip"]
# Per-source extra flags.
# The tree kernel contracts a*b+c into fma (-ffp-contract=fast-honor-pragmas after COMMON's
# =off; plain "fast" ignores the `#pragma clang fp contract(off)` that keeps the tube
# interpolation uncontracted like K5's and the reference's, tests/test_plan_gpu.py): 8 % fewer
# VALU instructions in its time loop, +3.5 % end to end (A/B, profiles/r02ac_contract_ab.txt);
# its results stay within the parity tolerances (the reference's own build with FMA
# contraction differs from its -O2 build by up to 5.7e-9 over a second).  The
# plan kernel (K5, the reference's discrete constriction decisions) and the lane kernel (the
# reference's operation order) keep COMMON's -ffp-contract=off.
# The tree kernel is built without machine-level loop-invariant code motion: hoisting the
# lanes' loop-invariant comparisons out of the time loop kept ~50 lane masks alive in SGPR
# pairs, more than the wave has, and their spills cost ~100 v_readlane/v_writelane and ~130
# AGPR moves per sample (A/B: 89.0 vs 89.25 ms per launch).
# The machine scheduler's iterative-ilp strategy (re-schedules each region for latency once
# the register budget is known): 25.9 k -> 25.2 k cycles per wave-sample, +1.5-2 % end to
# end (A/B alternated, profiles/r03k_sched_ab.txt; iterative-minreg -16 %, post-RA machine
# scheduler / no machine sinking / no memop clustering neutral or slower).  Instruction order
# only: the results are bit-identical.
# -fno-signed-zeros: the reference's accumulations from 0.0 (`double u = 0.0; u += x;`, ~35 per
# sample) are kept as written in the source and compile to x; they differ from x only for x = -0,
# and no comparison, product or sum in this kernel tells -0 from +0 except in a zero result (no
# division by a possibly-zero value, no copysign).  A/B: profiles/r04n_nsz_ab.txt.
TREE_FLAGS = ["-mllvm", "-disable-machine-licm", "-ffp-contract=fast-honor-pragmas", "-fno-signed-zeros", "-mllvm", "-amdgpu-sched-strategy=iterative-ilp"]
# The arithmetic probe (device_math.hip, afs_device_math) runs tree_core.h's device-only forms on their
# own: it takes exactly TREE_FLAGS, so that a test of it measures the arithmetic as the synthesis
# kernel's compilation makes it (contraction, no signed zeros).
PER_SOURCE: dict = {"tds_tree.hip": list(TREE_FLAGS), "device_math.hip": list(TREE_FLAGS)}
# (AFS_TREE_FLAGS: extra compiler flags for the tree kernel, for A/B builds of scheduler options)
if os.environ.get("AFS_TREE_FLAGS"):
    PER_SOURCE["tds_tree.hip"] = TREE_FLAGS + os.environ["AFS_TREE_FLAGS"].split()

COMMON = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
          # keep the reference's rounding: no contraction of a*b+c into fma (except the tree
          # kernel, TREE_FLAGS)
          "-ffp-contract=off", "-fno-strict-aliasing", "-Wno-unknown-pragmas"]

_mtime = os.path.getmtime


def _hipcc() -> str:
    for p in ("/opt/rocm/bin/hipcc", "hipcc"):
        if os.path.sep not in p or os.path.exists(p):
            return p
    return "hipcc"


def compile_command(source: str, extra=(), objdir: str = OBJ, output: str | None = None, per_source: dict = PER_SOURCE) -> list:
    """The hipcc command that compiles one source: a name of SOURCES, or PROF_SOURCE, which
    instantiates tree_kernel.h and so takes the tree kernel's flags.  `extra` follows the
    source's own flags; the object (or whatever `extra` makes of it) goes to `output`, by
    default into `objdir`."""
    if source == PROF_SOURCE:
        path, flags = source, per_source.get("tds_tree.hip", []) + ["-I" + CSRC, "-I" + INCLUDE]
    else:
        path, flags = os.path.join(CSRC, source), per_source.get(source, [])
    output = output or os.path.join(objdir, os.path.splitext(os.path.basename(source))[0] + ".o")
    lang = ["-x", "hip"] if source.endswith(".cpp") else []
    return [_hipcc(), "-c"] + lang + [path, "-o", output, f"--offload-arch={ARCH}"] + COMMON + flags + list(extra)


def _output(cmd: list) -> str:
    return cmd[cmd.index("-o") + 1]


def deps_command(cmd: list) -> list:
    """The command that writes the depfile of a compile command's object, <object>.d: the same
    flags, preprocessing only.  (-MD in the compile command itself would do, but hipcc derives
    the object's unit id, the __hip_cuid_* symbol of the host object and the code object, from
    a hash of its whole command line, and the objects are to stay what they were before the
    compiler listed their dependencies.)"""
    obj = _output(cmd)
    rest = [a for a in cmd if a != "-c"]
    i = rest.index("-o")
    return rest[:i] + rest[i + 2:] + ["-M", "--cuda-host-only", "-MT", obj, "-MF", obj + ".d"]


def _depfile_rules(depfile: str) -> list:
    """A depfile's rules as (target, [dependencies]), the paths unescaped."""
    with open(depfile, encoding="utf-8") as fh:
        text = fh.read().replace("\\\n", " ")
    rules = []
    for rule in text.splitlines():
        target, sep, deps = rule.partition(": ")
        if sep:
            rules.append((target.replace("\\ ", " "), [d.replace("\\ ", " ") for d in re.split(r"(?<!\\)\s+", deps) if d]))
    return rules


def depfile_sources(depfile: str) -> set:
    """The files of this repository that a compiler's depfile names (a relative path is one
    below the repository's root: relocatable_depfile)."""
    deps = set()
    for _, names in _depfile_rules(depfile):
        for d in names:
            d = os.path.normpath(os.path.join(ROOT, d))  # (an absolute path stays what it is)
            if d.startswith(ROOT + os.sep):
                deps.add(d)
    return deps


def relocatable_depfile(depfile: str) -> None:
    """Rewrite a compiler's depfile with the repository's own files named relative to its root:
    the compiler writes absolute paths, and a built tree that is copied or moved elsewhere would
    no longer know what its objects were built from (every object stale, and the include scan
    with nothing to agree with)."""
    def rel(p):
        p = os.path.normpath(p)
        return os.path.relpath(p, ROOT) if p.startswith(ROOT + os.sep) else p
    esc = lambda p: p.replace(" ", "\\ ")  # noqa: E731
    lines = [esc(rel(t)) + ": " + " \\\n  ".join(esc(rel(d)) for d in deps) + "\n" for t, deps in _depfile_rules(depfile)]
    with open(depfile, "w", encoding="utf-8") as fh:
        fh.writelines(lines)


def stale_reason(cmd: list) -> str | None:
    """Why the object of this compile command has to be rebuilt (None: it is up to date)."""
    obj = _output(cmd)
    if not os.path.exists(obj):
        return "missing"
    if not os.path.exists(obj + ".d"):
        return "no depfile"
    t = _mtime(obj)
    for d in sorted(depfile_sources(obj + ".d")):
        if not os.path.exists(d) or _mtime(d) > t:
            return "older than " + os.path.relpath(d, ROOT)
    try:
        with open(obj + ".cmd", encoding="utf-8") as fh:
            if fh.read().split("\n") == cmd:
                return None
    except OSError:
        pass
    return "built by another command"


def _run(cmd: list) -> None:
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode:
        raise RuntimeError(f"{' '.join(cmd)}\nfailed with status {p.returncode}:\n{p.stdout}")
    if p.stdout:
        print(p.stdout, end="", flush=True)


def _compile(cmd: list) -> None:
    obj = _output(cmd)
    if os.path.exists(obj + ".cmd"):  # (an interrupted compile leaves the object stale)
        os.remove(obj + ".cmd")
    _run(cmd)
    _run(deps_command(cmd))
    relocatable_depfile(obj + ".d")
    with open(obj + ".cmd", "w", encoding="utf-8") as fh:
        fh.write("\n".join(cmd))


def _link(lib: str, objs: list, relink: bool, verbose: bool) -> None:
    if not relink and os.path.exists(lib) and all(_mtime(o) <= _mtime(lib) for o in objs):
        return
    cmd = [_hipcc(), "-shared", "-o", lib + ".tmp", f"--offload-arch={ARCH}", "-fPIC"] + objs + ["-ldl"]
    if verbose:
        print(" ".join(cmd), flush=True)
    _run(cmd)
    os.replace(lib + ".tmp", lib)


def build(force: bool = False, verbose: bool = True, tag: str = "", flags=(), tree_flags=None, tree_extra=(),
          plan_extra=(), profiler: bool = False) -> str:
    """Compile what is stale, concurrently, and link libafs.so (libafs_TAG.so for a variant:
    `flags` for every source, `tree_flags` in place of the tree kernel's, `tree_extra` and
    `plan_extra` after the tree and plan kernels' own); with `profiler` the phase profiler's
    two libraries as well, from the same objects."""
    objdir = os.path.join(OBJ, tag) if tag else OBJ
    suffix = f"_{tag}.so" if tag else ".so"
    per_source = PER_SOURCE if tree_flags is None else dict(PER_SOURCE, **{"tds_tree.hip": list(tree_flags)})
    extra = {"tds_tree.hip": list(tree_extra), "tds_plan.hip": list(plan_extra), PROF_SOURCE: list(tree_extra)}
    cmds = {s: compile_command(s, list(flags) + extra.get(s, []), objdir, None, per_source) for s in SOURCES}
    if profiler:
        for w64 in ("", "_w64"):
            cmds["phase_prof" + w64] = compile_command(
                PROF_SOURCE, list(flags) + extra[PROF_SOURCE] + (["-DPP_W=64"] if w64 else []), objdir,
                os.path.join(objdir, f"phase_prof{w64}.o"), per_source)
    todo = [c for c in cmds.values() if force or stale_reason(c)]
    if todo:
        os.makedirs(objdir, exist_ok=True)
        if verbose:
            for c in todo:
                print(" ".join(c), flush=True)
        jobs = min(len(todo), int(os.environ.get("MAX_JOBS") or 16), 16)
        with ThreadPoolExecutor(max(1, jobs)) as pool:
            for f in [pool.submit(_compile, c) for c in todo]:
                f.result()
    rebuilt = {_output(c) for c in todo}
    lib = os.path.join(HERE, "libafs" + suffix)
    objs = [_output(cmds[s]) for s in SOURCES]
    _link(lib, objs, any(o in rebuilt for o in objs), verbose)
    if profiler:
        for w64 in ("", "_w64"):
            objs = [_output(cmds["phase_prof" + w64])] + [_output(cmds[s]) for s in PROF_SOURCES]
            _link(os.path.join(PROF_DIR, f"libphase_prof{w64}{suffix}"), objs, any(o in rebuilt for o in objs), verbose)
    return lib


def include_graph(path: str) -> set:
    """The files of this repository that a source reaches through `#include "..."`, read from
    the text (no compiler: bench.py needs kernel_digest where only the library travelled)."""
    seen: set = set()
    todo = [path]
    while todo:
        f = todo.pop()
        for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', _code(f), flags=re.M):
            for d in (os.path.dirname(f), CSRC, INCLUDE):
                inc = os.path.normpath(os.path.join(d, name))
                if os.path.exists(inc):
                    if inc not in seen:
                        seen.add(inc)
                        todo.append(inc)
                    break
    return seen


def _code(path: str) -> str:
    """A source's text without its comments."""
    with open(path, encoding="utf-8") as fh:
        text = fh.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def kernel_digest(source: str = "tds_tree.hip") -> str:
    """Digest of what one kernel's object is built from (the source file, the headers it
    includes, its compiler flags): the committed PMC summaries (profiles/pmc_*.json) are keyed
    by it, so bench.py quotes a counter figure only for the kernel it is timing."""
    h = hashlib.sha1()
    path = os.path.join(CSRC, source)
    for f in [path] + sorted(include_graph(path)):
        h.update(os.path.relpath(f, ROOT).replace(os.sep, "/").encode())
        # (comments and blank space do not change the object: documentation edits keep the key)
        h.update(" ".join(_code(f).split()).encode())
    h.update(repr((COMMON, PER_SOURCE.get(source, []))).encode())
    return h.hexdigest()[:12]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--force", action="store_true", help="rebuild every object")
    ap.add_argument("--tag", default="", help="variant: libafs_TAG.so from objects under _obj/TAG/")
    ap.add_argument("--flags", default="", help="extra flags for every source (e.g. -DAFS_...)")
    ap.add_argument("--tree-flags", default=None, help="flags of tds_tree.hip in place of TREE_FLAGS")
    ap.add_argument("--tree-extra", default="", help="extra flags for tds_tree.hip")
    ap.add_argument("--plan-extra", default="", help="extra flags for tds_plan.hip")
    ap.add_argument("--profiler", action="store_true", help="also build tools/phase_prof's two libraries")
    a = ap.parse_args()
    build(force=a.force, tag=a.tag, flags=a.flags.split(), tree_flags=None if a.tree_flags is None else a.tree_flags.split(),
          tree_extra=a.tree_extra.split(), plan_extra=a.plan_extra.split(), profiler=a.profiler)


if __name__ == "__main__":
    main()
