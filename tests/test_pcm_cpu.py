"""The PCM output calls without a GPU: the packed int16 stores and the PCM form of the output filter as a
CPU program (tests/cpp/pcm_pack_main.cpp: csrc/tree_core.h PcmPack and output_filter_run_pcm, csrc/afs_audio.h
sample_to_int16) built with AddressSanitizer and UndefinedBehaviorSanitizer and run directly; the header,
the library and the binding name the new entry points."""
import os
import re
import subprocess

from areafunctionsynthesis_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "areafunctionsynthesis_amd", "csrc")
ENTRY_POINTS = ("afs_synthesize_pcm", "afs_synthesize_ragged_pcm", "afs_session_synthesize_pcm", "afs_memory_info_get")


def test_pack_loop_and_pcm_filter_form(tmp_path):
    """Every row alignment 0..7 and run length 0..40 against sample_to_int16 (values at and beside +-1,
    beyond it, +-inf, NaN, +-0, denormals, k/32767 and both neighbours), nothing written outside the run;
    the PCM filter form against the in-place form + sample_to_int16 for n = 1..70 at every split, with and
    without the tone filter: identical int16 and bit-equal state images."""
    exe = str(tmp_path / "pcm_pack_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                           "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-strict-aliasing", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "pcm_pack_main.cpp"), os.path.join(CSRC, "afs_tables.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr[-3000:]
    assert r.stdout.strip() == "pcm-ok"


def test_header_declares_the_entry_points():
    h = open(os.path.join(ROOT, "include", "afs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\bafs_status\s+" + name + r"\s*\(", code), name
    assert int(re.search(r"#define AFS_ABI_VERSION (\d+)", h).group(1)) == 5
    assert "typedef struct afs_memory_info" in code


def test_binding_and_library_name_them():
    lib = _native.load()
    assert lib.afs_abi_version() == 5
    for name in ENTRY_POINTS:
        assert name in _native.EXPORTED
        assert hasattr(lib, name), name
        assert getattr(lib, name).restype is not None and getattr(lib, name).argtypes


def test_adapter_pcm_program_builds(tmp_path):
    """tests/cpp/adapter_pcm_main.cpp (TdsVoices::synthesizeSignalTdsPcm) compiles and links against the library."""
    pkg = os.path.join(ROOT, "areafunctionsynthesis_amd")
    _native.load()
    exe = str(tmp_path / "adapter_pcm_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "adapter_pcm_main.cpp"), "-L", pkg, "-lafs",
                           f"-Wl,-rpath,{pkg}", "-o", exe])
    assert subprocess.run([exe], capture_output=True).returncode == 2  # (no arguments: the usage status)
