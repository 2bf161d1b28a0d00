"""afs_buf.h -- the owner of the library's device and pinned host buffers -- over a counting malloc /
free allocator, as a CPU program (tests/cpp/buf_main.cpp) built with AddressSanitizer and
UndefinedBehaviorSanitizer: reserve below or at the capacity allocates nothing and keeps the block;
growth frees the old block before it allocates (never two live blocks per buffer); a failing
allocation leaves the buffer empty and the next reserve recovers; a move leaves its source empty; at
scope exit every allocation is freed (the counter is back at zero and the leak checker silent)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_buffer_properties(tmp_path):
    exe = str(tmp_path / "buf_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "areafunctionsynthesis_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "buf_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr[-3000:]
    assert r.stdout.strip() == "buf-ok"
