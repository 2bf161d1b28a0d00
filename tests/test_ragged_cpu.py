"""afs_ragged_order.h -- the slot layout of afs_synthesize_ragged -- as a CPU program
(tests/cpp/ragged_order_main.cpp), built with AddressSanitizer and UndefinedBehaviorSanitizer, for
(B, slots per block) = (1, 8), (21, 8) with the frame counts of the GPU tests, (64, 8) all equal,
(9, 8) all distinct, (1025, 1) and (40, 16): every utterance in exactly one slot, padding slots hold a
value >= B and read a live utterance of their own block, the live utterances of a block share its end
(F - 1) * hop, blocks do not grow, at most (slots - 1) x distinct lengths padding slots, call order
inside a length, equal lengths give the identity in ceil(B / slots) blocks, and the result is
deterministic.  And the new entry point is declared and bound."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ragged_order_properties(tmp_path):
    exe = str(tmp_path / "ragged_order_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "areafunctionsynthesis_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ragged_order_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr[-3000:]
    assert r.stdout.strip() == "ragged-order-ok"


def test_entry_point_declared_and_bound():
    from areafunctionsynthesis_amd import _native
    with open(os.path.join(ROOT, "include", "afs.h"), encoding="utf-8") as fh:
        header = fh.read()
    assert re.search(r"\bafs_status\s+afs_synthesize_ragged\s*\(", header)
    assert re.search(r"#define\s+AFS_ABI_VERSION\s+5\b", header)  # (an addition only)
    assert "afs_synthesize_ragged" in _native.EXPORTED
