"""afs_xcd_order.h -- the slot order of utterances that share trajectories (afs_play_target_sequences)
-- as a CPU program (tests/cpp/xcd_order_main.cpp), built with AddressSanitizer and
UndefinedBehaviorSanitizer: (B, utterances per block, concurrent blocks) = (1, 8, 1), (5, 1, 4),
(21, 8, 2), (64, 8, 3), (130, 8, 256) with rows of period 3.  Every utterance sits in one slot, the
padding slots hold B, a block's utterances ascend in (row, utterance), and a round's blocks taken XCD
by XCD give the row-sorted list."""
import os
import subprocess


def test_xcd_order_properties(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "xcd_order_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(root, "areafunctionsynthesis_amd", "csrc"),
                           os.path.join(root, "tests", "cpp", "xcd_order_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr[-3000:]
    assert r.stdout.strip() == "xcd-order-ok"
