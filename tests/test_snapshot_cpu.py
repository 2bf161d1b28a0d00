"""Voice snapshots without a GPU: the four entry points are declared and bound (ABI 5 still); the record
layout, the vector map of the gather and scatter kernels and the header check as a CPU program
(tests/cpp/voice_state_main.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer; and the branching
behind Context.synthesize_candidates (synthesizer.branch_candidates) on a stand-in session in numpy whose
every "sample" encodes the frames that produced it, so that a row says which history its voice had."""
import os
import re
import subprocess

import numpy as np
import pytest

from areafunctionsynthesis_amd import _native
from areafunctionsynthesis_amd.frames import FRAME_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("afs_session_voice_state_bytes", "afs_session_save_voices", "afs_session_load_voices",
                "afs_session_copy_voices")


def test_entry_points_declared_and_bound():
    with open(os.path.join(ROOT, "include", "afs.h"), encoding="utf-8") as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in ENTRY_POINTS:
        kind = "int64_t" if name.endswith("_bytes") else "afs_status"
        assert re.search(r"\b" + kind + r"\s+" + name + r"\s*\(", header), name
        assert name in _native.EXPORTED
    assert re.search(r"#define\s+AFS_ABI_VERSION\s+5\b", header)  # (an addition only)
    lib = _native.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert lib.afs_abi_version() == 5
    assert lib.afs_session_voice_state_bytes(None) == 0  # (no session: no record)


def test_python_surface():
    from areafunctionsynthesis_amd.synthesizer import Context, Synthesizer
    for name in ("voice_state_bytes", "save_voices", "load_voices", "copy_voices", "fork"):
        assert hasattr(Synthesizer, name), name
    assert hasattr(Context, "synthesize_candidates")


def test_voice_state_layout_properties(tmp_path):
    exe = str(tmp_path / "voice_state_main")
    # (-Wno-unknown-pragmas: tree_core.h, which supplies sizeof(Lane<W>) and X_TOTAL, carries the device
    # compiler's unroll pragmas, as the library's own build allows)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "areafunctionsynthesis_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "voice_state_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr[-3000:]
    assert r.stdout.strip() == "voice-state-ok"


# ---- the branching on a stand-in session ----------------------------------------------------------

HOP = 4


def frames_of(tag, F, first=0):
    """F frames tagged (tag, first .. first + F - 1) in two of their fields."""
    fr = np.zeros(F, dtype=FRAME_DTYPE)
    fr["teeth_position_cm"] = tag
    fr["velum_opening_cm2"] = first + np.arange(F)
    return fr


def ident(f):
    return int(f["teeth_position_cm"]), int(f["velum_opening_cm2"])


def code(history, j):
    """The stand-in's sample j of the transition that ends a voice's history of frames: it depends on
    every frame the voice has seen, in order."""
    h = 0
    for tag, k in history:
        h = (h * 31 + tag * 7 + k + 1) % 100003
    return h * 10 + j


class StandIn:
    """What branch_candidates needs of a session -- batch, synthesize_frames, fork -- with the pool
    call's semantics (an unlatched voice latches its first frame; count 0 is idle), a voice's state being
    the list of frames it has seen, and a log of calls."""

    def __init__(self, batch):
        self.batch = batch
        self.history = [[] for _ in range(batch)]
        self.calls = []

    def synthesize_frames(self, frames, num_frames, hop, out=None, pcm=False):
        assert frames.shape[0] == self.batch and out is None
        rows = []
        for u, c in enumerate(num_frames):
            row = []
            for f in frames[u, :c]:
                latched = bool(self.history[u])
                self.history[u].append(ident(f))
                if latched:
                    row += [code(self.history[u], j) for j in range(hop)]
            rows.append(row)
        produced = np.array([len(r) for r in rows], dtype=np.int32)
        audio = np.zeros((self.batch, int(produced.max())), dtype=np.int16 if pcm else np.float64)
        for u, r in enumerate(rows):
            audio[u, :len(r)] = np.array(r) % (30000 if pcm else 10 ** 9)
        self.calls.append(("frames", [int(c) for c in num_frames], pcm))
        return audio, produced

    def fork(self, voice, into):
        into = [int(v) for v in into]
        assert len(set(into)) == len(into) and int(voice) not in into
        for v in into:
            self.history[v] = list(self.history[int(voice)])
        self.calls.append(("fork", int(voice), into))


@pytest.mark.parametrize("K,Fp,Fc,pcm", [(5, 4, 3, False), (3, 1, 4, True), (1, 3, 3, False)])
def test_branching_call_sequence(K, Fp, Fc, pcm):
    from areafunctionsynthesis_amd.synthesizer import branch_candidates
    s = StandIn(K)
    prefix = frames_of(1000, Fp)
    candidates = np.stack([frames_of(k + 1, Fc, first=Fp) for k in range(K)])
    audio = branch_candidates(s, prefix, candidates, HOP, pcm=pcm)
    # the prefix on voice 0 alone, one fork into every other voice, one call of the candidates
    want_calls = [("frames", [Fp] + [0] * (K - 1), pcm)]
    if K > 1:
        want_calls.append(("fork", 0, list(range(1, K))))
    want_calls.append(("frames", [Fc] * K, pcm))
    assert s.calls == want_calls
    assert audio.shape == (K, Fc * HOP) and audio.dtype == (np.int16 if pcm else np.float64)
    # row k: what a voice that saw prefix + candidates[k], and nothing else, produces for the candidate
    for k in range(K):
        history = [ident(f) for f in prefix]
        row = []
        for f in candidates[k]:
            history.append(ident(f))
            row += [code(history, j) for j in range(HOP)]
        assert np.array_equal(audio[k], np.array(row) % (30000 if pcm else 10 ** 9)), k
    assert len({tuple(audio[k]) for k in range(K)}) == K  # (the candidates differ, so do their rows)


def test_branching_refuses_bad_shapes():
    from areafunctionsynthesis_amd.synthesizer import branch_candidates
    s = StandIn(3)
    with pytest.raises(ValueError):
        branch_candidates(s, frames_of(1, 2), np.stack([frames_of(k, 3) for k in range(2)]), HOP)  # (2 rows, 3 voices)
    with pytest.raises(ValueError):
        branch_candidates(s, frames_of(1, 0), np.stack([frames_of(k, 3) for k in range(3)]), HOP)  # (no prefix frame)
    assert s.calls == []
