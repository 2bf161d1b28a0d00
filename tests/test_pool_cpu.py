"""The voice pool without a GPU: the four entry points are declared and bound (ABI 5 still); the launch
layout afs::pool_order as a CPU program (tests/cpp/pool_order_main.cpp) under AddressSanitizer and
UndefinedBehaviorSanitizer; and the continuous-batching scheduler (synthesizer.stream_utterances) on a
stand-in session in numpy whose every "sample" encodes (seed, frame index of the utterance, offset in the
hop), so that an utterance's audio says which frames produced it, in which order, under which seed."""
import os
import re
import subprocess

import numpy as np
import pytest

from areafunctionsynthesis_amd import _native
from areafunctionsynthesis_amd.frames import FRAME_DTYPE
from areafunctionsynthesis_amd.synthesizer import stream_utterances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("afs_session_restart_voices", "afs_session_synthesize_ragged", "afs_session_synthesize_ragged_pcm",
                "afs_session_latched")


def test_entry_points_declared_and_bound():
    with open(os.path.join(ROOT, "include", "afs.h"), encoding="utf-8") as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\bafs_status\s+" + name + r"\s*\(", header), name
        assert name in _native.EXPORTED
    assert re.search(r"#define\s+AFS_ABI_VERSION\s+5\b", header)  # (an addition only)
    lib = _native.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_pool_order_properties(tmp_path):
    exe = str(tmp_path / "pool_order_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "areafunctionsynthesis_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "pool_order_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr[-3000:]
    assert r.stdout.strip() == "pool-order-ok"


# ---- the scheduler on a stand-in session ----------------------------------------------------------

HOP = 4


def utterance(i, F):
    """F frames of utterance i: frame k carries (i, k) in two of its fields."""
    fr = np.zeros(F, dtype=FRAME_DTYPE)
    fr["teeth_position_cm"] = i
    fr["velum_opening_cm2"] = np.arange(F)
    return fr


def code(seed, k, j):
    """The stand-in's sample j of the transition into frame k of a voice seeded `seed`."""
    return (seed * 1000 + k) * 10 + j


class StandIn:
    """What stream_utterances needs of a session -- batch, restart, synthesize_frames -- with the pool
    call's semantics (an unlatched voice latches its first frame; count 0 is idle) and a log of calls."""

    def __init__(self, batch):
        self.batch = batch
        self.seed = [None] * batch
        self.latch = [None] * batch  # the latched frame's (utterance, frame index), None: unlatched
        self.calls = []              # ("restart", voices, seeds) | ("step", counts, [(utterance, first frame) | None])

    def restart(self, voices, seeds=None):
        assert len(set(voices)) == len(voices) and len(seeds) == len(voices)
        for v, s in zip(voices, seeds):
            self.seed[v], self.latch[v] = int(s), None
        self.calls.append(("restart", list(voices), [int(s) for s in seeds]))

    def synthesize_frames(self, frames, num_frames, hop, out=None, pcm=False, report=False):
        assert report and frames.shape[0] == self.batch and out.shape[0] == self.batch
        produced = np.zeros(self.batch, dtype=np.int32)
        heads = []
        for u, c in enumerate(num_frames):
            heads.append(None if c == 0 else (int(frames[u, 0]["teeth_position_cm"]), int(frames[u, 0]["velum_opening_cm2"])))
            n = 0
            for f in frames[u, :c]:
                i, k = int(f["teeth_position_cm"]), int(f["velum_opening_cm2"])
                if self.latch[u] is not None:
                    assert self.latch[u] == (i, k - 1), "a frame out of order"
                    out[u, n:n + hop] = [code(self.seed[u], k, j) for j in range(hop)]
                    n += hop
                else:
                    assert k == 0, "a restarted voice starts at frame 0"
                self.latch[u] = (i, k)
            produced[u] = n
        self.calls.append(("step", [int(c) for c in num_frames], heads))
        return out, produced, {"nonfinite": np.zeros(self.batch, dtype=np.uint8)}


LENGTHS = [5, 2, 9, 3, 3, 7, 2, 4, 11, 2, 6]


def want(i, F, seed):
    return np.array([code(seed, k, j) for k in range(1, F) for j in range(HOP)], dtype=np.float64)


@pytest.mark.parametrize("slots,chunk,seeds", [(3, 3, None), (4, 1, "own"), (16, 4, None), (1, 2, "own")])
def test_scheduler_yields_every_utterance_once(slots, chunk, seeds):
    s = StandIn(slots)
    corpus = (utterance(i, F) for i, F in enumerate(LENGTHS))  # (an iterable, not a list)
    seed_of = [i + 1 for i in range(len(LENGTHS))] if seeds is None else [500 + 3 * i for i in range(len(LENGTHS))]
    ended = []
    got = dict()
    for i, audio in stream_utterances(s, corpus, HOP, chunk, seeds=None if seeds is None else seed_of, pcm=False,
                                      finished=lambda i, u, sess, nf: ended.append((i, u, nf))):
        assert i not in got
        got[i] = audio
    assert sorted(got) == list(range(len(LENGTHS))) and [e[0] for e in ended] == list(got)
    for i, F in enumerate(LENGTHS):
        assert got[i].dtype == np.float64 and np.array_equal(got[i], want(i, F, seed_of[i])), i
    steps = [c for c in s.calls if c[0] == "step"]
    assert all(max(c[1]) <= chunk for c in steps)  # (no voice gets more than chunk_frames frames)
    # a voice that ended in step t starts the next utterance in step t + 1 while the corpus lasts: it is
    # restarted between the two steps with that utterance's seed, and never idles before the corpus is dry
    started = [v for c in s.calls if c[0] == "restart" for v in c[2]]
    assert started == seed_of  # (every utterance restarted once, in corpus order)
    first_dry = None
    for t, (_, counts, heads) in enumerate(steps):
        if any(c == 0 for c in counts) and first_dry is None:
            first_dry = t
    handed_out = 0
    for t, (_, counts, heads) in enumerate(steps):
        handed_out += sum(1 for h in heads if h is not None and h[1] == 0)
        if any(c == 0 for c in counts):  # an idle voice: only once every utterance has been handed out
            assert handed_out == len(LENGTHS)
    if 1 < slots < len(LENGTHS):
        # (the utterances end at different steps: the tail runs voices idle beside the last one playing)
        assert first_dry is not None and 0 < steps[-1][1].count(0) < slots
    elif slots > 1:
        assert steps[0][1].count(0) == slots - len(LENGTHS)  # (more slots than utterances: idle from the start)


def test_slot_refills_in_the_next_step():
    """3 slots, chunks of 3: utterance 1 (2 frames) ends in step 0, and step 1 plays utterance 3 in its slot."""
    s = StandIn(3)
    list(stream_utterances(s, [utterance(i, F) for i, F in enumerate(LENGTHS)], HOP, 3, pcm=False))
    assert s.calls[0] == ("restart", [0, 1, 2], [1, 2, 3])
    assert s.calls[1] == ("step", [3, 2, 3], [(0, 0), (1, 0), (2, 0)])
    assert s.calls[2] == ("restart", [1], [4])
    assert s.calls[3] == ("step", [2, 3, 3], [(0, 3), (3, 0), (2, 3)])
    assert s.calls[-1][0] == "step" and sorted(s.calls[-1][1])[:2] == [0, 0]  # (the last step: two voices idle)


def test_short_utterance_raises():
    s = StandIn(2)
    with pytest.raises(ValueError, match="at least 2"):
        list(stream_utterances(s, [utterance(0, 3), utterance(1, 1)], HOP, 3, pcm=False))
    with pytest.raises(ValueError):
        list(stream_utterances(s, [utterance(0, 3)], HOP, 0, pcm=False))


def test_pcm_audio_is_int16():
    s = StandIn(2)
    for i, audio in stream_utterances(s, [utterance(0, 3)], 2, 2, seeds=[1], pcm=True):
        assert audio.dtype == np.int16 and list(audio) == [code(1, 1, 0), code(1, 1, 1), code(1, 2, 0), code(1, 2, 1)]
