"""Indexed voice pools without a GPU: the two entry points are declared in afs.h as _native.py binds them;
the host side of the calls (csrc/afs_indexed.h: span bounds, INT64_MAX, the idle voice's ignored start,
the compaction of a host corpus' live spans) as a CPU program (tests/cpp/indexed_main.cpp) under
AddressSanitizer and UndefinedBehaviorSanitizer; and the corpus scheduler (synthesizer.stream_corpus) on a
stand-in session in numpy whose every "sample" encodes (seed, frame index in the corpus, offset in the
hop), so that the flat result says which frames produced each sample, under which seed, at which place."""
import ctypes
import heapq
import os
import re
import subprocess

import numpy as np
import pytest

from areafunctionsynthesis_amd import _native
from areafunctionsynthesis_amd.frames import FRAME_DTYPE
from areafunctionsynthesis_amd.synthesizer import ragged_offsets, stream_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("afs_session_synthesize_indexed", "afs_session_synthesize_indexed_packed")

C_TYPES = {"afs_session *": ctypes.c_void_p, "const afs_frame *": ctypes.c_void_p, "const int64_t *": ctypes.c_void_p,
           "const int32_t *": ctypes.c_void_p, "double *": ctypes.c_void_p, "void *": ctypes.c_void_p,
           "uint8_t *": ctypes.c_void_p, "int32_t *": ctypes.c_void_p, "int64_t": ctypes.c_int64,
           "int32_t": ctypes.c_int32, "afs_report *": ctypes.POINTER(_native.AfsReport)}


def prototype(header, name):
    """The parameter types of `name` as afs.h declares it: [(C type, parameter name)]."""
    m = re.search(r"\bafs_status\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, name
    params = []
    for p in m.group(1).split(","):
        t, n = re.fullmatch(r"\s*(.*?)(\w+)\s*", " ".join(p.split())).groups()
        params.append((t.strip(), n))
    return params


def test_prototypes_match_the_binding():
    with open(os.path.join(ROOT, "include", "afs.h"), encoding="utf-8") as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    want = {
        "afs_session_synthesize_indexed": ["s", "frames", "total_frames", "frame_start", "num_frames", "hop", "out",
                                           "out_stride", "taps_out", "nonfinite", "produced", "report"],
        "afs_session_synthesize_indexed_packed": ["s", "frames", "total_frames", "frame_start", "num_frames", "hop",
                                                  "format", "out", "offsets", "nonfinite", "produced", "report"],
    }
    assert re.search(r"#define\s+AFS_ABI_VERSION\s+5\b", header)  # (an addition only)
    lib = _native.load()
    for name in ENTRY_POINTS:
        params = prototype(header, name)
        assert [n for _, n in params] == want[name]
        assert name in _native.EXPORTED and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == [C_TYPES[t] for t, _ in params], name
    # (no session: refused before anything is looked at)
    assert lib.afs_session_synthesize_indexed(None, None, 0, None, None, 1, None, 0, None, None, None, None) == 1
    assert lib.afs_session_synthesize_indexed_packed(None, None, 0, None, None, 1, 0, None, None, None, None, None) == 1


def test_python_surface():
    import inspect

    from areafunctionsynthesis_amd.synthesizer import Context, Synthesizer
    assert "frame_start" in inspect.signature(Synthesizer.synthesize_frames).parameters
    assert list(inspect.signature(stream_corpus).parameters) == ["session", "frames", "frame_offsets", "hop", "chunk_frames",
                                                                 "seeds", "pcm", "f32", "out"]
    assert list(inspect.signature(Context.synthesize_corpus).parameters)[:6] == ["self", "frames", "frame_offsets", "hop",
                                                                                "slots", "chunk_frames"]


def test_indexed_host_side(tmp_path):
    exe = str(tmp_path / "indexed_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "areafunctionsynthesis_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "indexed_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr[-3000:]
    assert r.stdout.strip() == "indexed-ok"


def test_capi_runs_the_shared_header():
    """afs_capi.cpp makes its checks and its compaction with the header the CPU program tests."""
    with open(os.path.join(ROOT, "areafunctionsynthesis_amd", "csrc", "afs_capi.cpp"), encoding="utf-8") as fh:
        capi = fh.read()
    assert '#include "afs_indexed.h"' in capi
    for name in ("indexed_check", "indexed_spans", "indexed_rebase", "indexed_compact"):
        assert "afs::" + name + "(" in capi, name


# ---- the scheduler on a stand-in session ----------------------------------------------------------

HOP = 4
LENGTHS = [5, 2, 9, 3, 3, 7, 2, 4, 11, 2, 6, 10, 8, 2, 5]
assert len(LENGTHS) == 15 and min(LENGTHS) == 2 and max(LENGTHS) == 11
SLOTS = 4
LEAD = 3  # (frames before the first utterance that belong to none)


def flat_corpus():
    """(frames, frame_offsets): frame g of the flat array carries g; three frames of no utterance lead."""
    fo = LEAD + np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    frames = np.zeros(int(fo[-1]) + 2, dtype=FRAME_DTYPE)
    frames["velum_opening_cm2"] = np.arange(len(frames))
    frames.setflags(write=False)
    return frames, fo


def code(seed, g, j):
    """The stand-in's sample j of the transition into frame g of the corpus by a voice seeded `seed`."""
    return (seed * 1000 + g) * 10 + j


class StandIn:
    """What stream_corpus needs of a session -- batch, restart, synthesize_frames -- with the indexed packed
    pool call's semantics (an unlatched voice latches its first frame; count 0 is idle and neither its start
    nor its offset is looked at) and a log of calls."""

    def __init__(self, batch):
        self.batch = batch
        self.seed = [None] * batch
        self.latch = [None] * batch  # the corpus index of the latched frame, None: unlatched
        self.calls = []              # ("restart", voices, seeds) | ("step", counts, starts)
        self.frames_seen = []

    def restart(self, voices, seeds=None):
        voices = [int(v) for v in voices]
        assert len(set(voices)) == len(voices) and len(seeds) == len(voices)
        for v, s in zip(voices, seeds):
            self.seed[v], self.latch[v] = int(s), None
        self.calls.append(("restart", voices, [int(s) for s in seeds]))

    def synthesize_frames(self, frames, num_frames, hop, out=None, pcm=False, f32=False, packed=False, offsets=None,
                          frame_start=None, report=False):
        assert packed and report and (pcm or f32) and out is not None and out.ndim == 1
        assert len(num_frames) == len(frame_start) == len(offsets) == self.batch
        self.frames_seen.append(frames)
        produced = np.zeros(self.batch, dtype=np.int32)
        for u, c in enumerate(num_frames):
            n = 0
            for g in range(int(frame_start[u]), int(frame_start[u]) + int(c)):
                assert int(frames[g]["velum_opening_cm2"]) == g
                if self.latch[u] is not None:
                    assert self.latch[u] == g - 1, "a frame out of order"
                    at = int(offsets[u]) + n
                    assert (out[at:at + hop] == -1).all(), "a sample written twice"
                    out[at:at + hop] = [code(self.seed[u], g, j) for j in range(hop)]
                    n += hop
                self.latch[u] = g
            produced[u] = n
        t = sum(1 for c in self.calls if c[0] == "step")
        self.calls.append(("step", [int(c) for c in num_frames], [int(x) for x in frame_start]))
        # (the flag of voice u in step t: the parity of u + t, so that a flag tells its voice and its step)
        return out, np.asarray(offsets), produced, {"nonfinite": np.array([(u + t) % 2 for u in range(self.batch)], dtype=np.uint8)}


def minimum_steps(lengths, slots, chunk):
    """Utterances in order, each to the voice that is free first, ceil(F / chunk) steps each, a voice that
    ends in step t starting its next utterance in step t + 1: the steps until the last one ends."""
    free = [0] * slots
    heapq.heapify(free)
    end = 0
    for F in lengths:
        t = heapq.heappop(free) + -(-F // chunk)
        end = max(end, t)
        heapq.heappush(free, t)
    return end


@pytest.mark.parametrize("chunk", [3, 1, 50])
@pytest.mark.parametrize("seeds", [None, "own"])
def test_stream_corpus_places_every_sample(chunk, seeds):
    frames, fo = flat_corpus()
    n = len(LENGTHS)
    seed_of = [i + 1 for i in range(n)] if seeds is None else [500 + 3 * i for i in range(n)]
    s = StandIn(SLOTS)
    total = sum(F - 1 for F in LENGTHS) * HOP
    buf = np.full(total, -1, dtype=np.float32)  # (float32 holds the stand-in's codes exactly: below 2^24)
    assert code(max(seed_of), len(frames), HOP) < 2 ** 24
    flat, offsets, nonfinite = stream_corpus(s, frames, fo, HOP, chunk, seeds=None if seeds is None else seed_of,
                                             pcm=False, f32=True, out=buf)
    assert flat is buf
    assert offsets.dtype == np.int64 and np.array_equal(offsets, ragged_offsets(LENGTHS, HOP))
    want = np.concatenate([[code(seed_of[i], int(fo[i]) + k, j) for k in range(1, F) for j in range(HOP)]
                           for i, F in enumerate(LENGTHS)]).astype(np.float32)
    assert np.array_equal(flat, want)
    # no step passes a frame array other than the corpus itself
    assert s.frames_seen and all(f is frames for f in s.frames_seen)
    steps = [c for c in s.calls if c[0] == "step"]
    assert all(max(c[1]) <= chunk for c in steps)
    assert len(steps) == minimum_steps(LENGTHS, SLOTS, chunk)
    # every utterance restarted once, in corpus order, with its seed; the voices refill: more restarts than slots
    assert [x for c in s.calls if c[0] == "restart" for x in c[2]] == seed_of
    assert sum(len(c[1]) for c in s.calls if c[0] == "restart") == n > SLOTS
    # no voice idles while an utterance is left to hand out
    handed = 0
    for c in s.calls:
        if c[0] == "restart":
            handed += len(c[1])
        elif 0 in c[1]:
            assert handed == n
    # an utterance's flag is its voice's at the step it ended: the stand-in flags voice u in step t with
    # the parity of u + t, and the log says which voice was given an utterance's last frame in which step
    ends = {int(fo[i + 1]): i for i in range(n)}
    flag = np.full(n, 255, dtype=np.uint8)
    for t, (_, counts, starts) in enumerate(steps):
        for u, (c, at) in enumerate(zip(counts, starts)):
            if c and at + c in ends:
                flag[ends[at + c]] = (u + t) % 2
    assert nonfinite.dtype == np.uint8 and np.array_equal(nonfinite, flag) and set(flag) == {0, 1}


def test_stream_corpus_own_buffer_and_pcm():
    frames, fo = flat_corpus()
    s = StandIn(2)
    hop = 2
    # int16 holds a code below 32768: seeds 1 and 2, frames below 100 -- two utterances
    flat, offsets, _ = stream_corpus(s, frames, fo[:3], hop, 2, seeds=[1, 2], pcm=True,
                                     out=np.full((LENGTHS[0] - 1 + LENGTHS[1] - 1) * hop, -1, dtype=np.int16))
    assert flat.dtype == np.int16 and list(offsets) == [0, (LENGTHS[0] - 1) * hop, (LENGTHS[0] + LENGTHS[1] - 2) * hop]
    want = [code(i + 1, int(fo[i]) + k, j) for i in range(2) for k in range(1, LENGTHS[i]) for j in range(hop)]
    assert list(flat) == want


def test_stream_corpus_refuses_bad_input():
    frames, fo = flat_corpus()
    s = StandIn(2)
    with pytest.raises(ValueError, match="at least 2"):
        stream_corpus(s, frames, [0, 3, 4], HOP, 3)
    with pytest.raises(ValueError):
        stream_corpus(s, frames, fo, HOP, 0)
    with pytest.raises(ValueError):
        stream_corpus(s, frames, fo, 0, 3)
    with pytest.raises(ValueError, match="one seed"):
        stream_corpus(s, frames, fo, HOP, 3, seeds=[1, 2])
    with pytest.raises(ValueError):
        stream_corpus(s, frames, fo, HOP, 3, pcm=True, f32=True)
    assert s.calls == []
