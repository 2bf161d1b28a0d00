"""Indexed voice pools on the GPU (afs_session_synthesize_indexed, afs_session_synthesize_indexed_packed;
Synthesizer.synthesize_frames(frame_start=), Context.synthesize_corpus).

The corpus, seeds and single-call references are those of tests/test_pool_gpu.py: 15 utterances of 2 .. 11
frames that reach a fricative.  Here they lie back to back in one flat array with poisoned frames (every
double NaN) before and after them, and every comparison is on bit patterns: the indexed calls against the
rectangle pool calls on the same schedule, the corpus stream against the one-shot ragged call and against
each utterance alone, a corpus with canaries against one without."""
import ctypes

import numpy as np
import pytest

from areafunctionsynthesis_amd import _native
from areafunctionsynthesis_amd.frames import FRAME_DTYPE
from areafunctionsynthesis_amd.synthesizer import ragged_offsets
from test_pool_gpu import (CANARY, CANARY16, CHUNK, MIX, NF, SEEDS, bits, canaries, corpus,  # noqa: F401
                           make_ctx, monkeypatch_module, piece, poisoned, references, session)

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)
WILD = [I64.max, -1, I64.min, 10 ** 15]  # (frame starts of idle voices: never looked at)
CANARY32 = np.uint32(0x7FC0BEEF)  # (a float32 NaN no kernel computes)
LEAD, TAIL = 2, 3
FRAME = FRAME_DTYPE.itemsize


def poison_frame():
    p = np.zeros((), dtype=FRAME_DTYPE)
    for name in FRAME_DTYPE.names:
        if FRAME_DTYPE[name].base.kind == "f":
            p[name] = np.nan
    return p


def flat_corpus(oracle, lead=LEAD, tail=TAIL):
    """(flat, frame_offsets): the 15 utterances back to back, `lead` poisoned frames before and `tail` after."""
    fo = lead + np.concatenate([[0], np.cumsum(NF)]).astype(np.int64)
    flat = np.empty(int(fo[-1]) + tail, dtype=FRAME_DTYPE)
    flat[...] = poison_frame()
    for i, fr in enumerate(corpus(oracle)):
        flat[fo[i]:fo[i + 1]] = fr
    return flat, fo


def to_device(flat, shift=0):
    """The frames' bytes in GPU memory: a uint8 tensor, `shift` bytes into a larger allocation."""
    import torch
    raw = np.frombuffer(flat.tobytes(), dtype=np.uint8)
    buf = torch.zeros(raw.size + 16, dtype=torch.uint8, device="cuda")
    view = buf[shift:shift + raw.size]
    view.copy_(torch.from_numpy(raw.copy()))
    assert view.data_ptr() % 16 == shift
    return view


def schedule(ids, chunk=CHUNK):
    """[(first frame of the step within each utterance, counts[B])]: every voice its next `chunk` frames."""
    return [(start, np.clip(NF[ids] - start, 0, chunk).astype(np.int32)) for start in range(0, int(NF[ids].max()), chunk)]


def starts_of(fo, ids, start, counts):
    return np.array([int(fo[i]) + start if c else WILD[q % len(WILD)] for q, (i, c) in enumerate(zip(ids, counts))],
                    dtype=np.int64)


# ---- 1. indexed equals rectangle --------------------------------------------------------------------

CONFIGS = {"pair16-hop33": (16, 11, 33, None), "pair16-hop5": (16, 11, 5, None), "pair64-hop33": (64, 3, 33, None),
           "pair64-hop5": (64, 3, 5, None), "pair16-launch50": (16, 11, 33, {"AFS_LAUNCH_SAMPLES": "50"})}
IDS = {11: list(range(11)), 3: [0, 3, 8]}  # (3 voices: utterances of 7, 11 and 6 frames)


@pytest.mark.parametrize("place", ["device", "host"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_indexed_equals_rectangle(make_ctx, session, oracle, config, place):
    """The same schedule -- chunks of 3, voices that end turning idle with wild starts -- through the
    rectangle pool calls on one session and the indexed calls on another: rows, the eight tap rows,
    produced, non-finite flags, rand() counts and latch flags agree after every step, as fp64, int16 and
    float32 (the packed forms at offsets in reverse voice order with gaps); the fp64 rows are those of
    afs_synthesize on each utterance alone."""
    lanes, B, hop, env = CONFIGS[config]
    ids = IDS[B]
    ctx = make_ctx(lanes, env)
    flat, fo = flat_corpus(oracle)
    src = to_device(flat) if place == "device" else flat
    refs = references(make_ctx, oracle, lanes, hop)
    pitch = CHUNK * hop + 7
    off = ((B - 1 - np.arange(B)) * pitch + 3).astype(np.int64)
    ctx.set_taps(MIX)
    try:
        for form in ("fp64", "i16", "f32"):
            a, b = session(B, lanes, SEEDS[ids], env), session(B, lanes, SEEDS[ids], env)
            got = [[] for _ in range(B)]
            for start, counts in schedule(ids):
                rows = [piece(oracle, i, start) for i in ids]
                starts = starts_of(fo, ids, start, counts)
                was = a.latched.copy()
                if form == "fp64":
                    width = CHUNK * hop + 5
                    oa, ob = canaries((B, width)), canaries((B, width))
                    ta, tb = canaries((B, len(MIX), width)), canaries((B, len(MIX), width))
                    ra = a.synthesize_frames(poisoned(rows, CHUNK), counts, hop, out=oa, taps=True, taps_out=ta, report=True)
                    rb = b.synthesize_frames(src, counts, hop, out=ob, taps=True, taps_out=tb, report=True,
                                             frame_start=starts)
                    assert np.array_equal(bits(oa), bits(ob)), f"step {start}: rows"
                    assert np.array_equal(bits(ta), bits(tb)), f"step {start}: tap rows"
                    pa, pb = ra[1], rb[1]
                    for q in range(B):
                        got[q].append(ob[q, :pb[q]].copy())
                else:
                    kw = dict(pcm=form == "i16", f32=form == "f32", packed=True, offsets=off, report=True)
                    if form == "i16":
                        fa, fb = (np.full(B * pitch + 3, CANARY16, dtype=np.int16) for _ in range(2))
                    else:
                        fa, fb = (np.full(B * pitch + 3, CANARY32, dtype=np.uint32).view(np.float32) for _ in range(2))
                    ra = a.synthesize_frames(poisoned(rows, CHUNK), counts, hop, out=fa, **kw)
                    rb = b.synthesize_frames(src, counts, hop, out=fb, frame_start=starts, **kw)
                    assert rb[0] is fb
                    assert np.array_equal(fa.view(np.uint8), fb.view(np.uint8)), f"step {start}: {form} samples"
                    pa, pb = ra[2], rb[2]
                want = np.where(counts > 0, counts - 1 + was, 0) * hop
                assert np.array_equal(pa, want) and np.array_equal(pb, want), f"step {start}: produced"
                assert np.array_equal(ra[-1]["nonfinite"], rb[-1]["nonfinite"]) and not rb[-1]["nonfinite"].any()
                assert ra[-1]["samples"] == rb[-1]["samples"] == int(want.sum())
                assert np.array_equal(a.rng_draws(), b.rng_draws()), f"step {start}: rand() counts"
                assert np.array_equal(a.latched, b.latched) and np.array_equal(b.latched, np.where(counts > 0, 1, was))
            # (hop 5: 50 samples at most, and no noise source has fired by then; at hop 33 they do)
            assert (b.rng_draws() > 0).any() == (hop == 33)
            for q, i in enumerate(ids):
                assert b.rng_draws()[q] == refs[i][1], f"voice {q}: rand() count"
                if form == "fp64":
                    assert np.array_equal(bits(np.concatenate(got[q])), bits(refs[i][0])), f"voice {q}, utterance {i}"
    finally:
        ctx.set_taps([])


# ---- 2. the corpus stream against the single calls --------------------------------------------------

@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("lanes,hop", [(16, 33), (16, 5), (64, 33)])
def test_corpus_equals_single_calls(make_ctx, oracle, lanes, hop, f32):
    """Context.synthesize_corpus, 4 slots and chunks of 3 over the device corpus -- the voices refill three
    times over -- against synthesize_ragged(packed=True) of the padded corpus and against every utterance
    alone, on the same context."""
    ctx = make_ctx(lanes)
    flat, fo = flat_corpus(oracle)
    kw = dict(pcm=not f32, f32=f32)
    got, offsets, nonfinite = ctx.synthesize_corpus(to_device(flat), fo, hop, 4, CHUNK, seeds=SEEDS, **kw)
    assert isinstance(got, np.ndarray) and got.dtype == (np.float32 if f32 else np.int16)
    assert np.array_equal(offsets, ragged_offsets(NF, hop)) and got.shape == (int(offsets[-1]),)
    assert not nonfinite.any() and nonfinite.shape == (len(NF),)
    want, woff = ctx.synthesize_ragged(poisoned(corpus(oracle)), NF, hop, seeds=SEEDS, packed=True, **kw)
    assert np.array_equal(woff, offsets)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    for i, fr in enumerate(corpus(oracle)):
        one = ctx.synthesize(np.ascontiguousarray(fr[None]), hop, seeds=SEEDS[i:i + 1], **kw)
        assert np.array_equal(got[offsets[i]:offsets[i + 1]].view(np.uint8), np.ascontiguousarray(one[0]).view(np.uint8)), i
    assert np.abs(got.astype(np.float64)).max() > 0


def test_corpus_from_host_into_own_device_buffer(make_ctx, oracle):
    """A host corpus (the live spans staged per step) into the caller's GPU tensor: the same samples, and
    nothing written past them."""
    import torch
    ctx, hop = make_ctx(16), 33
    flat, fo = flat_corpus(oracle)
    total = int(ragged_offsets(NF, hop)[-1])
    buf = torch.full((total + 9,), int(CANARY16), dtype=torch.int16, device="cuda")
    got, offsets, _ = ctx.synthesize_corpus(flat, fo, hop, 4, CHUNK, seeds=SEEDS, pcm=True, out=buf)
    assert got is buf
    want, _ = ctx.synthesize_ragged(poisoned(corpus(oracle)), NF, hop, seeds=SEEDS, packed=True, pcm=True)
    host = buf.cpu().numpy()
    assert np.array_equal(host[:total], want) and (host[total:] == CANARY16).all()


# ---- 3. in place ------------------------------------------------------------------------------------

def test_canary_frames_around_the_corpus(make_ctx, oracle):
    """Poisoned frames before and after the device corpus: the audio is that of a corpus without them, and
    no byte of the corpus -- canaries included -- has changed."""
    ctx, hop = make_ctx(16), 33
    flat, fo = flat_corpus(oracle, lead=4, tail=4)
    dev = to_device(flat)
    got, _, _ = ctx.synthesize_corpus(dev, fo, hop, 4, CHUNK, seeds=SEEDS, pcm=True)
    bare, fo0 = flat_corpus(oracle, lead=0, tail=0)
    want, _, _ = ctx.synthesize_corpus(to_device(bare), fo0, hop, 4, CHUNK, seeds=SEEDS, pcm=True)
    assert np.array_equal(got, want) and np.abs(got.astype(np.int32)).max() > 0
    assert dev.cpu().numpy().tobytes() == flat.tobytes()


def test_frames_outside_the_live_spans_are_not_read(make_ctx, session, oracle):
    """One step of 11 voices, frames 3-5 of their utterances after frames 0-2: with every frame of the
    corpus that lies in no live span of the step poisoned -- inside the utterances as well as around them
    -- the step's audio and tap rows are the same bits."""
    hop, B = 33, 11
    ids = list(range(B))
    ctx = make_ctx(16)
    flat, fo = flat_corpus(oracle)
    steps = schedule(ids)
    (s0, c0), (s1, c1) = steps[0], steps[1]
    holed = flat.copy()
    live = np.zeros(len(flat), dtype=bool)
    for i, c in zip(ids, c1):
        live[fo[i] + s1:fo[i] + s1 + c] = True
    holed[~live] = poison_frame()
    assert (~live[fo[0]:fo[B]]).sum() >= 3 * B  # (the frames just played, and those still to come)
    ctx.set_taps(MIX)
    try:
        outs = []
        for second in (flat, holed):
            s = session(B, 16, SEEDS[ids])
            s.synthesize_frames(to_device(flat), c0, hop, frame_start=starts_of(fo, ids, s0, c0))
            out, tout = canaries((B, CHUNK * hop)), canaries((B, len(MIX), CHUNK * hop))
            res = s.synthesize_frames(to_device(second), c1, hop, out=out, taps=True, taps_out=tout,
                                      frame_start=starts_of(fo, ids, s1, c1))
            assert np.array_equal(res[1], c1 * hop)
            outs.append((out, tout))
        assert np.array_equal(bits(outs[0][0]), bits(outs[1][0])) and np.array_equal(bits(outs[0][1]), bits(outs[1][1]))
        assert not np.isnan(outs[1][0][c1 > 0, :hop]).any()
    finally:
        ctx.set_taps([])


def test_memory_does_not_follow_the_corpus(oracle):
    """11 voices x 3 frames from a device corpus of 10 000 frames hold no more device memory in the context
    than the same step from a corpus of those 33 frames alone (two fresh contexts: buffers only grow)."""
    from areafunctionsynthesis_amd.synthesizer import Context, Synthesizer
    from taps_lib import FS
    hop, B = 33, 11
    rows = [piece(oracle, u, 0) for u in range(B)]
    assert all(len(r) == CHUNK for r in rows if len(r) > 2) and sum(len(r) for r in rows) <= 33
    counts = np.array([len(r) for r in rows], dtype=np.int32)
    small = np.concatenate(rows + [np.repeat(poison_frame()[None], 33 - int(counts.sum()))]).astype(FRAME_DTYPE)
    small_starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    big = np.empty(10000, dtype=FRAME_DTYPE)
    big[...] = poison_frame()
    big_starts = (np.arange(B, dtype=np.int64) * 907 + 11)  # (spread over the corpus, the last span ends at 9084)
    for u, r in enumerate(rows):
        big[big_starts[u]:big_starts[u] + len(r)] = r
    held, audio = [], []
    for frames, starts in ((small, small_starts), (big, big_starts)):
        ctx = Context(FS, lanes=16)
        try:
            s = Synthesizer(ctx, B, SEEDS[:B])
            out, _ = s.synthesize_frames(to_device(frames), counts, hop, frame_start=starts)
            held.append(ctx.memory_info()["total_bytes"])
            audio.append(out)
            s.close()
        finally:
            ctx.close()
    print(f"total_bytes: corpus of 33 frames {held[0]}, of 10 000 frames {held[1]}")
    assert np.array_equal(bits(audio[0]), bits(audio[1]))
    assert held[1] <= held[0]


# ---- 4. shared spans --------------------------------------------------------------------------------

def test_shared_spans(make_ctx, session, oracle):
    """Voices 0 and 1 read utterance 3 from the same frames under the same seed, voice 2 the same frames
    under another, voice 3 a stretch from its third frame on under a third: 0 and 1 agree bit for bit, and
    each voice is afs_synthesize of its frames with its seed."""
    hop, lanes = 33, 16
    ctx = make_ctx(lanes)
    flat, fo = flat_corpus(oracle)
    dev = to_device(flat)
    base = np.array([fo[3], fo[3], fo[3], fo[3] + 2], dtype=np.int64)
    length = np.array([NF[3], NF[3], NF[3], NF[3] - 4], dtype=np.int64)  # (frames 2 .. 8 of the 11)
    seeds = np.array([SEEDS[3], SEEDS[3], 555, 777], dtype=np.uint32)
    s = session(4, lanes, seeds)
    got = [[] for _ in range(4)]
    for start in range(0, int(length.max()), CHUNK):
        counts = np.clip(length - start, 0, CHUNK).astype(np.int32)
        out, produced = s.synthesize_frames(dev, counts, hop, frame_start=np.where(counts > 0, base + start, -1))
        for q in range(4):
            got[q].append(out[q, :produced[q]].copy())
    got = [np.concatenate(g) for g in got]
    assert np.array_equal(bits(got[0]), bits(got[1]))
    draws = s.rng_draws()
    print(f"rand() counts {list(draws)}; voices 0 and 2 differ in {int((bits(got[0]) != bits(got[2])).sum())} samples")
    assert draws[0] == draws[1] > 0
    assert not np.array_equal(bits(got[0]), bits(got[2]))  # (another seed: other noise)
    for q in range(4):
        fr = np.ascontiguousarray(flat[base[q]:base[q] + length[q]][None])
        y = ctx.synthesize(fr, hop, seeds=seeds[q:q + 1])
        assert np.array_equal(bits(got[q]), bits(y[0])), f"voice {q}"
        assert draws[q] == ctx.rng_draws(1)[0], f"voice {q}: rand() count"


# ---- 5. alignment -----------------------------------------------------------------------------------

def test_misaligned_device_corpus(make_ctx, oracle):
    """A device corpus 8 bytes off a 16-byte boundary (the fallback: the hull of each step's live spans
    through the staging buffer) gives the audio of an aligned one."""
    ctx, hop = make_ctx(16), 33
    flat, fo = flat_corpus(oracle)
    off8 = to_device(flat, shift=8)
    assert off8.data_ptr() % 16 == 8
    got, _, _ = ctx.synthesize_corpus(off8, fo, hop, 4, CHUNK, seeds=SEEDS, pcm=True)
    want, _, _ = ctx.synthesize_corpus(to_device(flat), fo, hop, 4, CHUNK, seeds=SEEDS, pcm=True)
    assert np.array_equal(got, want) and np.abs(got.astype(np.int32)).max() > 0
    assert off8.cpu().numpy().tobytes() == flat.tobytes()


# ---- 6. idle voices and refusals --------------------------------------------------------------------

def test_idle_voices_and_refusals(make_ctx, session, oracle):
    import torch
    hop, B = 33, 11
    ids = list(range(B))
    flat, fo = flat_corpus(oracle)
    dev = to_device(flat)
    total = len(flat)
    s = session(B, 16, SEEDS[ids])
    (s0, c0), (s1, c1) = schedule(ids)[:2]
    s.synthesize_frames(dev, c0, hop, frame_start=starts_of(fo, ids, s0, c0))
    # idle voices with wild starts beside playing ones: accepted, their rows keep every canary
    idle = [3, 5, 9]
    counts = c1.copy()
    counts[idle] = 0
    starts = starts_of(fo, ids, s1, c1)
    starts[idle] = [I64.max, -10 ** 12, I64.min]
    fork = session(B, 16, SEEDS[ids])
    fork.copy_voices(np.arange(B), np.arange(B), src=s)
    out = canaries((B, CHUNK * hop))
    _, produced = fork.synthesize_frames(dev, counts, hop, out=out, frame_start=starts)
    assert np.array_equal(produced, counts * hop) and not produced[idle].any() and produced.any()
    assert (bits(out[idle]) == CANARY).all()
    for q in range(B):
        assert (bits(out[q, produced[q]:]) == CANARY).all()

    # the refusals: straight to the library, all of s's voices byte for byte what they were
    before = s.save_voices(np.arange(B))
    latched = s.latched.copy()
    vp, lib, h = ctypes.c_void_p, s._lib, s._h
    good_counts, good_starts = c1.copy(), starts_of(fo, ids, s1, c1)
    assert (good_counts > 0).sum() == 7  # (the utterances of 4 frames and more among the first 11)
    width = CHUNK * hop
    outbuf = canaries((B, width))
    pcmbuf = np.full(B * width, CANARY16, dtype=np.int16)
    produced = np.full(B, -7, dtype=np.int32)
    tight = (np.arange(B) * width).astype(np.int64)

    def fp64(frames=dev, total=total, starts=good_starts, counts=good_counts, hop=hop, out=outbuf, stride=width):
        return lib.afs_session_synthesize_indexed(h, vp(frames.data_ptr() if frames is not None else 0), total,
                                                  vp(_ptr(starts)), vp(_ptr(counts)), hop, vp(_ptr(out)), stride, None,
                                                  None, vp(produced.ctypes.data), None)

    def packed(starts=good_starts, counts=good_counts, fmt=_native.AFS_SAMPLE_I16, out=pcmbuf, offsets=tight, total=total):
        return lib.afs_session_synthesize_indexed_packed(h, vp(dev.data_ptr()), total, vp(_ptr(starts)), vp(_ptr(counts)),
                                                         hop, fmt, vp(_ptr(out)), vp(_ptr(offsets)), None,
                                                         vp(produced.ctypes.data), None)

    def changed(at, value, base=good_starts):
        x = base.copy()
        x[at] = value
        return x

    live = int(np.flatnonzero(good_counts > 0)[2])
    refusals = {
        "total_frames < 0": lambda: fp64(total=-1),
        "NULL frame_start": lambda: fp64(starts=None),
        "NULL num_frames": lambda: fp64(counts=None),
        "a start below 0": lambda: fp64(starts=changed(live, -1)),
        "a span past the end": lambda: fp64(starts=changed(live, total - int(good_counts[live]) + 1)),
        "a span past a short total": lambda: fp64(total=int(good_starts[good_counts > 0].max())),
        "a start at INT64_MAX": lambda: fp64(starts=changed(live, I64.max)),
        "a count below 0": lambda: fp64(counts=changed(live, -1, good_counts)),
        "frame_start in device memory": lambda: fp64(starts=torch.from_numpy(good_starts).cuda()),
        "num_frames in device memory": lambda: fp64(counts=torch.from_numpy(good_counts).cuda()),
        "NULL frames": lambda: fp64(frames=None),
        "hop 0": lambda: fp64(hop=0),
        "out_stride below produced": lambda: fp64(stride=width - 1),
        "NULL out": lambda: fp64(out=None),
        "packed: a start below 0": lambda: packed(starts=changed(live, -1)),
        "packed: a span past the end": lambda: packed(starts=changed(live, total - 1)),
        "packed: a count below 0": lambda: packed(counts=changed(live, -1, good_counts)),
        "packed: total_frames < 0": lambda: packed(total=-5),
        "packed: an unknown format": lambda: packed(fmt=7),
        "packed: a negative offset": lambda: packed(offsets=changed(live, -1, tight)),
        "packed: rows that overlap": lambda: packed(offsets=changed(2, 1, tight)),
        "packed: offsets in device memory": lambda: packed(offsets=torch.from_numpy(tight).cuda()),
        "packed: NULL out": lambda: packed(out=None),
        "packed: NULL frame_start": lambda: packed(starts=None),
    }
    assert good_counts[0] > 0 and good_counts[2] > 0  # (rows 0 and 2 both hold samples: they can overlap)
    for what, call in refusals.items():
        assert call() == 1, what
        assert (bits(outbuf) == CANARY).all() and (pcmbuf == CANARY16).all() and (produced == -7).all(), what
        assert np.array_equal(s.latched, latched), what
        assert s.save_voices(np.arange(B)).tobytes() == before.tobytes(), what
    # the same arguments unchanged are accepted, and the session played on from where it was
    assert fp64() == 0 and np.array_equal(produced, good_counts * hop)
    refs = references(make_ctx, oracle, 16, hop)
    for q, i in enumerate(ids):
        n = int(produced[q])
        assert np.array_equal(bits(outbuf[q, :n]), bits(refs[i][0][2 * hop:2 * hop + n])), f"voice {q}"
    # the one-lane solvers have no pool
    chol = session(B, solver="cholesky")
    assert lib.afs_session_synthesize_indexed(chol._h, vp(dev.data_ptr()), total, vp(_ptr(good_starts)),
                                              vp(_ptr(good_counts)), hop, vp(_ptr(outbuf)), width, None, None, None, None) == 5


def _ptr(x):
    if x is None:
        return 0
    return int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x.ctypes.data)


# ---- 7. alternation ---------------------------------------------------------------------------------

def test_alternation_with_the_other_session_calls(make_ctx, session, oracle):
    """The utterances of 7 frames and more: frames 0-2 through an indexed call, 3-4 through a rectangle pool
    call, frame 5 through the lock-step synthesize_signal_tds, the rest through an indexed call again --
    the uninterrupted utterance, bit for bit."""
    hop = 33
    ids = [u for u in range(len(NF)) if NF[u] >= 7]
    B = len(ids)
    assert B == 5
    refs = references(make_ctx, oracle, 16, hop)
    flat, fo = flat_corpus(oracle)
    dev = to_device(flat)
    s = session(B, 16, SEEDS[ids])
    parts = [[] for _ in range(B)]

    def keep(out, produced):
        for q in range(B):
            parts[q].append(np.array(out[q, :produced[q]]))

    three = np.full(B, 3, dtype=np.int32)
    keep(*s.synthesize_frames(dev, three, hop, frame_start=fo[ids]))
    keep(*s.synthesize_frames(poisoned([piece(oracle, i, 3, 2) for i in ids]), np.full(B, 2, dtype=np.int32), hop))
    y = s.synthesize_signal_tds(np.array([corpus(oracle)[i][5] for i in ids], dtype=FRAME_DTYPE), hop)
    keep(y, np.full(B, hop))
    rest = (NF[ids] - 6).astype(np.int32)
    keep(*s.synthesize_frames(dev, rest, hop, frame_start=fo[ids] + 6))
    for q, i in enumerate(ids):
        assert np.array_equal(bits(np.concatenate(parts[q])), bits(refs[i][0])), f"voice {q}, utterance {i}"
        assert s.rng_draws()[q] == refs[i][1]
