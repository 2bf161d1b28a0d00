"""Session voice pools on the GPU (afs_session_restart_voices, afs_session_synthesize_ragged and its PCM
twin, afs_session_latched; Synthesizer.restart / latched / synthesize_frames, Context.synthesize_stream).

The corpus: 15 utterances of 2 .. 11 frames (a: -> s glides with a velum of their own, so the noise
sources fire), seeds 101 + 7u.  The yardstick is each utterance alone through Context.synthesize on a
context of the same lane width, computed once per (lanes, hop) and left unchanged: whatever way an
utterance is cut into pool calls, whichever voice plays it, beside whatever idle, restarted or finished
voices, its audio, tap rows, rand() count and non-finite flag are those bits.  Frames past each count are
poisoned (every double NaN) and every output is filled with a canary no kernel computes: nothing outside
a voice's frames is read, nothing outside the samples it produces is written."""
import ctypes

import numpy as np
import pytest

from areafunctionsynthesis_amd import _native
from areafunctionsynthesis_amd.frames import FRAME_DTYPE
from taps_lib import CURRENT, FS, PRESSURE, glide_frames

pytestmark = pytest.mark.gpu

NF = np.array([7, 2, 5, 11, 3, 9, 2, 4, 6, 5, 3, 11, 2, 7, 4], dtype=np.int32)
assert sorted(set(NF)) == [2, 3, 4, 5, 6, 7, 9, 11]
SEEDS = (101 + 7 * np.arange(len(NF))).astype(np.uint32)
ONE_WAVE_B = 1025  # (64 lanes: batches above TREE_PAIR64_MAX = 1024 run one wave per utterance)
MIX = [(CURRENT, 24), (PRESSURE, 25), (PRESSURE, 22), (CURRENT, 93), (CURRENT, 96), (PRESSURE, 83), (PRESSURE, 60),
       (CURRENT, 65)]  # (the eight taps of tests/test_taps_gpu.py)
CANARY = np.uint64(0x7FF8C0DECAFE0123)  # (a NaN no kernel computes)
CANARY16 = np.int16(0x5A5B)
GOLD_TOL = 1e-9  # (tests/test_gpu_parity.py: golden / oracle, first samples)
CHUNK = 3

_CACHE = {}


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.fixture(scope="module")
def make_ctx(monkeypatch_module):
    from areafunctionsynthesis_amd.synthesizer import Context
    made = {}

    def make(lanes=16, env=None, solver="tree"):
        key = (lanes, tuple(sorted((env or {}).items())), solver)
        if key not in made:
            for k, v in (env or {}).items():
                monkeypatch_module.setenv(k, v)
            try:
                made[key] = Context(FS, solver=solver, lanes=lanes if solver == "tree" else None)
            finally:
                for k in env or {}:
                    monkeypatch_module.delenv(k)
        return made[key]

    yield make
    for c in made.values():
        c.close()


@pytest.fixture
def session(make_ctx):
    """make(batch, lanes=16, seeds=None, env=None) -> a Synthesizer, closed after the test."""
    from areafunctionsynthesis_amd.synthesizer import Synthesizer
    made = []

    def make(batch, lanes=16, seeds=None, env=None, solver="tree"):
        made.append(Synthesizer(make_ctx(lanes, env, solver), batch, seeds))
        return made[-1]

    yield make
    for s in made:
        s.close()


def corpus(oracle):
    """The 15 utterances' frames (read-only)."""
    if "corpus" not in _CACHE:
        utts = [glide_frames(oracle, int(F), 0.3 + 0.03 * u) for u, F in enumerate(NF)]
        for f in utts:
            f.setflags(write=False)
        _CACHE["corpus"] = utts
    return _CACHE["corpus"]


def references(make_ctx, oracle, lanes, hop, taps=None):
    """Utterance u alone through afs_synthesize (afs_synthesize_taps) on a context of the same lane
    width: [(audio[T_u], draws, nonfinite flag, taps[n, T_u] or None)] x 15."""
    key = ("ref", lanes, hop, None if taps is None else tuple(taps))
    if key not in _CACHE:
        ctx = make_ctx(lanes)
        refs = []
        for u, fr in enumerate(corpus(oracle)):
            fr = np.ascontiguousarray(fr[None])
            if taps is None:
                y, rep = ctx.synthesize(fr, hop, seeds=SEEDS[u:u + 1], report=True)
                rows = None
            else:
                ctx.set_taps(taps)
                try:
                    y, rows, rep = ctx.synthesize(fr, hop, seeds=SEEDS[u:u + 1], report=True, taps=True)
                finally:
                    ctx.set_taps([])
                rows = rows[0]
                rows.setflags(write=False)
            y[0].setflags(write=False)
            refs.append((y[0], int(ctx.rng_draws(1)[0]), int(rep["nonfinite"][0]), rows))
        _CACHE[key] = refs
    return _CACHE[key]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def canaries(shape):
    return np.full(shape, CANARY, dtype=np.uint64).view(np.float64)


def poisoned(rows, fstride=None):
    """frames[B, fstride] holding row u's frames first, poison (every double NaN, every byte 0) after."""
    poison = np.zeros((), dtype=FRAME_DTYPE)
    for name in FRAME_DTYPE.names:
        if FRAME_DTYPE[name].base.kind == "f":
            poison[name] = np.nan
    fstride = fstride or max([len(r) for r in rows] + [1])
    frames = np.empty((len(rows), fstride), dtype=FRAME_DTYPE)
    frames[...] = poison
    for u, r in enumerate(rows):
        frames[u, :len(r)] = r
    return frames


def pool_call(s, rows, hop, taps=False, pcm=False, device=False, extra=5):
    """One synthesize_frames call of per-voice frame arrays (empty: idle) into canary-filled outputs
    `extra` samples wider than the most any voice can produce: (out, produced, taps or None, report);
    every produced count, the flags and the canaries past each row's samples are checked here."""
    B = s.batch
    counts = np.array([len(r) for r in rows], dtype=np.int32)
    was = s.latched.copy()
    width = int(counts.max()) * hop + extra
    out = np.full((B, width), CANARY16, dtype=np.int16) if pcm else canaries((B, width))
    tout = canaries((B, s.ctx.n_taps, width)) if taps else None
    if device:
        import torch
        out = torch.from_numpy(out).cuda()
        tout = torch.from_numpy(tout).cuda() if taps else None
    res = s.synthesize_frames(poisoned(rows), counts, hop, out=out, taps=taps, taps_out=tout, pcm=pcm, report=True)
    produced, rep = res[1], res[-1]
    if device:
        out = out.cpu().numpy()
        tout = tout.cpu().numpy() if taps else None
    want = np.where(counts > 0, counts - 1 + was, 0) * hop
    assert np.array_equal(produced, want)
    assert np.array_equal(s.latched, np.where(counts > 0, 1, was))
    assert rep["samples"] == int(want.sum()) and rep["nonfinite_utterances"] == 0 and not rep["nonfinite"].any()
    for u in range(B):
        if pcm:
            assert (out[u, want[u]:] == CANARY16).all(), f"voice {u}: written past its samples"
        else:
            assert (bits(out[u, want[u]:]) == CANARY).all(), f"voice {u}: written past its samples"
        if taps:
            assert (bits(tout[u, :, want[u]:]) == CANARY).all(), f"voice {u}: taps written past its samples"
    return out, produced, tout, rep


def piece(oracle, u, start, n=CHUNK):
    """Frames start .. start + n - 1 of utterance u (fewer, or none, at and past its end)."""
    return corpus(oracle)[u][start:start + n]


# ---- 1. stream equals trajectories --------------------------------------------------------------------

KERNELS = {"pair16": (16, 11, "tree_pair_kernel"), "pair64": (64, 3, "tree_pair64_kernel"),
           "one_wave64": (64, ONE_WAVE_B, "tree_synth_kernel")}


def stream_equals_trajectories(make_ctx, oracle, kernel, hop, env=None):
    lanes, slots, name = KERNELS[kernel]
    ctx = make_ctx(lanes, env)
    assert ctx.synthesis_kernel(slots) == name
    refs = references(make_ctx, oracle, lanes, hop)
    utts, ids, seeds = list(corpus(oracle)), list(range(len(NF))), list(SEEDS)
    if kernel == "one_wave64":  # 15 voices play the corpus, 200 the 2-frame utterance 1, 810 stay idle
        utts, ids, seeds = utts + [utts[1]] * 200, ids + [1] * 200, seeds + [SEEDS[1]] * 200
    ended = {}

    def finished(i, slot, sess, nonfinite):
        ended[i] = (int(sess.rng_draws()[slot]), nonfinite)

    got = dict(ctx.synthesize_stream(iter(utts), hop, slots, CHUNK, seeds=seeds, pcm=False, finished=finished))
    assert sorted(got) == list(range(len(utts)))
    for i, u in enumerate(ids):
        y, draws, nf, _ = refs[u]
        assert np.array_equal(bits(got[i]), bits(y)), f"utterance {i}"
        assert ended[i] == (draws, nf) and nf == 0, f"utterance {i}: rand() count, non-finite flag"
    # (hop 5: 50 samples at most, and no noise source has fired by then -- the references count no
    # rand() call either; at hop 33 they do)
    assert any(refs[u][1] > 0 for u in ids) == (hop == 33)


@pytest.mark.parametrize("hop", [33, 5])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_stream_equals_trajectories(make_ctx, oracle, kernel, hop):
    """hop 33: hop records, launches of odd length (the pairs' X_RELX2 copy); hop 5, below
    AFS_PLAN_HOP_MIN: the dense plan.  11 slots at 16 lanes are more than one block of 8: length groups
    with padding slots and stand-ins."""
    assert 5 < _native.AFS_PLAN_HOP_MIN <= 33
    stream_equals_trajectories(make_ctx, oracle, kernel, hop)


# ---- 2. launch splits ---------------------------------------------------------------------------------

@pytest.mark.parametrize("per", [50, 66])
def test_launch_splits(make_ctx, oracle, per):
    """Launches of 50 and 66 samples at hop 33 (a step's blocks end at 33, 66 or 99): blocks end inside
    a launch, at a launch boundary and before a launch starts.  The same bits."""
    stream_equals_trajectories(make_ctx, oracle, "pair16", 33, env={"AFS_LAUNCH_SAMPLES": str(per)})


# ---- 3. idle voices -----------------------------------------------------------------------------------

IDLE = (3, 7, 9)  # (11, 4 and 5 frames: all three have frames left after the first three)


@pytest.mark.parametrize("form", ["fp64+taps", "pcm"])
def test_idle_voices_untouched(make_ctx, session, oracle, form):
    """11 voices play utterances 0 .. 10.  Run A: frames 0-2, then 3-5.  Run B: frames 0-2, then 3-5 with
    voices 3, 7, 9 idle, then 3-5 for those three alone.  The idle voices' rows keep every canary, they
    produce 0, their latch flags stay, and what they play later is run A's, bit for bit."""
    hop, B = 33, 11
    taps, pcm = form != "pcm", form == "pcm"
    ctx = make_ctx(16)
    ctx.set_taps(MIX if taps else [])
    try:
        a, b = session(B, seeds=SEEDS[:B]), session(B, seeds=SEEDS[:B])
        kw = dict(taps=taps, pcm=pcm, device=pcm)
        a1 = pool_call(a, [piece(oracle, u, 0) for u in range(B)], hop, **kw)
        a2 = pool_call(a, [piece(oracle, u, 3) for u in range(B)], hop, **kw)
        b1 = pool_call(b, [piece(oracle, u, 0) for u in range(B)], hop, **kw)
        assert np.array_equal(a1[0], b1[0]) if pcm else np.array_equal(bits(a1[0]), bits(b1[0]))
        b2 = pool_call(b, [piece(oracle, u, 3 if u not in IDLE else 99) for u in range(B)], hop, **kw)
        b3 = pool_call(b, [piece(oracle, u, 3 if u in IDLE else 99) for u in range(B)], hop, **kw)
        assert list(b2[1][list(IDLE)]) == [0, 0, 0]  # (pool_call checked the canaries of those rows, taps too)
        for u in range(B):
            late = b3 if u in IDLE else b2
            n = int(a2[1][u])
            assert late[1][u] == n
            if pcm:
                assert np.array_equal(late[0][u, :n], a2[0][u, :n]), f"voice {u}"
            else:
                assert np.array_equal(bits(late[0][u, :n]), bits(a2[0][u, :n])), f"voice {u}"
                assert np.array_equal(bits(late[2][u, :, :n]), bits(a2[2][u, :, :n])), f"voice {u}: taps"
        assert np.array_equal(a.rng_draws(), b.rng_draws()) and (a.rng_draws() > 0).any()
        # every voice idle: nothing is written, nothing produced, no flag moves
        before = b.latched.copy()
        out, produced, _, rep = pool_call(b, [piece(oracle, u, 99) for u in range(B)], hop, **kw)
        assert not produced.any() and rep["samples"] == 0 and np.array_equal(b.latched, before)
        assert np.array_equal(a.rng_draws(), b.rng_draws())
    finally:
        ctx.set_taps([])


# ---- 4. restart isolates voices -----------------------------------------------------------------------

def test_restart_isolates_voices(make_ctx, session, oracle):
    """11 voices play utterances 0 .. 10; after 3 frames voices 2 and 5 (mid-utterance: 5 and 9 frames)
    are restarted with the seeds of utterances 12 and 14 and play those.  The other nine go on as if
    nothing had happened; the two equal fresh trajectories of their new utterances, draw counts from 0."""
    hop, B = 33, 11
    refs = references(make_ctx, oracle, 16, hop)
    s = session(B, seeds=SEEDS[:B])
    new = {2: 12, 5: 14}
    c1 = pool_call(s, [piece(oracle, u, 0) for u in range(B)], hop)
    d1 = s.rng_draws()
    s.restart(list(new), [SEEDS[i] for i in new.values()])
    assert list(s.latched) == [0 if u in new else 1 for u in range(B)]
    d = s.rng_draws()
    assert all(d[u] == (0 if u in new else d1[u]) for u in range(B))
    c2 = pool_call(s, [piece(oracle, new[u], 0) if u in new else piece(oracle, u, 3) for u in range(B)], hop)
    c3 = pool_call(s, [piece(oracle, new[u], 3) if u in new else piece(oracle, u, 6) for u in range(B)], hop)
    draws = s.rng_draws()
    assert (draws > 0).any()
    for u in range(B):
        i = new.get(u, u)
        y, want_draws, _, _ = refs[i]
        parts = ([] if u in new else [c1[0][u, :c1[1][u]]]) + [c2[0][u, :c2[1][u]], c3[0][u, :c3[1][u]]]
        got = np.concatenate(parts)
        played = min(int(NF[i]), 6 if u in new else 9)
        assert got.size == (played - 1) * hop
        assert np.array_equal(bits(got), bits(y[:got.size])), f"voice {u}, utterance {i}"
        if played == NF[i]:
            assert draws[u] == want_draws, f"voice {u}: rand() count"
    assert np.array_equal(bits(c1[0][2, :c1[1][2]]), bits(refs[2][0][:2 * hop]))  # (before the restart: their old utterances)
    with pytest.raises(_native.AfsError, match="invalid argument"):
        s.restart([3, 3])
    with pytest.raises(_native.AfsError, match="invalid argument"):
        s.restart([B])
    with pytest.raises(_native.AfsError, match="invalid argument"):
        s.restart([-1], [5])


# ---- 5. PCM -------------------------------------------------------------------------------------------

def test_pcm_rows_strided_device(make_ctx, session, oracle):
    """11 voices play utterances 0 .. 10 in chunks of 3 into a strided int16 GPU tensor whose rows start
    at odd 2-byte offsets (row stride odd, first sample at element 1): the rows equal Context.to_int16 of
    the float64 references, and every element outside [0, produced[u]) keeps its canary."""
    import torch
    hop, B = 33, 11
    ctx = make_ctx(16)
    refs = references(make_ctx, oracle, 16, hop)
    s = session(B, seeds=SEEDS[:B])
    width, pitch = CHUNK * hop + 2, CHUNK * hop + 8
    assert pitch % 2 == 1
    got = [[] for _ in range(B)]
    for start in range(0, int(NF[:B].max()), CHUNK):
        big = torch.full((B, pitch), int(CANARY16), dtype=torch.int16, device="cuda")
        out = big[:, 1:1 + width]
        assert all((out[u].data_ptr() // 2) % 2 == (u + 1) % 2 for u in range(B))  # (odd and even 2-byte offsets)
        rows = [piece(oracle, u, start) for u in range(B)]
        counts = np.array([len(r) for r in rows], dtype=np.int32)
        res = s.synthesize_frames(poisoned(rows, CHUNK), counts, hop, out=out, pcm=True)
        assert res[0] is out
        host = big.cpu().numpy()
        for u in range(B):
            n = int(res[1][u])
            got[u].append(host[u, 1:1 + n].copy())
            host[u, 1:1 + n] = CANARY16
        assert (host == CANARY16).all(), "written outside a voice's samples"
    for u in range(B):
        want = ctx.to_int16(np.ascontiguousarray(refs[u][0]))
        assert np.array_equal(np.concatenate(got[u]), want), f"voice {u}"
        print(f"voice {u}: {want.size} samples, max |int16| = {np.abs(want.astype(np.int32)).max()}")


# ---- 6. taps ------------------------------------------------------------------------------------------

def test_taps_rows_bitwise(make_ctx, session, oracle):
    """The eight MIX taps: 11 voices play utterances 4 .. 14 in chunks of 3 into device tensors; audio and
    tap rows equal afs_synthesize_taps on each utterance alone."""
    hop, B, first = 33, 11, 4
    ctx = make_ctx(16)
    refs = references(make_ctx, oracle, 16, hop, taps=MIX)
    ctx.set_taps(MIX)
    try:
        s = session(B, seeds=SEEDS[first:first + B])
        audio, rows = [[] for _ in range(B)], [[] for _ in range(B)]
        for start in range(0, int(NF[first:].max()), CHUNK):
            out, produced, tout, _ = pool_call(s, [piece(oracle, first + u, start) for u in range(B)], hop, taps=True,
                                               device=True)
            for u in range(B):
                audio[u].append(out[u, :produced[u]])
                rows[u].append(tout[u, :, :produced[u]])
        for u in range(B):
            y, _, _, want = refs[first + u]
            assert np.array_equal(bits(np.concatenate(audio[u])), bits(y)), f"voice {u}"
            assert np.array_equal(bits(np.concatenate(rows[u], axis=1)), bits(want)), f"voice {u}: taps"
    finally:
        ctx.set_taps([])


# ---- 7. interplay with the lock-step calls ------------------------------------------------------------

def test_lock_step_calls_continue_a_pool(make_ctx, session, oracle):
    """Ten voices (the utterances of 4 frames and more) play frames 0-2 through a pool call; all latched,
    synthesize_signal_tds(frame 3, hop) then continues each one, and a pool call after that plays on from
    frame 4: the trajectories' bits throughout.  On mixed latch state the lock-step call refuses."""
    hop = 33
    ids = [u for u in range(len(NF)) if NF[u] >= 4]
    B = len(ids)
    assert B == 10
    refs = references(make_ctx, oracle, 16, hop)
    s = session(B, seeds=SEEDS[ids])
    pool_call(s, [piece(oracle, i, 0) for i in ids], hop)
    assert s.latched.all()
    y = s.synthesize_signal_tds(np.array([corpus(oracle)[i][3] for i in ids], dtype=FRAME_DTYPE), hop)
    assert y.shape == (B, hop)
    for q, i in enumerate(ids):
        assert np.array_equal(bits(y[q]), bits(refs[i][0][2 * hop:3 * hop])), f"voice {q}"
    out, produced, _, _ = pool_call(s, [piece(oracle, i, 4) for i in ids], hop)
    for q, i in enumerate(ids):
        n = int(produced[q])
        assert n == (min(int(NF[i]), 7) - 4) * hop
        assert np.array_equal(bits(out[q, :n]), bits(refs[i][0][3 * hop:3 * hop + n])), f"voice {q}"
    s.restart([1])
    for kw in ({}, {"pcm": True}):
        with pytest.raises(_native.AfsError, match="latch state"):
            s.synthesize_signal_tds(corpus(oracle)[0][0], hop, **kw)
    s.reset(SEEDS[ids])  # (afs_session_reset takes the session from any state)
    assert not s.latched.any()
    assert s.synthesize_signal_tds(corpus(oracle)[0][0], hop).shape == (B, 0) and s.latched.all()


# ---- 8. one anchor to the oracle ----------------------------------------------------------------------

def test_streamed_utterances_vs_oracle(make_ctx, oracle):
    """Utterances of 2, 5 and 7 frames streamed through two voices against the oracle's incremental
    calls (the latch, then one call per frame), at the bound of the first samples (tests/test_gpu_parity.py)."""
    pick = [1, 2, 0]
    assert list(NF[pick]) == [2, 5, 7]
    utts = [corpus(oracle)[u] for u in pick]
    got = dict(make_ctx(16).synthesize_stream(utts, 33, 2, CHUNK, seeds=[int(SEEDS[u]) for u in pick], pcm=False))
    for q, u in enumerate(pick):
        x, _ = oracle.utterance_draws(np.ascontiguousarray(utts[q]), 33, int(SEEDS[u]), FS)
        assert x.size == got[q].size == (NF[u] - 1) * 33
        err = float(np.abs(got[q] - x).max())
        print(f"utterance of {NF[u]} frames: max |gpu - oracle| = {err:.3e}")
        assert err <= GOLD_TOL


# ---- 9. refusals --------------------------------------------------------------------------------------

def test_refusals(make_ctx, session, oracle):
    hop, B = 33, 11
    ctx = make_ctx(16)
    s = session(B)
    rows = [piece(oracle, u, 0) for u in range(B)]
    frames = poisoned(rows, CHUNK)
    counts = np.array([len(r) for r in rows], dtype=np.int32)
    Tmax = (CHUNK - 1) * hop

    def refused(status, sess=s, counts=counts, out=None, hop=hop, **kw):
        out = canaries((B, Tmax + 5)) if out is None else out
        with pytest.raises(_native.AfsError, match=_native.STATUS[status]):
            sess.synthesize_frames(frames, counts, hop, out=out, **kw)
        if out.dtype == np.float64:
            assert (bits(out) == CANARY).all()
        assert not sess.latched.any()  # (a refused call latches nothing)

    long = counts.copy()
    long[4] = CHUNK + 1
    refused(1, counts=long)
    neg = counts.copy()
    neg[0] = -1
    refused(1, counts=neg)
    refused(1, counts=None)
    refused(1, hop=0)
    refused(1, out=canaries((B, Tmax - 1)))
    refused(1, out=np.full((B, Tmax - 1), CANARY16, dtype=np.int16), pcm=True)
    ctx.set_taps([])
    refused(1, taps=True, taps_out=canaries((B, 1, Tmax + 5)))
    # a NULL out / pcm when a voice produces samples (straight to the library: the binding always has one)
    vp, produced = ctypes.c_void_p, np.zeros(B, dtype=np.int32)
    lib, h = s._lib, s._h
    assert lib.afs_session_synthesize_ragged(h, vp(frames.ctypes.data), CHUNK, vp(counts.ctypes.data), hop, None,
                                             Tmax, None, None, vp(produced.ctypes.data), None) == 1
    assert lib.afs_session_synthesize_ragged_pcm(h, vp(frames.ctypes.data), CHUNK, vp(counts.ctypes.data), hop, None,
                                                 Tmax, None, vp(produced.ctypes.data), None) == 1
    assert lib.afs_session_restart_voices(h, vp(np.array([0, 11], dtype=np.int32).ctypes.data), None, 2) == 1
    assert lib.afs_session_restart_voices(h, vp(np.array([4, 4], dtype=np.int32).ctypes.data), None, 2) == 1
    assert not s.latched.any() and not produced.any()
    # voices that only latch produce nothing and need no out
    one = np.minimum(counts, 1)
    out, produced = s.synthesize_frames(frames, one, hop)
    assert out.shape == (B, 0) and not produced.any() and s.latched.all()
    # the one-lane solvers have no pool
    chol = session(B, solver="cholesky")
    refused(5, sess=chol)
    with pytest.raises(_native.AfsError, match=_native.STATUS[5]):
        chol.restart([0])
