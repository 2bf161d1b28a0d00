"""Signal taps on the GPU (afs_set_taps, afs_synthesize_taps, afs_session_synthesize_taps): every
tap of every kernel against the oracle's state per sample, the hop-record and dense kernels, what
must be bit for bit (launch splits, sessions, the slot order, pairs against one wave, the rest of the
batch), the edges of device tap rows, and the refusals.  The bound against the oracle is
taps_lib.TAP_TOL; everything else is exact."""
import numpy as np
import pytest

from areafunctionsynthesis_amd import _native
from taps_lib import (ALL_TAPS, CURRENT, FS, GROUPS, PRESSURE, TAP_TOL, glide_batch, glide_frames, oracle_state,
                      rel_err, want_rows)

pytestmark = pytest.mark.gpu

ONE_WAVE_B = 1025  # (64 lanes: batches above TREE_PAIR64_MAX = 1024 run one wave per utterance)
MIX = [(CURRENT, 24), (PRESSURE, 25), (PRESSURE, 22), (CURRENT, 93), (CURRENT, 96), (PRESSURE, 83), (PRESSURE, 60),
       (CURRENT, 65)]  # dynamic and static owners, both radiation ends


@pytest.fixture(scope="module")
def make_ctx(monkeypatch_module):
    from areafunctionsynthesis_amd.synthesizer import Context
    made = []

    def make(lanes=16, env=None, **kw):
        for k, v in (env or {}).items():
            monkeypatch_module.setenv(k, v)
        try:
            made.append(Context(FS, solver=kw.pop("solver", "tree"), lanes=lanes, **kw))
        finally:
            for k in env or {}:
                monkeypatch_module.delenv(k)
        return made[-1]

    yield make
    for c in made:
        c.close()


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.fixture(scope="module")
def ctx16(make_ctx):
    return make_ctx(16)


@pytest.fixture(scope="module")
def ctx64(make_ctx):
    return make_ctx(64)


def run(ctx, frames, hop, seeds, taps, **kw):
    ctx.set_taps(taps)
    return ctx.synthesize(np.ascontiguousarray(frames), hop, seeds=seeds, taps=True, **kw)


def tiled(frames, seeds, B):
    """The utterances repeated up to a batch of B (rows u and u + len repeat each other)."""
    idx = np.arange(B) % frames.shape[0]
    return np.ascontiguousarray(frames[idx]), np.ascontiguousarray(seeds[idx])


@pytest.mark.parametrize("kernel", ["pair16", "pair64", "one_wave64"])
def test_every_tap_vs_oracle_per_sample(ctx16, ctx64, oracle, parity_report, kernel):
    """The hop-1 a: -> s glide: 5 utterances at 16 lanes (a full group of four and a ragged one), 3 at
    64 lanes as pairs and through the one-wave kernel; 24 launches of 8 taps cover the 93 pressures
    and 97 currents once per kernel; the oracle is driven with one-sample calls on the same frames."""
    n = 5 if kernel == "pair16" else 3
    ctx = ctx16 if kernel == "pair16" else ctx64
    frames, seeds = glide_batch(oracle, n)
    B = ONE_WAVE_B if kernel == "one_wave64" else n
    assert ctx.synthesis_kernel(B) == {"pair16": "tree_pair_kernel", "pair64": "tree_pair64_kernel",
                                       "one_wave64": "tree_synth_kernel"}[kernel]
    fb, sb = tiled(frames, seeds, B)
    state = [oracle_state(oracle, frames[u], 1, seeds[u]) for u in range(n)]
    plain = ctx.synthesize(fb, 1, seeds=sb)
    e_audio = max(rel_err(plain[u], state[u][0]) for u in range(n))
    worst = (0.0, None)
    for taps in GROUPS:
        audio, rows = run(ctx, fb, 1, sb, taps)
        assert np.array_equal(audio, plain)  # the audio of a _taps call is the plain call's
        assert rows.shape == (B, len(taps), 47)
        for u in range(n):
            want = want_rows(state[u][1], state[u][2], taps)
            for q, t in enumerate(taps):
                e = rel_err(rows[u, q], want[q])
                print(f"{kernel} u={u} tap={t} e={e:.3e}")
                if e > worst[0]:
                    worst = (e, (u, t))
    parity_report.append(f"taps vs oracle [{kernel}]: {n} utterances x 190 traces x 47 samples: max e {worst[0]:.2e} at "
                         f"(utterance, tap) {worst[1]}, e_audio {e_audio:.2e}")
    assert worst[0] <= TAP_TOL, worst
    assert worst[0] <= 100.0 * e_audio, (worst, e_audio)  # (beyond that a tap is wrong, not rounded)


def test_hop_records_checkpoints_and_dense_kernel(ctx16, make_ctx, oracle, parity_report):
    """hop = 33 (above AFS_PLAN_HOP_MIN, not a multiple of 16), 4 frames: the oracle's state after each
    of its three calls checks samples 32, 65 and 98 of all 190 quantities; the same call under
    AFS_PLAN_DENSE=1 checks every sample of the dense kernel at a hop >= 32.  The hop records' words are
    within 1e-12 relative of the dense records' (README), and 99 samples of a passive, damped network
    do not amplify a source's relative change: the traces agree within 100 x that."""
    hop, B = 33, 5
    frames = np.stack([glide_frames(oracle, 4, 0.6 + 0.1 * u) for u in range(B)])
    seeds = np.arange(11, 11 + B, dtype=np.uint32)
    dense = make_ctx(16, env={"AFS_PLAN_DENSE": "1"})
    state = [oracle_state(oracle, frames[u], hop, seeds[u]) for u in range(B)]
    worst, worst_d = 0.0, 0.0
    e_audio = max(rel_err(a, state[u][0]) for u, a in enumerate(ctx16.synthesize(frames, hop, seeds=seeds)))
    for taps in GROUPS:
        audio, rows = run(ctx16, frames, hop, seeds, taps)
        audio_d, rows_d = run(dense, frames, hop, seeds, taps)
        for u in range(B):
            want = want_rows(state[u][1], state[u][2], taps)
            assert np.count_nonzero(~np.isnan(want[0])) == 3
            for q, t in enumerate(taps):
                for got in (rows[u, q], rows_d[u, q]):
                    e = rel_err(got, want[q])
                    assert e <= TAP_TOL, (u, t, e)
                    worst = max(worst, e)
                peak = np.abs(rows_d[u, q]).max()
                d = float(np.abs(rows[u, q] - rows_d[u, q]).max() / peak) if peak else float(np.abs(rows[u, q]).max())
                print(f"u={u} tap={t} hop records vs dense: {d:.3e}")
                worst_d = max(worst_d, d)
    parity_report.append(f"taps, hop 33 [pair16]: checkpoints vs oracle max e {worst:.2e} (e_audio {e_audio:.2e}); hop records vs dense "
                         f"records over 99 samples: max relative diff {worst_d:.2e}")
    assert worst <= 100.0 * e_audio, (worst, e_audio)  # (beyond that a tap is wrong, not rounded)
    assert worst_d <= 1e-10


def test_launch_split_is_bitwise(ctx16, make_ctx, oracle):
    """AFS_LAUNCH_SAMPLES=40: the rows go on in the next launch where the last one stopped (hop 33:
    launches end inside hops and inside 128-byte lines)."""
    frames = np.stack([glide_frames(oracle, 4, 0.6 + 0.1 * u) for u in range(5)])
    seeds = np.arange(11, 16, dtype=np.uint32)
    split = make_ctx(16, env={"AFS_LAUNCH_SAMPLES": "40"})
    for f, hop in ((frames, 33), (glide_batch(oracle, 5)[0], 1)):
        a, r = run(ctx16, f, hop, seeds, MIX)
        a2, r2 = run(split, f, hop, seeds, MIX)
        assert np.array_equal(a, a2) and np.array_equal(r, r2)


@pytest.mark.parametrize("lanes", [16, 64])
def test_session_call_lengths(ctx16, ctx64, make_ctx, oracle, lanes):
    """A session driven with call lengths 1, 7, 16, 17 and 441 (the dense and the hop-record kernels
    alternating on one saved state): its audio is the plain session's, its taps the same bit for bit
    when every call is split into launches of 40 samples, and the last sample of each call is the
    oracle's state after its call of that length."""
    from areafunctionsynthesis_amd.synthesizer import Synthesizer
    lengths, B = (1, 7, 16, 17, 441), 3
    frames = np.stack([glide_frames(oracle, len(lengths) + 1, 0.6 + 0.1 * u) for u in range(B)])
    seeds = np.arange(11, 11 + B, dtype=np.uint32)
    ctx = ctx16 if lanes == 16 else ctx64
    split = make_ctx(lanes, env={"AFS_LAUNCH_SAMPLES": "40"})

    def session(c, taps):
        c.set_taps(MIX)
        syn = Synthesizer(c, B, seeds)
        try:
            latch = syn.synthesize_signal_tds(frames[:, 0], 5, taps=taps)
            assert (latch[0] if taps else latch).shape == (B, 0)
            return [syn.synthesize_signal_tds(frames[:, k + 1], n, taps=taps) for k, n in enumerate(lengths)]
        finally:
            syn.close()

    with_taps, plain, chopped = session(ctx, True), session(ctx, False), session(split, True)
    for k, n in enumerate(lengths):
        assert with_taps[k][1].shape == (B, len(MIX), n)
        assert np.array_equal(with_taps[k][0], plain[k][:, :n])
        assert np.array_equal(with_taps[k][1], chopped[k][1])
    for u in range(B):
        h = oracle.create(FS, int(seeds[u]))
        try:
            oracle.call(h, frames[u, 0], 5)
            for k, n in enumerate(lengths):
                oracle.call(h, frames[u, k + 1], n)
                P, U = oracle.pressures(h), oracle.currents(h)
                for q, (kind, index) in enumerate(MIX):
                    want = (P if kind == PRESSURE else U)[index]
                    peak = max(np.abs(c[1][u, q]).max() for c in with_taps)  # (of the whole trace)
                    assert abs(with_taps[k][1][u, q, -1] - want) <= TAP_TOL * max(peak, abs(want)), (u, k, q)
        finally:
            oracle.destroy(h)


def test_slot_order_and_batch_do_not_matter(ctx16, make_ctx, oracle):
    """21 utterances of different shapes (the slot order sorts them by shape: rows are indexed by
    utterance, not by slot): AFS_SHAPE_ORDER=0 gives the same rows, and an utterance alone gives the
    rows it has in the batch."""
    vowels, fric = ("a:", "i:", "u:", "e:", "o:", "@", "E"), ("s", "f", "S")
    frames = np.stack([glide_frames(oracle, 4, 0.3 * (u % 3), vowels[u % 7], fric[u % 3]) for u in range(21)])
    seeds = np.arange(31, 52, dtype=np.uint32)
    plain_order = make_ctx(16, env={"AFS_SHAPE_ORDER": "0"})
    a, r = run(ctx16, frames, 33, seeds, MIX)
    a2, r2 = run(plain_order, frames, 33, seeds, MIX)
    assert np.array_equal(a, a2) and np.array_equal(r, r2)
    assert len({r[u].tobytes() for u in range(21)}) == 21  # (no two utterances alike: a swap would show)
    for u in (0, 8, 20):
        a1, r1 = run(ctx16, frames[u:u + 1], 33, seeds[u:u + 1], MIX)
        assert np.array_equal(a1[0], a[u]) and np.array_equal(r1[0], r[u])


def test_voice_pairs_equal_one_wave_bitwise(ctx64, oracle):
    frames, seeds = glide_batch(oracle, 3)
    fb, sb = tiled(frames, seeds, ONE_WAVE_B)
    for taps in (MIX, GROUPS[5], GROUPS[20]):
        a, r = run(ctx64, frames, 1, seeds, taps)
        a1, r1 = run(ctx64, fb, 1, sb, taps)
        assert np.array_equal(a, a1[:3]) and np.array_equal(r, r1[:3])


@pytest.mark.parametrize("T", [1, 15, 16, 17, 99])
@pytest.mark.parametrize("offset", [1, 3, 15])
def test_device_rows_at_any_alignment(ctx16, ctx64, oracle, offset, T):
    """Device taps_out whose rows start `offset` doubles past a 128-byte boundary (the rows follow one
    another T doubles apart: every position in a line occurs), canaries on both sides: the rows are
    the host buffer's, and nothing else is written."""
    import torch
    hop, F = (33, 4) if T == 99 else (T, 2)
    B = 5
    frames = np.stack([glide_frames(oracle, F, 0.6 + 0.1 * u) for u in range(B)])
    seeds = np.arange(11, 11 + B, dtype=np.uint32)
    for ctx in (ctx16, ctx64):
        _, want = run(ctx, frames, hop, seeds, MIX)
        n = B * len(MIX) * T
        buf = torch.full((n + 64,), -7.25, dtype=torch.float64, device="cuda")
        base = (-(buf.data_ptr() // 8) % 16 + offset) % 16 + 16  # first double of the rows
        assert (buf.data_ptr() // 8 + base) % 16 == offset
        rows = buf[base:base + n]
        ctx.synthesize(frames, hop, seeds=seeds, taps=True, taps_out=rows)
        ctx.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(got[base:base + n].reshape(B, len(MIX), T), want)
        assert (got[:base] == -7.25).all() and (got[base + n:] == -7.25).all()


def test_refusals(ctx16, make_ctx, oracle):
    frames, seeds = glide_batch(oracle, 2)
    frames = np.ascontiguousarray(frames)
    lane = make_ctx(None, solver="cholesky")
    with pytest.raises(_native.AfsError, match="unsupported"):
        lane.set_taps(MIX)
    with pytest.raises(_native.AfsError, match="unsupported"):
        lane.synthesize(frames, 1, seeds=seeds, taps=True, taps_out=np.zeros((2, 1, 47)))
    with pytest.raises(_native.AfsError, match="invalid argument"):
        ctx16.set_taps(ALL_TAPS[:9])
    with pytest.raises(_native.AfsError, match="invalid argument"):
        ctx16.set_taps([(PRESSURE, 93)])
    with pytest.raises(_native.AfsError, match="invalid argument"):
        ctx16.set_taps([(CURRENT, 97)])
    with pytest.raises(_native.AfsError, match="invalid argument"):
        ctx16.set_taps([(2, 0)])
    ctx16.set_taps([])
    with pytest.raises(_native.AfsError, match="invalid argument"):
        ctx16.synthesize(frames, 1, seeds=seeds, taps=True, taps_out=np.zeros((2, 1, 47)))


def test_nan_area_reaches_flags_and_tap_rows(ctx16, oracle):
    frames, seeds = glide_batch(oracle, 2)
    frames = frames.copy()
    frames["area_cm2"][1, 10:, 20] = np.nan
    flags = np.zeros(2, dtype=np.uint8)
    audio, rows = run(ctx16, frames, 1, seeds, MIX, nonfinite=flags)
    assert list(flags) == [0, 1]
    assert np.isfinite(rows[0]).all() and np.isfinite(audio[0]).all()
    assert np.isnan(rows[1, :, -1]).all() and np.isfinite(rows[1, :, :9]).all()
