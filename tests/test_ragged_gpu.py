"""afs_synthesize_ragged on the GPU: 21 utterances of 2 .. 7 frames (a: -> s glides, so the noise
sources fire) in one call, every row bit for bit the single-utterance afs_synthesize call's -- audio,
rand() count, non-finite flag, tap rows -- through the three synthesis kernels, the hop-record and the
dense plan paths, launches that split inside, at and after a block's end, the chunked hop path and a
reversed batch; three rows against the oracle; the refusals.  Frames at or past each count are
poisoned (every double NaN, every byte field 0) and the outputs carry a canary past each row's end:
nothing there may be read or written.  Every reference is computed once and left unchanged."""
import numpy as np
import pytest

from areafunctionsynthesis_amd import _native
from areafunctionsynthesis_amd.frames import FRAME_DTYPE
from taps_lib import CURRENT, FS, PRESSURE, glide_frames

pytestmark = pytest.mark.gpu

NF = np.array([7, 2, 5, 5, 3, 7, 2, 5, 5, 5, 5, 5, 5, 5, 5, 4, 5, 6, 6, 2, 3], dtype=np.int32)
FSTRIDE = 8
ONE_WAVE_B = 1025  # (64 lanes: batches above TREE_PAIR64_MAX = 1024 run one wave per utterance)
MIX = [(CURRENT, 24), (PRESSURE, 25), (PRESSURE, 22), (CURRENT, 93), (CURRENT, 96), (PRESSURE, 83), (PRESSURE, 60),
       (CURRENT, 65)]  # (the eight taps of tests/test_taps_gpu.py)
CANARY = np.uint64(0x7FF8C0DECAFE0123)  # (a NaN no kernel computes)
GOLD_TOL = 1e-9  # (tests/test_gpu_parity.py: golden / oracle, first samples)

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


def base(oracle):
    """(frames[21, 8], seeds[21]): utterance u glides a: -> s over its NF[u] frames with a velum of its
    own; the frames past its count are poison."""
    if "base" not in _CACHE:
        poison = np.zeros((), dtype=FRAME_DTYPE)
        for name in FRAME_DTYPE.names:
            if FRAME_DTYPE[name].base.kind == "f":
                poison[name] = np.nan
        frames = np.empty((len(NF), FSTRIDE), dtype=FRAME_DTYPE)
        frames[...] = poison
        for u, F in enumerate(NF):
            frames[u, :F] = glide_frames(oracle, int(F), 0.3 + 0.03 * u)
        seeds = (101 + 7 * np.arange(len(NF))).astype(np.uint32)
        frames.setflags(write=False)
        seeds.setflags(write=False)
        _CACHE["base"] = (frames, seeds)
    return _CACHE["base"]


def batch(oracle, B):
    """The first B utterances, or the 21 tiled up to B: (frames, counts, seeds, index into the 21)."""
    frames, seeds = base(oracle)
    idx = np.arange(B) % len(NF)
    return np.ascontiguousarray(frames[idx]), np.ascontiguousarray(NF[idx]), np.ascontiguousarray(seeds[idx]), idx


def references(make_ctx, oracle, lanes, hop, taps=None):
    """Utterance u alone through afs_synthesize (afs_synthesize_taps) with its own frame count, on a
    context of the same lane width: [(audio[T_u], draws, nonfinite flag, taps[n, T_u] or None)] x 21."""
    key = ("ref", lanes, hop, None if taps is None else tuple(taps))
    if key not in _CACHE:
        ctx = make_ctx(lanes)
        frames, seeds = base(oracle)
        refs = []
        for u, F in enumerate(NF):
            fr = np.ascontiguousarray(frames[u:u + 1, :F])
            if taps is None:
                y, rep = ctx.synthesize(fr, hop, seeds=seeds[u:u + 1], report=True)
                rows = None
            else:
                ctx.set_taps(taps)
                y, rows, rep = ctx.synthesize(fr, hop, seeds=seeds[u:u + 1], report=True, taps=True)
                rows = rows[0]
            refs.append((y[0], int(ctx.rng_draws(1)[0]), int(rep["nonfinite"][0]), rows))
        _CACHE[key] = refs
    return _CACHE[key]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def canaries(shape):
    return np.full(shape, CANARY, dtype=np.uint64).view(np.float64)


def ragged(ctx, frames, counts, hop, seeds, device=False, taps=False):
    """One afs_synthesize_ragged call into canary-filled outputs of stride Tmax + 5 (device tensors
    when asked): (out, taps or None, report, draws)."""
    B = frames.shape[0]
    stride = int(counts.max() - 1) * hop + 5
    out = canaries((B, stride))
    tout = canaries((B, ctx.n_taps, stride)) if taps else None
    if device:
        import torch
        out = torch.from_numpy(out).cuda()
        tout = torch.from_numpy(tout).cuda() if taps else None
    res = ctx.synthesize_ragged(frames, counts, hop, seeds=seeds, out=out, report=True, taps=taps, taps_out=tout)
    lengths, rep = res[1], res[-1]
    assert np.array_equal(lengths, (counts.astype(np.int64) - 1) * hop)
    if device:
        out = out.cpu().numpy()
        tout = tout.cpu().numpy() if taps else None
    return out, tout, rep, ctx.rng_draws(B)


def check_rows(out, tout, rep, draws, counts, hop, idx, refs, noise_fires=True):
    """Every row and what belongs to it equals its reference bit for bit; nothing past its end changed."""
    T = (counts.astype(np.int64) - 1) * hop
    for u in range(out.shape[0]):
        y, d, nf, rows = refs[idx[u]]
        assert np.array_equal(bits(out[u, :T[u]]), bits(y)), f"row {u}"
        assert (bits(out[u, T[u]:]) == CANARY).all(), f"row {u}: written past its end"
        assert draws[u] == d, f"row {u}: rand() count"
        assert rep["nonfinite"][u] == nf == 0, f"row {u}: non-finite flag"
        if tout is not None:
            assert np.array_equal(bits(tout[u, :, :T[u]]), bits(rows)), f"row {u}: taps"
            assert (bits(tout[u, :, T[u]:]) == CANARY).all(), f"row {u}: taps written past its end"
    assert (draws > 0).any() == noise_fires  # (equal to the references' counts row by row, above)
    assert rep["nonfinite_utterances"] == 0
    assert rep["samples"] == int(T.sum())


KERNELS = {"pair16": (16, len(NF), "tree_pair_kernel"), "pair64": (64, 5, "tree_pair64_kernel"),
           "one_wave64": (64, ONE_WAVE_B, "tree_synth_kernel")}


def rows_equal_single_calls(make_ctx, oracle, kernel, hop):
    lanes, B, name = KERNELS[kernel]
    ctx = make_ctx(lanes)
    assert ctx.synthesis_kernel(B) == name
    frames, counts, seeds, idx = batch(oracle, B)
    out, _, rep, draws = ragged(ctx, frames, counts, hop, seeds, device=kernel == "pair16")
    # (hop 5: the longest utterance has 30 samples, and no noise source has fired by then -- the
    # single-utterance references count no rand() call either; at hop 33 they do)
    check_rows(out, None, rep, draws, counts, hop, idx, references(make_ctx, oracle, lanes, hop), noise_fires=hop == 33)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_rows_equal_single_calls_bitwise(make_ctx, oracle, kernel):
    """hop 33 (hop records): 21 utterances at 16 lanes into device tensors, 5 at 64 lanes as pairs,
    the 21 tiled to 1025 through the one-wave kernel."""
    rows_equal_single_calls(make_ctx, oracle, kernel, 33)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_dense_kernel_rows_bitwise(make_ctx, oracle, kernel):
    """hop 5, below AFS_PLAN_HOP_MIN: the dense chunked path and K1's dense form."""
    assert 5 < _native.AFS_PLAN_HOP_MIN
    rows_equal_single_calls(make_ctx, oracle, kernel, 5)


@pytest.mark.parametrize("per", [50, 66])
def test_launch_edges(make_ctx, oracle, per):
    """Launches of 50 and 66 samples at hop 33 (blocks end at 33, 66, .. 198): blocks end inside a
    launch, exactly at a launch boundary and before a launch starts, after launches of odd length (the
    pairs' X_RELX2 copy).  Bit for bit the unsplit ragged call, at 16 lanes and as 64-lane pairs."""
    for kernel in ("pair16", "pair64"):
        lanes, B, _ = KERNELS[kernel]
        frames, counts, seeds, idx = batch(oracle, B)
        whole = ragged(make_ctx(lanes), frames, counts, 33, seeds)
        split = ragged(make_ctx(lanes, env={"AFS_LAUNCH_SAMPLES": str(per)}), frames, counts, 33, seeds)
        assert np.array_equal(bits(split[0]), bits(whole[0])), kernel
        assert np.array_equal(split[3], whole[3]) and (whole[3] > 0).any()
        check_rows(split[0], None, split[2], split[3], counts, 33, idx, references(make_ctx, oracle, lanes, 33))


def test_chunked_hop_path(make_ctx, oracle):
    """1025 rows x 6 hop records exceed a plan budget of 1 MB: run_chunked plays one hop per chunk
    (K5 and K1 per chunk, rows ending from chunk to chunk).  Bit for bit the default call."""
    frames, counts, seeds, idx = batch(oracle, ONE_WAVE_B)
    whole = ragged(make_ctx(16), frames, counts, 33, seeds)
    chunked = ragged(make_ctx(16, env={"AFS_PLAN_BUDGET_MB": "1"}), frames, counts, 33, seeds)
    assert np.array_equal(bits(chunked[0]), bits(whole[0]))
    assert np.array_equal(chunked[3], whole[3])
    check_rows(chunked[0], None, chunked[2], chunked[3], counts, 33, idx, references(make_ctx, oracle, 16, 33))


def test_reversed_batch_reverses_rows(make_ctx, oracle):
    frames, counts, seeds, _ = batch(oracle, len(NF))
    fwd = ragged(make_ctx(16), frames, counts, 33, seeds)
    rev = ragged(make_ctx(16), np.ascontiguousarray(frames[::-1]), np.ascontiguousarray(counts[::-1]), 33,
                 np.ascontiguousarray(seeds[::-1]))
    assert np.array_equal(bits(rev[0][::-1]), bits(fwd[0]))
    assert np.array_equal(rev[3][::-1], fwd[3])


def test_taps_rows_bitwise(make_ctx, oracle):
    """The eight MIX taps at 16 lanes: audio and tap rows equal afs_synthesize_taps on each utterance
    alone, canaries past each row's end in the tap rows too."""
    ctx = make_ctx(16)
    frames, counts, seeds, idx = batch(oracle, len(NF))
    refs = references(make_ctx, oracle, 16, 33, taps=MIX)
    ctx.set_taps(MIX)
    try:
        out, tout, rep, draws = ragged(ctx, frames, counts, 33, seeds, device=True, taps=True)
    finally:
        ctx.set_taps([])
    check_rows(out, tout, rep, draws, counts, 33, idx, refs)


def test_rows_vs_oracle(make_ctx, oracle):
    """Utterances of 2, 5 and 7 frames in one call against the oracle, at the bound of the first
    samples (tests/test_gpu_parity.py)."""
    frames, seeds = base(oracle)
    pick = [1, 2, 0]
    assert list(NF[pick]) == [2, 5, 7]
    # (the list form: per-utterance arrays, padded by the binding, into an array it allocates)
    out, lengths = make_ctx(16).synthesize_ragged([frames[u, :NF[u]] for u in pick], None, 33,
                                                  seeds=np.ascontiguousarray(seeds[pick]))
    assert out.shape == (3, 6 * 33) and list(lengths) == [33, 4 * 33, 6 * 33]
    for q, u in enumerate(pick):
        x = oracle.utterance(np.ascontiguousarray(frames[u, :NF[u]]), 33, int(seeds[u]), FS)
        assert x.size == lengths[q]
        err = float(np.abs(out[q, :x.size] - x).max())
        print(f"utterance of {NF[u]} frames: max |gpu - oracle| = {err:.3e}")
        assert err <= GOLD_TOL
        assert not out[q, x.size:].any()  # (zero past the row's end)


def test_refusals(make_ctx, oracle):
    ctx = make_ctx(16)
    frames, counts, seeds, _ = batch(oracle, len(NF))
    Tmax = int(counts.max() - 1) * 33

    def refused(status, counts=counts, out=None, **kw):
        out = canaries((len(NF), Tmax + 5)) if out is None else out
        with pytest.raises(_native.AfsError, match=_native.STATUS[status]):
            kw.pop("ctx", ctx).synthesize_ragged(frames, counts, 33, seeds=seeds, out=out, **kw)
        assert (bits(out) == CANARY).all()

    one = counts.copy()
    one[3] = 1
    refused(1, counts=one)
    long = counts.copy()
    long[4] = FSTRIDE + 1
    refused(1, counts=long)
    refused(1, out=canaries((len(NF), Tmax - 1)))
    refused(1, counts=None)
    ctx.set_taps([])
    refused(1, taps=True, taps_out=canaries((len(NF), 1, Tmax + 5)))
    refused(5, ctx=make_ctx(None, solver="cholesky"))
