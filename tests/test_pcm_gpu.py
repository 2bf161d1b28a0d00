"""The PCM output calls on the GPU (afs_synthesize_pcm, afs_synthesize_ragged_pcm,
afs_session_synthesize_pcm, afs_memory_info_get).  The yardstick is the two-step path on a context of the
same configuration -- synthesize, then to_int16 -- which the parity tests pin to the oracle: every row
must equal it bit for bit, so there is no tolerance; flags, rand() counts and reports must be the fp64
call's.  Destinations carry canaries: rows that start 1 int16 into their allocation, strides with
padding, the samples past a ragged row's end.  Every reference is computed once per configuration."""
import ctypes

import numpy as np
import pytest

from areafunctionsynthesis_amd import _native
from areafunctionsynthesis_amd.frames import FRAME_DTYPE
from taps_lib import FS, glide_frames

pytestmark = pytest.mark.gpu

CANARY = np.int16(0x5A5B)
_vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.fixture(scope="module")
def make_ctx(monkeypatch_module):
    """Contexts by (lanes, environment at creation, solver, options), each made once."""
    from areafunctionsynthesis_amd.synthesizer import Context
    made = {}

    def make(lanes=None, env=None, solver="tree", fs=FS, fresh=False, **options):
        key = (lanes, tuple(sorted((env or {}).items())), solver, fs, tuple(sorted(options.items())))
        if fresh or key not in made:
            for k, v in (env or {}).items():
                monkeypatch_module.setenv(k, v)
            try:
                ctx = Context(fs, solver=solver, lanes=lanes, **options)
            finally:
                for k in env or {}:
                    monkeypatch_module.delenv(k)
            made[(key, len(made)) if fresh else key] = ctx
            return ctx
        return made[key]

    yield make
    for c in made.values():
        c.close()


# ---- uniform calls ------------------------------------------------------------------------------

_BATCH = {}


def uniform_batch(oracle, two_mass, F=5):
    """11 utterances of F frames: six a: -> s glides, four static vowels of workloads.static_vowels, and
    one glide whose lung pressure is NaN from the second frame on (tests/test_gpu_parity.py's recipe for
    a non-finite utterance).  11 crosses one 8-slot block and leaves K6's wave partly filled."""
    if (two_mass, F) not in _BATCH:
        from areafunctionsynthesis_amd.workloads import static_vowels
        rows = [glide_frames(oracle, F, 0.3 + 0.1 * u) for u in range(6)]
        w = static_vowels(4, seconds=0.05)
        for u in range(4):
            f = oracle.af_to_frame(w.params[u, 0])
            f["velum_opening_cm2"] = 0.0
            f["glottis"] = w.glottis[u, 0]
            rows.append(np.repeat(f[None], F))
        bad = glide_frames(oracle, F, 0.5)
        bad["glottis"][1:, 1] = np.nan
        rows.append(bad)
        frames = np.stack(rows).astype(FRAME_DTYPE)
        if two_mass:  # (control 5 is the two-mass model's damping factor)
            frames["glottis"][:, :, 5] = 1.2
        seeds = (31 + 5 * np.arange(len(rows))).astype(np.uint32)
        frames.setflags(write=False)
        _BATCH[(two_mass, F)] = (frames, seeds)
    return _BATCH[(two_mass, F)]


BAD = 10  # (the non-finite utterance's row)

# (lanes, hop, environment, glottis model, radiation_from_skin): hop 33 takes the hop records, hop 7 the
# dense chunked path; 11 utterances run tree_pair64_kernel by default and tree_pair_kernel at 16 lanes;
# launches of 50 and 37 samples give K6 even and odd first samples s0.  Five frames each; at hop 7 those
# are 28 samples, in which the voice has not yet reached one int16 step (the oracle: 2e-4 of a step), so
# the two hop-7 configurations run once more with 21 frames, where the audio spans hundreds of steps.
CONFIGS = {
    "pair64-hop33-l50": (None, 33, {"AFS_LAUNCH_SAMPLES": "50"}, 0, 1),
    "pair16-hop33-l37": (16, 33, {"AFS_LAUNCH_SAMPLES": "37"}, 0, 1),
    "pair16-hop7-l37-noskin": (16, 7, {"AFS_LAUNCH_SAMPLES": "37"}, 0, 0),
    "pair64-hop7-l50-twomass": (None, 7, {"AFS_LAUNCH_SAMPLES": "50"}, 1, 1),
    "pair16-hop33-dense-l50-twomass-noskin": (16, 33, {"AFS_PLAN_DENSE": "1", "AFS_LAUNCH_SAMPLES": "50"}, 1, 0),
    "pair16-hop33-one-launch": (16, 33, {}, 0, 1),
    "pair64-hop33-l37-twomass-noskin": (None, 33, {"AFS_LAUNCH_SAMPLES": "37"}, 1, 0),
    "pair16-hop7-l37-noskin-21frames": (16, 7, {"AFS_LAUNCH_SAMPLES": "37"}, 0, 0, 21),
    "pair64-hop7-l50-twomass-21frames": (None, 7, {"AFS_LAUNCH_SAMPLES": "50"}, 1, 1, 21),
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_uniform_rows_equal_two_step(make_ctx, oracle, name):
    import torch
    lanes, hop, env, model, skin = CONFIGS[name][:5]
    ctx = make_ctx(lanes, env, glottis_model=model, radiation_from_skin=skin)
    frames, seeds = uniform_batch(oracle, bool(model), *CONFIGS[name][5:])
    B, F = frames.shape
    T = (F - 1) * hop
    assert ctx.synthesis_kernel(B) == ("tree_pair_kernel" if lanes == 16 else "tree_pair64_kernel")
    y, rep = ctx.synthesize(frames, hop, seeds=seeds, report=True)
    want = ctx.to_int16(y)
    draws = ctx.rng_draws(B)
    assert list(np.flatnonzero(rep["nonfinite"])) == [BAD] and not np.isfinite(y[BAD]).all()
    assert (want[BAD][~np.isfinite(y[BAD])] == 0).all()
    print(f"{name}: T = {T}, peak |int16| = {np.abs(want[:BAD].astype(np.int32)).max()}, draws up to {draws.max()}")
    if T >= 100:  # (not the 28-sample calls)
        assert np.abs(want[:BAD].astype(np.int32)).max() > 100  # (the audio is not silence)
    # a device pcm that starts 1 int16 into its allocation, rows of T + 3, canaries around and between
    stride = T + 3
    buf = torch.full((1 + B * stride + 8,), int(CANARY), dtype=torch.int16, device="cuda")
    rows = buf[1:1 + B * stride].view(B, stride)
    flags = torch.zeros(B, dtype=torch.uint8, device="cuda")
    got = ctx.synthesize(frames, hop, seeds=seeds, out=rows[:, :T], pcm=True, nonfinite=flags)
    assert got.data_ptr() == buf.data_ptr() + 2
    host = buf.cpu().numpy()
    grid = host[1:1 + B * stride].reshape(B, stride)
    for u in range(B):
        assert np.array_equal(grid[u, :T], want[u]), f"row {u}"
    assert (grid[:, T:] == CANARY).all() and host[0] == CANARY and (host[1 + B * stride:] == CANARY).all()
    assert np.array_equal(flags.cpu().numpy(), rep["nonfinite"])
    assert np.array_equal(ctx.rng_draws(B), draws)
    # a host pcm with pcm_stride = T, with the report
    pcm, prep = ctx.synthesize(frames, hop, seeds=seeds, pcm=True, report=True)
    assert pcm.dtype == np.int16 and np.array_equal(pcm, want)
    assert np.array_equal(prep["nonfinite"], rep["nonfinite"])
    assert (prep["samples"], prep["nonfinite_utterances"]) == (rep["samples"], rep["nonfinite_utterances"]) == (B * T, 1)
    assert np.array_equal(ctx.rng_draws(B), draws)
    # a host pcm whose rows have padding: the padding is the caller's
    wide = np.full((B, T + 5), CANARY, dtype=np.int16)
    ctx.synthesize(frames, hop, seeds=seeds, out=wide[:, :T], pcm=True)
    assert np.array_equal(wide[:, :T], want) and (wide[:, T:] == CANARY).all()


# ---- ragged calls -------------------------------------------------------------------------------

NF = np.array([7, 2, 5, 5, 3, 7, 2, 5, 5, 5, 5, 5, 5, 5, 5, 4, 5, 6, 6, 2, 3], dtype=np.int32)
FSTRIDE = 8
RAGGED_HOP = 33


def ragged_batch(oracle):
    """As tests/test_ragged_gpu.py: 21 a: -> s glides of 2 .. 7 frames, the frames past each count poison
    (every double NaN, every byte field 0)."""
    if "ragged" not in _BATCH:
        poison = np.zeros((), dtype=FRAME_DTYPE)
        for field in FRAME_DTYPE.names:
            if FRAME_DTYPE[field].base.kind == "f":
                poison[field] = np.nan
        frames = np.empty((len(NF), FSTRIDE), dtype=FRAME_DTYPE)
        frames[...] = poison
        for u, F in enumerate(NF):
            frames[u, :F] = glide_frames(oracle, int(F), 0.3 + 0.03 * u)
        seeds = (101 + 7 * np.arange(len(NF))).astype(np.uint32)
        frames.setflags(write=False)
        _BATCH["ragged"] = (frames, seeds)
    return _BATCH["ragged"]


@pytest.mark.parametrize("launch", ["50", "66"])
@pytest.mark.parametrize("order", ["call", "reversed"])
def test_ragged_rows_equal_two_step(make_ctx, oracle, launch, order):
    import torch
    ctx = make_ctx(16, {"AFS_LAUNCH_SAMPLES": launch})
    frames, seeds = ragged_batch(oracle)
    idx = np.arange(len(NF))[::-1] if order == "reversed" else np.arange(len(NF))
    frames, counts, seeds = np.ascontiguousarray(frames[idx]), np.ascontiguousarray(NF[idx]), np.ascontiguousarray(seeds[idx])
    B, hop = len(counts), RAGGED_HOP
    T = (counts.astype(np.int64) - 1) * hop
    y, lengths, rep = ctx.synthesize_ragged(frames, counts, hop, seeds=seeds, report=True)
    assert np.array_equal(lengths, T)
    draws = ctx.rng_draws(B)
    want = [ctx.to_int16(np.ascontiguousarray(y[u, :T[u]])) for u in range(B)]
    stride = int(T.max()) + 3
    for device in (True, False):
        if device:
            buf = torch.full((1 + B * stride + 8,), int(CANARY), dtype=torch.int16, device="cuda")
            out = buf[1:1 + B * stride].view(B, stride)
        else:
            out = np.full((B, stride), CANARY, dtype=np.int16)
        res = ctx.synthesize_ragged(frames, counts, hop, seeds=seeds, out=out, pcm=True, report=True)
        assert np.array_equal(res[1], T)
        grid = out.cpu().numpy() if device else out
        for u in range(B):
            assert np.array_equal(grid[u, :T[u]], want[u]), f"row {u}"
            assert (grid[u, T[u]:] == CANARY).all(), f"row {u}: written past its end"
        if device:
            host = buf.cpu().numpy()
            assert host[0] == CANARY and (host[1 + B * stride:] == CANARY).all()
        assert np.array_equal(res[-1]["nonfinite"], rep["nonfinite"]) and res[-1]["samples"] == rep["samples"] == int(T.sum())
        assert np.array_equal(ctx.rng_draws(B), draws)
    assert (draws > 0).any()


# ---- sessions -----------------------------------------------------------------------------------

CALLS = (1, 2, 33, 441, 50, 1102)
SESSION_FS = 22050.0


def session_frames(oracle, voices):
    key = ("session", voices)
    if key not in _BATCH:
        fr = np.stack([glide_frames(oracle, len(CALLS) + 1, 0.4 + 0.2 * v) for v in range(voices)])
        fr.setflags(write=False)
        _BATCH[key] = fr
    return _BATCH[key]


@pytest.mark.parametrize("voices", [1, 3])
def test_session_stream_equals_two_step(make_ctx, oracle, voices):
    from areafunctionsynthesis_amd.synthesizer import Synthesizer
    ctx = make_ctx(None, fs=SESSION_FS)
    frames = session_frames(oracle, voices)
    seeds = np.arange(5, 5 + voices, dtype=np.uint32)
    s64, s16, smix = (Synthesizer(ctx, voices, seeds) for _ in range(3))
    try:
        assert s64.synthesize_signal_tds(frames[:, 0], 1102).shape == (voices, 0)
        # the latch call: produced == 0, pcm untouched
        pcm = np.full((voices, 1102), CANARY, dtype=np.int16)
        produced = ctypes.c_int32(-1)
        fr0 = np.ascontiguousarray(frames[:, 0])
        st = ctx._lib.afs_session_synthesize_pcm(s16._h, _vp(fr0.ctypes.data), 1102, _vp(pcm.ctypes.data), None,
                                                 ctypes.byref(produced), None)
        assert st == 0 and produced.value == 0 and (pcm == CANARY).all()
        assert smix.synthesize_signal_tds(frames[:, 0], 1102, pcm=True).shape == (voices, 0)
        want, got, mixed = [], [], []
        for k, n in enumerate(CALLS, start=1):
            want.append(ctx.to_int16(np.ascontiguousarray(s64.synthesize_signal_tds(frames[:, k], n))))
            got.append(s16.synthesize_signal_tds(frames[:, k], n, pcm=True))
            if k % 2:
                mixed.append(smix.synthesize_signal_tds(frames[:, k], n, pcm=True))
            else:
                mixed.append(ctx.to_int16(np.ascontiguousarray(smix.synthesize_signal_tds(frames[:, k], n))))
            assert got[-1].shape == (voices, n) and got[-1].dtype == np.int16
        want, got, mixed = (np.concatenate(x, axis=1) for x in (want, got, mixed))
        assert np.abs(want).max() > 100
        assert np.array_equal(got, want)
        assert np.array_equal(mixed, want)
        assert np.array_equal(s16.rng_draws(), s64.rng_draws()) and np.array_equal(smix.rng_draws(), s64.rng_draws())
    finally:
        for s in (s64, s16, smix):
            s.close()


# ---- memory -------------------------------------------------------------------------------------

def test_sample_buffers_do_not_grow_with_the_call(make_ctx, oracle):
    """Device frames and a device pcm, launches of 64 samples, hop 32, B = 11: the fp64 value per
    utterance-sample the library holds after a PCM call is the two launch windows (64 samples rounded up,
    one line of slack each) whether the call has 3 frames or 33; an fp64 call with a host out stages the
    whole call."""
    import torch
    B, hop = 11, 32
    bound = 2 * B * 80 * 8 + 1024
    seen = []
    for F in (3, 33):
        ctx = make_ctx(16, {"AFS_LAUNCH_SAMPLES": "64"}, fresh=True)
        frames = np.stack([glide_frames(oracle, F, 0.3 + 0.05 * u) for u in range(B)])
        dframes = torch.from_numpy(np.ascontiguousarray(frames).view(np.uint8).reshape(B, F, FRAME_DTYPE.itemsize)).cuda()
        T = (F - 1) * hop
        out = torch.zeros((B, T), dtype=torch.int16, device="cuda")
        assert ctx.memory_info()["sample_buffer_bytes"] == 0
        ctx.synthesize(dframes, hop, out=out, pcm=True)
        ctx.synchronize()
        info = ctx.memory_info()
        print(f"PCM call, {F} frames: {info}")
        assert 0 < info["sample_buffer_bytes"] <= bound and info["total_bytes"] > info["sample_buffer_bytes"]
        seen.append(info["sample_buffer_bytes"])
        if F == 33:
            want = ctx.to_int16(ctx.synthesize(frames, hop))
            assert np.array_equal(out.cpu().numpy(), want)
            ctx = make_ctx(16, {"AFS_LAUNCH_SAMPLES": "64"}, fresh=True)
            ctx.synthesize(frames, hop)
            info = ctx.memory_info()
            print(f"fp64 call with a host out, {F} frames: {info}")
            assert info["sample_buffer_bytes"] >= B * T * 8
    assert seen[0] == seen[1]


# ---- refusals -----------------------------------------------------------------------------------

def test_refusals(make_ctx, oracle):
    frames, seeds = uniform_batch(oracle, False)
    B, F = frames.shape
    hop = 33
    T = (F - 1) * hop
    ctx = make_ctx(16)
    lib = ctx._lib
    pcm = np.zeros((B, T), dtype=np.int16)
    args = (_vp(frames.ctypes.data), _vp(seeds.ctypes.data), B, F, hop)
    invalid, unsupported = 1, 5
    assert lib.afs_synthesize_pcm(ctx.handle, *args, _vp(pcm.ctypes.data), T - 1, None, None) == invalid
    assert lib.afs_synthesize_pcm(ctx.handle, *args, None, T, None, None) == invalid
    counts = np.full(B, F, dtype=np.int32)
    rargs = (_vp(frames.ctypes.data), F, _vp(counts.ctypes.data), _vp(seeds.ctypes.data), B, hop)
    assert lib.afs_synthesize_ragged_pcm(ctx.handle, *rargs, _vp(pcm.ctypes.data), T - 1, None, None) == invalid
    assert lib.afs_synthesize_ragged_pcm(ctx.handle, *rargs, None, T, None, None) == invalid
    assert lib.afs_synthesize_pcm(ctx.handle, *args, _vp(pcm.ctypes.data), T, None, None) == 0
    with pytest.raises(ValueError):
        ctx.synthesize(frames, hop, pcm=True, taps=True)
    lane = make_ctx(None, solver="cholesky")
    assert lib.afs_synthesize_pcm(lane.handle, *args, _vp(pcm.ctypes.data), T, None, None) == unsupported
    assert lib.afs_synthesize_ragged_pcm(lane.handle, *rargs, _vp(pcm.ctypes.data), T, None, None) == unsupported
    from areafunctionsynthesis_amd.synthesizer import Synthesizer
    voice = Synthesizer(lane, 1)
    try:
        with pytest.raises(_native.AfsError, match="unsupported"):
            voice.synthesize_signal_tds(frames[0, 0], 10, pcm=True)
    finally:
        voice.close()
