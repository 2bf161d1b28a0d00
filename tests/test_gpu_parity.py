"""GPU parity: the HIP kernels (through the C ABI) against the oracle and the golden
vectors of the reference build.

Two kernels are checked: "cholesky" keeps the reference's operation order (differences only
from device libm: exp for noise cutoffs below the 2 kHz clamp, pow for the aspiration
gain); "tree" solves the same system with an LDL^T in arm order (rounding-level differences,
~1e-12 on the CPU emulator).  Such differences are amplified by the chaotic glottis/tube
dynamics (trap 3).  Bounds used below:
  * golden / oracle, first 2048 samples:   max |err| <= 1e-9
  * oracle, 1 s @ 44.1 kHz (north star):   per-utterance RMS <= 1e-4, reported max-abs
Integer/bookkeeping behaviour (batch independence, session == trajectory, seeds,
latching) is checked bit for bit.
"""
import os

import numpy as np
import pytest

from areafunctionsynthesis_amd.frames import DEFAULT_GLOTTIS, FRAME_DTYPE
from areafunctionsynthesis_amd.params import default_shapes

pytestmark = pytest.mark.gpu

GOLD_TOL = 1e-9
RMS_TOL = 1e-4
# the cooperative kernel (K1) at both lane widths: "tree16" the throughput kernel (16 lanes per
# utterance), "tree64" the voice kernel (64 lanes per utterance); "tree" lets the library pick
TREE_SOLVERS = ("tree16", "tree64")
SOLVERS = ("cholesky",) + TREE_SOLVERS
LANES = {"tree16": 16, "tree64": 64}


@pytest.fixture(scope="module")
def contexts():
    from areafunctionsynthesis_amd.synthesizer import Context
    cache = {}

    def get(fs, solver="cholesky", **opt):
        key = (fs, solver, tuple(sorted(opt.items())))
        if key not in cache:
            if solver in LANES:
                cache[key] = Context(fs, solver="tree", lanes=LANES[solver], **opt)
            else:
                cache[key] = Context(fs, solver=solver, **opt)
        return cache[key]

    yield get
    for c in cache.values():
        c.close()


def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "utterances.npz"), allow_pickle=False)
    return g, g["frames"].view(FRAME_DTYPE)


def static_frames(oracle, name, F, velum=0.0, glottis=DEFAULT_GLOTTIS):
    f = oracle.af_to_frame(default_shapes()[name])
    f["velum_opening_cm2"] = velum
    f["glottis"] = glottis
    return np.repeat(f[None], F)


@pytest.mark.parametrize("solver", SOLVERS)
def test_golden_utterances(contexts, golden_dir, solver):
    g, frames = golden(golden_dir)
    n = g["out"].shape[1]
    for i, name in enumerate(g["names"]):
        fr = frames[i, : g["num_frames"][i]][None]
        ctx = contexts(float(g["fs"][i]), solver)
        y = ctx.synthesize(np.ascontiguousarray(fr), int(g["hop"][i]), seeds=np.array([g["seed"][i]], np.uint32))
        err = np.abs(y[0, :n] - g["out"][i]).max()
        assert err <= GOLD_TOL, (name, err)


@pytest.mark.parametrize("solver", SOLVERS)
def test_golden_per_step_outputs(contexts, golden_dir, solver):
    g = np.load(os.path.join(golden_dir, "steps_a.npz"), allow_pickle=False)
    fr = g["frames"]
    ctx = contexts(float(g["fs"]), solver)
    y = ctx.synthesize(np.ascontiguousarray(fr[None]), 64, seeds=np.array([g["seed"]], np.uint32))
    assert np.abs(y[0] - g["out"]).max() <= GOLD_TOL


@pytest.mark.parametrize("solver", SOLVERS)
def test_batch_vs_oracle_mixed(contexts, oracle, solver):
    """70 utterances (ragged: not a multiple of 64) of mixed vowels, fricatives with an
    open velum and laterality, random glottis settings, vs the oracle."""
    sh = default_shapes()
    names = ["a:", "i:", "u:", "e:", "o:", "s", "f", "x", "S", "(a)b(a):", "l", "C"]
    rng = np.random.default_rng(7)
    B, F, hop, fs = 70, 9, 256, 22050.0
    frames = np.zeros((B, F), FRAME_DTYPE)
    for u in range(B):
        for k in range(F):
            f = oracle.af_to_frame(sh[names[(u + k // 4) % len(names)]] * (1 + 0.01 * rng.standard_normal(16)))
            f["velum_opening_cm2"] = (0.0, 1.0)[u % 2]
            f["laterality"] = np.clip(rng.uniform(-0.5, 0.3, 40), 0, 1) if u % 5 == 0 else 0.0
            f["glottis"] = [rng.uniform(90, 180), rng.uniform(6000, 10000), 0.01, 0.01, 0.0, -40.0 + 20 * (u % 3)]
            frames[u, k] = f
    seeds = np.arange(1, B + 1, dtype=np.uint32)
    y = contexts(fs, solver).synthesize(frames, hop, seeds=seeds)
    for u in range(B):
        x = oracle.utterance(frames[u], hop, int(seeds[u]), fs)
        err = np.abs(y[u] - x).max()
        assert err <= GOLD_TOL, (u, err)


def test_lane_widths(contexts, oracle):
    """The library picks the voice kernel (64 lanes per utterance) for batches up to the GPU's
    SIMD count and the throughput kernel (16) above, unless forced; both widths give the oracle's
    audio (first 2048 samples within GOLD_TOL) on a mixed batch."""
    from areafunctionsynthesis_amd.synthesizer import Context
    auto = Context(22050.0, solver="tree")
    try:
        assert auto.lanes_per_utterance(1) == 64
        assert auto.lanes_per_utterance(1024) == 64  # (MI355X: 256 CUs x 4 SIMDs)
        assert auto.lanes_per_utterance(1025) == 16 and auto.lanes_per_utterance(8192) == 16
    finally:
        auto.close()
    assert contexts(22050.0, "tree16").lanes_per_utterance(1) == 16
    assert contexts(22050.0, "tree64").lanes_per_utterance(8192) == 64
    assert contexts(22050.0, "cholesky").lanes_per_utterance(8) == 1
    frames = np.stack([static_frames(oracle, n, 6, velum=v) for n, v in (("a:", 0.0), ("s", 1.0), ("(a)d(a):", 0.3))])
    seeds = np.array([2, 3, 4], np.uint32)
    y16 = contexts(22050.0, "tree16").synthesize(frames, 410, seeds=seeds)
    y64 = contexts(22050.0, "tree64").synthesize(frames, 410, seeds=seeds)
    for u in range(3):
        x = oracle.utterance(frames[u], 410, int(seeds[u]), 22050.0)
        assert np.abs(y16[u, :2048] - x[:2048]).max() <= GOLD_TOL
        assert np.abs(y64[u, :2048] - x[:2048]).max() <= GOLD_TOL
    assert np.abs(y16 - y64).max() <= 1e-8


@pytest.mark.parametrize("solver", SOLVERS)
def test_batch_independence_bitwise(contexts, oracle, solver):
    """An utterance's audio does not depend on its batch-mates or its slot."""
    ctx = contexts(22050.0, solver)
    a = static_frames(oracle, "a:", 4)
    s = static_frames(oracle, "s", 4, velum=1.0)
    alone = ctx.synthesize(np.ascontiguousarray(s[None]), 128, seeds=np.array([9], np.uint32))
    batch = np.stack([a] * 40 + [s] + [a] * 30)
    seeds = np.arange(1, 72, dtype=np.uint32)
    seeds[40] = 9
    y = ctx.synthesize(batch, 128, seeds=seeds)
    assert np.array_equal(y[40], alone[0])


@pytest.mark.parametrize("solver", SOLVERS)
def test_session_equals_trajectory(contexts, oracle, solver):
    """afs_session_synthesize called frame by frame == afs_synthesize on the whole
    trajectory (Synthesizer::synthesizeSignalTds incremental semantics)."""
    from areafunctionsynthesis_amd.synthesizer import Synthesizer
    ctx = contexts(22050.0, solver)
    sh = default_shapes()
    B, F, hop = 3, 6, 150
    frames = np.zeros((B, F), FRAME_DTYPE)
    for u in range(B):
        for k in range(F):
            f = oracle.af_to_frame(sh[["a:", "(a)d(a):", "i:", "s"][(u + k) % 4]])
            f["glottis"] = [100 + 10 * k, 8000, 0.01, 0.01, 0, -40]
            frames[u, k] = f
    seeds = np.array([3, 4, 5], np.uint32)
    y = ctx.synthesize(frames, hop, seeds=seeds)
    syn = Synthesizer(ctx, B, seeds)
    assert syn.synthesize_signal_tds(frames[:, 0], hop).shape == (B, 0)   # latch only
    parts = [syn.synthesize_signal_tds(frames[:, k], hop) for k in range(1, F)]
    assert np.array_equal(np.concatenate(parts, axis=1), y)
    syn.reset(seeds)
    syn.synthesize_signal_tds(frames[:, 0], hop)
    assert np.array_equal(syn.synthesize_signal_tds(frames[:, 1], hop), y[:, :hop])
    # numNewSamples < 1 produces one sample (Synthesizer.cpp:543-546)
    assert syn.synthesize_signal_tds(frames[:, 2], 0).shape == (B, 1)
    syn.close()


@pytest.mark.parametrize("solver", TREE_SOLVERS)
def test_launch_split_is_bitwise(oracle, solver, monkeypatch):
    """The tree path's launches (one per second of audio by default; AFS_LAUNCH_SAMPLES lowers it)
    carry the lane and LDS state, the hop records and the frame cache across their boundaries: a
    call split into launches of 1000 samples -- boundaries inside hops of 441 -- gives the same
    audio bit for bit, static vowels and fricatives with their noise sources.  So do launches of 999
    samples (odd: the wave pairs' displacement double buffer ends each launch in its second half)
    and of 17 (odd, below the hop records' minimum hop and one more than an output line)."""
    from areafunctionsynthesis_amd.synthesizer import Context
    frames = np.stack([static_frames(oracle, v, 12, velum=vel)
                       for v, vel in (("a:", 0.0), ("s", 1.0), ("i:", 0.0), ("S", 0.0), ("u:", 0.5))])
    seeds = np.arange(7, 7 + len(frames), dtype=np.uint32)
    ys = []
    for env in (None, "1000", "999", "17"):
        if env is None:
            monkeypatch.delenv("AFS_LAUNCH_SAMPLES", raising=False)
        else:
            monkeypatch.setenv("AFS_LAUNCH_SAMPLES", env)
        ctx = Context(44100.0, solver="tree", lanes=LANES[solver], profile=True)
        try:
            ys.append(ctx.synthesize(frames, 441, seeds=seeds))
            kt = ctx.kernel_times()
        finally:
            ctx.close()
        assert kt["synth_launches"] == (1 if env is None else -(-11 * 441 // int(env)))
    assert np.array_equal(ys[0], ys[1])
    assert np.isfinite(ys[0]).all()
    for y, env in zip(ys[2:], ("999", "17")):
        assert np.array_equal(ys[0], y), (env, float(np.abs(ys[0] - y).max()))


def test_plan_budget_chunked_hop_mode(oracle, monkeypatch):
    """The hop-mode fallback for calls whose plans exceed the budget (AFS_PLAN_BUDGET_MB): launches
    of whole hops, each with its own K5 pass and the compact dense records of its listed hops sized
    for the worst case (every hop of the chunk listed).  Frame-rate VCV trajectories list and mix
    many hops.  Chunks of whole hops decide every hop exactly as the single call does: bit for bit
    equal.  Chunks that start inside hops (AFS_LAUNCH_SAMPLES=300 with hop 441) decide partial hops,
    so a hop mixed in the whole call may be uniform in a part (hop-record words instead of dense
    records: a few ulps), checked against the single call within 1e-7 (as hop vs dense records)."""
    from areafunctionsynthesis_amd.synthesizer import Context
    from areafunctionsynthesis_amd.workloads import build_frames, vcv
    w = vcv(64, fs=44100.0)
    ys = {}
    for label, env in (("single", {}), ("chunks", {"AFS_PLAN_BUDGET_MB": "1"}),
                       ("straddle", {"AFS_PLAN_BUDGET_MB": "1", "AFS_LAUNCH_SAMPLES": "300"})):
        for k in ("AFS_PLAN_BUDGET_MB", "AFS_LAUNCH_SAMPLES"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = Context(44100.0, solver="tree", lanes=16, profile=True)
        try:
            frames = build_frames(w, ctx.af_to_frames)
            if label == "single":
                hops, _ = ctx.noise_plan_hops(frames, w.hop)
                mixed = int(np.count_nonzero(hops[..., 528:532].view(np.uint32)))
                assert mixed > 0
            ys[label] = ctx.synthesize(frames, w.hop, seeds=w.seeds)
            kt = ctx.kernel_times()
        finally:
            ctx.close()
        T = (w.num_frames - 1) * w.hop
        assert kt["synth_launches"] == {"single": 1, "chunks": T // w.hop, "straddle": -(-T // 300)}[label]
    assert np.isfinite(ys["single"]).all()
    assert np.array_equal(ys["chunks"], ys["single"])
    assert np.abs(ys["straddle"] - ys["single"]).max() < 1e-7


@pytest.mark.parametrize("solver", TREE_SOLVERS)
def test_noise_variants_are_bitwise(oracle, solver, monkeypatch):
    """K1 runs each wave's launch in the lightest noise-phase variant its hop records allow
    (tree_core.h NoiseV: the glottis source alone, glottis + first tongue constriction below dipole
    32, or all).  The variants compute the full phases' values: the audio and the rand() call counts
    equal those of the full phases (AFS_NOISE_VARIANTS=0) bit for bit -- static vowels (most waves
    in a light variant), fricatives with their tongue and lip sources, frame-rate VCV trajectories
    (constrictions forming within a launch), and launches of 1000 samples (a dipole's amplitude
    decaying across a launch boundary keeps its slot in the heavier variant).  (AFS_NOISE_VARIANTS=2
    forces the variants; by default a call uses them when most of its batch is light.)"""
    from areafunctionsynthesis_amd.synthesizer import Context
    from areafunctionsynthesis_amd.workloads import build_frames, fricatives, static_vowels, vcv
    cases = [("static", static_vowels(48, seconds=0.25)), ("fricatives", fricatives(40, seconds=0.25, velum_cm2=1.0)),
             ("vcv", vcv(32))]
    for label, w in cases:
        for launch in (None, "1000"):
            ys, draws = [], []
            for env in ("0", "2"):  # (2: the variants for every call, whatever the batch's mix)
                monkeypatch.setenv("AFS_NOISE_VARIANTS", env)
                if launch is None:
                    monkeypatch.delenv("AFS_LAUNCH_SAMPLES", raising=False)
                else:
                    monkeypatch.setenv("AFS_LAUNCH_SAMPLES", launch)
                ctx = Context(44100.0, solver="tree", lanes=LANES[solver])
                try:
                    frames = build_frames(w, ctx.af_to_frames)
                    ys.append(ctx.synthesize(frames, w.hop, seeds=w.seeds))
                    draws.append(ctx.rng_draws(w.batch))
                finally:
                    ctx.close()
            assert np.isfinite(ys[0]).all(), label
            assert np.array_equal(ys[0], ys[1]), (label, launch)
            assert np.array_equal(draws[0], draws[1]), (label, launch)


def test_slot_order_is_invisible(oracle, monkeypatch):
    """afs_synthesize places a batch's utterances in the 16-lane kernel's slots sorted by the shape
    of their first frame (afs_capi.cpp shape_order); each utterance's audio is the same wherever it
    runs: a permuted batch gives the permuted audio bit for bit, and so does the call order
    (AFS_SHAPE_ORDER=0)."""
    from areafunctionsynthesis_amd.synthesizer import Context
    names = ("a:", "i:", "s", "u:", "S", "e:", "f", "o:")
    B = 40  # (three blocks of 16 utterances)
    frames = np.stack([static_frames(oracle, names[u % len(names)], 4, velum=0.5 * (u % 3 == 0)) for u in range(B)])
    seeds = np.arange(100, 100 + B, dtype=np.uint32)
    perm = np.random.default_rng(5).permutation(B)
    ys = {}
    for env in ("1", "0"):
        monkeypatch.setenv("AFS_SHAPE_ORDER", env)
        ctx = Context(44100.0, solver="tree", lanes=16)
        try:
            ys[env] = ctx.synthesize(frames, 441, seeds=seeds)
            yp = ctx.synthesize(np.ascontiguousarray(frames[perm]), 441, seeds=seeds[perm])
        finally:
            ctx.close()
        assert np.array_equal(yp, ys[env][perm])
    assert np.array_equal(ys["1"], ys["0"])
    assert np.isfinite(ys["1"]).all()


@pytest.mark.parametrize("solver", SOLVERS)
def test_edge_cases(contexts, oracle, solver):
    ctx = contexts(44100.0, solver)
    fr = static_frames(oracle, "u:", 2)
    # hop = 1, two frames, single utterance
    y = ctx.synthesize(np.ascontiguousarray(fr[None]), 1, seeds=np.array([1], np.uint32))
    assert y.shape == (1, 1)
    assert np.abs(y[0] - oracle.utterance(fr, 1, 1, 44100.0)).max() <= GOLD_TOL
    # seed 0 behaves as glibc's srand(0) == srand(1)
    s = static_frames(oracle, "s", 3, velum=1.0)
    y0 = ctx.synthesize(np.ascontiguousarray(s[None]), 300, seeds=np.array([0], np.uint32))
    y1 = ctx.synthesize(np.ascontiguousarray(s[None]), 300, seeds=np.array([1], np.uint32))
    assert np.array_equal(y0, y1)
    # invalid arguments are rejected with a status, not a crash
    from areafunctionsynthesis_amd._native import AfsError
    with pytest.raises(AfsError):
        ctx.synthesize(np.ascontiguousarray(fr[None][:, :1]), 10)


@pytest.mark.parametrize("solver", SOLVERS)
def test_nonfinite_is_reported(contexts, oracle, solver):
    """The reference keeps going after a non-finite value (it prints "matrix is not positive
    definite" and continues, TdsModel.cpp:2267); the library reproduces the NaN audio and flags
    exactly the affected utterances of a mixed batch (afs_synthesize's nonfinite array)."""
    ctx = contexts(22050.0, solver)
    sh = default_shapes()
    B, F, hop = 9, 4, 120
    frames = np.zeros((B, F), FRAME_DTYPE)
    for u in range(B):
        f = oracle.af_to_frame(sh[("a:", "s", "i:")[u % 3]])
        f["glottis"] = DEFAULT_GLOTTIS
        frames[u] = np.repeat(f[None], F)
    bad = [2, 5, 6]
    frames["area_cm2"][2, 2, 10] = np.nan      # a NaN section area from the second transition on
    frames["glottis"][5, 1:, 1] = np.nan       # a NaN lung pressure
    frames["length_cm"][6, 3, 30] = np.inf     # an infinite section length in the last frame
    seeds = np.arange(1, B + 1, dtype=np.uint32)
    x = np.stack([oracle.utterance(frames[u], hop, int(seeds[u]), 22050.0) for u in range(B)])
    assert [u for u in range(B) if not np.isfinite(x[u]).all()] == bad  # the fixture really goes non-finite
    y, rep = ctx.synthesize(frames, hop, seeds=seeds, report=True)
    assert list(np.flatnonzero(rep["nonfinite"])) == bad
    assert rep["nonfinite_utterances"] == len(bad)
    for u in range(B):
        assert np.array_equal(np.isfinite(y[u]), np.isfinite(x[u])), u
        if u not in bad:
            assert np.abs(y[u] - x[u]).max() <= GOLD_TOL
    # device-resident flag array, no report
    import torch
    flags = torch.zeros(B, dtype=torch.uint8, device="cuda")
    ctx.synthesize(frames, hop, seeds=seeds, nonfinite=flags)
    assert list(np.flatnonzero(flags.cpu().numpy())) == bad


@pytest.mark.parametrize("solver", SOLVERS)
def test_null_seeds_are_u_plus_1(contexts, oracle, solver):
    """A NULL seed array seeds utterance / voice u with u + 1 (afs.h): identical fricative
    frames give distinct noise, equal to explicit seeds 1..B."""
    import ctypes
    from areafunctionsynthesis_amd import _native
    ctx = contexts(22050.0, solver)
    B, F, hop = 5, 3, 200
    fr = np.ascontiguousarray(np.stack([static_frames(oracle, "s", F, velum=1.0)] * B))
    ref = ctx.synthesize(fr, hop, seeds=np.arange(1, B + 1, dtype=np.uint32))
    out = np.zeros((B, (F - 1) * hop))
    lib = ctx._lib
    _native.check(lib.afs_synthesize(ctx.handle, fr.ctypes.data, None, B, F, hop, out.ctypes.data, None, None),
                  ctx.handle, "afs_synthesize")
    assert np.array_equal(out, ref)
    assert not np.array_equal(out[0], out[1])
    # sessions: afs_session_create / reset with NULL seeds
    h = ctypes.c_void_p()
    _native.check(lib.afs_session_create(ctx.handle, B, None, ctypes.byref(h)), ctx.handle, "afs_session_create")
    try:
        got = []
        for k in range(F):
            o = np.zeros((B, hop))
            n = ctypes.c_int32(0)
            fk = np.ascontiguousarray(fr[:, k])  # (kept alive over the call)
            _native.check(lib.afs_session_synthesize(h, fk.ctypes.data, hop, o.ctypes.data, None, ctypes.byref(n),
                                                     None), ctx.handle, "session")
            got.append(o[:, : n.value])
        assert np.array_equal(np.concatenate(got, axis=1), ref)
    finally:
        lib.afs_session_destroy(h)


@pytest.mark.parametrize("solver", SOLVERS)
def test_long_utterance_chunked_launches(contexts, oracle, solver):
    """An utterance longer than one kernel launch (state carried across launches)."""
    ctx = contexts(22050.0, solver)
    f = oracle.af_to_frame(default_shapes()["i:"])
    f["glottis"] = DEFAULT_GLOTTIS
    fr = np.repeat(f[None], 160)
    fr["glottis"][:, 0] = np.linspace(100, 140, 160)
    y = ctx.synthesize(np.ascontiguousarray(fr[None]), 441, seeds=np.array([5], np.uint32))
    x = oracle.utterance(fr, 441, 5, 22050.0)
    assert y.shape[1] == 159 * 441 > 65536
    assert float(np.sqrt(np.mean((y[0] - x) ** 2))) < RMS_TOL


def test_af_to_frames_vs_restatement(contexts, golden_dir):
    g = np.load(os.path.join(golden_dir, "af_frames.npz"), allow_pickle=False)
    fr = contexts(22050.0).af_to_frames(g["params"])
    assert np.array_equal(fr["articulator"], g["articulator"])
    assert np.array_equal(fr["length_cm"], g["length"])
    assert np.array_equal(fr["teeth_position_cm"], g["teeth"])
    assert np.allclose(fr["area_cm2"], g["area"], rtol=1e-12, atol=1e-14)


def _full_length_check(ctx, w, frames, stride, parity_report, label, solver):
    """Synthesize the whole batch on the GPU, re-synthesize every `stride`-th utterance with the
    oracle (worker processes) and check the north-star bound per utterance; record the RMS
    distribution and the rand() call-count comparison (a noise source that switched on or off
    at a different sample than in the reference changes the count, TdsModel.cpp:1647-1666)."""
    from oracle_lib import oracle_parallel
    B = frames.shape[0]
    y, rep = ctx.synthesize(frames, w.hop, seeds=w.seeds, report=True)
    assert rep["nonfinite_utterances"] == 0
    idx = np.arange(0, B, stride)
    x, draws = oracle_parallel(frames[idx], w.hop, w.seeds[idx], w.fs)
    err = y[idx] - x
    rms = np.sqrt(np.mean(err ** 2, axis=1))
    mx = np.abs(err).max(axis=1)
    flips = None
    if solver in TREE_SOLVERS or solver == "tree":
        gd = ctx.rng_draws(B)[idx]
        flips = int(np.count_nonzero(gd != draws))
    parity_report.append(
        f"{label} [{solver}]: {len(idx)}/{B} utterances x {y.shape[1]} samples vs oracle: per-utterance RMS "
        f"max {rms.max():.2e} p99 {np.percentile(rms, 99):.2e} median {np.median(rms):.2e}; max |err| {mx.max():.2e}; "
        f"pass (RMS < {RMS_TOL:g}) {int(np.count_nonzero(rms < RMS_TOL))}/{len(idx)}; rand() call counts differing "
        f"from the oracle: {flips if flips is not None else 'n/a (lane solver)'} (oracle total {int(draws.sum())})")
    for k, u in enumerate(idx):
        assert rms[k] < RMS_TOL, (int(u), float(rms[k]), float(mx[k]))
    if flips is not None:
        assert flips == 0
    return y


@pytest.mark.parametrize("solver", SOLVERS)
def test_full_second_static_vowels_rms(contexts, solver, parity_report):
    """Config 2 at full length: 1024 utterances x 1 s @ 44.1 kHz on the GPU; every 16th
    utterance (64) re-synthesised by the oracle.  North-star bound: RMS < 1e-4 per utterance."""
    from areafunctionsynthesis_amd.workloads import build_frames, static_vowels
    ctx = contexts(44100.0, solver)
    w = static_vowels(1024, seconds=1.0, fs=44100.0)
    frames = build_frames(w, ctx.af_to_frames)
    y = _full_length_check(ctx, w, frames, 16, parity_report, "config 2 (static vowels, 1 s @ 44.1 kHz)", solver)
    # deterministic: a second run is bitwise identical
    y2 = ctx.synthesize(frames, w.hop, seeds=w.seeds)
    assert np.array_equal(y, y2)


@pytest.mark.parametrize("solver", TREE_SOLVERS)
def test_full_second_fricatives_config5(contexts, parity_report, solver):
    """Config 5 at its defined length: fricatives s f z S Z x C R v (Default.params:44-52) with the
    velum open 1.0 cm^2 (MainPage.cpp:127-131), 1 s @ 44.1 kHz, noise sources active; 512
    utterances on the GPU, every 8th (64) against the oracle over the whole second, with the
    rand() call counts compared utterance by utterance."""
    from areafunctionsynthesis_amd.workloads import build_frames, fricatives
    ctx = contexts(44100.0, solver)
    w = fricatives(512, seconds=1.0, fs=44100.0, velum_cm2=1.0)
    frames = build_frames(w, ctx.af_to_frames)
    _full_length_check(ctx, w, frames, 8, parity_report, "config 5 (fricatives + velum 1.0 cm^2, 1 s @ 44.1 kHz)",
                       solver)


def test_frame_rate_vcv_hop_records(contexts, parity_report, monkeypatch):
    """Hop records (K5's hop mode, tree solver, hops >= 32) on frame-rate VCV trajectories
    (workloads.vcv: hop 441, the constrictions form and release inside hops, so hops with one
    decision and mixed hops -- which read dense records -- both occur): against the oracle over
    the whole utterance with the rand() call counts, and against the dense-record kernel
    (AFS_PLAN_DENSE=1)."""
    from areafunctionsynthesis_amd.synthesizer import Context
    from areafunctionsynthesis_amd.workloads import build_frames, vcv
    ctx = contexts(44100.0, "tree")
    w = vcv(256, fs=44100.0)
    frames = build_frames(w, ctx.af_to_frames)
    hops, _ = ctx.noise_plan_hops(frames, w.hop)
    mixed = int(np.count_nonzero(hops[..., 528:532].view(np.uint32)))
    assert 0 < mixed < hops.shape[0] * hops.shape[1]
    y = _full_length_check(ctx, w, frames, 4, parity_report, "frame-rate VCV (hop 441, hop records)", "tree")
    monkeypatch.setenv("AFS_PLAN_DENSE", "1")
    dense = Context(44100.0, solver="tree")
    try:
        yd = dense.synthesize(frames, w.hop, seeds=w.seeds)
    finally:
        dense.close()
    diff = np.abs(y - yd).max()
    parity_report.append(f"hop records vs dense records [tree] (frame-rate VCV, {w.batch} utterances, "
                         f"{mixed}/{hops.shape[0] * hops.shape[1]} hops mixed): max |diff| {diff:.2e}")
    assert diff < 1e-7


@pytest.mark.parametrize("solver", TREE_SOLVERS)
def test_full_length_vcv_config3(contexts, parity_report, solver):
    """Config 3 at the reference's playTargetSequence timing (stationary 0.2/0.05/0.2/0.1 s,
    transitions 0.05 s: 30870 samples @ 44.1 kHz): 512 VCV utterances (V, (V)C(V):, V, V over
    the 15 vowel-consonant pairs, Synthesizer.cpp:1299-1422) through afs_play_target_sequences,
    every 8th (64) against the oracle over the whole utterance, with the rand() call counts
    compared utterance by utterance (TdsModel.cpp:1647-1666)."""
    from oracle_lib import oracle_target_parallel
    from areafunctionsynthesis_amd.workloads import vcv_targets
    ctx = contexts(44100.0, solver)
    B = 512
    shapes, targets, seeds = vcv_targets(B)
    y, rep = ctx.play_target_sequences(shapes, targets, seeds=seeds, report=True)
    assert y.shape == (B, 30870)
    assert rep["nonfinite_utterances"] == 0
    idx = np.arange(0, B, 8)
    x, draws = oracle_target_parallel(shapes[targets[idx]], seeds[idx], 44100.0)
    err = y[idx] - x
    rms = np.sqrt(np.mean(err ** 2, axis=1))
    mx = np.abs(err).max(axis=1)
    gd = ctx.rng_draws(B)[idx]
    flips = int(np.count_nonzero(gd != draws))
    parity_report.append(
        f"config 3 (VCV playTargetSequence, 30870 samples @ 44.1 kHz) [{solver}]: {len(idx)}/{B} utterances vs "
        f"oracle: per-utterance RMS max {rms.max():.2e} p99 {np.percentile(rms, 99):.2e} median {np.median(rms):.2e}; "
        f"max |err| {mx.max():.2e}; pass (RMS < {RMS_TOL:g}) {int(np.count_nonzero(rms < RMS_TOL))}/{len(idx)}; "
        f"rand() call counts differing from the oracle: {flips} (oracle total {int(draws.sum())})")
    for k, u in enumerate(idx):
        assert rms[k] < RMS_TOL, (int(u), float(rms[k]), float(mx[k]))
    assert flips == 0


OPTION_VARIANTS = [
    {"turbulence_losses": 0}, {"soft_walls": 0}, {"generate_noise_sources": 0},
    {"radiation_from_skin": 0}, {"piriform_fossa": 1}, {"inner_length_corrections": 0},
    {"turbulence_losses": 0, "soft_walls": 0, "generate_noise_sources": 0, "radiation_from_skin": 0,
     "piriform_fossa": 1, "inner_length_corrections": 0},
    {"transvelar_coupling": 1}, {"glottis_loss": 1}, {"glottis_loss": 2}, {"flow_separation_area_ratio": 1.2},
    {"transvelar_coupling": 1, "glottis_loss": 2, "piriform_fossa": 1},
]


@pytest.mark.parametrize("solver", SOLVERS)
def test_options_vs_oracle(contexts, oracle, solver):
    """TdsModel::Options variants (afs_options) on the GPU against the oracle (which is
    pinned to the reference build for the same variants in test_oracle.py)."""
    sh = default_shapes()
    f = oracle.af_to_frame(sh["s"])
    f["velum_opening_cm2"] = 0.6
    f["glottis"] = DEFAULT_GLOTTIS
    g = oracle.af_to_frame(sh["(a)b(a):"])
    g["velum_opening_cm2"] = 0.2
    g["glottis"] = [140.0, 9000.0, 0.01, 0.02, 0.0, -20.0]
    frames = np.stack([f, f, g, g, f])
    for opt in OPTION_VARIANTS:
        ctx = contexts(22050.0, solver, **opt)
        y = ctx.synthesize(np.ascontiguousarray(frames[None]), 150, seeds=np.array([3], np.uint32))
        x = oracle.utterance(frames, 150, 3, 22050.0, opt=opt)
        assert np.abs(y[0] - x).max() <= GOLD_TOL, (opt, float(np.abs(y[0] - x).max()))


@pytest.mark.parametrize("opt", [{}, {"glottis_loss": 2, "transvelar_coupling": 1}, {"piriform_fossa": 1}],
                         ids=["default", "variable_loss+transvelar", "fossa"])
def test_sor_solver_vs_oracle(contexts, oracle, opt):
    """TdsModel::SOR_GAUSS_SEIDEL (afs_solver AFS_SOLVER_SOR, lane kernel) against the oracle's
    SOR, which test_oracle.py pins bit-exactly to the reference build."""
    sh = default_shapes()
    f = oracle.af_to_frame(sh["a:"])
    f["velum_opening_cm2"] = 0.3
    f["glottis"] = DEFAULT_GLOTTIS
    g = oracle.af_to_frame(sh["s"])
    g["velum_opening_cm2"] = 0.3
    g["glottis"] = [130.0, 9000.0, 0.01, 0.02, 0.0, -25.0]
    frames = np.stack([f, g, g, f, f])
    for fs, hop in ((22050.0, 150), (44100.0, 441)):
        ctx = contexts(fs, "sor", **opt)
        y = ctx.synthesize(np.ascontiguousarray(frames[None]), hop, seeds=np.array([9], np.uint32))
        x = oracle.utterance(frames, hop, 9, fs, opt=dict(opt, solver=1))
        assert np.abs(y[0, :2048] - x[:2048]).max() <= GOLD_TOL, (fs, float(np.abs(y[0] - x).max()))
        assert float(np.sqrt(np.mean((y[0] - x) ** 2))) < RMS_TOL
        # SOR's coarse residual bound makes it a different solution from the Cholesky's
        z = oracle.utterance(frames, hop, 9, fs, opt=opt)
        assert not np.array_equal(x, z)


@pytest.mark.parametrize("solver", SOLVERS + ("sor",))
def test_two_mass_glottis_vs_oracle(contexts, oracle, solver):
    """afs_options.glottis_model = AFS_GLOTTIS_TWO_MASS (TwoMassModel.cpp; control 5 is the
    damping factor) against the oracle, which test_oracle.py pins to the reference's own
    TwoMassModel bit for bit."""
    sh = default_shapes()
    f = oracle.af_to_frame(sh["a:"])
    f["glottis"] = [120.0, 8000.0, 0.01, 0.01, 0.0, 1.0]
    g = oracle.af_to_frame(sh["i:"])
    g["velum_opening_cm2"] = 0.3
    g["glottis"] = [160.0, 9000.0, 0.02, -0.01, 0.02, 1.5]
    frames = np.stack([f, f, g, g, f])
    for fs, hop in ((22050.0, 220), (44100.0, 441)):
        ctx = contexts(fs, solver, glottis_model=1)
        y = ctx.synthesize(np.ascontiguousarray(frames[None]), hop, seeds=np.array([4], np.uint32))
        x = oracle.utterance(frames, hop, 4, fs, opt={"glottis_model": 1, "solver": int(solver == "sor")})
        assert np.abs(x).max() > 1e-4
        assert np.abs(y[0, :2048] - x[:2048]).max() <= GOLD_TOL, (fs, float(np.abs(y[0] - x).max()))
        assert float(np.sqrt(np.mean((y[0] - x) ** 2))) < RMS_TOL
