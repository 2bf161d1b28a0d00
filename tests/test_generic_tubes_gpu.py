"""The HIP kernels on tubes the area-function model cannot make (tests/generic_tubes.py: unequal section
lengths, tongue runs broken by other articulators, teeth anywhere, lengths that change from frame to
frame): the synthesis kernels at both lane widths and the lane solver against the reference build's
recorded audio and the oracle, K5's records word by word against the host restatement, the tube
interpolation bit for bit, and what must not depend on slots, launches, sessions or the output format.

Bounds: GOLD_TOL = 1e-9 over the first 2048 samples and RMS_TOL against the oracle, as in
test_gpu_parity.py; the rand() call counts and everything between two GPU paths bit for bit; the plan
words with test_plan_gpu.py's comparisons (plan_lib.py); the taps with taps_lib.TAP_TOL."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import generic_tubes as gt
from oracle_lib import CALL_SCHEDULE
from plan_lib import HOP_DTYPE, PLAN_WORDS, PW_GAIN_G, _compare, _compare_hop_words, _compare_hops

pytestmark = pytest.mark.gpu

GOLD_TOL = 1e-9
RMS_TOL = 1e-4
FS, HOP = 22050.0, 97
TREE_SOLVERS = ("tree16", "tree64")
SOLVERS = ("cholesky",) + TREE_SOLVERS
LANES = {"tree16": 16, "tree64": 64}
EMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


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


_CACHE = {}


def the_set(oracle):
    """(labels, frames[28, 6], seeds) of generic_tubes.generic_set, built once and left unchanged."""
    if "set" not in _CACHE:
        labels, frames, seeds = gt.generic_set(oracle)
        frames.setflags(write=False)
        _CACHE["set"] = (labels, frames, seeds)
    return _CACHE["set"]


def oracle_rows(oracle, frames, hop, seeds, fs, opt=None):
    """(audio[rows, T], rand() calls[rows]) of the oracle's incremental calls; computed once per input."""
    key = (frames.tobytes(), hop, tuple(int(s) for s in seeds), fs, tuple(sorted((opt or {}).items())))
    if key not in _CACHE:
        xs, ds = [], []
        for r in range(frames.shape[0]):
            h = oracle.create(fs, int(seeds[r]), opt)
            try:
                xs.append(np.concatenate([oracle.call(h, frames[r, k], hop) for k in range(frames.shape[1])]))
                ds.append(oracle.rng_calls(h))
            finally:
                oracle.destroy(h)
        _CACHE[key] = (np.stack(xs), np.array(ds, dtype=np.int64))
    return _CACHE[key]


def check_vs_oracle(ctx, oracle, labels, frames, seeds, solver, opt=None, report=None, what=""):
    frames = np.ascontiguousarray(frames)
    x, draws = oracle_rows(oracle, frames, HOP, seeds, FS, opt)
    y = ctx.synthesize(frames, HOP, seeds=seeds)
    assert np.isfinite(y).all()
    err = np.abs(y[:, :2048] - x[:, :2048]).max(axis=1)
    rms = np.sqrt(np.mean((y - x) ** 2, axis=1))
    fams = [gt.family_of(label) for label in labels]
    for fam in dict.fromkeys(fams):
        m = np.array([f == fam for f in fams])
        line = f"generic tubes{what} [{solver}] {fam}: {int(m.sum())} utterances, max |gpu - oracle| {err[m].max():.2e}"
        print(line)
        if report is not None:
            report.append(line)
    for r, label in enumerate(labels):
        assert err[r] <= GOLD_TOL, (label, float(err[r]))
        assert rms[r] < RMS_TOL, (label, float(rms[r]))
    if solver in TREE_SOLVERS:
        got = ctx.rng_draws(frames.shape[0])
        assert np.array_equal(got, draws), [(labels[r], int(got[r]), int(draws[r])) for r in np.flatnonzero(got != draws)]


# --- audio ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("solver", SOLVERS)
def test_golden(contexts, golden_dir, solver):
    """The reference build's recorded audio (golden/generic_tubes.npz: both rates, hops 33 / 97 / 441) and,
    for the tree kernels, its rand() call counts."""
    gold = gt.load_golden(golden_dir)
    for fs, hop in sorted({(g[4], g[2]) for g in gold}):  # (one call per rate and hop: the lane solver's rows run side by side)
        rows = [g for g in gold if (g[4], g[2]) == (fs, hop)]
        ctx = contexts(fs, solver)
        frames = np.ascontiguousarray(np.stack([g[1] for g in rows]))
        y = ctx.synthesize(frames, hop, seeds=np.array([g[3] for g in rows], np.uint32))
        draws = ctx.rng_draws(len(rows)) if solver in TREE_SOLVERS else None
        for r, (label, _, _, _, _, want, calls) in enumerate(rows):
            err = float(np.abs(y[r, : want.size] - want).max())
            print(f"{solver} {label} hop {hop} fs {fs:.0f}: max |gpu - reference| {err:.2e}")
            assert err <= GOLD_TOL, (label, err)
            if draws is not None:
                assert int(draws[r]) == calls, label


@pytest.mark.parametrize("solver", SOLVERS)
def test_whole_set_vs_oracle(contexts, oracle, parity_report, solver):
    """Every family (4 utterances each) and the edge cases at hop 97, 22.05 kHz, in one batch of 28."""
    labels, frames, seeds = the_set(oracle)
    check_vs_oracle(contexts(FS, solver), oracle, labels, frames, seeds, solver, report=parity_report)


@pytest.mark.parametrize("opt", [{"inner_length_corrections": 0}, {"glottis_model": 1}],
                         ids=["inner_length_corrections=0", "glottis_model=1"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_options(contexts, oracle, solver, opt):
    """`breathing` (one utterance of each other family with its lengths changing per frame) without the
    inner length corrections (the per-section lengths alone) and with the two-mass glottis."""
    fam = gt.family(oracle, "breathing")
    if opt.get("glottis_model"):
        fam = gt.two_mass(fam)
    labels = [f"breathing{u}" for u in range(fam.shape[0])]
    check_vs_oracle(contexts(FS, solver, **opt), oracle, labels, fam, np.arange(61, 61 + fam.shape[0], dtype=np.uint32),
                    solver, opt=opt, what=f" {opt}")


def test_tube_interpolate_between_unequal_lengths(contexts, oracle):
    """K1's frame_load + phase_interpolate on `breathing` pairs, whose left and right lengths differ in
    every section: bit for bit the uncontracted r1 * a + ratio * b (Tube::interpolate) at every ratio of
    hop 97 and random ones."""
    fam = gt.family(oracle, "breathing", 8)
    rng = np.random.default_rng(9)
    left = np.ascontiguousarray(fam[:, :-1]).reshape(-1)
    right = np.ascontiguousarray(fam[:, 1:]).reshape(-1)
    assert (left["length_cm"] != right["length_cm"]).all()
    reps = HOP + 3
    ratio = np.tile(np.concatenate([np.arange(HOP) / HOP, rng.random(3)]), left.size)
    left, right = np.repeat(left, reps), np.repeat(right, reps)
    area, length = contexts(FS, "tree16").tube_interpolate(left, right, ratio)
    amin = 0.001
    aL, aR = np.maximum(left["area_cm2"], amin), np.maximum(right["area_cm2"], amin)
    r1, r = (1.0 - ratio)[:, None], ratio[:, None]
    a_ref = r1 * aL + r * aR  # numpy rounds each product: no fma
    a_ref = np.where(a_ref < amin, amin, a_ref)
    l_ref = r1 * left["length_cm"] + r * right["length_cm"]
    assert np.array_equal(area, a_ref), int(np.count_nonzero(area != a_ref))
    assert np.array_equal(length, l_ref), int(np.count_nonzero(length != l_ref))
    ld = np.longdouble  # (the check has teeth on the lengths: a contracted fma rounds some of them differently)
    l_fma = (r1.astype(ld) * left["length_cm"].astype(ld) + (r * right["length_cm"]).astype(ld)).astype(np.float64)
    assert np.count_nonzero(l_fma != l_ref) > 0


# --- K5 --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host():
    if not os.path.exists(os.path.join(EMU, "libplan_emu.so")):
        subprocess.check_call(["make", "-s", "-C", EMU])
    lib = ctypes.CDLL(os.path.join(EMU, "libplan_emu.so"))
    vp = ctypes.c_void_p
    sig = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_long, ctypes.c_double, ctypes.c_int, vp]
    lib.emu_plan_records.restype = lib.emu_plan_hops.restype = ctypes.c_int
    lib.emu_plan_records.argtypes = lib.emu_plan_hops.argtypes = sig

    def plans(frames, hop, s0, s1, fs, two_mass):
        frames = np.ascontiguousarray(frames)
        rows, F = frames.shape
        out = np.zeros((rows, s1 - s0, PLAN_WORDS), dtype=np.uint64)
        assert lib.emu_plan_records(frames.ctypes.data, rows, F, hop, s0, s1, fs, int(two_mass), out.ctypes.data) == 0
        return out

    def hops(frames, hop, s0, s1, fs, two_mass):
        frames = np.ascontiguousarray(frames)
        rows, F = frames.shape
        out = np.zeros((rows, (s1 - 1) // hop - s0 // hop + 1), dtype=HOP_DTYPE)
        assert lib.emu_plan_hops(frames.ctypes.data, rows, F, hop, s0, s1, fs, int(two_mass), out.ctypes.data) == 0
        return out
    return plans, hops


def default_aspiration(frames):
    """The frames with the aspiration strength at the -40 dB of the other plan tests.  _compare holds the
    glottis gain word, 0.5e-7 * 10^(dB / 20) from the device's pow, to 1 ulp of glibc's, which is what the
    two give at -40 dB; at some of the set's other strengths (-36 .. -28 dB) they are 2 ulps apart.  The
    library's claim for the gain is 1e-13 relative (README; test_device_math_gpu.py over -100 .. 40 dB),
    which check_gain_words asserts on the set's own strengths."""
    out = frames.copy()
    out["glottis"][..., 5] = -40.0
    return out


def check_gain_words(gpu, host_records, label):
    g, h = gpu[..., PW_GAIN_G].view(np.float64), host_records[..., PW_GAIN_G].view(np.float64)
    rel = float((np.abs(g - h) / h).max())
    print(f"{label}: glottis gain, device pow vs glibc: {rel:.2e} relative")
    assert rel <= 1e-13, (label, rel)
    other = np.arange(PLAN_WORDS) != PW_GAIN_G
    assert np.array_equal(gpu[..., other], host_records[..., other]), label


def test_plan_records_word_by_word(contexts, oracle, host):
    """K5's dense records against plan_sample on the host: a `scrambled` trajectory expanded to one frame
    per sample (hop 1: the global-memory path; constrictions at 12 and 30 swapping roles, the third at the
    lips) and the whole set at hop 97 (the frames staged in LDS)."""
    plans, _ = host
    ctx = contexts(FS, "tree16")
    fam = gt.family(oracle, "scrambled", 3)
    own = np.ascontiguousarray(np.stack([gt.per_sample(fam[u], 60) for u in range(fam.shape[0])]))
    frames = default_aspiration(own)
    n = frames.shape[1] - 1
    g = ctx.noise_plans(frames, 1, 0, n)
    _compare(g, plans(frames, 1, 0, n, FS, False), "scrambled, hop 1")
    assert len(np.unique(g[..., 0])) > 2  # (the decisions do change along the trajectory)
    check_gain_words(ctx.noise_plans(own, 1, 0, n), plans(own, 1, 0, n, FS, False), "scrambled, hop 1")
    _, own, _ = the_set(oracle)
    frames = default_aspiration(own)
    n = (frames.shape[1] - 1) * HOP
    for s0, s1 in ((0, n), (HOP // 3, n - HOP // 2)):
        g = ctx.noise_plans(frames, HOP, s0, s1)
        _compare(g, plans(frames, HOP, s0, s1, FS, False), f"the set, hop {HOP}, samples {s0}..{s1}")
    check_gain_words(ctx.noise_plans(np.ascontiguousarray(own), HOP, 0, n), plans(own, HOP, 0, n, FS, False), "the set")
    flags = g[..., 0] & 0xFF
    assert np.count_nonzero(flags & 2) and np.count_nonzero(flags & 4) and np.count_nonzero(flags & 8)


def test_plan_hop_records_and_words(contexts, oracle, host):
    """K5's hop records against plan_hop_host, the mixed hops' dense records against plan_sample, and the
    words K1 evaluates from the hop records against the dense records, on the whole set."""
    plans, hops = host
    ctx = contexts(FS, "tree16")
    _, own, _ = the_set(oracle)
    frames = default_aspiration(own)  # (the gain word's 1 ulp: see default_aspiration)
    n = (frames.shape[1] - 1) * HOP
    mixed, total = _compare_hops(ctx, hops, plans, frames, HOP, 0, n, FS, False, "the set")
    assert 0 < mixed < total
    _compare_hops(ctx, hops, plans, frames, HOP, HOP // 3, n - HOP // 2, FS, False, "the set, cut inside hops")
    worst = _compare_hop_words(ctx, np.ascontiguousarray(own), HOP, np.random.default_rng(5), "the set")
    print("hop words vs dense records on the set, max ulps by kind:", worst)


# --- slots, launches, sessions ---------------------------------------------------------------------

def test_slot_order_and_batch_invariance(oracle, monkeypatch):
    """40 generic utterances (three blocks of the 16-lane kernel; utterance_key_kernel runs plan_decide on
    their first frames to sort them into slots): a permuted batch gives the permuted audio bit for bit, and
    so does the call order (AFS_SHAPE_ORDER=0)."""
    from areafunctionsynthesis_amd.synthesizer import Context
    rows = [gt.family(oracle, name, 6) for name in gt.FAMILIES] + [np.stack([gt.edge(oracle, e) for e in gt.EDGES])]
    frames = np.ascontiguousarray(np.concatenate(rows))
    B = frames.shape[0]
    assert B == 40
    seeds = np.arange(100, 100 + B, dtype=np.uint32)
    perm = np.random.default_rng(5).permutation(B)
    ys = {}
    for env in ("1", "0"):
        monkeypatch.setenv("AFS_SHAPE_ORDER", env)
        ctx = Context(FS, solver="tree", lanes=16)
        try:
            ys[env] = ctx.synthesize(frames, HOP, seeds=seeds)
            yp = ctx.synthesize(np.ascontiguousarray(frames[perm]), HOP, seeds=seeds[perm])
        finally:
            ctx.close()
        assert np.array_equal(yp, ys[env][perm])
    assert np.array_equal(ys["1"], ys["0"])
    assert np.isfinite(ys["1"]).all()
    assert len({ys["1"][u].tobytes() for u in range(B)}) == B  # (no two alike: a swap would show)


@pytest.mark.parametrize("solver", TREE_SOLVERS)
def test_launch_split_is_bitwise(oracle, solver, monkeypatch):
    """`breathing` in launches of one hop (97) and of 33 samples (boundaries inside hops) against the
    single launch: the lane state, the hop records and the frame cache cross the joins."""
    from areafunctionsynthesis_amd.synthesizer import Context
    frames = gt.family(oracle, "breathing")
    seeds = np.arange(7, 7 + frames.shape[0], dtype=np.uint32)
    ys = []
    for env in (None, "97", "33"):
        if env is None:
            monkeypatch.delenv("AFS_LAUNCH_SAMPLES", raising=False)
        else:
            monkeypatch.setenv("AFS_LAUNCH_SAMPLES", env)
        ctx = Context(FS, solver="tree", lanes=LANES[solver], profile=True)
        try:
            ys.append(ctx.synthesize(frames, HOP, seeds=seeds))
            kt = ctx.kernel_times()
        finally:
            ctx.close()
        assert kt["synth_launches"] == (1 if env is None else -(-5 * HOP // int(env)))
    assert np.isfinite(ys[0]).all()
    assert np.array_equal(ys[0], ys[1]) and np.array_equal(ys[0], ys[2])


@pytest.mark.parametrize("solver", SOLVERS)
def test_session_call_schedule_vs_oracle(contexts, oracle, solver):
    """One session playing oracle_lib.CALL_SCHEDULE (call lengths 0 .. 441, the dense and the hop-record
    kernels alternating on one saved state) on `breathing` frames, against the oracle's calls."""
    from areafunctionsynthesis_amd.synthesizer import Synthesizer
    frames = gt.family(oracle, "breathing", 4, F=len(CALL_SCHEDULE) + 1)
    B = frames.shape[0]
    seeds = np.arange(21, 21 + B, dtype=np.uint32)
    key = ("session", frames.tobytes())
    if key not in _CACHE:
        want, draws = [[] for _ in CALL_SCHEDULE], []
        for u in range(B):
            h = oracle.create(FS, int(seeds[u]))
            try:
                assert oracle.call(h, frames[u, 0], 441).size == 0
                for k, n in enumerate(CALL_SCHEDULE):
                    want[k].append(oracle.call(h, frames[u, k + 1], n))
                draws.append(oracle.rng_calls(h))
            finally:
                oracle.destroy(h)
        _CACHE[key] = ([np.stack(w) for w in want], np.array(draws, dtype=np.int64))
    want, draws = _CACHE[key]
    syn = Synthesizer(contexts(FS, solver), B, seeds)
    try:
        assert syn.synthesize_signal_tds(np.ascontiguousarray(frames[:, 0]), 441).shape == (B, 0)
        worst = 0.0
        for k, n in enumerate(CALL_SCHEDULE):
            y = syn.synthesize_signal_tds(np.ascontiguousarray(frames[:, k + 1]), n)
            assert y.shape == (B, max(n, 1)) and np.isfinite(y).all(), (k, n)
            worst = max(worst, float(np.abs(y - want[k]).max()))
            assert np.abs(y - want[k]).max() <= GOLD_TOL, (k, n)
        print(f"{solver} session on breathing frames: max |gpu - oracle| {worst:.2e}")
        if solver in TREE_SOLVERS:
            assert np.array_equal(syn.rng_draws(), draws)
    finally:
        syn.close()


# --- outputs ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("solver", TREE_SOLVERS)
def test_pcm_equals_to_int16_of_the_rows(contexts, oracle, solver):
    labels, frames, seeds = the_set(oracle)
    ctx = contexts(FS, solver)
    frames = np.ascontiguousarray(frames)
    y = ctx.synthesize(frames, HOP, seeds=seeds)
    pcm = ctx.synthesize(frames, HOP, seeds=seeds, pcm=True)
    assert pcm.dtype == np.int16 and pcm.shape == y.shape
    assert np.array_equal(pcm, oracle.to_int16(y).reshape(y.shape))
    assert np.abs(pcm).max() > 1000


@pytest.mark.parametrize("lanes", [16, 64])
def test_taps_vs_oracle_per_sample(oracle, lanes):
    """The pressure behind the tongue constriction at section 12 and the flow out of the mouth on a
    `scrambled` trajectory played with one frame per sample, against the oracle's state after every sample."""
    import taps_lib
    from areafunctionsynthesis_amd.synthesizer import Context, pharynx_mouth_pressure
    fam = gt.family(oracle, "scrambled", 2)
    frames = np.ascontiguousarray(np.stack([gt.per_sample(fam[u], 24) for u in range(2)]))
    seeds = np.array([11, 12], dtype=np.uint32)
    taps = [pharynx_mouth_pressure(11), "mouth_radiation_r"]
    want_taps = [(taps_lib.PRESSURE, 25 + 11), (taps_lib.CURRENT, 93)]
    ctx = Context(taps_lib.FS, solver="tree", lanes=lanes)
    try:
        ctx.set_taps(taps)
        audio, rows = ctx.synthesize(frames, 1, seeds=seeds, taps=True)
    finally:
        ctx.close()
    assert rows.shape == (2, 2, frames.shape[1] - 1)
    for u in range(2):
        a, P, U = taps_lib.oracle_state(oracle, frames[u], 1, seeds[u])
        e_audio = taps_lib.rel_err(audio[u], a)
        want = taps_lib.want_rows(P, U, want_taps)
        for q in range(2):
            e = taps_lib.rel_err(rows[u, q], want[q])
            print(f"lanes {lanes} u={u} tap={taps[q]} e={e:.3e} (e_audio {e_audio:.3e})")
            assert np.abs(want[q]).max() > 0
            assert e <= taps_lib.TAP_TOL, (u, taps[q], e)
