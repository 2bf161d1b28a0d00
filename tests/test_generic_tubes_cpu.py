"""The oracle, the CPU emulators and the noise-source plan on tubes the area-function model cannot make
(tests/generic_tubes.py: unequal section lengths, tongue runs broken by other articulators, teeth
anywhere, lengths that change from frame to frame).

  * the oracle against the reference build's recorded audio and rand() counts (golden/generic_tubes.npz)
    and, where the reference build is at hand, against it live on the whole set: bit for bit;
  * the tree emulator (csrc/tree_core.h on the CPU) against the oracle within test_tree_emu.TOL, every
    lane width bitwise the 16-lane one, the wave-pair emulator bitwise the one-wave one;
  * the interval decisions, the hop records' words and their noise masks against the per-sample plan,
    with the bounds of test_plan_hops.py;
  * the three conditions that keep the set hard (finite; lengths and articulators matter; both plan paths).
"""
import ctypes
import os

import numpy as np
import pytest

import generic_tubes as gt
from oracle_lib import OPTION_DEFAULTS, ref_available
from test_plan_hops import HOP_DTYPE, PLAN_WORDS, PW_FDN, PW_GAIN_G, _header_noise, lib  # noqa: F401 (lib: a fixture)
from test_tree_emu import TOL, emu, hop_mode, pair_emu  # noqa: F401 (fixtures)

FS, HOP = 22050.0, 97
OPTION_SETS = [{}, {"inner_length_corrections": 0}, {"glottis_model": 1}]
OPT_IDS = ["default", "inner_length_corrections=0", "glottis_model=1"]


class Set:
    """The generic set with the oracle's audio and rand() counts at hop 97, 22.05 kHz (computed once)."""

    def __init__(self, oracle):
        self.labels, self.frames, self.seeds = gt.generic_set(oracle)
        self.frames.setflags(write=False)
        self._oracle = oracle
        self._runs = {}

    def frames_for(self, opt):
        return gt.two_mass(self.frames) if opt.get("glottis_model") else self.frames

    def oracle_audio(self, opt=None):
        """(audio[rows, T], rand() calls[rows]) of the oracle with these options."""
        opt = opt or {}
        key = tuple(sorted(opt.items()))
        if key not in self._runs:
            fr = self.frames_for(opt)
            xs, ds = [], []
            for r in range(fr.shape[0]):
                h = self._oracle.create(FS, int(self.seeds[r]), opt)
                try:
                    xs.append(np.concatenate([self._oracle.call(h, fr[r, k], HOP) for k in range(fr.shape[1])]))
                    ds.append(self._oracle.rng_calls(h))
                finally:
                    self._oracle.destroy(h)
            self._runs[key] = (np.stack(xs), np.array(ds, dtype=np.int64))
        return self._runs[key]


@pytest.fixture(scope="module")
def gset(oracle):
    return Set(oracle)


# --- the oracle --------------------------------------------------------------------------------

def test_golden_file_regenerates(oracle, golden_dir):
    """The generator still makes the frames the golden file holds (the file is make_golden.py generic's
    output for today's generator)."""
    gold = gt.load_golden(golden_dir)
    cases = gt.golden_cases(oracle)
    assert [c[0] for c in cases] == [g[0] for g in gold]
    for (label, fr, hop, seed, fs), g in zip(cases, gold):
        assert (hop, seed, fs) == g[2:5], label
        assert fr.tobytes() == g[1].tobytes(), label
    assert {g[2] for g in gold} == {33, 97, 441} and {g[4] for g in gold} == {22050.0, 44100.0}


def test_oracle_equals_golden_bit_for_bit(oracle, golden_dir):
    for label, fr, hop, seed, fs, want, calls in gt.load_golden(golden_dir):
        x, d = oracle.utterance_draws(fr, hop, seed, fs)
        assert np.isfinite(want).all() and np.abs(want).max() > 1e-4, label
        assert np.array_equal(x[:gt.GOLDEN_SAMPLES], want), label
        assert d == calls and calls > 0, (label, d, calls)


@pytest.mark.skipif(not ref_available(), reason="reference build not available")
@pytest.mark.parametrize("opt", OPTION_SETS, ids=OPT_IDS)
def test_oracle_equals_live_reference(oracle, gset, opt):
    """The whole set through the reference's own TdsModel / Tube, audio and rand() counts bit for bit."""
    from oracle_lib import RefLib
    ref = RefLib()
    x, draws = gset.oracle_audio(opt)
    fr = gset.frames_for(opt)
    for r, label in enumerate(gset.labels):
        c0 = int(ref.lib.afsref_rand_calls())
        y = ref.utterance(fr[r], HOP, int(gset.seeds[r]), FS, opt=opt)
        assert np.array_equal(x[r], y), label
        assert int(ref.lib.afsref_rand_calls()) - c0 == draws[r], label


# --- the three conditions on the inputs ----------------------------------------------------------

def test_set_is_finite(gset):
    x, draws = gset.oracle_audio()
    assert np.isfinite(x).all()
    assert (np.abs(x).max(axis=1) > 1e-3).all()  # (and audible: no silent tube passes trivially)
    assert (draws > 0).all()


def test_lengths_and_articulators_matter(oracle, gset):
    """Per family: equalising the lengths moves the oracle's audio by more than 1e-6, and (all but
    `unequal`, which keeps the area-function articulators) the area-function articulator pattern changes
    the rand() count of at least one utterance.  A kernel that ignored either could not pass."""
    x, draws = gset.oracle_audio()
    by_len, by_art = {}, {}
    for r, label in enumerate(gset.labels):
        fam = gt.family_of(label)
        xe = oracle.utterance(gt.equal_lengths(gset.frames[r]), HOP, int(gset.seeds[r]), FS)
        by_len[fam] = max(by_len.get(fam, 0.0), float(np.abs(x[r] - xe).max()))
        _, da = oracle.utterance_draws(gt.af_pattern(gset.frames[r]), HOP, int(gset.seeds[r]), FS)
        by_art[fam] = by_art.get(fam, 0) + int(da != draws[r])
    print("max |audio - audio with equal lengths| per family:", by_len)
    print("utterances whose rand() count the area-function articulators change:", by_art)
    for fam in gt.FAMILIES:
        assert by_len[fam] > 1e-6, (fam, by_len[fam])
        if fam != "unequal":
            assert by_art[fam] >= 1, fam


def _dense(lib, frames, hop, fs=FS, two_mass=0):
    rows, F = frames.shape
    n = (F - 1) * hop
    dense = np.zeros((rows, n, PLAN_WORDS), dtype=np.uint64)
    fr = np.ascontiguousarray(frames)
    assert lib.emu_plan_records(fr.ctypes.data, rows, F, hop, 0, n, fs, two_mass, dense.ctypes.data) == 0
    return dense


def _hops(lib, frames, hop, fs=FS):
    rows, F = frames.shape
    hops = np.zeros((rows, F - 1), dtype=HOP_DTYPE)
    fr = np.ascontiguousarray(frames)
    assert lib.emu_plan_hops(fr.ctypes.data, rows, F, hop, 0, (F - 1) * hop, fs, 0, hops.ctypes.data) == 0
    return hops


def plan_shares(lib, frames, hop):
    """(share of hops with one decision throughout, share whose decision changes inside the hop), from the
    per-sample records' headers (flags and obstacle sections; for "one decision" the narrowest sections'
    words too) -- not from the interval evaluation under test."""
    rows, F = frames.shape
    d = _dense(lib, frames, hop).reshape(rows, F - 1, hop, PLAN_WORDS)
    disc = d[..., :PW_FDN]
    uniform = (disc == disc[:, :, :1]).all(axis=(2, 3))
    mixed = (d[..., 0] != d[:, :, :1, 0]).any(axis=2)
    return float(uniform.mean()), float(mixed.mean()), uniform, mixed


def test_both_plan_paths_are_hit(lib, gset):
    uni, mix, uniform, mixed = plan_shares(lib, gset.frames, HOP)
    fams = [gt.family_of(label) for label in gset.labels]
    for fam in sorted(set(fams)):
        m = np.array([f == fam for f in fams])
        print(f"{fam}: uniform hops {uniform[m].mean():.2f}, mixed hops {mixed[m].mean():.2f}")
    print(f"whole set at hop {HOP}: uniform {uni:.3f}, mixed {mix:.3f}")
    assert uni >= 0.25, uni
    assert mix >= 0.10, mix


# --- the emulators -----------------------------------------------------------------------------

@pytest.mark.parametrize("opt", OPTION_SETS, ids=OPT_IDS)
def test_tree_emulator_vs_oracle(emu, gset, opt):
    """The 16-lane emulator (dense plan records) against the oracle over the first 2048 samples."""
    x, _ = gset.oracle_audio(opt)
    fr = gset.frames_for(opt)
    worst = {}
    for r, label in enumerate(gset.labels):
        y = emu.opt(fr[r], HOP, int(gset.seeds[r]), FS, opt)
        e = float(np.abs(y[:2048] - x[r, :2048]).max())
        worst[gt.family_of(label)] = max(worst.get(gt.family_of(label), 0.0), e)
    print("emulator vs oracle, max |err| per family:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= TOL, worst


def test_tree_emulator_hop_records_vs_oracle(emu, hop_mode, gset):
    """With hop records (the device's path at hops >= 32): decided hops evaluate their words from the hop's
    inputs, mixed hops read dense records; both kinds occur on the set."""
    x, _ = gset.oracle_audio()
    for r, label in enumerate(gset.labels):
        y = emu(gset.frames[r], HOP, int(gset.seeds[r]), FS)
        assert np.abs(y[:2048] - x[r, :2048]).max() <= TOL, label
    hops, mixed = hop_mode()
    assert 0 < mixed < hops, (hops, mixed)


@pytest.mark.parametrize("W", [32, 64])
def test_lane_width_invariance(emu, gset, W):
    for r, label in enumerate(gset.labels):
        args = (gset.frames[r], HOP, int(gset.seeds[r]), FS)
        assert np.array_equal(emu(*args, W=W), emu(*args, W=16)), label


@pytest.mark.parametrize("opt", OPTION_SETS, ids=OPT_IDS)
def test_wave_pair_equals_one_wave(emu, pair_emu, gset, opt):
    """The wave pairs' step (two roles on two threads) gives the one-wave step's audio bit for bit (tone
    filter in K6, as on the device; 16 lanes with options, 64 lanes at the defaults too) and the oracle's
    rand() count (the one-wave emulator reports none)."""
    o = dict(OPTION_DEFAULTS, **opt)
    iopt = np.array([o[k] for k in ("turbulence_losses", "soft_walls", "generate_noise_sources", "radiation_from_skin",
                                    "piriform_fossa", "inner_length_corrections", "transvelar_coupling",
                                    "glottis_loss", "glottis_model")], dtype=np.int32)
    _, draws = gset.oracle_audio(opt)
    fr = gset.frames_for(opt)
    emu.lib.emu_tree_set_tone_k6.argtypes = [ctypes.c_int]
    for r, label in enumerate(gset.labels):
        f = np.ascontiguousarray(fr[r])
        for W in (16, 64) if not opt else (16,):
            y = np.zeros((f.size - 1) * HOP)
            d = np.zeros(1, np.uint64)
            n = pair_emu.emu_pair_utterance(f.ctypes.data, f.size, HOP, int(gset.seeds[r]), FS, W, iopt.ctypes.data,
                                            float(o["flow_separation_area_ratio"]), y.ctypes.data, d.ctypes.data)
            assert n == y.size
            emu.lib.emu_tree_set_tone_k6(1)
            try:
                x = emu.opt(f, HOP, int(gset.seeds[r]), FS, opt) if W == 16 else emu(f, HOP, int(gset.seeds[r]), FS, W=W)
            finally:
                emu.lib.emu_tree_set_tone_k6(0)
            assert np.array_equal(x, y), (label, W, float(np.abs(x - y).max()))
            assert int(d[0]) == draws[r], (label, W)


# --- the plan ----------------------------------------------------------------------------------

@pytest.mark.parametrize("hop", [97, 441])
def test_interval_decisions_never_disagree(lib, gset, hop):
    frames = np.ascontiguousarray(gset.frames)
    rows, F = frames.shape
    n = (F - 1) * hop
    for s0, s1 in ((0, n), (hop // 3, n - hop // 2)):  # whole utterances; ranges cut inside hops
        c = np.zeros(4, dtype=np.int64)
        assert lib.emu_plan_iv_check(frames.ctypes.data, rows, F, hop, s0, s1, c.ctypes.data) == 0
        decided, undecided, violations, mixed = (int(v) for v in c)
        print(f"hop {hop} samples {s0}..{s1}: decided {decided}, undecided {undecided}, mixed {mixed}")
        assert violations == 0, (hop, s0, s1)
        assert mixed <= undecided
        assert decided > 0 and mixed > 0  # (both kinds of hop are in the set)


def hop_word_distances(lib, frames, hop, stride=7):
    """max distance of the hop records' words from the dense records per row: (factors: absolute, gain:
    relative, hops checked); the discrete words and the area terms are asserted bitwise."""
    rows, F = frames.shape
    hops, dense = _hops(lib, frames, hop), _dense(lib, frames, hop)
    exact = np.ones(PLAN_WORDS, dtype=bool)
    exact[PW_FDN:PW_FDN + 4] = False
    exact[PW_GAIN_G] = False
    fac, gain, checked = np.zeros(rows), np.zeros(rows), np.zeros(rows, dtype=np.int64)
    for r in range(rows):
        for q in range(F - 1):
            if hops[r, q]["mixed"]:
                continue
            hc = np.ascontiguousarray(hops[r, q])
            checked[r] += 1
            for i in range(0, hop, stride):
                w = np.zeros(PLAN_WORDS, dtype=np.uint64)
                lib.emu_plan_hop_words(hc.ctypes.data, i / hop, w.ctypes.data)
                d = dense[r, q * hop + i]
                assert np.array_equal(w[exact], d[exact]), (r, q, i)
                fw, fd = w[PW_FDN:PW_FDN + 4].view(np.float64), d[PW_FDN:PW_FDN + 4].view(np.float64)
                fac[r] = max(fac[r], float(np.abs(fw - fd).max()))
                gw, gd = w[PW_GAIN_G:].view(np.float64), d[PW_GAIN_G:].view(np.float64)
                gain[r] = max(gain[r], float((np.abs(gw - gd) / np.abs(gd)).max()))
    return fac, gain, checked


@pytest.mark.parametrize("hop", [97, 441])
def test_hop_record_words_equal_dense_records(lib, gset, hop):
    """test_plan_hops.py's bounds on the set: discrete words and area terms bit for bit, the downstream
    factors within 1e-12 absolute (ratios of interpolated end values instead of sequential position sums:
    on `breathing` tubes the positions differ at the two ends of the hop), the gain within 1e-13."""
    fac, gain, checked = hop_word_distances(lib, gset.frames, hop)
    fams = [gt.family_of(label) for label in gset.labels]
    for fam in sorted(set(fams)):
        m = np.array([f == fam for f in fams])
        print(f"hop {hop} {fam}: {int(checked[m].sum())} hops, factors {fac[m].max():.2e}, gain {gain[m].max():.2e}")
        assert checked[m].sum() > 0, fam
    assert fac.max() <= 1e-12, (float(fac.max()), gset.labels[int(fac.argmax())])
    assert gain.max() <= 1e-13, float(gain.max())


@pytest.mark.parametrize("hop", [97, 441])
def test_hop_noise_mask_covers_every_sample(lib, gset, hop):
    rows, F = gset.frames.shape
    hops, dense = _hops(lib, gset.frames, hop), _dense(lib, gset.frames, hop)
    want = np.bitwise_or.reduce(_header_noise(dense[..., 0]).reshape(rows, F - 1, hop), axis=2)
    assert np.array_equal(hops["noise"], want)
    assert (hops["noise"] >> np.uint64(48) & np.uint64(1)).all()
    # (tongue and lip constrictions both occur: the masks are not the glottis' alone)
    assert (hops["noise"] >> np.uint64(49) & np.uint64(1)).any() and (hops["noise"] >> np.uint64(51) & np.uint64(1)).any()
