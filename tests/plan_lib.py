"""Shared by the tests of K5, the noise-source plan kernel (test_plan_gpu.py, test_generic_tubes_gpu.py):
the comparisons of its dense records and hop records with the host restatement (tests/emu/plan_emu.cpp)."""
import numpy as np

PW_GAIN_G = 15
PLAN_WORDS = 16
HOP_DTYPE = np.dtype([("p", "<u8", (PLAN_WORDS, 4)), ("kind", "u1", (PLAN_WORDS,)), ("mixed", "<u4"),
                      ("dense", "<u4"), ("noise", "<u8")])
assert HOP_DTYPE.itemsize == 544


def _compare(gpu, host, label):
    assert gpu.shape == host.shape
    exact = np.ones(PLAN_WORDS, dtype=bool)
    exact[PW_GAIN_G] = False
    diff = gpu[..., exact] != host[..., exact]
    if diff.any():
        r, t, w = np.argwhere(diff)[0]
        words = np.flatnonzero(exact)
        raise AssertionError(f"{label}: {int(diff.sum())} words differ; first: row {r} sample {t} word "
                             f"{words[w]}: gpu {int(gpu[r, t, words[w]]):#x} host {int(host[r, t, words[w]]):#x}")
    g = gpu[..., PW_GAIN_G].view(np.int64)
    h = host[..., PW_GAIN_G].view(np.int64)
    ulps = np.abs(g - h)  # (positive doubles: the bit patterns are ordered)
    assert ulps.max() <= 1, (label, int(ulps.max()))
    return int(np.count_nonzero(ulps))


def _compare_hops(ctx, host_hops, host_plans, frames, hop, s0, s1, fs, two_mass, label):
    gh, gp = ctx.noise_plan_hops(frames, hop, s0, s1)
    gh = gh.view(HOP_DTYPE)[..., 0]
    hh = host_hops(frames, hop, s0, s1, fs, two_mass)
    assert np.array_equal(gh["mixed"], hh["mixed"]), label
    assert np.array_equal(gh["kind"], hh["kind"]), label
    assert np.array_equal(gh["noise"], hh["noise"]), label  # (the dipoles and constrictions of every sample)
    gw, hw = gh["p"].copy(), hh["p"].copy()
    # the glottis gain (a constant word: p[15][0]) comes from the device pow: 1 ulp
    ulps = np.abs(gw[..., 15, 0].view(np.int64) - hw[..., 15, 0].view(np.int64))
    assert ulps.max() <= 1, (label, int(ulps.max()))
    gw[..., 15, 0] = hw[..., 15, 0] = 0
    diff = gw != hw
    if diff.any():
        r, q, w, j = np.argwhere(diff)[0]
        raise AssertionError(f"{label}: {int(diff.sum())} inputs differ; first: row {r} slot {q} word {w} input {j}")
    # the mixed hops' samples: their dense records
    mixed_samples = np.zeros(gp.shape[:2], dtype=bool)
    for r, q in np.argwhere(gh["mixed"] != 0):
        h = s0 // hop + q
        lo, hi = max(h * hop, s0), min((h + 1) * hop, s1)
        mixed_samples[r, lo - s0:hi - s0] = True
    if mixed_samples.any():
        hp = host_plans(frames, hop, s0, s1, fs, two_mass)
        _compare(gp[mixed_samples][None], hp[mixed_samples][None], label + " (mixed hops' dense records)")
    assert not gp[~mixed_samples].any(), label  # nothing written for the other samples
    return int(np.count_nonzero(gh["mixed"])), gh.size


def _compare_hop_words(ctx, frames, hop, rng, label, per_hop=24):
    """test_plan_gpu.py test_hop_words_vs_dense_records' comparison, with its bounds, on any frames: the
    words the synthesis kernel evaluates from K5's hop records (afs_plan_hop_words) against K5's dense
    records of the same samples, at the first, the last and `per_hop` random samples of every hop that is
    not mixed.  Constants and sqrt(A) bit for bit; 1/A and 1/d within 1e-14 relative and 16 ulps; the
    downstream factors within 1e-12 relative; the gain within 1e-13.  Returns the worst ulps by kind."""
    n = (frames.shape[1] - 1) * hop
    hops, _ = ctx.noise_plan_hops(frames, hop, 0, n)
    dense = ctx.noise_plans(frames, hop, 0, n)
    rec = hops.view(HOP_DTYPE)[..., 0]
    rows, slots = rec.shape
    pick = []
    for r in range(rows):
        for q in range(slots):
            if rec["mixed"][r, q]:
                continue
            for i in np.unique(np.concatenate([[0, hop - 1], rng.integers(0, hop, per_hop)])):
                pick.append((r, q, int(i)))
    assert pick, label
    hrec = np.stack([hops[r, q] for r, q, _ in pick])
    ratio = np.array([i / hop for _, _, i in pick])
    got = ctx.plan_hop_words(hrec, ratio)
    want = np.stack([dense[r, q * hop + i] for r, q, i in pick])
    kinds = np.stack([rec["kind"][r, q] for r, q, _ in pick])
    worst = {}
    for k, name in ((0, "const"), (1, "1/A"), (2, "sqrtA"), (3, "1/d"), (4, "N/D")):
        m = kinds == k
        m[:, PW_GAIN_G] = False  # (the gain: hop-constant, checked below)
        if not m.any():
            continue
        g, h = got[m].view(np.int64), want[m].view(np.int64)
        if k in (0, 2):
            assert np.array_equal(g, h), (label, name, int(np.count_nonzero(g != h)))
            worst[name] = 0
            continue
        gf, hf = got[m].view(np.float64), want[m].view(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):  # (a word that is exactly 0 must be exactly 0)
            rel = np.where(hf == 0.0, np.where(gf == 0.0, 0.0, np.inf), np.abs(gf - hf) / np.abs(hf))
        ulps = np.abs(g - h)
        worst[name] = max(worst.get(name, 0), int(ulps.max()))
        bound = 1e-12 if k == 4 else 1e-14
        assert rel.max() <= bound, (label, name, float(rel.max()), int(ulps.max()))
    gain = got[:, PW_GAIN_G].view(np.float64)
    assert np.all(np.abs(gain - want[:, PW_GAIN_G].view(np.float64)) <= 1e-13 * np.abs(gain)), label
    assert worst.get("1/A", 0) <= 16 and worst.get("1/d", 0) <= 16, worst
    return worst
