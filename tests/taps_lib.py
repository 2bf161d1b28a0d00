"""Shared by the signal-tap tests (test_taps_emu.py, test_taps_gpu.py): the trajectories, the oracle's
per-sample state and the error measure.  Every reference is computed once and left unchanged."""
import numpy as np

from areafunctionsynthesis_amd.frames import DEFAULT_GLOTTIS, FRAME_DTYPE

FS = 44100.0
NS, NC = 93, 97
PRESSURE, CURRENT = 0, 1
# all 190 quantities, 8 at a time: 24 tap lists (the last holds 6)
ALL_TAPS = [(PRESSURE, s) for s in range(NS)] + [(CURRENT, c) for c in range(NC)]
GROUPS = [ALL_TAPS[i:i + 8] for i in range(0, len(ALL_TAPS), 8)]
assert len(GROUPS) == 24

# Relative bound on max |tap - oracle| / max |oracle| per trace over (at most) the first 2048 samples.
# Measured ("Signal taps"): the largest e of the first GPU run against the oracle was
# 5.5e-13 (the hop-33 checkpoints; the hop-1 glide per sample: 3.9e-14 beside an e_audio of 3.6e-14;
# the CPU emulator on the glide: 3.0e-14 beside 1.6e-14), times 10 for the device's libm in the noise
# cutoffs and the aspiration gain, rounded up to a power of ten.
TAP_TOL = 1e-11


def glide_frames(oracle, F=48, velum=0.6, a="a:", b="s"):
    """F frames gliding shape a -> b (area-function parameters interpolated linearly) with the velum
    open, so that the nose, the sinuses and, towards the fricative, the noise sources are live."""
    from areafunctionsynthesis_amd.params import default_shapes
    sh = default_shapes()
    pa, pb = np.asarray(sh[a], dtype=np.float64), np.asarray(sh[b], dtype=np.float64)
    out = np.zeros(F, dtype=FRAME_DTYPE)
    for k in range(F):
        r = k / (F - 1)
        f = oracle.af_to_frame((1.0 - r) * pa + r * pb)
        f["velum_opening_cm2"] = velum
        f["glottis"] = DEFAULT_GLOTTIS
        out[k] = f
    return out


_CACHE = {}


def glide_batch(oracle, B, F=48):
    """frames[B, F]: utterance u plays the a: -> s glide with velum opening 0.6 + 0.1 u; seeds 11 + u."""
    key = ("glide", B, F)
    if key not in _CACHE:
        fr = np.stack([glide_frames(oracle, F, 0.6 + 0.1 * u) for u in range(B)])
        fr.setflags(write=False)
        _CACHE[key] = fr
    return _CACHE[key], np.arange(11, 11 + B, dtype=np.uint32)


def oracle_state(oracle, frames, hop, seed):
    """One utterance on the oracle: (audio[T], pressures[93, T], currents[97, T]) after every sample
    when hop == 1 (one-sample calls), else after every call (columns (k + 1) hop - 1, NaN elsewhere)."""
    key = ("state", frames.tobytes(), hop, int(seed))
    if key not in _CACHE:
        F = frames.shape[0]
        T = (F - 1) * hop
        audio = np.zeros(T)
        P, U = np.full((NS, T), np.nan), np.full((NC, T), np.nan)
        h = oracle.create(FS, int(seed))
        try:
            assert oracle.call(h, frames[0], hop).size == 0  # the latch
            for k in range(1, F):
                audio[(k - 1) * hop:k * hop] = oracle.call(h, frames[k], hop)
                P[:, k * hop - 1] = oracle.pressures(h)
                U[:, k * hop - 1] = oracle.currents(h)
        finally:
            oracle.destroy(h)
        for x in (audio, P, U):
            x.setflags(write=False)
        _CACHE[key] = (audio, P, U)
    return _CACHE[key]


def want_rows(P, U, taps):
    """The oracle's traces of a tap list: [len(taps), T]."""
    return np.stack([(P if kind == PRESSURE else U)[index] for kind, index in taps])


def rel_err(got, want):
    """e = max |got - want| / max |want| of one trace over the samples the oracle has (at most the
    first 2048); a trace whose oracle peak is exactly 0 (a closed branch) must be exactly 0: then 0.0,
    else inf."""
    have = ~np.isnan(want)
    have[2048:] = False
    g, w = got[have], want[have]
    peak = np.abs(w).max()
    if peak == 0.0:
        return 0.0 if not g.any() else float("inf")
    return float(np.abs(g - w).max() / peak)
