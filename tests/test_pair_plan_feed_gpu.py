"""The wave pairs' plan-word feed (tree_kernel.h tree_pair_run): the DYN wave holds the hop records,
evaluates the words of sample t + 1 in P3 of sample t and hands them to the STAT wave through LDS.
16 utterances of 5 frames at hop 33 -- static vowels, whose hops K5 decides (their waves run the
NZ_GLOTTIS variant), beside a: -> s glides, whose hops come out mixed and read dense records, in the
same blocks and waves and in blocks of their own -- in one launch, in launches of 33 samples (each ends
exactly on a hop's end: the first word of every launch comes from the prologue, the next hop's record
is never loaded ahead) and in launches of 50 (they start and end inside hops, odd and even lengths).
Every row bit for bit the same three ways, and bit for bit the one-wave kernel's: at 64 lanes the
one-wave kernel of the same library (the batch tiled to 1025 utterances); at 16 lanes, where the
one-wave form is a build of its own (-DAFS_PAIR=0), its rows recorded in
tests/golden/pair_plan_feed_one_wave16.npz:

    python -m areafunctionsynthesis_amd.build --tag onewave --flags=-DAFS_PAIR=0
    AFS_LIB=areafunctionsynthesis_amd/libafs_onewave.so python tests/test_pair_plan_feed_gpu.py write
"""
import hashlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pair_plan_feed_one_wave16.npz")
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

from areafunctionsynthesis_amd.frames import DEFAULT_GLOTTIS, FRAME_DTYPE  # noqa: E402
from areafunctionsynthesis_amd.params import default_shapes  # noqa: E402
from taps_lib import FS, glide_frames  # noqa: E402

pytestmark = pytest.mark.gpu

HOP, F, B = 33, 5, 16
T = (F - 1) * HOP
ONE_WAVE_B = 1025  # (64 lanes: batches above TREE_PAIR64_MAX = 1024 run one wave per utterance)
VOWELS = ("a:", "e:", "i:", "o:", "u:")
# 16 lanes: rows 0-3 one wave pair of vowels alone, 4-7 one of glides alone, 8-15 both in a pair
GLIDE = np.array([0, 0, 0, 0, 1, 1, 1, 1, 0, 1, 0, 1, 1, 0, 0, 1], dtype=bool)
HOLD = {9: [0, 1, 2, 2, 2], 11: [0, 0, 0, 1, 2]}  # (glide rows: the glide's frames each of their frames plays)
KERNELS = {16: "tree_pair_kernel", 64: "tree_pair64_kernel"}

_CACHE = {}


def batch(oracle):
    """(frames[16, 5], seeds[16]), computed once and left unchanged."""
    if "batch" not in _CACHE:
        sh = default_shapes()
        frames = np.zeros((B, F), dtype=FRAME_DTYPE)
        for u in range(B):
            if u in HOLD:  # a three-frame glide held at one end: mixed hops beside decided ones in one row
                frames[u] = glide_frames(oracle, 3, 0.3 + 0.05 * u)[HOLD[u]]
            elif GLIDE[u]:
                frames[u] = glide_frames(oracle, F, 0.3 + 0.05 * u)
            else:
                f = oracle.af_to_frame(sh[VOWELS[u % len(VOWELS)]])
                f["velum_opening_cm2"] = 0.0
                f["glottis"] = DEFAULT_GLOTTIS
                frames[u] = f
        seeds = (211 + 3 * np.arange(B)).astype(np.uint32)
        frames.setflags(write=False)
        seeds.setflags(write=False)
        _CACHE["batch"] = (frames, seeds)
    return _CACHE["batch"]


def frames_digest(frames):
    return hashlib.sha1(np.ascontiguousarray(frames).tobytes()).hexdigest()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def run(ctx, frames, seeds):
    """(audio[n, T], rand() counts[n], non-finite flags[n]) of one call."""
    n = frames.shape[0]
    y, rep = ctx.synthesize(np.ascontiguousarray(frames), HOP, seeds=np.ascontiguousarray(seeds), report=True)
    return y, ctx.rng_draws(n), np.asarray(rep["nonfinite"])[:n]


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.fixture(scope="module")
def make_ctx(monkeypatch_module):
    from areafunctionsynthesis_amd.synthesizer import Context
    made = []

    def make(lanes, launch=None):
        if launch is not None:
            monkeypatch_module.setenv("AFS_LAUNCH_SAMPLES", str(launch))
        try:
            made.append(Context(FS, solver="tree", lanes=lanes))
        finally:
            if launch is not None:
                monkeypatch_module.delenv("AFS_LAUNCH_SAMPLES")
        return made[-1]

    yield make
    for c in made:
        c.close()


def one_wave_rows(make_ctx, ctx, lanes, frames, seeds):
    if lanes == 64:
        idx = np.arange(ONE_WAVE_B) % B
        assert ctx.synthesis_kernel(ONE_WAVE_B) == "tree_synth_kernel"
        y, d, nf = run(ctx, frames[idx], seeds[idx])
        return y[:B], d[:B], nf[:B]
    g = np.load(GOLDEN)
    assert str(g["frames_sha1"]) == frames_digest(frames), "the golden rows were recorded for other frames"
    return g["audio"], g["draws"], np.zeros(B, dtype=np.int64)


@pytest.mark.parametrize("lanes", [16, 64])
def test_plan_feed_rows_bitwise(make_ctx, oracle, lanes):
    frames, seeds = batch(oracle)
    ctx = make_ctx(lanes)
    assert ctx.synthesis_kernel(B) == KERNELS[lanes]
    # both feeds are exercised: every vowel hop is decided, some glide hop is mixed (K5's hop records)
    hops, _ = ctx.noise_plan_hops(np.ascontiguousarray(frames), HOP)
    mixed = hops[..., 528:532].copy().view(np.uint32)[..., 0] != 0
    assert mixed.shape == (B, F - 1)
    print(f"lanes {lanes}: mixed hops per row {mixed.sum(axis=1).tolist()}")
    assert mixed[GLIDE].any(), "no mixed hop in the batch"
    assert not mixed[~GLIDE].any() and (~mixed).any(), "no decided hop in the batch"
    # ... and a row goes from a mixed hop to a decided one, another the other way
    assert (mixed[:, :-1] & ~mixed[:, 1:]).any() and (~mixed[:, :-1] & mixed[:, 1:]).any()
    whole = run(ctx, frames, seeds)
    assert np.isfinite(whole[0]).all() and whole[0].shape == (B, T) and not whole[2].any()
    for launch in (33, 50):
        split = run(make_ctx(lanes, launch), frames, seeds)
        for u in range(B):
            assert np.array_equal(bits(split[0][u]), bits(whole[0][u])), (launch, u)
        assert np.array_equal(split[1], whole[1]) and np.array_equal(split[2], whole[2]), launch
    one = one_wave_rows(make_ctx, ctx, lanes, frames, seeds)
    for u in range(B):
        assert np.array_equal(bits(whole[0][u]), bits(one[0][u])), u
    assert np.array_equal(whole[1], one[1]) and np.array_equal(whole[2], one[2])
    print(f"lanes {lanes}: rand() counts {whole[1].tolist()}")


if __name__ == "__main__":
    assert sys.argv[1:] == ["write"], __doc__
    from oracle_lib import Oracle

    from areafunctionsynthesis_amd.synthesizer import Context
    frames, seeds = batch(Oracle())
    ctx = Context(FS, solver="tree", lanes=16)
    assert ctx.synthesis_kernel(B) == "tree_synth_kernel", "load the one-wave build (AFS_LIB)"
    y, d, nf = run(ctx, frames, seeds)
    ctx.close()
    assert np.isfinite(y).all() and not nf.any()
    np.savez(GOLDEN, audio=y, draws=d, frames_sha1=np.array(frames_digest(frames)))
    print("wrote", GOLDEN, y.shape, d.tolist())
