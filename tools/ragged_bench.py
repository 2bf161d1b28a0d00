"""afs_synthesize_ragged against afs_synthesize on the same frames padded to the longest utterance
(DESIGN.md 2.8): B a:-vowel utterances at 44.1 kHz, hop 441, frame counts drawn uniformly from
26 .. 101 with a fixed seed, device-resident frames and audio, an AFS_PROFILE context; the two calls
alternated, medians over --reps.  Prints one JSON line: K1 / K5 / K6 device time of each, the calls'
wall time, useful samples/s (the samples of the utterances' own lengths) and the share of padding
slots in the ragged launch.

Usage: python tools/ragged_bench.py [--batch 8192] [--reps 3] [--lanes 16]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lanes", type=int, default=None)
    ap.add_argument("--fmin", type=int, default=26)
    ap.add_argument("--fmax", type=int, default=101)
    a = ap.parse_args()
    import torch

    from areafunctionsynthesis_amd.frames import DEFAULT_GLOTTIS, FRAME_DTYPE
    from areafunctionsynthesis_amd.params import default_shapes
    from areafunctionsynthesis_amd.synthesizer import Context

    fs, hop, B = 44100.0, 441, a.batch
    ctx = Context(fs, profile=True, lanes=a.lanes)
    f = ctx.af_to_frames(np.asarray(default_shapes()["a:"], dtype=np.float64)[None])[0]
    f["velum_opening_cm2"] = 0.0
    f["glottis"] = DEFAULT_GLOTTIS
    counts = np.random.default_rng(20261020).integers(a.fmin, a.fmax + 1, size=B).astype(np.int32)
    Fmax = int(counts.max())
    frames = np.repeat(np.repeat(f[None, None], B, axis=0), Fmax, axis=1)
    dframes = torch.from_numpy(frames.view(np.uint8).reshape(B, Fmax, FRAME_DTYPE.itemsize)).cuda()
    seeds = torch.arange(1, B + 1, dtype=torch.int32).cuda()  # (the bits of uint32 1 .. B)
    T = (Fmax - 1) * hop
    out = torch.zeros((B, T), dtype=torch.float64, device="cuda")
    useful = int((counts.astype(np.int64) - 1).sum()) * hop
    upb = 1 if ctx.lanes_per_utterance(B) == 64 else 8
    groups = np.unique(counts, return_counts=True)[1]
    slots = int(((groups + upb - 1) // upb).sum()) * upb

    def run(ragged: bool) -> dict:
        ctx.kernel_times()
        t0 = time.perf_counter()
        if ragged:
            ctx.synthesize_ragged(dframes, counts, hop, seeds=seeds, out=out)
        else:
            ctx.synthesize(dframes, hop, seeds=seeds, out=out)
        ctx.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        return dict(ctx.kernel_times(), wall_ms=wall)

    run(True), run(False)  # (warm-up: buffers grown, code objects resident)
    got = {True: [], False: []}
    for _ in range(a.reps):
        for ragged in (True, False):
            got[ragged].append(run(ragged))
    res = {"batch": B, "hop": hop, "frames": [a.fmin, a.fmax], "longest": Fmax, "reps": a.reps,
           "kernel": ctx.synthesis_kernel(B), "useful_samples": useful, "padded_samples": B * T,
           "ragged_slots": slots, "padding_slot_share": (slots - B) / slots, "distinct_lengths": int(groups.size)}
    for ragged, name in ((True, "ragged"), (False, "padded")):
        med = {k: float(np.median([r[k] for r in got[ragged]])) for k in ("synth_ms", "plan_ms", "output_ms", "wall_ms")}
        med["synth_ms_runs"] = [round(r["synth_ms"], 3) for r in got[ragged]]
        med["useful_samples_per_s"] = useful / (med["wall_ms"] * 1e-3)
        res[name] = med
    res["k1_ragged_over_padded"] = res["ragged"]["synth_ms"] / res["padded"]["synth_ms"]
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
