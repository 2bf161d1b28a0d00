"""afs_synthesize_pcm against the two-step path, afs_synthesize then afs_to_int16: B
static vowels (workloads.static_vowels) x --seconds at 44.1 kHz, hop 441, device-resident frames, seeds
and audio, AFS_PROFILE contexts -- one per path, so that memory_info() shows what each path alone
allocates; the two paths alternated, medians over --reps.  Prints one JSON line: per path the K1 / K5 /
K6 device times, K3's (HIP events around to_int16; the two-step path only), the call's wall time and
memory_info(); and whether the PCM rows equal the two-step rows.

Usage: python tools/pcm_bench.py [--batch 8192] [--seconds 0.25] [--reps 3] [--lanes 16]
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
    ap.add_argument("--seconds", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lanes", type=int, default=None)
    a = ap.parse_args()
    import torch

    from areafunctionsynthesis_amd.frames import FRAME_DTYPE
    from areafunctionsynthesis_amd.synthesizer import Context
    from areafunctionsynthesis_amd.workloads import build_frames, static_vowels

    B = a.batch
    w = static_vowels(B, seconds=a.seconds)
    ctxs = {"pcm": Context(w.fs, profile=True, lanes=a.lanes), "two_step": Context(w.fs, profile=True, lanes=a.lanes)}
    frames = build_frames(w, ctxs["pcm"].af_to_frames)
    F, hop, T = w.num_frames, w.hop, w.samples_per_utterance
    dframes = torch.from_numpy(np.ascontiguousarray(frames).view(np.uint8).reshape(B, F, FRAME_DTYPE.itemsize)).cuda()
    seeds = torch.from_numpy(w.seeds.view(np.int32)).cuda()
    pcm = {k: torch.zeros((B, T), dtype=torch.int16, device="cuda") for k in ctxs}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(path: str) -> dict:
        ctx = ctxs[path]
        ctx.kernel_times()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k3 = 0.0
        if path == "pcm":
            ctx.synthesize(dframes, hop, seeds=seeds, out=pcm[path], pcm=True)
            ctx.synchronize()
        else:
            out = torch.empty((B, T), dtype=torch.float64, device="cuda")  # (the call-long fp64 buffer)
            ctx.synthesize(dframes, hop, seeds=seeds, out=out)
            ctx.synchronize()
            ev0.record()
            ctx.to_int16(out, out=pcm[path])
            ev1.record()
            torch.cuda.synchronize()
            k3 = float(ev0.elapsed_time(ev1))
            del out
        wall = (time.perf_counter() - t0) * 1e3
        return dict(ctx.kernel_times(), to_int16_ms=k3, wall_ms=wall)

    for path in ctxs:  # (warm-up: buffers grown, code objects resident)
        run(path)
    got = {k: [] for k in ctxs}
    for _ in range(a.reps):
        for path in ctxs:
            got[path].append(run(path))
    res = {"batch": B, "hop": hop, "frames": F, "samples_per_utterance": T, "reps": a.reps,
           "kernel": ctxs["pcm"].synthesis_kernel(B), "rows_equal": bool(torch.equal(pcm["pcm"], pcm["two_step"]))}
    for path in ctxs:
        keys = ("synth_ms", "plan_ms", "output_ms", "to_int16_ms", "wall_ms")
        med = {k: float(np.median([r[k] for r in got[path]])) for k in keys}
        med["output_plus_to_int16_ms_runs"] = [round(r["output_ms"] + r["to_int16_ms"], 3) for r in got[path]]
        med["wall_ms_runs"] = [round(r["wall_ms"], 3) for r in got[path]]
        med["memory_info"] = ctxs[path].memory_info()
        med["caller_fp64_bytes"] = 0 if path == "pcm" else B * T * 8
        res[path] = med
    res["k6_pcm_over_k6_plus_k3"] = res["pcm"]["output_ms"] / (res["two_step"]["output_ms"] + res["two_step"]["to_int16_ms"])
    print(json.dumps(res))
    for c in ctxs.values():
        c.close()


if __name__ == "__main__":
    main()
