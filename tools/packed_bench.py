"""afs_synthesize_ragged_packed against the strided ragged calls: B a:-vowel utterances
at 44.1 kHz, hop 441, frame counts drawn uniformly from 26 .. 101 with a fixed seed (tools/ragged_bench.py's
corpus), device-resident frames, seeds and audio, AFS_PROFILE contexts -- one per path, so that
memory_info() shows what each path alone allocates; the four paths alternated, medians over --reps.  The
paths: packed int16 and strided ragged int16 (afs_synthesize_ragged_pcm), packed float32 and the float64
ragged call (afs_synthesize_ragged).  Prints one JSON line: per path the K1 / K5 / K6 device times, the
call's wall time, memory_info() and the bytes of the caller's audio buffer; the K6 ratios with the runs
they are medians of; the useful / padded sample ratio (arithmetic on the lengths) beside the measured
buffer ratios; and whether the packed rows equal the strided ones.

Usage: python tools/packed_bench.py [--batch 8192] [--reps 3] [--lanes 16]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PATHS = ("packed_i16", "strided_i16", "packed_f32", "strided_f64")


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
    from areafunctionsynthesis_amd.synthesizer import Context, ragged_offsets

    fs, hop, B = 44100.0, 441, a.batch
    ctxs = {p: Context(fs, profile=True, lanes=a.lanes) for p in PATHS}
    f = ctxs[PATHS[0]].af_to_frames(np.asarray(default_shapes()["a:"], dtype=np.float64)[None])[0]
    f["velum_opening_cm2"] = 0.0
    f["glottis"] = DEFAULT_GLOTTIS
    counts = np.random.default_rng(20261020).integers(a.fmin, a.fmax + 1, size=B).astype(np.int32)
    Fmax = int(counts.max())
    frames = np.repeat(np.repeat(f[None, None], B, axis=0), Fmax, axis=1)
    dframes = torch.from_numpy(frames.view(np.uint8).reshape(B, Fmax, FRAME_DTYPE.itemsize)).cuda()
    seeds = torch.arange(1, B + 1, dtype=torch.int32).cuda()  # (the bits of uint32 1 .. B)
    T = (Fmax - 1) * hop
    off = ragged_offsets(counts, hop)
    useful = int(off[-1])
    out = {"packed_i16": torch.zeros(useful, dtype=torch.int16, device="cuda"),
           "strided_i16": torch.zeros((B, T), dtype=torch.int16, device="cuda"),
           "packed_f32": torch.zeros(useful, dtype=torch.float32, device="cuda"),
           "strided_f64": torch.zeros((B, T), dtype=torch.float64, device="cuda")}

    def run(path: str) -> dict:
        ctx = ctxs[path]
        ctx.kernel_times()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if path.startswith("packed"):
            ctx.synthesize_ragged(dframes, counts, hop, seeds=seeds, out=out[path], packed=True,
                                  pcm=path == "packed_i16", f32=path == "packed_f32")
        else:
            ctx.synthesize_ragged(dframes, counts, hop, seeds=seeds, out=out[path], pcm=path == "strided_i16")
        ctx.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        return dict(ctx.kernel_times(), wall_ms=wall)

    for path in PATHS:  # (warm-up: buffers grown, code objects resident)
        run(path)
    got = {p: [] for p in PATHS}
    for _ in range(a.reps):
        for path in PATHS:
            got[path].append(run(path))
    # the packed rows against the strided ones (row by row on the host)
    host = {p: out[p].cpu().numpy() for p in PATHS}
    lengths = np.diff(off)
    equal_i16 = all(np.array_equal(host["packed_i16"][off[u]:off[u + 1]], host["strided_i16"][u, :lengths[u]]) for u in range(B))
    equal_f32 = all(np.array_equal(host["packed_f32"][off[u]:off[u + 1]].view(np.uint32),
                                   np.float32(host["strided_f64"][u, :lengths[u]]).view(np.uint32)) for u in range(B))
    res = {"batch": B, "hop": hop, "frames": [a.fmin, a.fmax], "longest": Fmax, "reps": a.reps,
           "kernel": ctxs[PATHS[0]].synthesis_kernel(B), "useful_samples": useful, "padded_samples": B * T,
           "useful_over_padded": useful / (B * T), "rows_equal_i16": bool(equal_i16), "rows_equal_f32": bool(equal_f32)}
    for path in PATHS:
        med = {k: float(np.median([r[k] for r in got[path]])) for k in ("synth_ms", "plan_ms", "output_ms", "wall_ms")}
        med["output_ms_runs"] = [round(r["output_ms"], 3) for r in got[path]]
        med["wall_ms_runs"] = [round(r["wall_ms"], 3) for r in got[path]]
        med["memory_info"] = ctxs[path].memory_info()
        med["caller_buffer_bytes"] = int(out[path].numel() * out[path].element_size())
        res[path] = med
    res["k6_packed_i16_over_strided_i16"] = res["packed_i16"]["output_ms"] / res["strided_i16"]["output_ms"]
    res["k6_packed_f32_over_strided_f64"] = res["packed_f32"]["output_ms"] / res["strided_f64"]["output_ms"]
    res["buffer_packed_i16_over_strided_i16"] = res["packed_i16"]["caller_buffer_bytes"] / res["strided_i16"]["caller_buffer_bytes"]
    res["buffer_packed_f32_over_strided_f64"] = res["packed_f32"]["caller_buffer_bytes"] / res["strided_f64"]["caller_buffer_bytes"]
    print(json.dumps(res))
    for c in ctxs.values():
        c.close()


if __name__ == "__main__":
    main()
