"""Context.synthesize_corpus against Context.synthesize_stream and one afs_synthesize_ragged_pcm call
 on the workload of tools/stream_bench.py: B a:-vowel utterances at 44.1 kHz, hop 441,
frame counts drawn uniformly from 26 .. 101 with a fixed seed, int16 audio.  The corpus stream reads one
flat device array of frames by index and writes into one flat device buffer; it runs with --slots voices
and --chunks frames per step.  The old stream takes the corpus as host arrays through B voices; the single
call keeps frames and audio in device buffers.  One context per path, so that memory_info() shows what
each path alone holds; the paths alternated, medians over --reps.  Then one corpus run on an AFS_PROFILE
context with the session's calls timed from outside: wall time against the time inside the pool calls,
inside the restarts, and in the kernels (afs_kernel_times_ex).  Prints one JSON line.

Usage: python tools/corpus_bench.py [--batch 8192] [--reps 3] [--slots 8192,2048,512] [--chunks 10,25]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Timed:
    """A session seen through a stopwatch: what stream_corpus needs of it, with the time spent inside."""

    def __init__(self, session):
        self.session, self.batch, self.ctx = session, session.batch, session.ctx
        self.steps, self.step_ms, self.restarts, self.restart_ms = 0, 0.0, 0, 0.0

    def restart(self, voices, seeds=None):
        t0 = time.perf_counter()
        self.session.restart(voices, seeds)
        self.restarts += 1
        self.restart_ms += (time.perf_counter() - t0) * 1e3

    def synthesize_frames(self, *args, **kw):
        t0 = time.perf_counter()
        res = self.session.synthesize_frames(*args, **kw)
        self.steps += 1
        self.step_ms += (time.perf_counter() - t0) * 1e3
        return res


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slots", default="8192,2048,512")
    ap.add_argument("--chunks", default="10,25")
    ap.add_argument("--fmin", type=int, default=26)
    ap.add_argument("--fmax", type=int, default=101)
    ap.add_argument("--profile-slots", type=int, default=0, help="the profiled run's voices (0: --batch)")
    ap.add_argument("--profile-chunk", type=int, default=10)
    a = ap.parse_args()
    import torch

    from areafunctionsynthesis_amd.frames import DEFAULT_GLOTTIS, FRAME_DTYPE
    from areafunctionsynthesis_amd.params import default_shapes
    from areafunctionsynthesis_amd.synthesizer import Context, Synthesizer, ragged_offsets, stream_corpus

    fs, hop, B = 44100.0, 441, a.batch
    chunks = [int(c) for c in a.chunks.split(",")]
    slots = [min(int(s), B) for s in a.slots.split(",")]
    paths = ["ragged"] + [f"stream{c}" for c in chunks] + [f"corpus{s}x{c}" for s in slots for c in chunks]
    # (the same stream over a device corpus 8 bytes off a 16-byte boundary: every step copies the hull of its
    # live spans to the staging buffer first)
    paths += [f"corpus{slots[0]}x{chunks[0]}_misaligned", f"corpus{slots[-1]}x{chunks[0]}_misaligned"]
    ctxs = {p: Context(fs) for p in paths}
    f = ctxs["ragged"].af_to_frames(np.asarray(default_shapes()["a:"], dtype=np.float64)[None])[0]
    f["velum_opening_cm2"] = 0.0
    f["glottis"] = DEFAULT_GLOTTIS
    counts = np.random.default_rng(20261020).integers(a.fmin, a.fmax + 1, size=B).astype(np.int32)
    Fmax = int(counts.max())
    frames = np.repeat(np.repeat(f[None, None], B, axis=0), Fmax, axis=1)
    utterances = [frames[u, :counts[u]] for u in range(B)]  # (views of the host corpus)
    dframes = torch.from_numpy(frames.view(np.uint8).reshape(B, Fmax, FRAME_DTYPE.itemsize)).cuda()
    frame_offsets = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    flat_frames = torch.from_numpy(np.repeat(f[None], int(frame_offsets[-1])).view(np.uint8)).cuda()  # (one flat corpus)
    shifted = torch.zeros(flat_frames.numel() + 16, dtype=torch.uint8, device="cuda")[8:8 + flat_frames.numel()]
    shifted.copy_(flat_frames)
    assert shifted.data_ptr() % 16 == 8
    seeds = torch.arange(1, B + 1, dtype=torch.int32).cuda()  # (the bits of uint32 1 .. B)
    offsets = ragged_offsets(counts, hop)
    useful = int(offsets[-1])
    out = torch.zeros((B, (Fmax - 1) * hop), dtype=torch.int16, device="cuda")
    flat_out = torch.zeros(useful, dtype=torch.int16, device="cuda")
    probe = [0, B // 2, B - 1]  # (the utterances compared between the paths)
    check = {}

    def run(path: str) -> float:
        ctx = ctxs[path]
        t0 = time.perf_counter()
        if path == "ragged":
            ctx.synthesize_ragged(dframes, counts, hop, seeds=seeds, out=out, pcm=True)
        elif path.startswith("stream"):
            n = 0
            for i, audio in ctx.synthesize_stream(utterances, hop, B, int(path[6:]), pcm=True):
                n += audio.size
                if i in probe:
                    check[path, i] = audio
            assert n == useful
        else:
            s, c = (int(x) for x in path[6:].split("_")[0].split("x"))
            src = shifted if path.endswith("_misaligned") else flat_frames
            ctx.synthesize_corpus(src, frame_offsets, hop, s, c, pcm=True, out=flat_out)
        ctx.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        for i in probe:
            if path == "ragged":
                check[path, i] = out[i, :(counts[i] - 1) * hop].cpu().numpy()
            elif path.startswith("corpus"):
                check[path, i] = flat_out[offsets[i]:offsets[i + 1]].cpu().numpy()
        return ms

    for p in paths:  # (warm-up: buffers grown, code objects resident)
        run(p)
    got = {p: [] for p in paths}
    for _ in range(a.reps):
        for p in paths:
            got[p].append(run(p))
    res = {"batch": B, "hop": hop, "frames": [a.fmin, a.fmax], "longest": Fmax, "reps": a.reps,
           "kernel": ctxs["ragged"].synthesis_kernel(B), "useful_samples": useful, "corpus_frames": int(frame_offsets[-1]),
           "probed_utterances_equal": all(np.array_equal(check[p, i], check["ragged", i]) for p in paths for i in probe)}
    for p in paths:
        wall = float(np.median(got[p]))
        res[p] = {"wall_ms": wall, "wall_ms_runs": [round(x, 1) for x in got[p]],
                  "useful_samples_per_s": useful / (wall * 1e-3), "vs_ragged": float(np.median(got["ragged"])) / wall,
                  "memory_info": ctxs[p].memory_info()}
    for c in ctxs.values():
        c.close()

    # where a step's time goes: one corpus run on a profiling context, the session's calls timed from outside
    ps, pc = min(a.profile_slots or B, B), a.profile_chunk
    ctx = Context(fs, profile=True)
    split = {}
    for rep in range(2):  # (the first run grows the buffers)
        session = Timed(Synthesizer(ctx, ps))
        ctx.kernel_times()
        t0 = time.perf_counter()
        stream_corpus(session, flat_frames, frame_offsets, hop, pc, pcm=True, out=flat_out)
        wall = (time.perf_counter() - t0) * 1e3
        kt = ctx.kernel_times()
        session.session.close()
        split = {"slots": ps, "chunk_frames": pc, "wall_ms": wall, "steps": session.steps,
                 "in_pool_calls_ms": session.step_ms, "restarts": session.restarts, "in_restarts_ms": session.restart_ms,
                 "scheduler_ms": wall - session.step_ms - session.restart_ms,
                 "kernel_ms": kt["synth_ms"] + kt["plan_ms"] + kt["output_ms"], "kernel_times": kt}
    ctx.close()
    res["profile_split"] = split
    print(json.dumps(res))


if __name__ == "__main__":
    main()
