"""Generate the golden vectors in tests/golden/ from the REFERENCE build.

Run in the build container (needs /root/reference for oracle/_ref):
    python tests/golden/make_golden.py          (all files)
    python tests/golden/make_golden.py int16    (int16.npz only)
    python tests/golden/make_golden.py target_seq (target_seq.npz only)
    python tests/golden/make_golden.py generic  (generic_tubes.npz only)

Every expected value comes from oracle/_ref/libafsref.so -- the reference's own
TdsModel / Tube / TriangularGlottis / IirFilter sources compiled unmodified and driven
through their public API -- or from glibc itself (rand).  Inputs (frames) are stored
next to the outputs so the GPU box needs neither the reference nor the generator.

The one exception is af_frames.npz: OneDimAreaFunction is not buildable from the
reference here (wxWidgets), so those expected frames come from the C restatement and
are marked "restatement" (parity against the reference unpinned for that row).
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from oracle_lib import Oracle, RefLib  # noqa: E402

from areafunctionsynthesis_amd.frames import DEFAULT_GLOTTIS, FRAME_DTYPE  # noqa: E402
from areafunctionsynthesis_amd.params import default_shapes  # noqa: E402


def static(o: Oracle, shape, F, velum=0.0, glottis=DEFAULT_GLOTTIS):
    f = o.af_to_frame(shape)
    f["velum_opening_cm2"] = velum
    f["glottis"] = glottis
    return np.repeat(f[None], F)


def trajectory(o: Oracle, shapes, names, F, rng, lateral=False):
    fr = np.zeros(F, FRAME_DTYPE)
    for k in range(F):
        f = o.af_to_frame(shapes[names[k * len(names) // F]] * (1 + 0.01 * rng.standard_normal(16)))
        f["velum_opening_cm2"] = 0.3 if k % 3 == 0 else 0.0
        if lateral:
            f["laterality"] = np.clip(rng.uniform(-0.2, 0.3, 40), 0, 1)
        f["glottis"] = [110 + 20 * np.sin(k), 8000 - 200 * k, 0.01, 0.012, 0.01 * (k % 2), -40 + 3 * k]
        fr[k] = f
    return fr


def int16_inputs() -> np.ndarray:
    """Edge cases of the output stage (Synthesizer.cpp:955-973): exact +-1, just past +-1,
    large magnitudes, signed zeros, NaN, values on and between int16 steps, random audio."""
    eps = np.finfo(np.float64).eps
    edge = [0.0, -0.0, 1.0, -1.0, 1.0 + eps, -1.0 - eps, 1.0 - eps / 2, -1.0 + eps / 2, 2.0, -2.0, 1e300,
            -1e300, np.inf, -np.inf, np.nan, 0.5, -0.5, 1 / 32767, -1 / 32767, 0.99999 / 32767,
            -0.99999 / 32767, 32766.5 / 32767, -32766.5 / 32767, 1e-320]
    rng = np.random.default_rng(16)
    return np.concatenate([np.array(edge), rng.uniform(-1.2, 1.2, 4000), rng.standard_normal(4000) * 0.3])


def write_int16(ref: RefLib) -> None:
    x = int16_inputs()
    np.savez_compressed(os.path.join(HERE, "int16.npz"), x=x, out=ref.to_int16(x))


def write_target_seq(o: Oracle, ref: RefLib) -> None:
    """playTargetSequence (Synthesizer.cpp:1299-1422): the trajectory frames come from the
    restatement (Synthesizer.cpp is not buildable here), the audio from the reference build
    playing them with one synthesizeSignalTds(.., 1) call per sample."""
    sh = default_shapes()
    names = ["a:", "(a)b(a):", "u:", "(u)g(u):", "i:", "(i)d(i):"]
    shapes = np.stack([sh[n] for n in names])
    targets = np.array([[0, 1, 0, 0], [2, 3, 2, 2], [4, 5, 4, 4], [1, 0, 5, 2]], dtype=np.int32)
    seeds = np.array([1, 2, 3, 11], dtype=np.uint32)
    st, tr, fs = [0.02, 0.01, 0.02, 0.01], [0.01, 0.01, 0.01], 44100.0
    timing = {"stationary_s": st, "transition_s": tr}
    outs = [ref.utterance(o.target_frames(shapes[t], fs, timing), 1, int(s), fs) for t, s in zip(targets, seeds)]
    np.savez_compressed(os.path.join(HERE, "target_seq.npz"), names=np.array(names), shapes=shapes,
                        targets=targets, seeds=seeds, stationary_s=np.array(st), transition_s=np.array(tr),
                        fs=fs, out=np.stack(outs))


def write_fulcher(ref: RefLib) -> None:
    """The reference's own printout of Fulcher et al. (2011) Table I
    (TdsModel::checkGlottalEntranceLossCoeffFlucher2011, TdsModel.cpp:1100-1181)."""
    with open(os.path.join(HERE, "fulcher_table.txt"), "w") as fh:
        fh.write(ref.fulcher_table())


def write_generic(o: Oracle, ref: RefLib) -> None:
    """Tubes the area-function model cannot make (tests/generic_tubes.py golden_cases: unequal section
    lengths, broken tongue runs, teeth anywhere): the frames, and the reference build's first 2048
    samples and rand() call count of every utterance."""
    from generic_tubes import GOLDEN_SAMPLES, golden_cases
    cases = golden_cases(o)
    outs = np.zeros((len(cases), GOLDEN_SAMPLES))
    num_out, calls = [], []
    for i, (label, fr, hop, seed, fs) in enumerate(cases):
        c0 = int(ref.lib.afsref_rand_calls())
        y = ref.utterance(fr, hop, seed, fs)[:GOLDEN_SAMPLES]
        calls.append(int(ref.lib.afsref_rand_calls()) - c0)
        outs[i, : y.size] = y
        num_out.append(y.size)
    frames = np.ascontiguousarray(np.stack([c[1] for c in cases]))
    np.savez_compressed(os.path.join(HERE, "generic_tubes.npz"), names=np.array([c[0] for c in cases]),
                        frames=frames.view(np.uint8).reshape(frames.shape + (FRAME_DTYPE.itemsize,)),
                        hop=np.array([c[2] for c in cases]), seed=np.array([c[3] for c in cases]),
                        fs=np.array([c[4] for c in cases]), out=outs, num_out=np.array(num_out),
                        rand_calls=np.array(calls, dtype=np.int64))


def main() -> None:
    if sys.argv[1:] == ["generic"]:
        write_generic(Oracle(), RefLib())
        return
    if sys.argv[1:] == ["fulcher"]:
        write_fulcher(RefLib())
        return
    if sys.argv[1:] == ["int16"]:
        write_int16(RefLib())
        return
    if sys.argv[1:] == ["target_seq"]:
        write_target_seq(Oracle(), RefLib())
        return
    o = Oracle()
    r = RefLib()
    sh = default_shapes()

    # glibc rand() streams (srand(seed) then rand()), seeds 1..4 and two large ones
    seeds = np.array([1, 2, 3, 4, 12345, 4294967295], dtype=np.uint64)
    np.savez_compressed(os.path.join(HERE, "rand_glibc.npz"), seeds=seeds,
                        values=np.stack([r.glibc_rand(int(s), 4096) for s in seeds]))

    # IirFilter::createChebyshev for the output filter at both rates, plus other orders
    cases = [(7000 / 22050, 8), (7000 / 44100, 8), (25 / 44100, 4), (50 / 22050, 4), (0.1, 6)]
    a_all, b_all = [], []
    for ratio, poles in cases:
        a, b = r.chebyshev(ratio, poles)
        a_all.append(np.pad(a, (0, 9 - a.size)))
        b_all.append(np.pad(b, (0, 9 - b.size)))
    np.savez_compressed(os.path.join(HERE, "chebyshev.npz"), ratio=np.array([c[0] for c in cases]),
                        poles=np.array([c[1] for c in cases]), a=np.stack(a_all), b=np.stack(b_all))

    # per-step state of static /a:/ at 22050 Hz: pressures and currents after every sample
    fr = static(o, sh["a:"], 2)
    h = r.create(22050.0, 1)
    r.call(h, fr[0], 64)
    P, U, Y = [], [], []
    for _ in range(64):
        Y.append(r.call(h, fr[1], 1)[0])
        P.append(r.pressures(h))
        U.append(r.currents(h))
    r.destroy(h)
    np.savez_compressed(os.path.join(HERE, "steps_a.npz"), frames=fr, fs=22050.0, seed=1,
                        pressures=np.stack(P), currents=np.stack(U), out=np.array(Y))

    # whole utterances: inputs + reference outputs
    rng = np.random.default_rng(2024)
    cases = [
        ("a:", static(o, sh["a:"], 11), 220, 1, 22050.0),
        ("i:", static(o, sh["i:"], 11), 220, 2, 22050.0),
        ("u:@44k", static(o, sh["u:"], 11), 441, 3, 44100.0),
        ("s+velum", static(o, sh["s"], 11, velum=1.0), 220, 4, 22050.0),
        ("f", static(o, sh["f"], 11), 220, 5, 22050.0),
        ("(a)b(a):", static(o, sh["(a)b(a):"], 11), 220, 6, 22050.0),
        ("vcv-aba@44k", trajectory(o, sh, ["a:", "(a)b(a):", "a:"], 12, rng), 200, 7, 44100.0),
        ("x-lateral", trajectory(o, sh, ["x", "S", "C"], 12, rng, lateral=True), 200, 0, 22050.0),
    ]
    names, frames, hops, useeds, fss, outs = [], [], [], [], [], []
    for name, fr, hop, seed, fs in cases:
        y = r.utterance(fr, hop, seed, fs)[:2048]
        names.append(name)
        frames.append(fr)
        hops.append(hop)
        useeds.append(seed)
        fss.append(fs)
        outs.append(y)
    Fmax = max(f.size for f in frames)
    fpad = np.zeros((len(frames), Fmax), FRAME_DTYPE)
    nfr = np.array([f.size for f in frames])
    for i, f in enumerate(frames):
        fpad[i, : f.size] = f
    np.savez_compressed(os.path.join(HERE, "utterances.npz"), names=np.array(names), frames=fpad.view(np.uint8),
                        num_frames=nfr, hop=np.array(hops), seed=np.array(useeds), fs=np.array(fss),
                        out=np.stack(outs))

    # area function -> tube (restatement; reference unbuildable for this row)
    names = sorted(sh)
    P = np.stack([sh[n] for n in names])
    F = np.stack([o.af_to_frame(p) for p in P])
    np.savez_compressed(os.path.join(HERE, "af_frames.npz"), names=np.array(names), params=P,
                        area=F["area_cm2"], length=F["length_cm"], articulator=F["articulator"],
                        teeth=F["teeth_position_cm"], source=np.array("restatement"))
    write_int16(r)
    write_fulcher(r)
    write_target_seq(o, r)
    write_generic(o, r)
    print("golden vectors written to", HERE)


if __name__ == "__main__":
    main()
