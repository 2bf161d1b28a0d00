"""Packed ragged output and float32 samples on the GPU (afs_synthesize_f32, afs_synthesize_ragged_packed,
afs_session_synthesize_ragged_packed; Context.synthesize(f32=True), Context.synthesize_ragged(packed=True),
Synthesizer.synthesize_frames(packed=True)).

The corpus is tests/test_ragged_gpu.py's: 21 utterances of 2 .. 7 frames (a: -> s glides with a velum of
their own, so the noise sources fire), seeds 101 + 7u, here at hop 37 -- odd, so that tightly packed rows
start at every alignment mod 4 (float32) and, with the odd-based and reversed layouts, mod 8 (int16; in
call order alone the 21 lengths reach 7 of the 8, tests/test_packed_cpu.py).  The yardstick is the call
that exists without the packed form: row u of a packed int16 call is row u of synthesize_ragged(...,
pcm=True), row u of a packed float32 call is np.float32 of synthesize_ragged's float64 row, bit for bit,
with the rand() counts, the non-finite flags and report.samples equal.  Those references are computed once
per lane width and left unchanged.  Every destination is filled with a canary no kernel computes, with a
margin before the first and after the last row: a whole-buffer comparison shows that nothing outside the
rows is written."""
import ctypes

import numpy as np
import pytest

from areafunctionsynthesis_amd import _native
from areafunctionsynthesis_amd.frames import DEFAULT_GLOTTIS, FRAME_DTYPE
from areafunctionsynthesis_amd.params import default_shapes
from areafunctionsynthesis_amd.synthesizer import ragged_offsets
from taps_lib import FS, glide_frames

pytestmark = pytest.mark.gpu

NF = np.array([7, 2, 5, 5, 3, 7, 2, 5, 5, 5, 5, 5, 5, 5, 5, 4, 5, 6, 6, 2, 3], dtype=np.int32)
FSTRIDE = 8
HOP = 37
ONE_WAVE_B = 1025  # (64 lanes: batches above TREE_PAIR64_MAX = 1024 run one wave per utterance)
MARGIN = 8         # canary samples before the first and after the last row (16 bytes of int16: a whole store)
FORMATS = ("i16", "f32")
DTYPE = {"i16": np.int16, "f32": np.float32}
UINT = {"i16": np.uint16, "f32": np.uint32}
CANARY = {"i16": np.uint16(0x5A5B), "f32": np.uint32(0x7FA5C3E1)}  # (the float: a NaN no cast of a double gives)
KERNELS = {"pair16": (16, len(NF), "tree_pair_kernel"), "pair64": (64, 5, "tree_pair64_kernel"),
           "one_wave64": (64, ONE_WAVE_B, "tree_synth_kernel")}

_CACHE = {}


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.fixture(scope="module")
def make_ctx(monkeypatch_module):
    from areafunctionsynthesis_amd.synthesizer import Context
    made = {}

    def make(lanes=16, env=None, solver="tree"):
        key = (lanes, tuple(sorted((env or {}).items())), solver)
        if key not in made:
            for k, v in (env or {}).items():
                monkeypatch_module.setenv(k, v)
            try:
                made[key] = Context(FS, solver=solver, lanes=lanes if solver == "tree" else None)
            finally:
                for k in env or {}:
                    monkeypatch_module.delenv(k)
        return made[key]

    yield make
    for c in made.values():
        c.close()


def base(oracle):
    """(frames[21, 8], seeds[21]): utterance u glides a: -> s over its NF[u] frames with a velum of its own;
    the frames past its count are poison (every double NaN)."""
    if "base" not in _CACHE:
        poison = np.zeros((), dtype=FRAME_DTYPE)
        for name in FRAME_DTYPE.names:
            if FRAME_DTYPE[name].base.kind == "f":
                poison[name] = np.nan
        frames = np.empty((len(NF), FSTRIDE), dtype=FRAME_DTYPE)
        frames[...] = poison
        for u, F in enumerate(NF):
            frames[u, :F] = glide_frames(oracle, int(F), 0.3 + 0.03 * u)
        seeds = (101 + 7 * np.arange(len(NF))).astype(np.uint32)
        frames.setflags(write=False)
        seeds.setflags(write=False)
        _CACHE["base"] = (frames, seeds)
    return _CACHE["base"]


def batch(oracle, B):
    """The first B utterances, or the 21 tiled up to B: (frames, counts, seeds)."""
    frames, seeds = base(oracle)
    idx = np.arange(B) % len(NF)
    return np.ascontiguousarray(frames[idx]), np.ascontiguousarray(NF[idx]), np.ascontiguousarray(seeds[idx])


def lengths_of(counts, hop=HOP):
    return (counts.astype(np.int64) - 1) * hop


def references(make_ctx, oracle, kernel):
    """The strided calls on a default context of the kernel's lane width: {"i16": rows of
    synthesize_ragged(pcm=True) as uint16, "f32": np.float32 of synthesize_ragged's rows as uint32, "draws",
    "nonfinite", "samples"}.  Computed once, read-only."""
    key = ("ref", kernel)
    if key not in _CACHE:
        lanes, B, name = KERNELS[kernel]
        ctx = make_ctx(lanes)
        assert ctx.synthesis_kernel(B) == name
        frames, counts, seeds = batch(oracle, B)
        T = lengths_of(counts)
        y, _, rep = ctx.synthesize_ragged(frames, counts, HOP, seeds=seeds, report=True)
        draws = ctx.rng_draws(B)
        p, _, prep = ctx.synthesize_ragged(frames, counts, HOP, seeds=seeds, report=True, pcm=True)
        assert np.array_equal(ctx.rng_draws(B), draws) and prep["samples"] == rep["samples"] == int(T.sum())
        assert (draws > 0).any()  # (the noise sources fire)
        ref = {"i16": [np.ascontiguousarray(p[u, :T[u]]).view(np.uint16) for u in range(B)],
               "f32": [np.float32(y[u, :T[u]]).view(np.uint32) for u in range(B)],
               "draws": draws, "nonfinite": rep["nonfinite"].copy(), "samples": rep["samples"]}
        for rows in (ref["i16"], ref["f32"]):
            for r in rows:
                r.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def canary_buffer(fmt, n):
    return np.full(n, CANARY[fmt], dtype=UINT[fmt])


def packed_call(ctx, oracle, kernel, fmt, offsets=None, device=False, shift=0):
    """One packed call of the kernel's batch into a canary-filled buffer whose first row sample sits MARGIN +
    shift samples in (device: a torch tensor sliced there): (buffer as unsigned ints, the row starts in the
    buffer, report, draws)."""
    lanes, B, _ = KERNELS[kernel]
    frames, counts, seeds = batch(oracle, B)
    T = lengths_of(counts)
    starts = ragged_offsets(counts, HOP)[:-1] if offsets is None else np.asarray(offsets, dtype=np.int64)
    span = int((starts + T).max())
    lead = MARGIN + shift
    buf = canary_buffer(fmt, lead + span + MARGIN)
    if device:
        import torch
        dev = torch.from_numpy(buf.view(DTYPE[fmt])).cuda()
        dest = dev[lead:lead + span]
        assert (dest.data_ptr() - dev.data_ptr()) == lead * buf.itemsize and dev.data_ptr() % 16 == 0
    else:
        dest = buf.view(DTYPE[fmt])[lead:lead + span]
    res = ctx.synthesize_ragged(frames, counts, HOP, seeds=seeds, out=dest, report=True, packed=True,
                                pcm=fmt == "i16", f32=fmt == "f32", offsets=offsets)
    flat, off, rep = res
    assert flat is dest
    if offsets is None:  # tight packing: no gaps, the total in offsets[B]
        assert off.dtype == np.int64 and off.shape == (B + 1,)
        assert off[0] == 0 and np.array_equal(np.diff(off), T) and off[B] == span == int(T.sum())
    else:
        assert np.array_equal(off, offsets)
    draws = ctx.rng_draws(B)
    if device:
        buf = dev.cpu().numpy().view(UINT[fmt])
    return buf, starts + lead, rep, draws


def check_packed(buf, at, rep, draws, ref, fmt):
    """The whole buffer: every row its reference bit for bit, a canary everywhere else; the counts equal."""
    want = canary_buffer(fmt, buf.size)
    for u, row in enumerate(ref[fmt]):
        want[at[u]:at[u] + row.size] = row
    bad = np.flatnonzero(buf != want)
    assert bad.size == 0, f"{fmt}: {bad.size} samples differ, the first at {bad[:5]} (row starts {at[:6]} ..)"
    assert np.array_equal(draws, ref["draws"])
    assert np.array_equal(rep["nonfinite"], ref["nonfinite"]) and rep["nonfinite_utterances"] == 0
    assert rep["samples"] == ref["samples"]


# ---- 1. packed rows equal the strided calls' --------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_tight_rows_equal_strided_rows(make_ctx, oracle, kernel, fmt):
    """Tight packing through the three synthesis kernels (hop records): 21 utterances at 16 lanes into a
    device tensor, 5 as 64-lane pairs and the 21 tiled to 1025 through the one-wave kernel into host arrays."""
    lanes, B, _ = KERNELS[kernel]
    assert HOP >= _native.AFS_PLAN_HOP_MIN and HOP % 2 == 1
    if kernel == "pair16":  # (arithmetic on the lengths: tests/test_packed_cpu.py has the same without a GPU)
        starts = ragged_offsets(NF, HOP)[:-1]
        assert set(starts % 4) == set(range(4))
        assert set(starts % 8) | set((starts + 1) % 8) == set(range(8))
    res = packed_call(make_ctx(lanes), oracle, kernel, fmt, device=kernel == "pair16")
    check_packed(*res, references(make_ctx, oracle, kernel), fmt)


@pytest.mark.parametrize("fmt", FORMATS)
def test_dense_plan(make_ctx, oracle, fmt):
    """AFS_PLAN_DENSE=1: the chunked path with dense records, K6 after every chunk."""
    res = packed_call(make_ctx(16, env={"AFS_PLAN_DENSE": "1"}), oracle, "pair16", fmt, device=True)
    check_packed(*res, references(make_ctx, oracle, "pair16"), fmt)


@pytest.mark.parametrize("per", [50, 66])
def test_rows_continue_across_launches(make_ctx, oracle, per):
    """Launches of 50 and 66 samples at hop 37 (rows end at 37, 74, .. 222): a row goes on at row_base[u] +
    s_begin in the next launch, so every row is written in pieces of alignments of their own, and rows end
    inside a launch and before one starts.  16 lanes and 64-lane pairs, both formats."""
    for kernel in ("pair16", "pair64"):
        ctx = make_ctx(KERNELS[kernel][0], env={"AFS_LAUNCH_SAMPLES": str(per)})
        for fmt in FORMATS:
            res = packed_call(ctx, oracle, kernel, fmt, device=fmt == "f32")
            check_packed(*res, references(make_ctx, oracle, kernel), fmt)


def test_chunked_hop_path(make_ctx, oracle):
    """1025 rows x 6 hop records exceed a plan budget of 1 MB: run_chunked plays one hop per chunk."""
    ctx = make_ctx(16, env={"AFS_PLAN_BUDGET_MB": "1"})
    lanes, B, _ = KERNELS["one_wave64"]
    key = ("ref", "chunk16")
    if key not in _CACHE:  # (the 1025 rows at 16 lanes: a reference of its own, from the default context)
        KERNELS["chunk16"] = (16, B, "tree_pair_kernel")
        _CACHE[key] = references(make_ctx, oracle, "chunk16")
    for fmt in FORMATS:
        res = packed_call(ctx, oracle, "chunk16", fmt)
        check_packed(*res, _CACHE[key], fmt)


# ---- 2. layouts -----------------------------------------------------------------------------------------

def gapped_offsets():
    """Row u starts 0 .. 3 samples after row u - 1 ends (u % 4: every gap beside every alignment)."""
    T = lengths_of(NF)
    at, offs = 0, []
    for u in range(len(NF)):
        at += u % 4
        offs.append(at)
        at += int(T[u])
    return np.array(offs, dtype=np.int64)


def reversed_offsets():
    """The last utterance first in the buffer, tightly."""
    T = lengths_of(NF)
    offs = np.zeros(len(NF), dtype=np.int64)
    offs[::-1] = ragged_offsets(NF[::-1], HOP)[:-1]
    assert offs[-1] == 0 and offs[0] == int(T[1:].sum()) and (np.diff(offs) < 0).all()
    return offs


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("where", ["device", "host"])
def test_caller_offsets_with_gaps(make_ctx, oracle, where, fmt):
    """Gaps of 0 .. 3 canary samples between the rows, margins before the first and after the last: all
    intact, in a device tensor and in a host array (staged: uploaded first, copied back whole)."""
    offs = gapped_offsets()
    assert set(np.diff(offs) - lengths_of(NF)[:-1]) == {0, 1, 2, 3}
    res = packed_call(make_ctx(16), oracle, "pair16", fmt, offsets=offs, device=where == "device")
    check_packed(*res, references(make_ctx, oracle, "pair16"), fmt)


@pytest.mark.parametrize("fmt", FORMATS)
def test_reversed_offsets(make_ctx, oracle, fmt):
    res = packed_call(make_ctx(16), oracle, "pair16", fmt, offsets=reversed_offsets(), device=True)
    check_packed(*res, references(make_ctx, oracle, "pair16"), fmt)


@pytest.mark.parametrize("fmt", FORMATS)
def test_device_base_at_an_odd_sample(make_ctx, oracle, fmt):
    """The destination starts one sample past a 16-byte boundary of a device tensor: every row's alignment
    moves by one (int16: the eighth residue mod 8 that tight packing in call order does not reach)."""
    res = packed_call(make_ctx(16), oracle, "pair16", fmt, device=True, shift=1)
    assert (res[1][0] - 0) % 2 == 1
    check_packed(*res, references(make_ctx, oracle, "pair16"), fmt)


# ---- 3. refusals ----------------------------------------------------------------------------------------

def test_refusals(make_ctx, oracle):
    """Overlapping rows, a negative offset, an unknown format, a missing or misaligned destination, offsets
    for a strided call, the one-lane solvers: refused on the host, the canary-filled buffer untouched."""
    import torch
    ctx = make_ctx(16)
    frames, counts, seeds = batch(oracle, len(NF))
    T = lengths_of(counts)
    tight = ragged_offsets(counts, HOP)
    span = int(tight[-1])

    def refused(status, fmt, offsets, device, ctx=ctx, code=None, dest=None):
        buf = canary_buffer(fmt, span + 64)
        out = torch.from_numpy(buf.view(DTYPE[fmt])).cuda() if device else buf.view(DTYPE[fmt])
        with pytest.raises(_native.AfsError, match=_native.STATUS[status]):
            if code is None:
                ctx.synthesize_ragged(frames, counts, HOP, seeds=seeds, out=out, packed=True, pcm=fmt == "i16",
                                      f32=fmt == "f32", offsets=offsets)
            else:  # (a format or a destination the binding would not pass)
                offs = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
                addr = int(out.data_ptr() if device else out.ctypes.data) if dest is None else dest
                st = ctx._lib.afs_synthesize_ragged_packed(
                    ctx.handle, ctypes.c_void_p(frames.ctypes.data), FSTRIDE, ctypes.c_void_p(counts.ctypes.data),
                    ctypes.c_void_p(seeds.ctypes.data), len(NF), HOP, code, ctypes.c_void_p(addr),
                    ctypes.c_void_p(offs.ctypes.data if offs is not None else 0), None, None)
                _native.check(st, ctx.handle, "afs_synthesize_ragged_packed")
        got = out.cpu().numpy().view(UINT[fmt]) if device else buf
        assert (got == CANARY[fmt]).all()

    for fmt in FORMATS:
        for device in (True, False):
            over = tight[:-1].copy()
            over[5] -= 1  # row 5 starts on row 4's last sample
            refused(1, fmt, over, device)
            inside = tight[:-1].copy()
            inside[20] = tight[0] + 3  # the last row inside the first (7 frames hold 3 + 2 * 37 samples)
            assert T[20] + 3 <= T[0]
            refused(1, fmt, inside, device)
            neg = tight[:-1] + 8
            neg[1] = -1
            refused(1, fmt, neg, device)
        refused(1, fmt, tight[:-1], True, code=2)
        refused(1, fmt, tight[:-1], True, code=-1)
        refused(1, fmt, tight[:-1], True, code=_native.AFS_SAMPLE_F32 if fmt == "f32" else 0, dest=0)
        refused(5, fmt, None, False, ctx=make_ctx(None, solver="cholesky"))
    # a float destination at an odd 2-byte address
    buf = canary_buffer("i16", 2 * span + 64)
    st = ctx._lib.afs_synthesize_ragged_packed(
        ctx.handle, ctypes.c_void_p(frames.ctypes.data), FSTRIDE, ctypes.c_void_p(counts.ctypes.data),
        ctypes.c_void_p(seeds.ctypes.data), len(NF), HOP, _native.AFS_SAMPLE_F32, ctypes.c_void_p(buf.ctypes.data + 2),
        None, None, None)
    assert st == 1 and (buf == CANARY["i16"]).all()
    # abutting rows in any order are no overlap (the reversed layout above); the binding's own refusals
    with pytest.raises(ValueError, match="no packed float64 form"):
        ctx.synthesize_ragged(frames, counts, HOP, seeds=seeds, packed=True)
    with pytest.raises(ValueError, match="pcm and f32"):
        ctx.synthesize_ragged(frames, counts, HOP, seeds=seeds, packed=True, pcm=True, f32=True)
    with pytest.raises(ValueError, match="pcm and f32"):
        ctx.synthesize(np.ascontiguousarray(frames[:2, :2]), HOP, pcm=True, f32=True)


# ---- 4. the uniform float32 call ---------------------------------------------------------------------------

def uniform_batch(oracle):
    if "uniform" not in _CACHE:
        frames = np.stack([glide_frames(oracle, 4, 0.3 + 0.05 * u) for u in range(9)])
        frames.setflags(write=False)
        _CACHE["uniform"] = frames
    return _CACHE["uniform"]


@pytest.mark.parametrize("lanes,env", [(16, None), (64, None), (16, {"AFS_LAUNCH_SAMPLES": "50"})])
def test_uniform_f32(make_ctx, oracle, lanes, env):
    """synthesize(f32=True) into rows of stride T + 6 (9 rows of 111 samples at stride 117: the rows start at every alignment mod
    4): np.float32 of the float64 call bit for bit, canaries in the padding, the same counts; also in launches
    of 50 samples (a row goes on at s_begin)."""
    import torch
    frames = uniform_batch(oracle)
    B, T = frames.shape[0], 3 * HOP
    assert set((np.arange(B) * (T + 6)) % 4) == set(range(4))
    key = ("uniform-ref", lanes)
    if key not in _CACHE:
        y, rep = make_ctx(lanes).synthesize(frames, HOP, report=True)
        _CACHE[key] = (np.float32(y).view(np.uint32), make_ctx(lanes).rng_draws(B), rep)
    want, draws, rep64 = _CACHE[key]
    ctx = make_ctx(lanes, env)
    for device in (True, False):
        buf = canary_buffer("f32", B * (T + 6)).reshape(B, T + 6)
        wide = torch.from_numpy(buf.view(np.float32)).cuda() if device else buf.view(np.float32)
        out, rep = ctx.synthesize(frames, HOP, out=wide[:, :T], report=True, f32=True)
        got = wide.cpu().numpy().view(np.uint32) if device else buf
        assert np.array_equal(got[:, :T], want)
        assert (got[:, T:] == CANARY["f32"]).all()
        assert np.array_equal(ctx.rng_draws(B), draws) and (draws > 0).any()
        assert rep["samples"] == rep64["samples"] == B * T and not rep["nonfinite"].any()
    y32 = ctx.synthesize(frames, HOP, f32=True)  # (an array of the binding's own)
    assert y32.dtype == np.float32 and y32.shape == (B, T) and np.array_equal(y32.view(np.uint32), want)


def test_uniform_f32_keeps_nonfinite_values(make_ctx, oracle):
    """tests/test_gpu_parity.py test_nonfinite_is_reported's batch: utterances 2, 5 and 6 go non-finite.  The
    flags are the float64 call's, and the float32 rows hold the casts of the float64 rows' NaNs and infinities
    -- where the int16 form stores 0 and the clipped value."""
    sh = default_shapes()
    B, F, hop = 9, 4, 120
    frames = np.zeros((B, F), FRAME_DTYPE)
    for u in range(B):
        f = oracle.af_to_frame(sh[("a:", "s", "i:")[u % 3]])
        f["glottis"] = DEFAULT_GLOTTIS
        frames[u] = np.repeat(f[None], F)
    bad = [2, 5, 6]
    frames["area_cm2"][2, 2, 10] = np.nan
    frames["glottis"][5, 1:, 1] = np.nan
    frames["length_cm"][6, 3, 30] = np.inf
    from areafunctionsynthesis_amd.synthesizer import Context
    ctx = Context(22050.0, lanes=16)  # (that test's sampling rate)
    try:
        y, rep = ctx.synthesize(frames, hop, report=True)
        y32, rep32 = ctx.synthesize(frames, hop, report=True, f32=True)
    finally:
        ctx.close()
    assert list(np.flatnonzero(rep["nonfinite"])) == bad == list(np.flatnonzero(rep32["nonfinite"]))
    assert rep32["nonfinite_utterances"] == len(bad)
    want = np.float32(y)
    assert np.array_equal(np.isnan(y32), np.isnan(y)) and np.array_equal(np.isinf(y32), np.isinf(y))
    for u in bad:
        assert not np.isfinite(y32[u]).all(), u
    assert np.array_equal(y32.view(np.uint32), want.view(np.uint32))


# ---- 5. voice pools ---------------------------------------------------------------------------------------

def test_pool_packed_calls_alternate(make_ctx, oracle):
    """A session of 5 voices over a strided float64 call, a packed float32 call at the caller's offsets, a
    tightly packed int16 call and a strided int16 call.  In the packed calls voice 4 is idle (in the first its
    offset lies inside voice 0's row: not looked at, nothing of it written), voice 3 is unlatched in the first
    and voices 0 .. 2 are latched.  Each voice's pieces, concatenated, are Context.synthesize on its utterance
    alone: the float64 piece bit for bit, the float32 pieces its np.float32, the int16 pieces the rows of
    synthesize(pcm=True) -- the filter state goes through all four forms."""
    from areafunctionsynthesis_amd.synthesizer import Synthesizer
    frames, seeds = base(oracle)
    voices = [0, 5, 17, 18]
    assert list(NF[voices]) == [7, 7, 6, 6]
    ctx = make_ctx(16)
    ref64, ref16 = [], []
    for u in voices:
        fr = np.ascontiguousarray(frames[u:u + 1, :NF[u]])
        ref64.append(ctx.synthesize(fr, HOP, seeds=seeds[u:u + 1])[0])
        ref16.append(ctx.synthesize(fr, HOP, seeds=seeds[u:u + 1], pcm=True)[0])
    s = Synthesizer(ctx, 5, list(seeds[voices]) + [999])
    try:
        pos = [0, 0, 0, 0]  # samples each voice has produced

        def rows(cuts):
            return [frames[voices[v], a:b] if v < 4 else frames[0, 0:0] for v, (a, b) in enumerate(cuts)]

        def pad(rs):
            fr = np.zeros((5, 3), dtype=FRAME_DTYPE)
            for v, r in enumerate(rs):
                fr[v, :len(r)] = r
            return fr, np.array([len(r) for r in rs], dtype=np.int32)

        # strided float64: voices 0 .. 2 latch frame 0 and play frame 1; 3 and 4 idle
        fr, counts = pad(rows([(0, 2), (0, 2), (0, 2), (0, 0), (0, 0)]))
        out, produced = s.synthesize_frames(fr, counts, HOP)
        assert list(produced) == [HOP, HOP, HOP, 0, 0] and list(s.latched) == [1, 1, 1, 0, 0]
        for v in range(3):
            assert np.array_equal(out[v, :HOP].view(np.uint64), ref64[v][:HOP].view(np.uint64)), v
            pos[v] = HOP
        # packed float32 at the caller's offsets: 0 .. 2 play two frames, 3 latches and plays two, 4 idle
        fr, counts = pad(rows([(2, 4), (2, 4), (2, 4), (0, 3), (0, 0)]))
        offs = np.array([MARGIN + 3, MARGIN + 3 + 2 * HOP + 2, MARGIN + 3 + 4 * HOP + 3, MARGIN + 3 + 6 * HOP + 3,
                         MARGIN + 10], dtype=np.int64)  # (voice 4's: inside voice 0's row)
        buf = canary_buffer("f32", int(offs[3]) + 2 * HOP + MARGIN)
        flat, off, produced, rep = s.synthesize_frames(fr, counts, HOP, out=buf.view(np.float32), packed=True,
                                                       f32=True, offsets=offs, report=True)
        assert list(produced) == [2 * HOP] * 4 + [0] and list(s.latched) == [1, 1, 1, 1, 0]
        assert rep["samples"] == 8 * HOP and not rep["nonfinite"].any()
        want = canary_buffer("f32", buf.size)
        for v in range(4):
            want[offs[v]:offs[v] + 2 * HOP] = np.float32(ref64[v][pos[v]:pos[v] + 2 * HOP]).view(np.uint32)
            pos[v] += 2 * HOP
        assert np.array_equal(buf, want)
        # packed int16, tight in voice order, into a device tensor: 0 .. 2 play two frames, 3 two, 4 idle
        import torch
        fr, counts = pad(rows([(4, 6), (4, 6), (4, 6), (3, 5), (0, 0)]))
        dev = torch.from_numpy(canary_buffer("i16", 8 * HOP + 2 * MARGIN + 1).view(np.int16)).cuda()
        dest = dev[MARGIN + 1:MARGIN + 1 + 8 * HOP]
        flat, off, produced = s.synthesize_frames(fr, counts, HOP, out=dest, packed=True, pcm=True)
        assert list(produced) == [2 * HOP] * 4 + [0] and list(off) == [0, 2 * HOP, 4 * HOP, 6 * HOP, 8 * HOP, 8 * HOP]
        got = dev.cpu().numpy().view(np.uint16)
        want = canary_buffer("i16", got.size)
        for v in range(4):
            at = MARGIN + 1 + int(off[v])
            want[at:at + 2 * HOP] = ref16[v][pos[v]:pos[v] + 2 * HOP].view(np.uint16)
            pos[v] += 2 * HOP
        assert np.array_equal(got, want)
        # strided int16: voices 0, 1 and 3 play their last frame; 2 has ended
        fr, counts = pad(rows([(6, 7), (6, 7), (0, 0), (5, 6), (0, 0)]))
        out, produced = s.synthesize_frames(fr, counts, HOP, pcm=True)
        assert list(produced) == [HOP, HOP, 0, HOP, 0]
        for v in (0, 1, 3):
            assert np.array_equal(out[v, :HOP], ref16[v][pos[v]:pos[v] + HOP]), v
            pos[v] += HOP
        assert pos == [r.size for r in ref64]  # (every utterance played to its end)
        # an all-idle packed call: nothing queued, nothing looked at
        flat, off, produced = s.synthesize_frames(fr, np.zeros(5, dtype=np.int32), HOP, packed=True, f32=True)
        assert flat.size == 0 and not produced.any() and not off.any()
    finally:
        s.close()
