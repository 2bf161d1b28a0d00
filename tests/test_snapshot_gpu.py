"""Voice snapshots on the GPU (afs_session_save_voices, _load_voices, _copy_voices; Synthesizer.save_voices /
load_voices / copy_voices / fork, Context.synthesize_candidates).

The corpus: 5 utterances of 8 frames, a: -> s glides that reach the fricative after 7, 2, 3, 5 and 4
transitions and hold it (so the noise sources fire before and after the cut), each with a velum of its own,
seeds 201 + 5u.  Every utterance is cut after frame 3: part 1 is frames 0-3 (the latch and three
transitions), part 2 frames 4-7 (four transitions).  The yardstick is each utterance alone through
Context.synthesize on a context of the same lane width, computed once per (lanes, hop) and left unchanged:
wherever a voice's state has been in between -- a host blob, a device blob, another slot, another session,
another context -- part 2 is the tail of that trajectory, bit for bit, with its rand() count and non-finite
flag.  5 voices on 16 lanes are one full wave of four utterances and a partial one; hop 33 runs the hop
records, hop 5 (below AFS_PLAN_HOP_MIN) the dense plan.  Everything is compared on bit patterns."""
import ctypes

import numpy as np
import pytest

from areafunctionsynthesis_amd import _native
from areafunctionsynthesis_amd.frames import FRAME_DTYPE
from taps_lib import CURRENT, FS, PRESSURE, glide_frames

pytestmark = pytest.mark.gpu

NU, F, CUT = 5, 8, 4
REACH = [7, 2, 3, 5, 4]  # transitions after which utterance u holds the fricative
SEEDS = (201 + 5 * np.arange(NU)).astype(np.uint32)
SHAPES = [(16, 5), (64, 3)]  # (lanes, voices)
HOPS = [33, 5]
MIX = [(CURRENT, 24), (PRESSURE, 25), (PRESSURE, 22), (CURRENT, 93), (CURRENT, 96), (PRESSURE, 83), (PRESSURE, 60),
       (CURRENT, 65)]  # (the eight taps of tests/test_taps_gpu.py)
# the header's fields (afs_voice_state.h VoiceStateHeader): byte offsets
H_MAGIC, H_LANES, H_LATCHED, H_SEED, H_RATE = 0, 8, 20, 24, 32

_CACHE = {}


@pytest.fixture(scope="module")
def make_ctx():
    from areafunctionsynthesis_amd.synthesizer import Context
    made = {}

    def make(lanes=16, tag="", solver="tree"):
        key = (lanes, tag, solver)
        if key not in made:
            made[key] = Context(FS, solver=solver, lanes=lanes if solver == "tree" else None)
        return made[key]

    yield make
    for c in made.values():
        c.close()


@pytest.fixture
def session(make_ctx):
    """make(batch, lanes=16, seeds=None, tag="", solver="tree") -> a Synthesizer, closed after the test."""
    from areafunctionsynthesis_amd.synthesizer import Synthesizer
    made = []

    def make(batch, lanes=16, seeds=None, tag="", solver="tree"):
        made.append(Synthesizer(make_ctx(lanes, tag, solver), batch, seeds))
        return made[-1]

    yield make
    for s in made:
        s.close()


def corpus(oracle):
    """The 5 utterances' frames (read-only)."""
    if "corpus" not in _CACHE:
        utts = []
        for u in range(NU):
            g = glide_frames(oracle, REACH[u] + 1, 0.3 + 0.05 * u)
            fr = np.concatenate([g, np.repeat(g[-1:], F - len(g))]).astype(FRAME_DTYPE)
            assert fr.shape == (F,)
            fr.setflags(write=False)
            utts.append(fr)
        _CACHE["corpus"] = utts
    return _CACHE["corpus"]


def part1(oracle, u):
    return corpus(oracle)[u][:CUT]


def part2(oracle, u):
    return corpus(oracle)[u][CUT:]


def alone(make_ctx, frames, seed, lanes, hop, taps=None):
    """One utterance alone through Context.synthesize: (audio[T], draws, nonfinite flag, taps[n, T] or None)."""
    ctx = make_ctx(lanes)
    fr = np.ascontiguousarray(frames[None])
    seeds = np.array([seed], dtype=np.uint32)
    if taps is None:
        y, rep = ctx.synthesize(fr, hop, seeds=seeds, report=True)
        rows = None
    else:
        ctx.set_taps(taps)
        try:
            y, rows, rep = ctx.synthesize(fr, hop, seeds=seeds, report=True, taps=True)
        finally:
            ctx.set_taps([])
        rows = rows[0]
        rows.setflags(write=False)
    y[0].setflags(write=False)
    return y[0], int(ctx.rng_draws(1)[0]), int(rep["nonfinite"][0]), rows


def references(make_ctx, oracle, lanes, hop):
    """Utterance u alone on a context of the same lane width: [(audio, draws, nonfinite, None)] x 5."""
    key = ("ref", lanes, hop)
    if key not in _CACHE:
        _CACHE[key] = [alone(make_ctx, corpus(oracle)[u], SEEDS[u], lanes, hop) for u in range(NU)]
        if hop == 33:  # (the generator state is really exercised: rand() is drawn, in the fast glide before the cut too)
            print("rand() draws of the references:", [r[1] for r in _CACHE[key]])
            assert any(r[1] > 0 for r in _CACHE[key])
    return _CACHE[key]


def tail(ref, hop):
    """Part 2 of a reference: the audio after the cut."""
    return ref[0][(CUT - 1) * hop:]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def play(s, rows, hop, taps=False, pcm=False):
    """One synthesize_frames call of per-voice frame arrays (empty: idle): ([audio_u], nonfinite[B],
    [taps_u] or None), each row cut to what its voice produced."""
    res = s.synthesize_frames([np.asarray(r, dtype=FRAME_DTYPE) for r in rows], None, hop, taps=taps, pcm=pcm, report=True)
    out, produced, rep = res[0], res[1], res[-1]
    audio = [out[u, :produced[u]].copy() for u in range(s.batch)]
    trows = [res[2][u, :, :produced[u]].copy() for u in range(s.batch)] if taps else None
    return audio, rep["nonfinite"].copy(), trows


def none():
    return np.zeros(0, dtype=FRAME_DTYPE)


def same(a, b):
    return a.dtype == b.dtype and (np.array_equal(a, b) if a.dtype == np.int16 else np.array_equal(bits(a), bits(b)))


# ---- 1. resume ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("lanes,B", SHAPES)
def test_resume(make_ctx, session, oracle, lanes, B, hop):
    """Part 1, save every voice, part 2 (audio A, draws D, flags N); every voice restarted and played on
    other frames; load, part 2 again: A, D and N exactly -- and A is the references' tail."""
    refs = references(make_ctx, oracle, lanes, hop)
    s = session(B, lanes, SEEDS[:B])
    voices = np.arange(B)
    play(s, [part1(oracle, u) for u in range(B)], hop)
    blob = s.save_voices(voices)
    assert blob.shape == (B, s.voice_state_bytes) and blob.dtype == np.uint8 and s.voice_state_bytes % 16 == 0
    cut_draws = s.rng_draws()
    A, N, _ = play(s, [part2(oracle, u) for u in range(B)], hop)
    D = s.rng_draws()
    for u in range(B):
        assert same(A[u], tail(refs[u], hop)), f"voice {u}"
        assert (D[u], N[u]) == (refs[u][1], refs[u][2])
    if hop == 33:
        assert (cut_draws > 0).any() and (D > cut_draws).any()  # (rand() drawn before the cut and after it)
    s.restart(voices, SEEDS[:B] + 1000)
    play(s, [corpus(oracle)[(u + 1) % NU][2:5] for u in range(B)], hop)
    s.load_voices(voices, blob)
    assert s.latched.all() and np.array_equal(s.rng_draws(), cut_draws)
    A2, N2, _ = play(s, [part2(oracle, u) for u in range(B)], hop)
    for u in range(B):
        assert same(A2[u], A[u]), f"voice {u} after the load"
    assert np.array_equal(s.rng_draws(), D) and np.array_equal(N2, N)


# ---- 2. move ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("lanes", [16, 64])
def test_move(make_ctx, session, oracle, lanes, hop):
    """Voice 1 of a 5-voice session, saved after part 1, loaded into voice 2 of a 3-voice session of the
    same context (a host blob) and of a second context of equal rate, options and lanes (a device
    blob): part 2 there is the tail of the utterance alone."""
    import torch
    refs = references(make_ctx, oracle, lanes, hop)
    a = session(5, lanes, SEEDS)
    play(a, [part1(oracle, u) for u in range(5)], hop)
    blob = a.save_voices([1])
    dblob = a.save_voices([1], out=torch.empty((1, a.voice_state_bytes), dtype=torch.uint8, device="cuda"))
    assert np.array_equal(dblob.cpu().numpy(), blob)
    for tag, state in (("", blob), ("second", dblob)):
        b = session(3, lanes, tag=tag)
        assert (b.ctx is a.ctx) == (tag == "")
        b.load_voices([2], state)
        assert list(b.latched) == [0, 0, 1]
        got, nf, _ = play(b, [none(), none(), part2(oracle, 1)], hop)
        assert same(got[2], tail(refs[1], hop)), f"context {tag!r}"
        assert (int(b.rng_draws()[2]), int(nf[2])) == (refs[1][1], refs[1][2])
        assert got[0].size == got[1].size == 0


# ---- 3. fork ------------------------------------------------------------------------------------------

def fork_case(oracle, K):
    """The prefix (utterance 0's part 1) and K candidates that differ (part 2 of utterances 0 .. K-1)."""
    return part1(oracle, 0), np.stack([part2(oracle, k) for k in range(K)])


def fork_references(make_ctx, oracle, lanes, K, hop, seed, taps=None):
    key = ("fork", lanes, K, hop, seed, None if taps is None else tuple(taps))
    if key not in _CACHE:
        prefix, cands = fork_case(oracle, K)
        _CACHE[key] = [alone(make_ctx, np.concatenate([prefix, cands[k]]), seed, lanes, hop, taps) for k in range(K)]
    return _CACHE[key]


@pytest.mark.parametrize("pcm", [False, True], ids=["fp64", "pcm"])
@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("lanes,K", SHAPES)
def test_fork_candidates(make_ctx, oracle, lanes, K, hop, pcm):
    """synthesize_candidates: the prefix once, K candidates; row k is the tail of concat(prefix,
    candidate k) alone with that seed."""
    ctx, seed = make_ctx(lanes), 77
    prefix, cands = fork_case(oracle, K)
    got = ctx.synthesize_candidates(prefix, cands, hop, seed=seed, pcm=pcm)
    assert got.shape == (K, CUT * hop) and got.dtype == (np.int16 if pcm else np.float64)
    refs = fork_references(make_ctx, oracle, lanes, K, hop, seed)
    for k in range(K):
        want = tail(refs[k], hop)
        if pcm:
            want = ctx.to_int16(np.ascontiguousarray(want))
        assert same(got[k], want), f"candidate {k}"
    if hop == 33 and not pcm:  # (the candidates differ, and so does their audio: not yet in the first 20
        # samples' int16, which is all zeros)
        assert len({got[k].tobytes() for k in range(K)}) == K


def test_fork_taps(make_ctx, session, oracle):
    """The eight MIX taps through copy_voices + synthesize_frames(taps=True): audio and tap rows of the
    five forked voices equal afs_synthesize_taps on concat(prefix, candidate k) alone."""
    lanes, K, hop, seed = 16, 5, 33, 77
    ctx = make_ctx(lanes)
    prefix, cands = fork_case(oracle, K)
    refs = fork_references(make_ctx, oracle, lanes, K, hop, seed, taps=MIX)
    ctx.set_taps(MIX)
    try:
        s = session(K, lanes, np.full(K, seed, dtype=np.uint32))
        play(s, [prefix] + [none()] * (K - 1), hop, taps=True)
        s.copy_voices([1, 2, 3, 4], [0, 0, 0, 0])
        assert s.latched.all() and len(set(s.rng_draws())) == 1
        audio, _, rows = play(s, list(cands), hop, taps=True)
        for k in range(K):
            n = (CUT - 1) * hop
            assert same(audio[k], refs[k][0][n:]), f"candidate {k}"
            assert np.array_equal(bits(rows[k]), bits(refs[k][3][:, n:])), f"candidate {k}: taps"
            assert int(s.rng_draws()[k]) == refs[k][1]
    finally:
        ctx.set_taps([])


# ---- 4. isolation -------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["load", "copy"])
@pytest.mark.parametrize("lanes", [16, 64])
def test_isolation(make_ctx, session, oracle, lanes, how):
    """Voices 1 and 3 of a 5-voice session get the state of another session's voices 4 and 0: the records
    of voices 0, 2 and 4 are the same bytes before and after, those three continue as in the references,
    and 1 and 3 continue as the voices they now are."""
    hop = 33
    refs = references(make_ctx, oracle, lanes, hop)
    b = session(5, lanes, SEEDS)
    donor = session(5, lanes, SEEDS)
    for s in (b, donor):
        play(s, [part1(oracle, u) for u in range(5)], hop)
    before = b.save_voices([0, 2, 4])
    if how == "load":
        b.load_voices([1, 3], donor.save_voices([4, 0]))
    else:
        b.copy_voices([1, 3], [4, 0], src=donor)
    assert np.array_equal(b.save_voices([0, 2, 4]), before)
    now = [0, 4, 2, 0, 4]  # the utterance each voice of b plays
    got, nf, _ = play(b, [part2(oracle, i) for i in now], hop)
    for u, i in enumerate(now):
        assert same(got[u], tail(refs[i], hop)), f"voice {u}"
        assert (int(b.rng_draws()[u]), int(nf[u])) == (refs[i][1], refs[i][2])


# ---- 5. overlap ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes,B", SHAPES)
def test_overlap_swap(make_ctx, session, oracle, lanes, B):
    """copy_voices([0, 1], [1, 0]) on one session: every source is read before any destination is
    written, so the two voices swap and each plays the other's continuation."""
    hop = 33
    refs = references(make_ctx, oracle, lanes, hop)
    s = session(B, lanes, SEEDS[:B])
    play(s, [part1(oracle, u) for u in range(B)], hop)
    r01 = s.save_voices([0, 1])
    s.copy_voices([0, 1], [1, 0])
    assert np.array_equal(s.save_voices([1, 0]), r01)
    now = [1, 0] + list(range(2, B))
    got, _, _ = play(s, [part2(oracle, i) for i in now], hop)
    for u, i in enumerate(now):
        assert same(got[u], tail(refs[i], hop)), f"voice {u}"
        assert int(s.rng_draws()[u]) == refs[i][1]


# ---- 6. round trip ------------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("lanes,B", SHAPES)
def test_round_trip(make_ctx, session, oracle, lanes, B, device):
    """save(load(save(x))) == save(x), byte for byte, through a host blob and a device blob; a voice saved
    unlatched loads unlatched, and its first frame only latches."""
    import torch
    hop = 33
    a = session(B, lanes, SEEDS[:B])
    play(a, [part1(oracle, u) for u in range(B)], hop)
    a.restart([B - 1], [4242])  # (the last voice: fresh, unlatched)
    voices = np.arange(B)
    out = torch.zeros((B, a.voice_state_bytes), dtype=torch.uint8, device="cuda") if device else None
    x = a.save_voices(voices, out=out)
    host = x.cpu().numpy() if device else x
    assert host[:, H_LATCHED].tolist() == [1] * (B - 1) + [0]
    assert host[:, H_SEED:H_SEED + 4].copy().view(np.uint32)[:, 0].tolist() == list(SEEDS[:B - 1]) + [4242]
    b = session(B + 1, lanes)
    play(b, [part1(oracle, 0)] * (B + 1), hop)  # (every voice of b latched, on other state)
    b.load_voices(voices + 1, x)
    assert list(b.latched) == [1] * B + [0]
    y = b.save_voices(voices + 1, out=torch.zeros_like(x) if device else None)
    assert np.array_equal(y.cpu().numpy() if device else y, host)
    # the unlatched voice: one frame only latches, then it plays utterance 2 from its start, seed 4242
    got, _, _ = play(b, [none()] * B + [corpus(oracle)[2][:1]], hop)
    assert got[B].size == 0 and b.latched.all()
    got, _, _ = play(b, [none()] * B + [corpus(oracle)[2][1:]], hop)
    want = alone(make_ctx, corpus(oracle)[2], 4242, lanes, hop)
    assert same(got[B], want[0]) and int(b.rng_draws()[B]) == want[1]


# ---- 7. refusals --------------------------------------------------------------------------------------

def test_refusals(make_ctx, session, oracle):
    import torch
    from areafunctionsynthesis_amd.synthesizer import Synthesizer
    hop, B = 33, 5
    s = session(B, 16, SEEDS)
    play(s, [part1(oracle, u) for u in range(B)], hop)
    everyone = np.arange(B)
    kept = s.save_voices(everyone)
    size = s.voice_state_bytes
    lib, vp = s._lib, ctypes.c_void_p

    def arr(*v):
        return np.array(v, dtype=np.int32)

    def unchanged(sess=s, want=kept):
        assert np.array_equal(sess.save_voices(np.arange(sess.batch)), want)

    def refused(call, status=1):
        with pytest.raises(_native.AfsError, match=_native.STATUS[status]):
            call()
        unchanged()

    def raw(status, fn, *args):
        assert getattr(lib, fn)(*args) == status, fn
        unchanged()

    two = kept[:2].copy()
    v01, v0 = arr(0, 1), arr(0)
    # a NULL pointer with n > 0, n < 0; n == 0 does nothing
    raw(1, "afs_session_save_voices", s._h, None, 2, vp(two.ctypes.data))
    raw(1, "afs_session_save_voices", s._h, vp(v01.ctypes.data), 2, None)
    raw(1, "afs_session_load_voices", s._h, None, 2, vp(two.ctypes.data))
    raw(1, "afs_session_load_voices", s._h, vp(v01.ctypes.data), 2, None)
    raw(1, "afs_session_copy_voices", s._h, None, s._h, vp(v01.ctypes.data), 2)
    raw(1, "afs_session_copy_voices", s._h, vp(v01.ctypes.data), s._h, None, 2)
    raw(1, "afs_session_copy_voices", s._h, vp(v01.ctypes.data), None, vp(v01.ctypes.data), 2)
    raw(1, "afs_session_save_voices", s._h, vp(v01.ctypes.data), -1, vp(two.ctypes.data))
    raw(1, "afs_session_load_voices", s._h, vp(v01.ctypes.data), -1, vp(two.ctypes.data))
    raw(1, "afs_session_copy_voices", s._h, vp(v01.ctypes.data), s._h, vp(v01.ctypes.data), -1)
    raw(0, "afs_session_save_voices", s._h, None, 0, None)
    raw(0, "afs_session_load_voices", s._h, None, 0, None)
    raw(0, "afs_session_copy_voices", s._h, None, s._h, None, 0)
    # a voice out of range; a destination, or a saved voice, listed twice (a source may repeat)
    for bad in ([0, B], [-1, 1]):
        refused(lambda: s.save_voices(bad))
        refused(lambda: s.load_voices(bad, two))
        refused(lambda: s.copy_voices(bad, [0, 1]))
        refused(lambda: s.copy_voices([0, 1], bad))
    refused(lambda: s.save_voices([2, 2]))
    refused(lambda: s.load_voices([2, 2], two))
    refused(lambda: s.copy_voices([2, 2], [0, 1]))
    # a misaligned device state
    flat = torch.zeros(2 * size + 16, dtype=torch.uint8, device="cuda")
    odd = flat[8:8 + 2 * size].view(2, size)
    assert odd.data_ptr() % 16 == 8
    refused(lambda: s.save_voices([0, 1], out=odd))
    odd.copy_(torch.from_numpy(two))
    refused(lambda: s.load_voices([0, 1], odd))
    # a header that does not fit: the magic, the lane-width field and the rate flipped in a valid record --
    # in the second record of two, so the first, valid one must not have been written either
    for at, what in ((H_MAGIC, "magic"), (H_LANES, "lane width"), (H_RATE + 6, "sampling rate")):
        bad = np.stack([kept[3], kept[4]])
        bad[1, at] ^= 0x10
        refused(lambda: s.load_voices([0, 1], bad))
        assert what in lib.afs_last_error(s.ctx.handle).decode(), what
        refused(lambda: s.load_voices([0, 1], torch.from_numpy(bad).cuda()))
    # a 64-lane record into a 16-lane session (its size differs: straight to the library), and back
    wide = session(3, 64)
    rec64 = wide.save_voices([0])
    assert rec64.shape[1] != size
    raw(1, "afs_session_load_voices", s._h, vp(v0.ctypes.data), 1, vp(rec64.ctypes.data))
    big = np.zeros((1, rec64.shape[1]), dtype=np.uint8)
    big[0, :size] = kept[0]
    kept64 = wide.save_voices(np.arange(3))
    assert lib.afs_session_load_voices(wide._h, vp(v0.ctypes.data), 1, vp(big.ctypes.data)) == 1
    unchanged(wide, kept64)
    # sessions of two contexts, and of two lane widths of one context, in a copy
    other = session(B, 16, SEEDS, tag="second")
    kept_other = other.save_voices(everyone)
    refused(lambda: s.copy_voices([0], [0], src=other))
    refused(lambda: other.copy_voices([0], [0], src=s))
    unchanged(other, kept_other)
    auto = make_ctx(None)
    small = 3
    large = next(n for n in (1025, 2049, 4097, 8193) if auto.lanes_per_utterance(n) == 16)
    assert auto.lanes_per_utterance(small) == 64
    s64, s16 = Synthesizer(auto, small), Synthesizer(auto, large)
    try:
        with pytest.raises(_native.AfsError, match=_native.STATUS[1]):
            s64.copy_voices([0], [0], src=s16)
        with pytest.raises(_native.AfsError, match=_native.STATUS[1]):
            s16.copy_voices([0], [0], src=s64)
    finally:
        s64.close()
        s16.close()
    # the one-lane solvers have no snapshots
    chol = session(2, solver="cholesky")
    assert lib.afs_session_voice_state_bytes(chol._h) == 0
    buf = np.zeros((1, size), dtype=np.uint8)
    assert lib.afs_session_save_voices(chol._h, vp(v0.ctypes.data), 1, vp(buf.ctypes.data)) == 5
    assert lib.afs_session_load_voices(chol._h, vp(v0.ctypes.data), 1, vp(kept.ctypes.data)) == 5
    assert lib.afs_session_copy_voices(chol._h, vp(v0.ctypes.data), chol._h, vp(v0.ctypes.data), 1) == 5
    for call in (lambda: chol.save_voices([0]), lambda: chol.load_voices([0], buf), lambda: chol.fork(0, [1])):
        with pytest.raises(_native.AfsError, match=_native.STATUS[5]):
            call()
    # and after all of it the session plays on as if nothing had happened
    refs = references(make_ctx, oracle, 16, hop)
    got, _, _ = play(s, [part2(oracle, u) for u in range(B)], hop)
    for u in range(B):
        assert same(got[u], tail(refs[u], hop)), f"voice {u}"
