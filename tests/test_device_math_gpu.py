"""The tree kernel's device-only arithmetic against IEEE references, one operation at a time.

csrc/tree_core.h replaces the compiler's division, square root and compare-and-select on the
synthesis kernel's hot path by shorter device forms (pivot_recip / fast_rcp, fast_sqrt, fast_div,
hop_ratio, at_least / at_most / nonneg) and takes two exponentials from the device's libm.  The CPU
emulator compiles the header's host branch and never runs them, and the end-to-end parity bounds
(1e-9 over 2048 samples of a chaotic system) would not notice a reciprocal a few hundred ulps off or
a square root wrong in its last bit for one mantissa pattern.  Context.device_math
(afs_device_math, csrc/device_math.hip) runs the header's own functions as device code built with the
synthesis kernel's flags; here each is held to the claim its comment in tree_core.h makes, the bounds
being those claims (the parity argument of DESIGN.md 4 rests on them), not figures of a run:

  RCP        |d| in [2^-300, 2^300], either sign: within 11 ulps of 1.0 / d; RCP(-d) is -RCP(d) bit for bit
  SQRT       x in [2^-767, 2^1023): np.sqrt(x) bit for bit.  Nothing is asserted below 2^-767 (LLVM's
             sequence scales such operands first; fast_sqrt leaves the scaling out)
  DIV        |a|, |b| in [2^-100, 2^100], every sign combination: within 1 ulp of a / b; a = 0 gives a zero
             (of either sign: the unit is built with -fno-signed-zeros)
  HOP_RATIO  i / hop bit for bit for every i < hop, hop = 1 .. 2048 and 441, 4096, 8191, 8192, 44100,
             65521, 65536
  clamps     equal (==) to the select forms x < c ? c : x, x > c ? c : x, x < 0 ? 0 : x for every x that is
             not a NaN -- zeros, subnormals, infinities included; a NaN gives c (0 for nonneg); the sign
             of a zero is not asserted
  DIPOLE_GAIN  within 1e-13 relative of 0.5e-7 * 10^(dB / 20) in long double, dB in [-100, 40]
  NOISE_COEF   exp(-2 pi (cut dt)) for cut in (0, 2000) Hz, dt = 1 / 22050 and 1 / 44100, against the
             long double exp of the same float64 argument: the device's largest error is at most the
             largest error of the host libm's exp on these arguments plus 1 ulp (an ulp-level libm
             difference is what the parity tests' "differences only from device libm" assumes)

The references are the host's IEEE operations in numpy (1.0 / d, np.sqrt, a / b: correctly rounded);
distances are counted in doubles on the int64 view (device_math_lib.ulp_distance).  The operands and
the call-site ranges they cover are described in tests/device_math_lib.py.  Each test prints its
measured maximum and the share of exactly rounded results.

Teeth: the probe also has three weakened forms that no kernel uses -- the bare hardware reciprocal,
the quotient without its residual correction, the square root without its last residual step -- and
on the same operands each must break the bound its full form keeps."""
import ctypes
import functools
import math

import numpy as np
import pytest

import device_math_lib as dm
from areafunctionsynthesis_amd import _native

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 5  # afs.h AFS_ERR_INVALID_ARGUMENT, AFS_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def ctx():
    from areafunctionsynthesis_amd.synthesizer import Context
    c = Context(22050.0, solver="tree")
    yield c
    c.close()


@pytest.fixture
def say(parity_report):
    def line(text):
        print(text)
        parity_report.append(text)
    return line


def bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def summary(name, d):
    return f"device math {name}: {len(d)} operands, max {int(d.max())} ulps, exactly rounded {np.mean(d == 0):.4f}"


# the operand sets and their references: made once, shared by an op's test and its weakened form's
@functools.lru_cache(maxsize=None)
def rcp_case():
    x = dm.rcp_operands()
    return x, 1.0 / x


@functools.lru_cache(maxsize=None)
def sqrt_case():
    x = dm.sqrt_operands()
    return x, np.sqrt(x)


@functools.lru_cache(maxsize=None)
def div_case():
    a, b = dm.div_operands()
    return a, b, a / b


def test_rcp_within_11_ulps_and_odd(ctx, say):
    x, ref = rcp_case()
    got = ctx.device_math("RCP", x)
    d = dm.ulp_distance(got, ref)
    say(summary("RCP", d))
    worst = int(np.argmax(d))
    assert d.max() <= 11, (x[worst].hex(), got[worst].hex(), ref[worst].hex())
    n = len(x) // 2
    assert np.array_equal(bits(got[n:]), bits(-got[:n]))


def test_sqrt_is_the_ieee_square_root(ctx, say):
    x, ref = sqrt_case()
    got = ctx.device_math("SQRT", x)
    d = dm.ulp_distance(got, ref)
    say(summary("SQRT", d))
    differ = np.flatnonzero(bits(got) != bits(ref))
    assert len(differ) == 0, (len(differ), [(x[k].hex(), got[k].hex(), ref[k].hex()) for k in differ[:4]])


def test_div_within_1_ulp(ctx, say):
    a, b, ref = div_case()
    got = ctx.device_math("DIV", a, b)
    d = dm.ulp_distance(got, ref)
    say(summary("DIV", d))
    g = 2 * dm.N_SITE  # the glottis shape: the tail of each sign combination's quarter
    tail = d.reshape(4, -1)[:, -g:]
    say(f"device math DIV, glottis_open_close_one's operands: max {int(tail.max())} ulps, exactly rounded {np.mean(tail == 0):.4f}")
    worst = int(np.argmax(d))
    assert d.max() <= 1, (a[worst].hex(), b[worst].hex(), got[worst].hex(), ref[worst].hex())


def test_div_of_zero_is_zero(ctx):
    a, b = dm.div_zero_operands()
    got = ctx.device_math("DIV", a, b)
    assert (got == 0.0).all()


def test_hop_ratio_is_the_division(ctx, say):
    i, hop = dm.hop_operands()
    got = ctx.device_math("HOP_RATIO", i, hop)
    ref = i / hop
    differ = np.flatnonzero(bits(got) != bits(ref))
    say(f"device math HOP_RATIO: {len(i)} (i, hop) pairs, {len(differ)} differ from i / hop")
    assert len(differ) == 0, [(i[k], hop[k], got[k].hex(), ref[k].hex()) for k in differ[:4]]


@pytest.mark.parametrize("op", ["AT_LEAST", "AT_MOST", "NONNEG"])
def test_clamps_equal_the_select_forms(ctx, say, op):
    constants = {"AT_LEAST": dm.AT_LEAST_CONSTANTS, "AT_MOST": dm.AT_MOST_CONSTANTS, "NONNEG": (0.0,)}[op]
    x = dm.clamp_numbers(constants)
    nans = dm.quiet_nans()
    total = 0
    for c in constants:
        cc = np.full(len(x), c)
        select = {"AT_LEAST": np.where(x < cc, cc, x), "AT_MOST": np.where(x > cc, cc, x),
                  "NONNEG": np.where(x < 0.0, 0.0, x)}[op]
        got = ctx.device_math(op, x, cc)
        differ = np.flatnonzero(~(got == select))
        assert len(differ) == 0, (c, [(x[k].hex(), got[k].hex(), select[k].hex()) for k in differ[:4]])
        got = ctx.device_math(op, nans, np.full(len(nans), c))
        assert (got == c).all(), (c, [v.hex() for v in got])
        total += len(x) + len(nans)
    say(f"device math {op}: {total} operands at c = {constants}, all equal to the select form; a NaN gives c")


def test_dipole_gain(ctx, say):
    assert dm.long_double_is_wider()
    db = dm.gain_operands()
    got = ctx.device_math("DIPOLE_GAIN", db)
    ref = dm.gain_reference(db)
    rel = np.abs((got.astype(np.longdouble) - ref) / ref)
    d = dm.ulp_distance(got, ref.astype(np.float64))
    say(f"device math DIPOLE_GAIN: {len(db)} operands, max relative error {float(rel.max()):.3e} "
        f"({int(d.max())} ulps), exactly rounded {np.mean(d == 0):.4f}")
    assert np.isfinite(got).all() and rel.max() <= 1e-13


def test_noise_coefficient(ctx, say):
    assert dm.long_double_is_wider()
    cut, dt = dm.noise_operands()
    arg = dm.noise_argument(cut, dt)
    ref = np.exp(arg.astype(np.longdouble)).astype(np.float64)
    host = np.array([math.exp(v) for v in arg.tolist()])  # the C library's exp
    got = ctx.device_math("NOISE_COEF", cut, dt)
    dh, dg = dm.ulp_distance(host, ref), dm.ulp_distance(got, ref)
    say(f"device math NOISE_COEF: {len(cut)} operands, device max {int(dg.max())} ulps (exactly rounded "
        f"{np.mean(dg == 0):.4f}), host libm max {int(dh.max())} ulps (exactly rounded {np.mean(dh == 0):.4f})")
    assert dg.max() <= dh.max() + 1


def test_teeth_bare_reciprocal_breaks_the_bound(ctx, say):
    x, ref = rcp_case()
    d = dm.ulp_distance(ctx.device_math("RCP_SEED", x), ref)
    say(summary("RCP_SEED (weakened)", d))
    assert d.max() > 11


def test_teeth_uncorrected_quotient_breaks_the_bound(ctx, say):
    a, b, ref = div_case()
    d = dm.ulp_distance(ctx.device_math("DIV_UNCORRECTED", a, b), ref)
    say(summary("DIV_UNCORRECTED (weakened)", d))
    assert d.max() > 1


def test_teeth_short_square_root_differs(ctx, say):
    x, ref = sqrt_case()
    got = ctx.device_math("SQRT_SHORT", x)
    d = dm.ulp_distance(got, ref)
    differ = int(np.count_nonzero(bits(got) != bits(ref)))
    say(summary("SQRT_SHORT (weakened)", d) + f", {differ} differ from np.sqrt")
    assert differ > 0


def test_argument_checks(ctx):
    from areafunctionsynthesis_amd.synthesizer import Context
    lib, h = ctx._lib, ctx.handle
    a = np.ones(4)
    b = np.ones(4)
    out = np.zeros(4)
    pa, pb, po = (ctypes.c_void_p(v.ctypes.data) for v in (a, b, out))
    assert lib.afs_device_math(h, _native.MATH_OPS["RCP"], pa, pb, 4, po) == _native.AFS_OK
    assert (out == 1.0).all()
    for op in (-1, len(_native.MATH_OPS), 1 << 20):
        assert lib.afs_device_math(h, op, pa, pb, 4, po) == INVALID
    for args in ((None, pb, 4, po), (pa, None, 4, po), (pa, pb, 4, None), (pa, pb, 0, po), (pa, pb, -4, po)):
        assert lib.afs_device_math(h, 0, *args) == INVALID
    assert lib.afs_device_math(None, 0, pa, pb, 4, po) == INVALID
    with pytest.raises(_native.AfsError, match="invalid argument"):
        ctx.device_math(99, a)
    chol = Context(22050.0, solver="cholesky")
    try:
        assert lib.afs_device_math(chol.handle, 0, pa, pb, 4, po) == UNSUPPORTED
    finally:
        chol.close()
