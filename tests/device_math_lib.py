"""Operands and measures for the tests of the tree kernel's device-only arithmetic
(csrc/tree_core.h pivot_recip / fast_rcp, fast_sqrt, fast_div, hop_ratio, at_least / at_most / nonneg,
the two exp forms), which Context.device_math runs one operation at a time
(tests/test_device_math_gpu.py; the generators themselves are checked in tests/test_device_math_cpu.py).

Every set is structured operands plus random ones with a fixed seed.

Structured, for an op with the domain [2^lo, 2^hi]:
  * every power of two of the domain (hi - lo + 1 of them);
  * for each of N_EXPONENTS exponents spread evenly over lo + 1 .. hi - 1, MANTISSAS_PER_EXPONENT
    operands: 1.0, 1 + 1 ulp, 1 - 1 ulp (the all-ones mantissa one exponent below), 2 - 1 ulp, the low
    32 mantissa bits all ones, the high 20 all ones, the two alternating bit patterns, and the sweep
    1 + j / 4096, j < 4096;
  * SQRT also gets N_SQUARES exact squares y^2 of 26-bit y at even scalings with both neighbours
    y^2 +- 1 ulp (the root is y exactly, or must round to y), and the operands of near_midpoints():
    roots within 2^-43 ulp of a tie between two doubles, which is where a root that is only nearly
    exact before its rounding goes wrong (random operands never come that close).

Random: uniform mantissa with the exponent uniform over the domain (N_WIDE operands), and a second set
over what the kernel's call sites reach (N_SITE operands per range, log-uniform).  Those ranges, from
the call sites in csrc/tree_core.h:
  RCP   areas [1e-3, 1e3] (clampA_num's floor AMIN; phase_network's inv_area, phase_targets' 1 / A),
        squared areas [1e-6, 1e6] (the Bernoulli and glottal entrance terms: fast_rcp(a * a)),
        the tension Q in [0.05, 20] (at_least(Q, 0.05); glottis_eval / two_mass_glottis inv_q),
        sqrt(Q) and the cord length 1.3 sqrt(Q) in [0.2, 6] (inv_f, inv_cord),
        the glottis determinant, either sign, 1e-9 <= |det| <= 1e3 (`if (fabs(det) < 1e-9) det = 1e-9`);
        the LDL^T pivots have no bound of their own (negative ones are met and flagged): the wide set.
  SQRT  areas [1e-3, 1e3], area / pi and 4 area / pi [3e-4, 1.3e3] (phase_network's r0,
        plan_word_fast), Q in [0.05, 20], mass x stiffness of the two-mass model [1e2, 1e5].
  DIV   the plan words: 1 / a and 1 / sqrt(4 a / pi) for a in [0.1, 1e3], the downstream factors
        N / D of areas in [1e-3, 1e3]; phase_network's E = dt TH / (C + alpha): dt TH = 0.515 / fs
        for fs in 8..96 kHz over the wall-loaded capacitance in [1e-12, 1e-1] (C = area length /
        (rho c^2) from 7e-12 up, alpha = surface / K with the surface floored at AMIN);
        glottis_open_close_one's fast_div(rel, r): rel in +-[1e-6, 1], r in +-[1e-9, 1]
        (`if (fabs(r) < 1e-9) r = 1e-9`), and rel = 0.
The clamps' constants: at_least at AMIN (areas, surfaces), 0.1 (the noise sources' area), 0.05 (the
tension floor of the triangular and of the two-mass glottis) and 50 (clamp_fc); at_most at 2000
(clamp_fc).  Their NaN operands are quiet NaNs: every operand of a clamp in the kernel is the result of
an arithmetic instruction, which never delivers a signalling one.
"""
import math

import numpy as np

# domains as exponents of two, both ends included unless noted
RCP_DOMAIN = (-300, 300)
SQRT_DOMAIN = (-767, 1023)  # [2^-767, 2^1023): the upper end excluded
DIV_DOMAIN = (-100, 100)

N_EXPONENTS = 64
SWEEP = 4096
SPECIAL_FRACTIONS = (0x0000000000000, 0x0000000000001, 0xFFFFFFFFFFFFF, 0x00000FFFFFFFF, 0xFFFFF00000000,
                     0x5555555555555, 0xAAAAAAAAAAAAA)
MANTISSAS_PER_EXPONENT = len(SPECIAL_FRACTIONS) + 1 + SWEEP  # (+ 1: 1 - 1 ulp, from the exponent below)
N_WIDE = 1 << 20
N_SITE = 1 << 17
N_SQUARES = 1 << 18
N_MIDPOINT_R = 1024
SEED = 20260117

AMIN = 0.1e-2
AT_LEAST_CONSTANTS = (AMIN, 0.1, 0.05, 50.0)
AT_MOST_CONSTANTS = (2000.0,)

HOPS_ALL = 2048
HOPS_EXTRA = (441, 4096, 8191, 8192, 44100, 65521, 65536)

NOISE_DTS = (1.0 / 22050.0, 1.0 / 44100.0)
NOISE_GRID = 1 << 19
NOISE_RANDOM = 1 << 18
GAIN_DB = (-100.0, 40.0)
GAIN_GRID_PER_DB = 4096
GAIN_RANDOM = 1 << 19

NEVER = 1 << 62  # the distance of a NaN from a number


def ordered(x):
    """The doubles' bit patterns as integers in the doubles' order (-0 and +0 both at 0)."""
    i = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
    return np.where(i < 0, -(i & np.int64(0x7FFFFFFFFFFFFFFF)), i)


def ulp_distance(got, ref):
    """How many doubles apart got and ref are (int64; NEVER where just one of them is a NaN)."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    d = np.abs(ordered(got) - ordered(ref))
    gn, rn = np.isnan(got), np.isnan(ref)
    return np.where(gn | rn, np.where(gn & rn, 0, NEVER), d)


def from_parts(fraction, exponent):
    """(1 + fraction / 2^52) * 2^exponent for 52-bit fractions and normal exponents."""
    f = np.asarray(fraction, dtype=np.uint64)
    e = (np.asarray(exponent, dtype=np.int64) + 1023).astype(np.uint64)
    return ((e << np.uint64(52)) | f).view(np.float64)


def powers_of_two(lo, hi):
    return np.ldexp(1.0, np.arange(lo, hi + 1))


def spread_exponents(lo, hi, n=N_EXPONENTS):
    """n exponents spread evenly over lo .. hi, both parities among them."""
    e = np.unique(np.round(np.linspace(lo, hi, n)).astype(np.int64))
    assert len(e) == n and (e % 2 == 0).any() and (e % 2 == 1).any()
    return e


def mantissa_set(exponents):
    """MANTISSAS_PER_EXPONENT operands per exponent (see the module docstring)."""
    fr = np.concatenate([np.array(SPECIAL_FRACTIONS, dtype=np.uint64), np.arange(SWEEP, dtype=np.uint64) << np.uint64(40)])
    out = []
    for e in exponents:
        out.append(from_parts(fr, np.full(len(fr), e)))
        out.append(np.array([np.nextafter(np.ldexp(1.0, int(e)), 0.0)]))
    return np.concatenate(out)


def structured(lo, hi, top_excluded=False):
    """The structured operands of the domain [2^lo, 2^hi] (or [2^lo, 2^hi))."""
    top = hi - 1 if top_excluded else hi
    return np.concatenate([powers_of_two(lo, top), mantissa_set(spread_exponents(lo + 1, hi - 1))])


def structured_size(lo, hi, top_excluded=False):
    return (hi - lo + (0 if top_excluded else 1)) + N_EXPONENTS * MANTISSAS_PER_EXPONENT


def wide(rng, lo, hi, n=N_WIDE):
    """Uniform mantissas, exponents uniform over lo .. hi - 1: operands in [2^lo, 2^hi)."""
    return from_parts(rng.integers(0, 1 << 52, n, dtype=np.uint64), rng.integers(lo, hi, n))


def log_uniform(rng, a, b, n=N_SITE):
    return np.clip(np.exp(rng.uniform(math.log(a), math.log(b), n)), a, b)


def with_signs(p):
    """p, then -p: result k + len(p) belongs to the negated operand k."""
    return np.concatenate([p, -p])


# --- RCP ---------------------------------------------------------------------------------------
RCP_SITES = {"area": (1e-3, 1e3), "area squared": (1e-6, 1e6), "Q": (0.05, 20.0), "sqrt Q, cord length": (0.2, 6.0),
             "|det|": (1e-9, 1e3)}


def rcp_positive():
    rng = np.random.default_rng(SEED)
    lo, hi = RCP_DOMAIN
    return np.concatenate([structured(lo, hi), wide(rng, lo, hi)] + [log_uniform(rng, a, b) for a, b in RCP_SITES.values()])


def rcp_operands():
    return with_signs(rcp_positive())


# --- SQRT --------------------------------------------------------------------------------------
SQRT_SITES = {"area": (1e-3, 1e3), "area / pi, 4 area / pi": (3e-4, 1.3e3), "Q": (0.05, 20.0),
              "mass x stiffness": (1e2, 1e5)}


def exact_squares(rng, n=N_SQUARES):
    """y^2 for 26-bit y in [1, 2) (exact in a double) at even scalings, and the root y at that scaling."""
    y = 1.0 + rng.integers(0, 1 << 25, n).astype(np.float64) * 2.0 ** -25
    s = rng.integers(-190, 250, n)  # (y 2^s)^2 in [2^-380, 2^502)
    return np.ldexp(y * y, 2 * s), np.ldexp(y, s)


def near_midpoints(n_r=N_MIDPOINT_R):
    """Operands whose root all but ties between two doubles, and the correctly rounded root.

    The midpoints of neighbouring doubles in [1, 2) are z = w / 2^53 for odd w in [2^53, 2^54).  z^2 is
    never a double, but for w^2 = r (mod 2^k) with a small r the double x = (w^2 - r) / 2^106 (k = 54:
    x in [1, 2); k = 55: x in [2, 4)) has sqrt(x) = z - r / (2 z 2^106): |r| 2^-55 ulps from the tie, below
    it for r > 0 and above it for r < 0.  The odd squares are the residues r = 1 (mod 8); w comes from
    lifting the root 1 of r modulo 8 one bit at a time.  A sequence that delivers the root to 2^-95
    relative and then rounds -- fast_sqrt without its last residual step -- gets random operands right
    and these wrong."""
    xs, roots, rs = [], [], []
    for k in (54, 55):
        m = 1 << k
        for j in range(-(n_r // 2), n_r // 2):
            r = 8 * j + 1
            w = 1
            for n in range(3, k):  # w^2 = r (mod 2^n)  ->  (mod 2^(n + 1))
                if (w * w - r) % (1 << (n + 1)):
                    w += 1 << (n - 1)
            for v in sorted({w % m, -w % m, (w + m // 2) % m, (-w + m // 2) % m}):
                xi = (v * v - r) >> k
                if (1 << 53) <= v < (1 << 54) and (1 << 52) <= xi < (1 << 53):
                    assert xi * m + r == v * v
                    xs.append(math.ldexp(xi, k - 106))
                    roots.append(math.ldexp((v - 1) // 2 if r > 0 else (v + 1) // 2, -52))
                    rs.append(r)
    return np.array(xs), np.array(roots), np.array(rs)


def sqrt_operands():
    rng = np.random.default_rng(SEED + 1)
    lo, hi = SQRT_DOMAIN
    sq, _ = exact_squares(rng)
    mid, _, _ = near_midpoints()
    mid_scaled = np.ldexp(mid, 2 * rng.integers((lo + 1) // 2, (hi - 2) // 2, len(mid)))  # (x 4^s: the same mantissas)
    return np.concatenate([structured(lo, hi, top_excluded=True), wide(rng, lo, hi), sq, np.nextafter(sq, np.inf),
                           np.nextafter(sq, 0.0), mid, mid_scaled] + [log_uniform(rng, a, b) for a, b in SQRT_SITES.values()])


# --- DIV ---------------------------------------------------------------------------------------
DIV_FS = (8000.0, 16000.0, 22050.0, 44100.0, 48000.0, 96000.0)
GLOTTIS_REL = (1e-6, 1.0)
GLOTTIS_REST = (1e-9, 1.0)
N_ZERO = 4096


def div_positive():
    """Pairs (a, b) of positive operands in the domain."""
    rng = np.random.default_rng(SEED + 2)
    lo, hi = DIV_DOMAIN
    p = powers_of_two(lo, hi)
    exps = spread_exponents(lo + 1, hi - 1)
    m = mantissa_set(exps)
    m_rev = mantissa_set(exps[::-1])
    one = np.repeat(np.ldexp(1.0, exps), MANTISSAS_PER_EXPONENT)
    a = [np.repeat(p, len(p)), m, m, one[::-1].copy()]
    b = [np.tile(p, len(p)), rng.permutation(m_rev), one[::-1].copy(), m]
    a.append(wide(rng, lo, hi))
    b.append(wide(rng, lo, hi))
    area = log_uniform(rng, 0.1, 1e3)  # the plan words
    a += [np.ones(N_SITE), np.ones(N_SITE), log_uniform(rng, 1e-3, 1e3)]
    b += [area, np.sqrt((4.0 * area) * (1.0 / math.pi)), log_uniform(rng, 1e-3, 1e3)]
    a.append(0.515 / rng.choice(np.array(DIV_FS), N_SITE))  # phase_network's E
    b.append(log_uniform(rng, 1e-12, 1e-1))
    a.append(log_uniform(rng, *GLOTTIS_REL, 2 * N_SITE))  # glottis_open_close_one
    b.append(log_uniform(rng, *GLOTTIS_REST, 2 * N_SITE))
    return np.concatenate(a), np.concatenate(b)


def div_positive_size():
    n = DIV_DOMAIN[1] - DIV_DOMAIN[0] + 1
    return n * n + 3 * N_EXPONENTS * MANTISSAS_PER_EXPONENT + N_WIDE + 6 * N_SITE


def div_operands():
    """The positive pairs under the four sign combinations."""
    a, b = div_positive()
    return np.concatenate([a, -a, a, -a]), np.concatenate([b, b, -b, -b])


def div_zero_operands():
    """a = +-0 over denominators of the glottis shape and of the domain's ends, either sign."""
    rng = np.random.default_rng(SEED + 3)
    b = np.concatenate([log_uniform(rng, *GLOTTIS_REST, N_ZERO - 2), np.ldexp(1.0, np.array(DIV_DOMAIN))])
    b = np.concatenate([b, -b])
    return np.concatenate([np.zeros(len(b)), -np.zeros(len(b))]), np.concatenate([b, b])


# --- HOP_RATIO ---------------------------------------------------------------------------------
def hop_operands():
    """Every (i, hop) with i < hop, for the hops 1 .. HOPS_ALL and HOPS_EXTRA."""
    hops = np.concatenate([np.arange(1, HOPS_ALL + 1), np.array(HOPS_EXTRA)])
    hop = np.repeat(hops, hops)
    start = np.repeat(np.cumsum(hops) - hops, hops)
    i = np.arange(len(hop)) - start
    return i.astype(np.float64), hop.astype(np.float64)


def hop_operands_size():
    return HOPS_ALL * (HOPS_ALL + 1) // 2 + sum(HOPS_EXTRA)


# --- clamps ------------------------------------------------------------------------------------
N_CLAMP_RANDOM = 1 << 18
CLAMP_NEIGHBOURS = 8
QUIET_NANS = (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFFC0000DEADBEEF)


def quiet_nans():
    return np.array(QUIET_NANS, dtype=np.uint64).view(np.float64)


def clamp_numbers(constants):
    """Every kind of double that is not a NaN: zeros, subnormals, the ends of the normal range,
    infinities, the constants and their neighbours, and random bit patterns."""
    rng = np.random.default_rng(SEED + 4)
    tiny = np.array([0x1, 0x2, 0x8000000000000, 0xFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)  # subnormals
    ends = np.array([0.0, np.finfo(np.float64).tiny, np.finfo(np.float64).max, np.inf, 1.0])
    near = []
    for c in constants:
        x = np.float64(c)
        up = dn = x
        near.append(x)
        for _ in range(CLAMP_NEIGHBOURS):
            up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
            near += [up, dn]
    bits = rng.integers(0, 1 << 64, N_CLAMP_RANDOM, dtype=np.uint64)
    rnd = bits.view(np.float64)
    rnd = rnd[np.isfinite(rnd)]
    # (around each constant; nonneg's zero: the flows, displacements and controls it clamps)
    site = np.concatenate([log_uniform(rng, (c or 1e-6) * 1e-3, (c or 1.0) * 1e3, 4096) for c in constants])
    pos = np.concatenate([tiny, ends, np.array(near), site])
    return np.concatenate([pos, -pos, rnd])


# --- exp forms ---------------------------------------------------------------------------------
def gain_operands():
    rng = np.random.default_rng(SEED + 5)
    lo, hi = GAIN_DB
    n = int(hi - lo) * GAIN_GRID_PER_DB
    grid = lo + np.arange(n + 1) / GAIN_GRID_PER_DB
    return np.concatenate([grid, rng.uniform(lo, hi, GAIN_RANDOM)])


def gain_reference(db):
    """0.5e-7 * 10^(dB / 20) in long double."""
    ld = np.longdouble
    return ld(0.5e-7) * np.power(ld(10.0), db.astype(ld) / ld(20.0))


def noise_operands():
    """(cut-off, dt): cut-offs in (0, 2000) Hz on a grid and random, for each sampling period."""
    rng = np.random.default_rng(SEED + 6)
    grid = np.arange(1, NOISE_GRID) * (2000.0 / NOISE_GRID)
    cut = np.concatenate([grid, np.nextafter(2000.0, 0.0) * rng.random(NOISE_RANDOM) + np.finfo(np.float64).tiny])
    return np.tile(cut, len(NOISE_DTS)), np.repeat(np.array(NOISE_DTS), len(cut))


def noise_argument(cut, dt):
    """The exponent as the kernel writes it, -2.0 * PI * (cut * dt), in float64 and in that order."""
    return (-2.0 * math.pi) * (cut * dt)


def long_double_is_wider():
    return np.finfo(np.longdouble).nmant >= 63
