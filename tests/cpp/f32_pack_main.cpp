// CPU checks of the float32 form of the output stage (csrc/tree_core.h F32Pack, output_filter_run_f32;
// csrc/afs_audio.h sample_to_f32), built with AddressSanitizer and UndefinedBehaviorSanitizer
// (tests/test_packed_cpu.py).  Prints "f32-ok", or the first mismatch and exits 1.
//   1. sample_to_f32 against the cast, bit for bit: +-0, denormals of both formats, values that round to
//      float denormals, ties of the rounding, the float range's edge, +-inf, NaN (which stays a NaN).
//   2. F32Pack against the casts sample by sample: every alignment of the row 0..3 floats, every run
//      length 0..24, in a heap block that ends with the run (the sanitizer sees a byte past it) with
//      canaries before it, and inside a block with canaries on both sides.
//   3. output_filter_run_f32 against the cast of output_filter_run's doubles: n = 1..40, every split into
//      two runs with the state carried through the image (so the second run's row starts at every
//      alignment), with and without the tone filter: the floats equal bit for bit, the images equal.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "tree_core.h"

using namespace afs;
using namespace afs::tree;

static uint32_t fbits(float x) {
  uint32_t b;
  std::memcpy(&b, &x, 4);
  return b;
}
static float canary() {  // (a NaN no cast of a double produces: a signalling pattern with a payload)
  const uint32_t b = 0x7fa5c3e1u;
  float x;
  std::memcpy(&x, &b, 4);
  return x;
}
static const uint32_t CANARY = 0x7fa5c3e1u;

static std::vector<double> special_values() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double fmin = (double)std::numeric_limits<float>::min(), fden = (double)std::numeric_limits<float>::denorm_min();
  const double fmax = (double)std::numeric_limits<float>::max();
  std::vector<double> v = {0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1.5, -1.5, inf, -inf, nan, -nan, 1e300, -1e300, 1e-300, -1e-300,
                           std::numeric_limits<double>::denorm_min(), -std::numeric_limits<double>::denorm_min(),
                           std::numeric_limits<double>::min(), fmin, -fmin, fmin / 2, fmin * 0.75, fden, -fden, fden / 2,
                           std::nextafter(fden / 2, 1.0), fden * 1.5, fden * 2.5, fmax, -fmax, std::nextafter(fmax, inf),
                           fmax * (1.0 + 0x1p-25), std::nextafter(fmax * (1.0 + 0x1p-25), 0.0), 2 * fmax,
                           // ties of the 24-bit rounding: to even both ways, and their neighbours
                           1.0 + 0x1p-24, 1.0 + 0x3p-24, std::nextafter(1.0 + 0x1p-24, 2.0), std::nextafter(1.0 + 0x1p-24, 0.0),
                           -(1.0 + 0x1p-24), -(1.0 + 0x3p-24), 0.1, -0.1, 1.0 / 3.0, 3.0517578125e-05, 0.004 / 32767};
  std::mt19937_64 rng(4242);
  std::uniform_real_distribution<double> d(-1.0, 1.0);
  for (int i = 0; i < 64; ++i) v.push_back(d(rng) * std::ldexp(1.0, -(i % 40)));
  return v;
}

static int check_cast() {
  for (double x : special_values()) {
    const float got = sample_to_f32(x), want = (float)x;
    if (fbits(got) != fbits(want)) {
      std::printf("sample_to_f32(%a) = %08x, want %08x\n", x, fbits(got), fbits(want));
      return 1;
    }
    if ((x != x) != (got != got) || (std::isinf(x) && got != (float)x)) {
      std::printf("sample_to_f32(%a) lost a non-finite value\n", x);
      return 1;
    }
  }
  if (fbits(sample_to_f32(0.0)) != 0u || fbits(sample_to_f32(-0.0)) != 0x80000000u) {
    std::printf("sample_to_f32 of a signed zero\n");
    return 1;
  }
  return 0;
}

static int check_pack() {
  const std::vector<double> vals = special_values();
  size_t next = 0;
  for (int a = 0; a < 4; ++a)
    for (int n = 0; n <= 24; ++n) {
      // the row ends the block: a store past row + n is a heap overflow
      float *base = (float *)std::malloc((size_t)(a + n) * sizeof(float) + (a + n == 0));
      if ((reinterpret_cast<uintptr_t>(base) & 15) != 0) {
        std::printf("malloc block not 16-byte aligned\n");
        return 1;
      }
      for (int i = 0; i < a; ++i) base[i] = canary();
      for (int i = 0; i < n; ++i) base[a + i] = -canary();
      std::vector<double> x((size_t)n);
      for (int i = 0; i < n; ++i) x[(size_t)i] = vals[next++ % vals.size()];
      F32Pack sink(base + a, n);
      for (int t = 0; t < n; ++t) sink.put(t, x[(size_t)t]);
      for (int i = 0; i < a; ++i)
        if (fbits(base[i]) != CANARY) {
          std::printf("pack: alignment %d, n %d: wrote before the row at %d\n", a, n, i - a);
          return 1;
        }
      for (int i = 0; i < n; ++i)
        if (fbits(base[a + i]) != fbits((float)x[(size_t)i])) {
          std::printf("pack: alignment %d, n %d: sample %d of %a is %08x, want %08x\n", a, n, i, x[(size_t)i],
                      fbits(base[a + i]), fbits((float)x[(size_t)i]));
          return 1;
        }
      std::free(base);
    }
  // ... and inside a block with canaries on both sides
  alignas(16) float buf[4 + 4 + 24 + 4];
  for (int a = 0; a < 4; ++a)
    for (int n = 0; n <= 24; ++n) {
      for (float &b : buf) b = canary();
      F32Pack sink(buf + 4 + a, n);
      for (int t = 0; t < n; ++t) sink.put(t, vals[(size_t)(t * 7 + a + n) % vals.size()]);
      for (int i = 0; i < (int)(sizeof buf / sizeof buf[0]); ++i) {
        const int t = i - 4 - a;
        const uint32_t want = t >= 0 && t < n ? fbits((float)vals[(size_t)(t * 7 + a + n) % vals.size()]) : CANARY;
        if (fbits(buf[i]) != want) {
          std::printf("pack: alignment %d, n %d: position %d is %08x, want %08x\n", a, n, t, fbits(buf[i]), want);
          return 1;
        }
      }
    }
  return 0;
}

template <bool TONE>
static int check_filter(const Tables &T, std::mt19937_64 &rng, bool poison) {
  std::uniform_real_distribution<double> flow(-300.0, 300.0), pres(-2000.0, 2000.0), st(-1e6, 1e6);
  for (int n = 1; n <= 40; ++n) {
    std::vector<double> f((size_t)n), p((size_t)n), X0(X_TOTAL, 0.0);
    for (double &v : f) v = flow(rng);
    for (double &v : p) v = pres(rng);
    if (poison) f[(size_t)(n / 2)] = n % 2 ? std::numeric_limits<double>::infinity() : std::numeric_limits<double>::quiet_NaN();
    for (int k = 0; k < 16; ++k) X0[X_OUTF + k] = st(rng);
    for (int k = 0; k < 8; ++k) X0[X_TONE + k] = pres(rng);
    X0[X_PREVFLOW] = flow(rng);
    const double *pp = TONE ? p.data() : nullptr;
    // the reference: output_filter_run (tone_output_run) over the whole run, in place
    std::vector<double> XA = X0, o = f;
    if (TONE) tone_output_run(XA.data(), T.consts, pp, o.data(), n);
    else output_filter_run(XA.data(), T.consts, o.data(), n);
    for (int s = 0; s <= n; ++s) {
      std::vector<double> XB = X0;
      const int a = (n + s) % 4;  // the row's alignment; the second run's is (a + s) % 4
      std::vector<float> out((size_t)(4 + a + n + 4 + 3), canary());
      // (a 16-byte aligned start inside the vector, so that `a` is the alignment in floats)
      float *al = out.data() + ((16 - (reinterpret_cast<uintptr_t>(out.data()) & 15)) & 15) / 4;
      float *row = al + 4 + a;
      output_filter_run_f32<TONE, 4>(XB.data(), T.consts, f.data(), s, pp, row);
      output_filter_run_f32<TONE, 4>(XB.data(), T.consts, f.data() + s, n - s, TONE ? pp + s : nullptr, row + s);
      for (int i = 0; i < n; ++i)
        // (two NaNs count as equal: which operand's payload an x86 sum of two NaNs keeps is the host
        // compiler's choice of operand order, not the filter's)
        if (fbits(row[i]) != fbits((float)o[(size_t)i]) && !(row[i] != row[i] && o[(size_t)i] != o[(size_t)i])) {
          std::printf("filter tone=%d n=%d split=%d: sample %d is %08x, want %08x (%a)\n", (int)TONE, n, s, i,
                      fbits(row[i]), fbits((float)o[(size_t)i]), o[(size_t)i]);
          return 1;
        }
      for (float *q = out.data(); q < out.data() + out.size(); ++q)
        if ((q < row || q >= row + n) && fbits(*q) != CANARY) {
          std::printf("filter tone=%d n=%d split=%d: wrote outside the row at %d\n", (int)TONE, n, s, (int)(q - row));
          return 1;
        }
      if (std::memcmp(XA.data(), XB.data(), sizeof(double) * X_TOTAL) != 0) {
        std::printf("filter tone=%d n=%d split=%d: state images differ\n", (int)TONE, n, s);
        return 1;
      }
      if (poison && XB[X_NONFIN] != 1.0) {
        std::printf("filter tone=%d n=%d split=%d: X_NONFIN not set\n", (int)TONE, n, s);
        return 1;
      }
    }
  }
  return 0;
}

int main() {
  if (check_cast() || check_pack()) return 1;
  static Tables T;
  build_tables(&T, 22050.0, default_options());
  std::mt19937_64 rng(20241021);
  if (check_filter<false>(T, rng, false) || check_filter<true>(T, rng, false)) return 1;
  if (check_filter<false>(T, rng, true) || check_filter<true>(T, rng, true)) return 1;
  std::printf("f32-ok\n");
  return 0;
}
