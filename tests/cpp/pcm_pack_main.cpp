// CPU checks of the PCM form of the output stage (csrc/tree_core.h PcmPack, output_filter_run_pcm;
// csrc/afs_audio.h sample_to_int16), built with AddressSanitizer and UndefinedBehaviorSanitizer
// (tests/test_pcm_cpu.py).  Prints "pcm-ok", or the first mismatch and exits 1.
//   1. PcmPack against sample_to_int16 sample by sample: every alignment of the row 0..7 int16, every
//      run length 0..40, in a heap block that ends with the run (the sanitizer sees a byte past it) and
//      with canaries before it.
//   2. output_filter_run_pcm against output_filter_run_t followed by sample_to_int16: n = 1..70, every
//      split into two runs with the state carried through the image, with and without the tone filter:
//      the int16 equal, the images equal bit for bit.
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

static const int16_t CANARY = 0x5a5a;

static std::vector<double> special_values() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> v = {1.0, -1.0, std::nextafter(1.0, 2.0), std::nextafter(1.0, 0.0), std::nextafter(-1.0, -2.0),
                           std::nextafter(-1.0, 0.0), 1.5, -1.5, 1e300, -1e300, inf, -inf, nan, 0.0, -0.0,
                           std::numeric_limits<double>::denorm_min(), -std::numeric_limits<double>::denorm_min(),
                           std::numeric_limits<double>::min() / 2, 0.5, -0.5, 0.999999, -0.999999};
  for (int k : {1, 2, 3, 100, 12345, 16384, 32766, 32767})
    for (double sgn : {1.0, -1.0}) {
      const double x = sgn * (double)k / 32767.0;
      v.push_back(x);
      v.push_back(std::nextafter(x, 2.0));
      v.push_back(std::nextafter(x, -2.0));
    }
  return v;
}

static int check_known_values() {
  struct { double x; int want; } known[] = {
      {1.0, 32767}, {-1.0, -32767}, {2.0, 32767}, {-2.0, -32768}, {std::nextafter(1.0, 2.0), 32767},
      {std::nextafter(-1.0, -2.0), -32768}, {std::numeric_limits<double>::infinity(), 32767},
      {-std::numeric_limits<double>::infinity(), -32768}, {std::numeric_limits<double>::quiet_NaN(), 0}, {0.0, 0},
      {-0.0, 0}, {std::numeric_limits<double>::denorm_min(), 0}, {0.5, 16383}, {-0.5, -16383},
      {std::nextafter(1.0, 0.0), 32766}, {std::nextafter(-1.0, 0.0), -32766}, {1.5 / 32767.0, 1}, {-1.5 / 32767.0, -1}};
  for (const auto &k : known)
    if (sample_to_int16(k.x) != k.want) {
      std::printf("sample_to_int16(%a) = %d, want %d\n", k.x, (int)sample_to_int16(k.x), k.want);
      return 1;
    }
  return 0;
}

static int check_pack() {
  const std::vector<double> vals = special_values();
  size_t next = 0;
  for (int a = 0; a < 8; ++a)
    for (int n = 0; n <= 40; ++n) {
      // the row ends the block: a store past pcm + n is a heap overflow
      int16_t *base = (int16_t *)std::malloc((size_t)(a + n) * sizeof(int16_t) + (a + n == 0));
      if ((reinterpret_cast<uintptr_t>(base) & 15) != 0) {
        std::printf("malloc block not 16-byte aligned\n");
        return 1;
      }
      for (int i = 0; i < a; ++i) base[i] = CANARY;
      for (int i = 0; i < n; ++i) base[a + i] = (int16_t)~CANARY;
      std::vector<double> x((size_t)n);
      for (int i = 0; i < n; ++i) x[(size_t)i] = vals[next++ % vals.size()];
      PcmPack sink(base + a, n);
      for (int t = 0; t < n; ++t) sink.put(t, x[(size_t)t]);
      for (int i = 0; i < a; ++i)
        if (base[i] != CANARY) {
          std::printf("pack: alignment %d, n %d: wrote before the row at %d\n", a, n, i - a);
          return 1;
        }
      for (int i = 0; i < n; ++i)
        if (base[a + i] != sample_to_int16(x[(size_t)i])) {
          std::printf("pack: alignment %d, n %d: sample %d of %a is %d, want %d\n", a, n, i, x[(size_t)i],
                      (int)base[a + i], (int)sample_to_int16(x[(size_t)i]));
          return 1;
        }
      std::free(base);
    }
  // ... and inside a block with canaries on both sides
  alignas(16) int16_t buf[8 + 8 + 40 + 8];
  for (int a = 0; a < 8; ++a)
    for (int n = 0; n <= 40; ++n) {
      for (int16_t &b : buf) b = CANARY;
      PcmPack sink(buf + 8 + a, n);
      for (int t = 0; t < n; ++t) sink.put(t, vals[(size_t)(t * 7 + a + n) % vals.size()]);
      for (int i = 0; i < (int)(sizeof buf / sizeof buf[0]); ++i) {
        const int t = i - 8 - a;
        const int16_t want = t >= 0 && t < n ? sample_to_int16(vals[(size_t)(t * 7 + a + n) % vals.size()]) : CANARY;
        if (buf[i] != want) {
          std::printf("pack: alignment %d, n %d: position %d is %d, want %d\n", a, n, t, (int)buf[i], (int)want);
          return 1;
        }
      }
    }
  return 0;
}

template <bool TONE>
static int check_filter(const Tables &T, std::mt19937_64 &rng, bool poison) {
  std::uniform_real_distribution<double> flow(-300.0, 300.0), pres(-2000.0, 2000.0), st(-1e6, 1e6);
  for (int n = 1; n <= 70; ++n) {
    std::vector<double> f((size_t)n), p((size_t)n), X0(X_TOTAL, 0.0);
    for (double &v : f) v = flow(rng);
    for (double &v : p) v = pres(rng);
    if (poison) f[(size_t)(n / 2)] = n % 2 ? std::numeric_limits<double>::infinity() : std::numeric_limits<double>::quiet_NaN();
    for (int k = 0; k < 16; ++k) X0[X_OUTF + k] = st(rng);
    for (int k = 0; k < 8; ++k) X0[X_TONE + k] = pres(rng);
    X0[X_PREVFLOW] = flow(rng);
    const double *pp = TONE ? p.data() : nullptr;
    for (int s = 0; s <= n; ++s) {
      std::vector<double> XA = X0, XB = X0, o = f;
      output_filter_run_t<TONE, 0>(XA.data(), T.consts, o.data(), s, pp);
      output_filter_run_t<TONE, 0>(XA.data(), T.consts, o.data() + s, n - s, TONE ? pp + s : nullptr);
      const int a = (n + s) % 8;  // the row's alignment; the second run's is (a + s) % 8
      std::vector<int16_t> pcm((size_t)(8 + a + n + 8), CANARY);
      int16_t *row = pcm.data() + 8 + a;
      output_filter_run_pcm<TONE, 2>(XB.data(), T.consts, f.data(), s, pp, row);
      output_filter_run_pcm<TONE, 2>(XB.data(), T.consts, f.data() + s, n - s, TONE ? pp + s : nullptr, row + s);
      for (int i = 0; i < n; ++i)
        if (row[i] != sample_to_int16(o[(size_t)i])) {
          std::printf("filter tone=%d n=%d split=%d: sample %d is %d, want %d (%a)\n", (int)TONE, n, s, i, (int)row[i],
                      (int)sample_to_int16(o[(size_t)i]), o[(size_t)i]);
          return 1;
        }
      for (int i = 0; i < (int)pcm.size(); ++i)
        if ((i < 8 + a || i >= 8 + a + n) && pcm[(size_t)i] != CANARY) {
          std::printf("filter tone=%d n=%d split=%d: wrote outside the row at %d\n", (int)TONE, n, s, i - 8 - a);
          return 1;
        }
      if (std::memcmp(XA.data(), XB.data(), sizeof(double) * X_TOTAL) != 0) {
        std::printf("filter tone=%d n=%d split=%d: state images differ\n", (int)TONE, n, s);
        return 1;
      }
      if (poison && XA[X_NONFIN] != 1.0) {
        std::printf("filter tone=%d n=%d split=%d: X_NONFIN not set\n", (int)TONE, n, s);
        return 1;
      }
    }
  }
  return 0;
}

int main() {
  if (check_known_values() || check_pack()) return 1;
  static Tables T;
  build_tables(&T, 22050.0, default_options());
  std::mt19937_64 rng(20240607);
  if (check_filter<false>(T, rng, false) || check_filter<true>(T, rng, false)) return 1;
  if (check_filter<false>(T, rng, true) || check_filter<true>(T, rng, true)) return 1;
  std::printf("pcm-ok\n");
  return 0;
}
