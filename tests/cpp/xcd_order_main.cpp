// xcd_order_main.cpp -- afs_xcd_order.h on the CPU (tests/test_xcd_order.py builds it with
// AddressSanitizer and UndefinedBehaviorSanitizer): the slot order of utterances that share
// trajectories, for batches of one block, many blocks, a partly padded last block and several
// rounds of concurrent blocks.  Prints "xcd-order-ok", or the first property that fails.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "afs_xcd_order.h"

namespace {

constexpr int XCDS = 8;  // (blocks are dealt to the XCDs round-robin: block b runs on XCD b % 8)

int fail(int B, int upb, int conc, const char *what, long at) {
  std::printf("B=%d upb=%d conc=%d: %s (at %ld)\n", B, upb, conc, what, at);
  return 1;
}

int check(int B, int upb, int conc) {
  std::vector<int32_t> row((size_t)B);
  for (int u = 0; u < B; ++u) row[(size_t)u] = u % 3;  // rows repeat with period 3
  const std::vector<int32_t> order = afs::xcd_order(row, B, upb, conc);
  const int nb = (B + upb - 1) / upb;
  if (order.size() != (size_t)nb * (size_t)upb) return fail(B, upb, conc, "size", (long)order.size());
  // every utterance once, every other entry the padding value B
  std::vector<int> seen((size_t)B, 0);
  for (size_t q = 0; q < order.size(); ++q) {
    const int32_t u = order[q];
    if (u < 0 || u > B) return fail(B, upb, conc, "entry out of range", (long)q);
    if (u < B && ++seen[(size_t)u] > 1) return fail(B, upb, conc, "utterance twice", (long)q);
  }
  for (int u = 0; u < B; ++u)
    if (seen[(size_t)u] != 1) return fail(B, upb, conc, "utterance missing", u);
  // within a block: the non-padding entries ascend in (row, utterance)
  for (int b = 0; b < nb; ++b) {
    std::pair<int32_t, int32_t> last{-1, -1};
    for (int g = 0; g < upb; ++g) {
      const int32_t u = order[(size_t)b * upb + g];
      if (u == B) continue;
      const std::pair<int32_t, int32_t> key{row[(size_t)u], u};
      if (!(last < key)) return fail(B, upb, conc, "block not ascending", (long)b * upb + g);
      last = key;
    }
  }
  // round by round, XCD 0's blocks, then XCD 1's, ...: the row-sorted list, the padding at its end
  std::vector<int32_t> sorted((size_t)B);
  for (int u = 0; u < B; ++u) sorted[(size_t)u] = u;
  std::sort(sorted.begin(), sorted.end(), [&](int32_t a, int32_t b) {
    return std::make_pair(row[(size_t)a], a) < std::make_pair(row[(size_t)b], b);
  });
  long q = 0;
  for (int r0 = 0; r0 < nb; r0 += conc)
    for (int x = 0; x < XCDS; ++x)
      for (int b = r0 + x; b < std::min(nb, r0 + conc); b += XCDS)
        for (int g = 0; g < upb; ++g, ++q) {
          const int32_t want = q < B ? sorted[(size_t)q] : B;
          if (order[(size_t)b * upb + g] != want) return fail(B, upb, conc, "not the row-sorted list", q);
        }
  if (q != (long)nb * upb) return fail(B, upb, conc, "blocks visited", q);
  return 0;
}

}  // namespace

int main() {
  static const int cases[][3] = {{1, 8, 1}, {5, 1, 4}, {21, 8, 2}, {64, 8, 3}, {130, 8, 256}};
  for (const auto &c : cases)
    if (check(c[0], c[1], c[2])) return 1;
  std::printf("xcd-order-ok\n");
  return 0;
}
