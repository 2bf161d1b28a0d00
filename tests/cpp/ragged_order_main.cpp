// ragged_order_main.cpp -- afs_ragged_order.h on the CPU (tests/test_ragged_cpu.py builds it with
// AddressSanitizer and UndefinedBehaviorSanitizer): the slot layout of utterances of different
// lengths, for one utterance, a mixed batch, equal lengths, all distinct lengths, one-slot blocks and
// 16-slot blocks.  Prints "ragged-order-ok", or the first property that fails.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "afs_ragged_order.h"

namespace {

constexpr int HOP = 33;

int fail(const char *name, const char *what, long at) {
  std::printf("%s: %s (at %ld)\n", name, what, at);
  return 1;
}

int check(const char *name, const std::vector<int32_t> &nf, int upb) {
  const int B = (int)nf.size();
  const afs::RaggedOrder r = afs::ragged_order(nf.data(), B, upb, HOP);
  if (r.grid <= 0 || r.block_end.size() != (size_t)r.grid) return fail(name, "grid", r.grid);
  if (r.order.size() != (size_t)r.grid * upb || r.standin.size() != r.order.size()) return fail(name, "size", (long)r.order.size());
  // every utterance in exactly one slot; every other slot is padding and holds a value >= B
  std::vector<int> seen((size_t)B, 0);
  long padding = 0;
  for (size_t q = 0; q < r.order.size(); ++q) {
    const int32_t u = r.order[q];
    if (u < 0) return fail(name, "negative entry", (long)q);
    if (u >= B) ++padding;
    else if (++seen[(size_t)u] > 1) return fail(name, "utterance twice", (long)q);
  }
  for (int u = 0; u < B; ++u)
    if (seen[(size_t)u] != 1) return fail(name, "utterance missing", u);
  const std::set<int32_t> distinct(nf.begin(), nf.end());
  if (padding > (long)(upb - 1) * (long)distinct.size()) return fail(name, "too many padding slots", padding);
  for (int b = 0; b < r.grid; ++b) {
    std::set<int32_t> live;
    for (int g = 0; g < upb; ++g) {
      const int32_t u = r.order[(size_t)b * upb + g];
      if (u < B) live.insert(u);
    }
    if (live.empty()) return fail(name, "block of padding only", b);
    for (int g = 0; g < upb; ++g) {
      const size_t q = (size_t)b * upb + g;
      const int32_t u = r.order[q], s = r.standin[q];
      // a live slot reads its own data, a padding slot a live utterance's of the same block
      if (u < B && s != u) return fail(name, "live slot with another's data", (long)q);
      if (u >= B && !live.count(s)) return fail(name, "stand-in not a live utterance of the block", (long)q);
      // all live utterances of a block end where the block ends
      if (u < B && (int64_t)(nf[(size_t)u] - 1) * HOP != r.block_end[(size_t)b]) return fail(name, "block_end", (long)q);
    }
    if (b > 0 && r.block_end[(size_t)b] > r.block_end[(size_t)b - 1]) return fail(name, "blocks grow", b);
  }
  // call order inside a length group: equal lengths appear in ascending utterance order
  std::vector<int32_t> last_of((size_t)1 << 16, -1);
  for (size_t q = 0; q < r.order.size(); ++q) {
    const int32_t u = r.order[q];
    if (u >= B) continue;
    int32_t &last = last_of[(size_t)nf[(size_t)u]];
    if (u < last) return fail(name, "group not in call order", (long)q);
    last = u;
  }
  if (distinct.size() == 1) {  // equal lengths: the identity in ceil(B / upb) blocks
    if (r.grid != (B + upb - 1) / upb) return fail(name, "equal lengths: blocks", r.grid);
    for (int u = 0; u < B; ++u)
      if (r.order[(size_t)u] != u) return fail(name, "equal lengths: not the identity", u);
  }
  // deterministic
  const afs::RaggedOrder again = afs::ragged_order(nf.data(), B, upb, HOP);
  if (again.order != r.order || again.standin != r.standin || again.block_end != r.block_end || again.grid != r.grid)
    return fail(name, "not deterministic", 0);
  return 0;
}

}  // namespace

int main() {
  const std::vector<int32_t> mixed = {7, 2, 5, 5, 3, 7, 2, 5, 5, 5, 5, 5, 5, 5, 5, 4, 5, 6, 6, 2, 3};
  std::vector<int32_t> distinct9, tiled1025, tiled40;
  for (int u = 0; u < 9; ++u) distinct9.push_back(2 + u);
  for (int u = 0; u < 1025; ++u) tiled1025.push_back(mixed[(size_t)u % mixed.size()]);
  for (int u = 0; u < 40; ++u) tiled40.push_back(mixed[(size_t)u % mixed.size()]);
  if (check("(1, 8)", {5}, 8)) return 1;
  if (check("(21, 8)", mixed, 8)) return 1;
  if (check("(64, 8) equal", std::vector<int32_t>(64, 6), 8)) return 1;
  if (check("(9, 8) distinct", distinct9, 8)) return 1;
  if (check("(1025, 1)", tiled1025, 1)) return 1;
  if (check("(40, 16)", tiled40, 16)) return 1;
  // the mixed batch, spelled out: lengths 7, 6, 5, 4, 3, 2 -> blocks of 2, 2, 8 + 3, 1, 2, 3 utterances
  const afs::RaggedOrder r = afs::ragged_order(mixed.data(), 21, 8, HOP);
  const int64_t ends[] = {6 * HOP, 5 * HOP, 4 * HOP, 4 * HOP, 3 * HOP, 2 * HOP, 1 * HOP};
  if (r.grid != 7) return fail("(21, 8)", "seven blocks", r.grid);
  for (int b = 0; b < 7; ++b)
    if (r.block_end[(size_t)b] != ends[b]) return fail("(21, 8)", "block ends", b);
  const int32_t first[] = {0, 5, 21, 21, 21, 21, 21, 21};
  for (int g = 0; g < 8; ++g)
    if (r.order[(size_t)g] != first[g] || r.standin[(size_t)g] != (g == 1 ? 5 : 0)) return fail("(21, 8)", "first block", g);
  std::printf("ragged-order-ok\n");
  return 0;
}
