// pool_order_main.cpp -- afs_ragged_order.h pool_order on the CPU (tests/test_pool_cpu.py builds it
// with AddressSanitizer and UndefinedBehaviorSanitizer): the slot layout of a session pool call, whose
// voices play different numbers of transitions and may play none.  Prints "pool-order-ok", or the
// first property that fails.
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

int check(const char *name, const std::vector<int32_t> &tr, int upb) {
  const int B = (int)tr.size();
  const afs::RaggedOrder r = afs::pool_order(tr.data(), B, upb, HOP);
  int live_voices = 0;
  for (int32_t t : tr) live_voices += t > 0;
  if (r.grid < 0 || r.block_end.size() != (size_t)r.grid) return fail(name, "grid", r.grid);
  if (r.order.size() != (size_t)r.grid * upb || r.standin.size() != r.order.size()) return fail(name, "size", (long)r.order.size());
  if (live_voices == 0 && r.grid != 0) return fail(name, "all idle: blocks", r.grid);
  if (live_voices > 0 && r.grid == 0) return fail(name, "live voices, no block", live_voices);
  // every live voice in exactly one slot, a voice without transitions in none; every other slot holds B
  std::vector<int> seen((size_t)B, 0);
  long padding = 0;
  for (size_t q = 0; q < r.order.size(); ++q) {
    const int32_t u = r.order[q];
    if (u < 0 || u > B) return fail(name, "entry outside 0..B", (long)q);
    if (u == B) ++padding;
    else if (tr[(size_t)u] <= 0) return fail(name, "idle voice in a slot", (long)q);
    else if (++seen[(size_t)u] > 1) return fail(name, "voice twice", (long)q);
  }
  for (int u = 0; u < B; ++u)
    if (seen[(size_t)u] != (tr[(size_t)u] > 0 ? 1 : 0)) return fail(name, "live voice missing", u);
  std::set<int32_t> distinct;
  for (int32_t t : tr)
    if (t > 0) distinct.insert(t);
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
      if (u < B && s != u) return fail(name, "live slot with another's data", (long)q);
      if (u >= B && !live.count(s)) return fail(name, "stand-in not a live voice of the block", (long)q);
      // a block holds one length, and ends there
      if (u < B && (int64_t)tr[(size_t)u] * HOP != r.block_end[(size_t)b]) return fail(name, "block_end", (long)q);
    }
    if (r.block_end[(size_t)b] <= 0) return fail(name, "empty block", b);
    if (b > 0 && r.block_end[(size_t)b] > r.block_end[(size_t)b - 1]) return fail(name, "blocks grow", b);
  }
  // call order inside a length group
  std::vector<int32_t> last_of((size_t)1 << 16, -1);
  for (size_t q = 0; q < r.order.size(); ++q) {
    const int32_t u = r.order[q];
    if (u >= B) continue;
    int32_t &last = last_of[(size_t)tr[(size_t)u]];
    if (u < last) return fail(name, "group not in call order", (long)q);
    last = u;
  }
  if (distinct.size() == 1 && live_voices == B) {  // equal lengths: the identity in ceil(B / upb) blocks
    if (r.grid != (B + upb - 1) / upb) return fail(name, "equal lengths: blocks", r.grid);
    for (int u = 0; u < B; ++u)
      if (r.order[(size_t)u] != u) return fail(name, "equal lengths: not the identity", u);
  }
  const afs::RaggedOrder again = afs::pool_order(tr.data(), B, upb, HOP);
  if (again.order != r.order || again.standin != r.standin || again.block_end != r.block_end || again.grid != r.grid)
    return fail(name, "not deterministic", 0);
  return 0;
}

}  // namespace

int main() {
  // (transitions: what a step of the streamed corpus looks like -- chunks of 3, ends of utterances,
  // latch-only and idle voices)
  const std::vector<int32_t> mixed = {3, 0, 2, 3, 1, 0, 3, 3, 3, 2, 0, 3, 3, 3, 3, 1, 3, 0, 3, 3, 3};
  std::vector<int32_t> distinct9, tiled1025, tiled40, tail;
  for (int u = 0; u < 9; ++u) distinct9.push_back(u);  // (voice 0 idle)
  for (int u = 0; u < 1025; ++u) tiled1025.push_back(u < 5 ? mixed[(size_t)u] : (u % 3 == 0 ? 0 : 1));
  for (int u = 0; u < 40; ++u) tiled40.push_back(mixed[(size_t)u % mixed.size()]);
  for (int u = 0; u < 11; ++u) tail.push_back(u == 7 ? 2 : 0);  // (a dry corpus: one voice left)
  if (check("(1, 8) idle", {0}, 8)) return 1;
  if (check("(1, 8)", {4}, 8)) return 1;
  if (check("(21, 8)", mixed, 8)) return 1;
  if (check("(64, 8) equal", std::vector<int32_t>(64, 3), 8)) return 1;
  if (check("(64, 8) all idle", std::vector<int32_t>(64, 0), 8)) return 1;
  if (check("(9, 8) distinct", distinct9, 8)) return 1;
  if (check("(1025, 1)", tiled1025, 1)) return 1;
  if (check("(40, 16)", tiled40, 16)) return 1;
  if (check("(11, 8) tail", tail, 8)) return 1;
  if (check("(3, 1) all idle", {0, 0, 0}, 1)) return 1;
  // the mixed step, spelled out: 13 voices of 3 transitions, 2 of 2, 2 of 1, 4 idle -> blocks of 8 + 5, 2, 2
  const afs::RaggedOrder r = afs::pool_order(mixed.data(), 21, 8, HOP);
  const int64_t ends[] = {3 * HOP, 3 * HOP, 2 * HOP, 1 * HOP};
  if (r.grid != 4) return fail("(21, 8)", "four blocks", r.grid);
  for (int b = 0; b < 4; ++b)
    if (r.block_end[(size_t)b] != ends[b]) return fail("(21, 8)", "block ends", b);
  const int32_t first[] = {0, 3, 6, 7, 8, 11, 12, 13}, third[] = {2, 9, 21, 21, 21, 21, 21, 21};
  for (int g = 0; g < 8; ++g) {
    if (r.order[(size_t)g] != first[g] || r.standin[(size_t)g] != first[g]) return fail("(21, 8)", "first block", g);
    if (r.order[(size_t)16 + g] != third[g] || r.standin[(size_t)16 + g] != (g < 2 ? third[g] : 2))
      return fail("(21, 8)", "third block", g);
  }
  // the tail: one block, voice 7 and seven padding slots that read it
  const afs::RaggedOrder t = afs::pool_order(tail.data(), 11, 8, HOP);
  if (t.grid != 1 || t.order[0] != 7 || t.block_end[0] != 2 * HOP) return fail("(11, 8) tail", "one block", t.grid);
  for (int g = 1; g < 8; ++g)
    if (t.order[(size_t)g] != 11 || t.standin[(size_t)g] != 7) return fail("(11, 8) tail", "padding", g);
  std::printf("pool-order-ok\n");
  return 0;
}
