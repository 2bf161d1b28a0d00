// indexed_main.cpp -- afs_indexed.h on the CPU (tests/test_indexed_cpu.py builds it with AddressSanitizer
// and UndefinedBehaviorSanitizer): the host side of the indexed pool calls as afs_capi.cpp runs it.  The
// check of the spans (bounds, INT64_MAX without overflow, the idle voice whose start is not looked at),
// their hull and rebased starts, and the compaction of a host corpus' live spans: sizes, order, the
// rewritten start indices, every frame read inside a live span only (the corpus is an exact-size heap
// block between canary-free bounds, so a read outside it is the sanitizer's to report).  Real frames
// (afs_frame, 1072 bytes).  Prints "indexed-ok", or the first property that fails.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "afs_indexed.h"
#include "afs_model.h"

namespace {

int fail(const char *name, const char *what, long at) {
  std::printf("%s: %s (at %ld)\n", name, what, at);
  return 1;
}

constexpr int64_t MAX64 = std::numeric_limits<int64_t>::max();
constexpr int64_t MIN64 = std::numeric_limits<int64_t>::min();
constexpr int32_t MAX32 = std::numeric_limits<int32_t>::max();

int check_bounds() {
  const char *name = "check";
  struct Case {
    int64_t total;
    std::vector<int64_t> start;
    std::vector<int32_t> count;
    afs::IndexedFault fault;
    int voice;
  };
  const std::vector<Case> cases = {
      {10, {0, 3, 7}, {3, 4, 3}, afs::INDEXED_OK, -1},              // spans abut, the last ends at total
      {10, {0, 0, 0}, {10, 10, 1}, afs::INDEXED_OK, -1},            // spans coincide and nest
      {10, {2, 1, 0}, {5, 5, 5}, afs::INDEXED_OK, -1},              // spans overlap, starts descending
      {0, {0, 0}, {0, 0}, afs::INDEXED_OK, -1},                     // an empty corpus, every voice idle
      {10, {MAX64, MIN64, -1, 10, 11}, {0, 0, 0, 0, 0}, afs::INDEXED_OK, -1},  // idle: any start passes
      {10, {0, MAX64, 5}, {2, 0, 5}, afs::INDEXED_OK, -1},          // an idle voice between live ones
      {-1, {0}, {0}, afs::INDEXED_TOTAL, -1},
      {MIN64, {0}, {1}, afs::INDEXED_TOTAL, -1},
      {10, {0, 4}, {2, -1}, afs::INDEXED_COUNT, 1},
      {10, {MAX64}, {-2147483647 - 1}, afs::INDEXED_COUNT, 0},
      {10, {-1}, {1}, afs::INDEXED_START, 0},
      {10, {0, MIN64}, {1, 1}, afs::INDEXED_START, 1},
      {10, {0, 8}, {10, 3}, afs::INDEXED_END, 1},                   // one frame past the end
      {10, {10}, {1}, afs::INDEXED_END, 0},                         // starts at the end
      {10, {0}, {11}, afs::INDEXED_END, 0},                         // more frames than the corpus has
      {0, {0}, {1}, afs::INDEXED_END, 0},                           // a live voice on an empty corpus
      {10, {MAX64}, {1}, afs::INDEXED_END, 0},                      // start + count would overflow
      {10, {MAX64}, {MAX32}, afs::INDEXED_END, 0},
      {MAX64, {MAX64}, {1}, afs::INDEXED_END, 0},                   // one past the largest corpus
      {MAX64, {MAX64 - 1}, {1}, afs::INDEXED_OK, -1},               // its last frame
      {MAX64, {MAX64 - MAX32}, {MAX32}, afs::INDEXED_OK, -1},       // its last 2^31 - 1 frames
      {MAX64, {MAX64 - MAX32 + 1}, {MAX32}, afs::INDEXED_END, 0},
  };
  for (size_t k = 0; k < cases.size(); ++k) {
    const Case &t = cases[k];
    const afs::IndexedCheck r = afs::indexed_check(t.start.data(), t.count.data(), (int)t.start.size(), t.total);
    if (r.fault != t.fault) return fail(name, "fault", (long)k);
    if (r.voice != t.voice) return fail(name, "voice at fault", (long)k);
  }
  const int64_t one64 = 0;
  const int32_t one32 = 1;
  if (afs::indexed_check(nullptr, &one32, 1, 10).fault != afs::INDEXED_NULL) return fail(name, "null start", 0);
  if (afs::indexed_check(&one64, nullptr, 1, 10).fault != afs::INDEXED_NULL) return fail(name, "null count", 0);
  if (afs::indexed_check(nullptr, nullptr, 0, -1).fault != afs::INDEXED_TOTAL) return fail(name, "total first", 0);
  return 0;
}

int check_spans() {
  const char *name = "spans";
  {  // idle voices with wild starts take no part in the hull
    const std::vector<int64_t> start = {40, MAX64, 12, MIN64, 30};
    const std::vector<int32_t> count = {5, 0, 3, 0, 20};
    const afs::IndexedSpans s = afs::indexed_spans(start.data(), count.data(), 5);
    if (s.first != 12 || s.end != 50 || s.sum != 28 || s.longest != 20) return fail(name, "hull", 0);
    std::vector<int64_t> re(5, -7);
    afs::indexed_rebase(start.data(), count.data(), 5, s.first, re.data());
    if (re != std::vector<int64_t>{28, 0, 0, 0, 18}) return fail(name, "rebased starts", 0);
    afs::indexed_rebase(start.data(), count.data(), 5, 0, re.data());
    if (re != std::vector<int64_t>{40, 0, 12, 0, 30}) return fail(name, "starts in place", 0);
  }
  {  // no live voice
    const std::vector<int64_t> start = {MAX64, -3};
    const std::vector<int32_t> count = {0, 0};
    const afs::IndexedSpans s = afs::indexed_spans(start.data(), count.data(), 2);
    if (s.first != 0 || s.end != 0 || s.sum != 0 || s.longest != 0) return fail(name, "empty hull", 0);
  }
  {  // the top of the index range: the hull's end is exact
    const std::vector<int64_t> start = {MAX64 - 4};
    const std::vector<int32_t> count = {4};
    const afs::IndexedSpans s = afs::indexed_spans(start.data(), count.data(), 1);
    if (s.first != MAX64 - 4 || s.end != MAX64 || s.sum != 4) return fail(name, "hull at INT64_MAX", 0);
  }
  return 0;
}

// frame k of the corpus carries k in every double it has
void tag(afs_frame *f, int64_t k) {
  double v[sizeof(afs_frame) / sizeof(double)];
  for (double &x : v) x = (double)k;
  std::memcpy(static_cast<void *>(f), v, sizeof v);
}
int64_t tag_of(const afs_frame *f) {
  double v[sizeof(afs_frame) / sizeof(double)];
  std::memcpy(v, static_cast<const void *>(f), sizeof v);
  for (double x : v)
    if (x != v[0]) return -1;
  return (int64_t)v[0];
}

int check_compact() {
  const char *name = "compact";
  static_assert(sizeof(afs_frame) == 1072 && sizeof(afs_frame) % sizeof(double) == 0, "frame");
  const int64_t total = 37;
  std::vector<afs_frame> corpus((size_t)total);  // (exactly total frames: a read past either end is out of bounds)
  for (int64_t k = 0; k < total; ++k) tag(&corpus[(size_t)k], k);
  // live spans in no order, two that coincide, two that overlap, one at each end; idle voices with wild starts
  const std::vector<int64_t> start = {30, MAX64, 0, 12, 12, MIN64, 14, 34, -1};
  const std::vector<int32_t> count = {4, 0, 2, 5, 5, 0, 6, 3, 0};
  const int B = (int)start.size();
  if (afs::indexed_check(start.data(), count.data(), B, total).fault != afs::INDEXED_OK) return fail(name, "refused", 0);
  const afs::IndexedSpans s = afs::indexed_spans(start.data(), count.data(), B);
  if (s.sum != 25 || s.first != 0 || s.end != 37 || s.longest != 6) return fail(name, "spans", (long)s.sum);
  std::vector<afs_frame> staging((size_t)s.sum);  // (exactly the sum of the counts: a write past it is out of bounds)
  std::vector<int64_t> packed((size_t)B, -7);
  const int64_t wrote = afs::indexed_compact(corpus.data(), start.data(), count.data(), B, staging.data(), packed.data());
  if (wrote != s.sum) return fail(name, "frames written", (long)wrote);
  int64_t at = 0;
  for (int u = 0; u < B; ++u) {
    if (count[(size_t)u] == 0) {
      if (packed[(size_t)u] != 0) return fail(name, "an idle voice's start", u);
      continue;
    }
    if (packed[(size_t)u] != at) return fail(name, "a live voice's start: back to back, in voice order", u);
    for (int k = 0; k < count[(size_t)u]; ++k)
      if (tag_of(&staging[(size_t)(at + k)]) != start[(size_t)u] + k) return fail(name, "a staged frame", u);
    at += count[(size_t)u];
  }
  // the rewritten call passes the same check against the staging's size, and reads the same frames
  if (afs::indexed_check(packed.data(), count.data(), B, wrote).fault != afs::INDEXED_OK) return fail(name, "packed refused", 0);
  for (int64_t k = 0; k < total; ++k)
    if (tag_of(&corpus[(size_t)k]) != k) return fail(name, "the corpus changed", (long)k);
  // every voice idle: nothing is read or written (null arrays pass)
  const std::vector<int32_t> none((size_t)B, 0);
  std::vector<int64_t> p2((size_t)B, -7);
  if (afs::indexed_compact<afs_frame>(nullptr, start.data(), none.data(), B, nullptr, p2.data()) != 0) return fail(name, "idle", 0);
  if (p2 != std::vector<int64_t>((size_t)B, 0)) return fail(name, "idle starts", 0);
  return 0;
}

}  // namespace

int main() {
  int bad = check_bounds();
  if (!bad) bad = check_spans();
  if (!bad) bad = check_compact();
  if (!bad) std::printf("indexed-ok\n");
  return bad;
}
