// afs_indexed.h -- the host side of the indexed pool calls (afs_session_synthesize_indexed and its packed
// twin, afs_capi.cpp pool_core): voice u plays frames[start[u] .. start[u] + count[u]) of one flat array
// of `total` frames.  The check of the spans, their hull, and the compaction of a host corpus' live spans
// into a staging array.  Host only, no HIP: tests/cpp/indexed_main.cpp runs it as a CPU program.
#pragma once

#include <cstdint>
#include <cstring>

namespace afs {

// the frame source of an indexed pool call, as the caller gave it
struct FrameIndex {
  const int64_t *start = nullptr;  // [batch], a host array
  int64_t total = 0;               // frames in the flat array
};

enum IndexedFault {
  INDEXED_OK = 0,
  INDEXED_TOTAL,  // total < 0
  INDEXED_NULL,   // start or count is null
  INDEXED_COUNT,  // a count below 0
  INDEXED_START,  // a live voice's start below 0
  INDEXED_END     // a live voice's span ends past total
};
struct IndexedCheck {
  IndexedFault fault = INDEXED_OK;
  int voice = -1;  // the first voice at fault (INDEXED_COUNT, _START, _END)
};

// Every live voice's span lies in [0, total).  An idle voice (count 0) passes whatever its start.  No sum
// is formed that can overflow: with 0 <= count and 0 <= total, total - count is exact.
inline IndexedCheck indexed_check(const int64_t *start, const int32_t *count, int B, int64_t total) {
  IndexedCheck r;
  if (total < 0) return r.fault = INDEXED_TOTAL, r;
  if (!start || !count) return r.fault = INDEXED_NULL, r;
  for (int u = 0; u < B; ++u) {
    const int64_t c = count[u];
    r.voice = u;
    if (c < 0) return r.fault = INDEXED_COUNT, r;
    if (c == 0) continue;
    if (start[u] < 0) return r.fault = INDEXED_START, r;
    if (start[u] > total - c) return r.fault = INDEXED_END, r;
  }
  r.voice = -1;
  return r;
}

// What the live spans of a checked call cover: the hull [first, end) (0, 0 without a live voice), the
// largest count and the sum of the counts.
struct IndexedSpans {
  int64_t first = 0, end = 0, sum = 0;
  int32_t longest = 0;
};
inline IndexedSpans indexed_spans(const int64_t *start, const int32_t *count, int B) {
  IndexedSpans s;
  bool any = false;
  for (int u = 0; u < B; ++u) {
    const int32_t c = count[u];
    if (c <= 0) continue;
    if (!any || start[u] < s.first) s.first = start[u];
    if (!any || start[u] + c > s.end) s.end = start[u] + c;
    any = true;
    s.sum += c;
    if (c > s.longest) s.longest = c;
  }
  return s;
}

// The start indices the gather is given when the frames it reads begin at frame `first` of the caller's
// array (the hull's first frame: a misaligned device corpus is copied from there); an idle voice's is 0.
inline void indexed_rebase(const int64_t *start, const int32_t *count, int B, int64_t first, int64_t *rebased) {
  for (int u = 0; u < B; ++u) rebased[u] = count[u] > 0 ? start[u] - first : 0;
}

// A host corpus: the live spans copied back to back, in voice order, into staging (room for the sum of
// the counts); packed[u] is where voice u's span now starts (0 for an idle voice).  Returns the frames
// written.  Spans that overlap in the corpus are copied once per voice.
template <class Frame>
inline int64_t indexed_compact(const Frame *frames, const int64_t *start, const int32_t *count, int B, Frame *staging,
                               int64_t *packed) {
  int64_t at = 0;
  for (int u = 0; u < B; ++u) {
    const int32_t c = count[u];
    packed[u] = c > 0 ? at : 0;
    if (c <= 0) continue;
    std::memcpy(static_cast<void *>(staging + at), static_cast<const void *>(frames + start[u]), (size_t)c * sizeof(Frame));
    at += c;
  }
  return at;
}

}  // namespace afs
