// afs_ragged_order.h -- the slot layout of the tree kernel for utterances of different lengths
// (host-only code: libafs.so calls it from afs_synthesize_ragged, tests/cpp/ragged_order_main.cpp
// from a CPU program).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace afs {

// K1's launch layout of a ragged call.  The waves of a block meet at workgroup barriers, so a block's
// time loop ends at one sample for all its slots: a block holds utterances of one length only.
//   order[block * upb + g]    the utterance of the slot, B for a padding slot
//   standin[block * upb + g]  the utterance whose frames, plans and state the slot reads: itself for
//                             a live slot, a live utterance of the same block for a padding slot
//                             (which computes on them and stores nothing).  Never utterance 0 as in
//                             the uniform calls: it may be shorter than the block, and its frames
//                             and hop records past its own end do not exist.
//   block_end[block]          (num_frames - 1) * hop of the block's utterances: the sample of the
//                             call at which its time loop ends
struct RaggedOrder {
  std::vector<int32_t> order, standin;
  std::vector<int64_t> block_end;
  int grid = 0;
};

// The utterances grouped by num_frames, each group in whole blocks of `upb` slots (its last block
// filled with padding slots: at most (upb - 1) x distinct lengths of them), the groups longest first
// -- the launch's tail is then short blocks -- and call order inside a group.  Equal lengths give
// the identity order in ceil(B / upb) blocks.
inline RaggedOrder ragged_order(const int32_t *num_frames, int B, int upb, int hop) {
  RaggedOrder r;
  if (B <= 0 || upb <= 0) return r;
  std::vector<int32_t> idx((size_t)B);
  for (int u = 0; u < B; ++u) idx[(size_t)u] = u;
  std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) { return num_frames[a] > num_frames[b]; });
  for (int q0 = 0; q0 < B;) {
    int q1 = q0;
    while (q1 < B && num_frames[idx[(size_t)q1]] == num_frames[idx[(size_t)q0]]) ++q1;  // one length: idx[q0 .. q1)
    for (int q = q0; q < q1; q += upb) {
      const int32_t first = idx[(size_t)q];
      for (int g = 0; g < upb; ++g) {
        const bool live = q + g < q1;
        r.order.push_back(live ? idx[(size_t)(q + g)] : B);
        r.standin.push_back(live ? idx[(size_t)(q + g)] : first);
      }
      r.block_end.push_back((int64_t)(num_frames[first] - 1) * hop);
    }
    q0 = q1;
  }
  r.grid = (int)r.block_end.size();
  return r;
}

// K1's launch layout of a session pool call (afs_session_synthesize_ragged): voice u plays
// transitions[u] frame transitions of `hop` samples, and a voice with none -- idle, or one that only
// latches its first frame -- takes no slot at all: K1 never sees it.  The live voices are laid out as
// ragged_order lays out utterances (grouped by length in whole blocks, longest first, call order
// inside a group, a padding slot reading the first live voice of its own block); a padding slot holds
// B.  block_end[block] = transitions x hop.  No live voice: grid 0, nothing to launch.  Equal
// non-zero lengths give the identity order.
inline RaggedOrder pool_order(const int32_t *transitions, int B, int upb, int hop) {
  RaggedOrder r;
  if (B <= 0 || upb <= 0) return r;
  std::vector<int32_t> idx;
  for (int u = 0; u < B; ++u)
    if (transitions[u] > 0) idx.push_back(u);
  const int L = (int)idx.size();
  std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) { return transitions[a] > transitions[b]; });
  for (int q0 = 0; q0 < L;) {
    int q1 = q0;
    while (q1 < L && transitions[idx[(size_t)q1]] == transitions[idx[(size_t)q0]]) ++q1;  // one length: idx[q0 .. q1)
    for (int q = q0; q < q1; q += upb) {
      const int32_t first = idx[(size_t)q];
      for (int g = 0; g < upb; ++g) {
        const bool live = q + g < q1;
        r.order.push_back(live ? idx[(size_t)(q + g)] : B);
        r.standin.push_back(live ? idx[(size_t)(q + g)] : first);
      }
      r.block_end.push_back((int64_t)transitions[first] * hop);
    }
    q0 = q1;
  }
  r.grid = (int)r.block_end.size();
  return r;
}

}  // namespace afs
