// afs_xcd_order.h -- the slot order of the tree kernel for utterances that share trajectories
// (host-only code: libafs.so calls it from afs_play_target_sequences, tests/cpp/xcd_order_main.cpp
// from a CPU program).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace afs {

// Slot order of the tree kernel for utterances that share trajectories (row[u]: the utterance's
// frame row): the utterances sorted by row, and the sorted list cut into contiguous chunks so that
// the blocks one XCD runs at the same time play as few rows as possible -- each of the 8 XCDs has
// its own L2, and blocks are dealt to them round-robin (block b shares an XCD with b + 8,
// MI355X_MICROARCH.md, workgroup dispatch), in rounds of `conc` blocks (the blocks the GPU holds
// at once).  Entry (block * upb + g) = the utterance of that slot, B for padding slots.
// (Against the utterance order: +2.2 %, profiles/r04f_xcd_order_ab.txt.)
inline std::vector<int32_t> xcd_order(const std::vector<int32_t> &row, int B, int upb, int conc) {
  constexpr int XCDS = 8;
  std::vector<int32_t> idx((size_t)B);
  for (int u = 0; u < B; ++u) idx[(size_t)u] = u;
  std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) { return row[(size_t)a] < row[(size_t)b]; });
  const int nb = (B + upb - 1) / upb;
  conc = std::max(conc, 1);
  std::vector<int32_t> order((size_t)nb * (size_t)upb, B);
  for (int r0 = 0; r0 < nb; r0 += conc) {  // one round: blocks r0 .. r0 + nr - 1
    const int nr = std::min(conc, nb - r0);
    int chunk = r0;  // (the sorted chunks of this round, XCD by XCD)
    for (int x = 0; x < XCDS; ++x)
      for (int b = r0 + x; b < r0 + nr; b += XCDS, ++chunk)
        for (int g = 0; g < upb; ++g) {
          const int64_t q = (int64_t)chunk * upb + g;
          if (q < B) order[(size_t)b * upb + g] = idx[(size_t)q];
        }
  }
  return order;
}

}  // namespace afs
