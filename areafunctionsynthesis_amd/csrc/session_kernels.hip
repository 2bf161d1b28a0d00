// session_kernels.hip -- the per-voice lifecycle of a session's voice pool (afs_session_kernels.h):
// the reset of listed voices and the frame rows of a pool call.  A translation unit of its own: the
// synthesis kernels' code object (tds_tree.hip) stays what it was, register counts included.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "afs_session_kernels.h"
#include "afs_tree.h"
#include "tree_core.h"

namespace afs {

using namespace tree;

namespace {

// tree_reset_kernel over a voice list: thread (i, gl) resets lane gl of voice voices[i], lane 0 its
// LDS image too (output and tone filter state, non-finite flag, rand() state and draw count)
template <int W>
__global__ void __launch_bounds__(256) voice_reset_kernel(Lane<W> *lanes, double *lds, const int32_t *voices,
                                                          const uint32_t *seeds, int n) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)n * W) return;
  const int i = (int)(id / W), gl = (int)(id % W);
  const int u = voices[i];
  Lane<W> R = Lane<W>{};
  reset_lane<W>(gl, R);
  lanes[(int64_t)u * W + gl] = R;
  if (gl == 0) reset_lds(lds + (int64_t)u * X_TOTAL, seeds ? seeds[i] : (uint32_t)u + 1u);
}

constexpr int FRAME_VECS = (int)(sizeof(afs_frame) / 16);  // 67
static_assert(sizeof(afs_frame) % 16 == 0 && FRAME_VECS <= 128, "a frame is at most two 16-byte vectors per lane");
constexpr int ROWS_WAVES = 4;  // waves per block: frames j = blockIdx.y * 4 + wave of voice blockIdx.x

// Wave (u, j) builds frame j of voice u's row; lane l moves vectors l and l + 64.  Wave (u, 0) alone
// touches pair[u][0]: it loads the old latch (a latched voice's row frame 0) and the new one, the last
// frame supplied, and only then stores either.
__global__ void __launch_bounds__(64 * ROWS_WAVES) pool_rows_kernel(const uint4 *frames, int64_t frame_stride,
                                                                     const int32_t *count, const int32_t *latched, int B,
                                                                     uint4 *rows, uint4 *pair) {
  const int u = blockIdx.x;
  const int lane = (int)threadIdx.x & 63;
  const int j = (int)blockIdx.y * ROWS_WAVES + (int)threadIdx.x / 64;
  if (u >= B) return;
  const int c = count[u];
  if (c <= 0) return;  // (idle: nothing of this voice is read or written)
  const int lat = latched[u] != 0 ? 1 : 0;
  if (j >= c + lat) return;  // (wave-uniform; c + lat <= frame_stride + 1)
  const uint4 *src_u = frames + (int64_t)u * frame_stride * FRAME_VECS;
  uint4 *latch = pair + (int64_t)u * 2 * FRAME_VECS;
  const uint4 *src = (j == 0 && lat) ? latch : src_u + (int64_t)(j - lat) * FRAME_VECS;
  uint4 *dst = rows + ((int64_t)u * (frame_stride + 1) + j) * FRAME_VECS;
  const bool two = lane + 64 < FRAME_VECS;
  const uint4 a0 = src[lane];
  uint4 a1 = a0;
  if (two) a1 = src[lane + 64];
  if (j == 0) {
    const uint4 *last = src_u + (int64_t)(c - 1) * FRAME_VECS;
    const uint4 n0 = last[lane];
    uint4 n1 = n0;
    if (two) n1 = last[lane + 64];
    latch[lane] = n0;  // (after this lane's loads of the old latch: the same addresses, the same lane)
    if (two) latch[lane + 64] = n1;
  }
  dst[lane] = a0;
  if (two) dst[lane + 64] = a1;
}

}  // namespace

hipError_t launch_voice_reset(void *lane_state, double *lds_state, const int32_t *voices, const uint32_t *seeds, int n,
                              int lanes, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int64_t t = (int64_t)n * lanes;
  const dim3 grid((unsigned)((t + 255) / 256)), block(256);
  if (lanes == 64)
    hipLaunchKernelGGL(voice_reset_kernel<64>, grid, block, 0, st, (Lane<64> *)lane_state, lds_state, voices, seeds, n);
  else
    hipLaunchKernelGGL(voice_reset_kernel<TREE_W>, grid, block, 0, st, (Lane<TREE_W> *)lane_state, lds_state, voices,
                       seeds, n);
  return hipGetLastError();
}

hipError_t launch_pool_rows(const afs_frame *frames, int64_t frame_stride, const int32_t *count,
                            const int32_t *latched, int B, afs_frame *rows, afs_frame *pair, hipStream_t st) {
  if (B <= 0 || frame_stride <= 0) return hipSuccess;
  if ((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(pair)) & 15)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)B, (unsigned)((frame_stride + 1 + ROWS_WAVES - 1) / ROWS_WAVES)), block(64 * ROWS_WAVES);
  hipLaunchKernelGGL(pool_rows_kernel, grid, block, 0, st, (const uint4 *)frames, frame_stride, count, latched, B,
                     (uint4 *)rows, (uint4 *)pair);
  return hipGetLastError();
}

hipError_t preload_session_kernels() {
  hipError_t e = hipSuccess;
  hipFuncAttributes at;
  for (const void *k : {reinterpret_cast<const void *>(voice_reset_kernel<TREE_W>),
                        reinterpret_cast<const void *>(voice_reset_kernel<64>),
                        reinterpret_cast<const void *>(pool_rows_kernel)}) {
    const hipError_t x = hipFuncGetAttributes(&at, k);
    if (e == hipSuccess) e = x;
  }
  return e;
}

}  // namespace afs
