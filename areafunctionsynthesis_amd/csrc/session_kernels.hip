// session_kernels.hip -- the per-voice lifecycle of a session's voice pool (afs_session_kernels.h):
// the reset of listed voices, the frame rows of a pool call, and the gather and scatter of voice
// records (afs_voice_state.h).  A translation unit of its own: the synthesis kernels' code object
// (tds_tree.hip) stays what it was, register counts included.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "afs_session_kernels.h"
#include "afs_tree.h"
#include "afs_voice_state.h"
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

// Where voice u's frames begin in the caller's array, in frames, and the frames a row holds besides the
// latch: the rectangle of afs_session_synthesize_ragged (u * frame_stride) or the start indices of
// afs_session_synthesize_indexed (start[u], a device array; the rows hold row_frames, the largest count).
struct RectFrames {
  int64_t frame_stride;
  __device__ int64_t base(int u) const { return (int64_t)u * frame_stride; }
  __device__ int64_t row_frames() const { return frame_stride; }
};
struct IndexedFrames {
  const int64_t *start;
  int64_t longest;
  __device__ int64_t base(int u) const { return start[u]; }
  __device__ int64_t row_frames() const { return longest; }
};

// Wave (u, j) builds frame j of voice u's row; lane l moves vectors l and l + 64.  Wave (u, 0) alone
// touches pair[u][0]: it loads the old latch (a latched voice's row frame 0) and the new one, the last
// frame supplied, and only then stores either.
template <class Source>
__device__ __forceinline__ void pool_rows_body(const uint4 *frames, const Source &at, const int32_t *count,
                                               const int32_t *latched, int B, uint4 *rows, uint4 *pair) {
  const int u = blockIdx.x;
  const int lane = (int)threadIdx.x & 63;
  const int j = (int)blockIdx.y * ROWS_WAVES + (int)threadIdx.x / 64;
  if (u >= B) return;
  const int c = count[u];
  if (c <= 0) return;  // (idle: nothing of this voice is read or written, its start index included)
  const int lat = latched[u] != 0 ? 1 : 0;
  if (j >= c + lat) return;  // (wave-uniform; c + lat <= row_frames + 1)
  const uint4 *src_u = frames + at.base(u) * FRAME_VECS;
  uint4 *latch = pair + (int64_t)u * 2 * FRAME_VECS;
  const uint4 *src = (j == 0 && lat) ? latch : src_u + (int64_t)(j - lat) * FRAME_VECS;
  uint4 *dst = rows + ((int64_t)u * (at.row_frames() + 1) + j) * FRAME_VECS;
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

__global__ void __launch_bounds__(64 * ROWS_WAVES) pool_rows_kernel(const uint4 *frames, int64_t frame_stride,
                                                                     const int32_t *count, const int32_t *latched, int B,
                                                                     uint4 *rows, uint4 *pair) {
  pool_rows_body(frames, RectFrames{frame_stride}, count, latched, B, rows, pair);
}

// the same rows from a flat array: voice u's frames are frames[start[u] .. start[u] + count[u])
__global__ void __launch_bounds__(64 * ROWS_WAVES) pool_rows_indexed_kernel(const uint4 *frames, const int64_t *start,
                                                                             int64_t longest, const int32_t *count,
                                                                             const int32_t *latched, int B, uint4 *rows,
                                                                             uint4 *pair) {
  pool_rows_body(frames, IndexedFrames{start, longest}, count, latched, B, rows, pair);
}

// ---- voice records: session buffers <-> packed records (afs_voice_state.h) ----

static_assert((sizeof(Lane<TREE_W>) * TREE_W) % 16 == 0 && (sizeof(Lane<64>) * 64) % 16 == 0 &&
                  (X_TOTAL * sizeof(double)) % 16 == 0 && sizeof(afs_frame) % 16 == 0,
              "every part of a voice record is whole 16-byte vectors");
constexpr int STATE_WAVES = 4;  // waves per block: 256 consecutive vectors (4 KiB) of one record

// Block (i, k) moves payload vectors 256 k .. 256 k + 255 of record i, the voice voices[i]: a thread one
// 16-byte vector, consecutive lanes consecutive vectors, a record (1607 vectors at 16 lanes, 2791 at 64)
// spread over 7 or 11 blocks.  The three parts sit in three buffers of the session; a wave that spans
// the border of two parts touches both.  False: the thread has no vector (past the record's end).
__device__ inline bool voice_state_thread(const VoiceStateBuffers &s, const int32_t *voices, int n,
                                          const VoiceStateLayout &L, char *records, uint4 **in_session,
                                          uint4 **in_record) {
  const int i = blockIdx.x;
  const int64_t v = (int64_t)blockIdx.y * (64 * STATE_WAVES) + threadIdx.x;
  if (i >= n || v >= voice_state_payload_vecs(L)) return false;
  const VoiceStateVec at = voice_state_vec(L, v, voices[i]);
  if (at.part < 0) return false;
  char *base = at.part == 0 ? s.lanes : at.part == 1 ? s.lds : s.pair;
  *in_session = reinterpret_cast<uint4 *>(base + at.session_off);
  *in_record = reinterpret_cast<uint4 *>(records + (int64_t)i * L.record_bytes + at.record_off);
  return true;
}

// session -> records: reads the session's buffers only (a voice may be listed more than once)
__global__ void __launch_bounds__(64 * STATE_WAVES) voice_gather_kernel(VoiceStateBuffers s, const int32_t *voices,
                                                                       int n, VoiceStateLayout L, char *records) {
  uint4 *in_session, *in_record;
  if (voice_state_thread(s, voices, n, L, records, &in_session, &in_record)) *in_record = *in_session;
}

// records -> session: writes the listed voices' parts and nothing else (the voices are distinct)
__global__ void __launch_bounds__(64 * STATE_WAVES) voice_scatter_kernel(VoiceStateBuffers s, const int32_t *voices,
                                                                        int n, VoiceStateLayout L, char *records) {
  uint4 *in_session, *in_record;
  if (voice_state_thread(s, voices, n, L, records, &in_session, &in_record)) *in_session = *in_record;
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

hipError_t launch_pool_rows_indexed(const afs_frame *frames, const int64_t *start, int64_t longest, const int32_t *count,
                                    const int32_t *latched, int B, afs_frame *rows, afs_frame *pair, hipStream_t st) {
  if (B <= 0 || longest <= 0) return hipSuccess;
  if ((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(pair)) & 15)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)B, (unsigned)((longest + 1 + ROWS_WAVES - 1) / ROWS_WAVES)), block(64 * ROWS_WAVES);
  hipLaunchKernelGGL(pool_rows_indexed_kernel, grid, block, 0, st, (const uint4 *)frames, start, longest, count, latched,
                     B, (uint4 *)rows, (uint4 *)pair);
  return hipGetLastError();
}

VoiceStateLayout voice_state_layout_for(int lanes) {
  return voice_state_layout(lanes, lanes == 64 ? (int64_t)sizeof(Lane<64>) : (int64_t)sizeof(Lane<TREE_W>), X_TOTAL,
                            (int64_t)sizeof(afs_frame));
}

static hipError_t launch_voice_state(bool gather, const VoiceStateBuffers &s, const int32_t *voices, int n, int lanes,
                                     void *records, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if ((reinterpret_cast<uintptr_t>(s.lanes) | reinterpret_cast<uintptr_t>(s.lds) | reinterpret_cast<uintptr_t>(s.pair) |
       reinterpret_cast<uintptr_t>(records)) & 15)
    return hipErrorInvalidValue;
  const VoiceStateLayout L = voice_state_layout_for(lanes);
  const int64_t vecs = voice_state_payload_vecs(L);
  const dim3 grid((unsigned)n, (unsigned)((vecs + 64 * STATE_WAVES - 1) / (64 * STATE_WAVES))), block(64 * STATE_WAVES);
  if (gather)
    hipLaunchKernelGGL(voice_gather_kernel, grid, block, 0, st, s, voices, n, L, (char *)records);
  else
    hipLaunchKernelGGL(voice_scatter_kernel, grid, block, 0, st, s, voices, n, L, (char *)records);
  return hipGetLastError();
}

hipError_t launch_voice_gather(const VoiceStateBuffers &s, const int32_t *voices, int n, int lanes, void *records,
                               hipStream_t st) {
  return launch_voice_state(true, s, voices, n, lanes, records, st);
}

hipError_t launch_voice_scatter(const VoiceStateBuffers &s, const int32_t *voices, int n, int lanes, const void *records,
                                hipStream_t st) {
  return launch_voice_state(false, s, voices, n, lanes, const_cast<void *>(records), st);
}

hipError_t preload_session_kernels() {
  hipError_t e = hipSuccess;
  hipFuncAttributes at;
  for (const void *k : {reinterpret_cast<const void *>(voice_reset_kernel<TREE_W>),
                        reinterpret_cast<const void *>(voice_reset_kernel<64>),
                        reinterpret_cast<const void *>(pool_rows_kernel),
                        reinterpret_cast<const void *>(pool_rows_indexed_kernel),
                        reinterpret_cast<const void *>(voice_gather_kernel),
                        reinterpret_cast<const void *>(voice_scatter_kernel)}) {
    const hipError_t x = hipFuncGetAttributes(&at, k);
    if (e == hipSuccess) e = x;
  }
  return e;
}

}  // namespace afs
