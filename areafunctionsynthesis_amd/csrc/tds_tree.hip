// tds_tree.hip -- the cooperative synthesis kernel (afs_solver AFS_SOLVER_TREE) and the
// small state kernels; the body and the wave mapping are described in tree_kernel.h.  (Its
// noise-source plan kernel K5 is in tds_plan.hip.)
#include "tree_kernel.h"

namespace afs {

using namespace tree;

namespace {

// one kernel per glottis model (TriangularGlottis, the reference's; TwoMassModel), plan mode
// (HOPS: hop records, hops >= PLAN_HOP_MIN; dense records otherwise) and lanes per utterance W
// (16: the throughput kernel; 64: the voice kernel, tree_kernel.h); TAPS: the form a launch with
// signal taps runs (TreeArgs::taps) -- the tap-less kernels hold none of its code
template <int MODEL, bool HOPS, int W, bool TAPS = false>
__global__ void __launch_bounds__(64 * Geom<W>::WPB, AFS_TREE_MIN_WAVES) tree_synth_kernel(TreeArgs a) {
  __shared__ WaveLdsT<W> lds;
  tree_synth_body<false, MODEL, HOPS, W, TAPS>(a, lds, nullptr);
}

// ... and the forms a ragged call launches (TreeArgs::block_end, pad_standin; afs_synthesize_ragged):
// kernels of their own, as TAPS has, so that the uniform calls' kernels stay what they were
template <int MODEL, bool HOPS, int W, bool TAPS = false>
__global__ void __launch_bounds__(64 * Geom<W>::WPB, AFS_TREE_MIN_WAVES) tree_synth_ragged_kernel(TreeArgs a) {
  __shared__ WaveLdsT<W> lds;
  tree_synth_body<false, MODEL, HOPS, W, TAPS, true>(a, lds, nullptr);
}

#if AFS_PAIR
// the wave-pair build of the throughput kernel (tree_kernel.h tree_pair_body): four waves per
// workgroup, two per SIMD
template <int MODEL, bool HOPS, bool TAPS = false>
__global__ void __launch_bounds__(256, 2) tree_pair_kernel(TreeArgs a) {
  __shared__ PairLdsT<TW> lds;
  __shared__ int pattern[5];
  tree_pair_body<MODEL, HOPS, false, TAPS>(a, lds, pattern);
}
// the voice kernel's pairs: two waves per utterance, each may take a whole SIMD's registers
template <int MODEL, bool HOPS, bool TAPS = false>
__global__ void __launch_bounds__(128, 2) tree_pair64_kernel(TreeArgs a) {
  __shared__ PairLdsT<64> lds;
  tree_pair64_body<MODEL, HOPS, false, TAPS>(a, lds);
}
template <int MODEL, bool HOPS, bool TAPS = false>
__global__ void __launch_bounds__(256, 2) tree_pair_ragged_kernel(TreeArgs a) {
  __shared__ PairLdsT<TW> lds;
  __shared__ int pattern[5];
  tree_pair_body<MODEL, HOPS, false, TAPS, true>(a, lds, pattern);
}
template <int MODEL, bool HOPS, bool TAPS = false>
__global__ void __launch_bounds__(128, 2) tree_pair64_ragged_kernel(TreeArgs a) {
  __shared__ PairLdsT<64> lds;
  tree_pair64_body<MODEL, HOPS, false, TAPS, true>(a, lds);
}
#endif

// K6: the output stage of a launch's samples -- dU/dt, the 8-pole Chebyshev low-pass, x 0.004 /
// 32767 (Synthesizer.cpp:614-627) -- over the radiated flows the synthesis kernel stored, in
// place, one thread per utterance; the filter state (X_OUTF, X_PREVFLOW, X_NONFIN, X_TONE) lives in
// the utterance's saved LDS image, which the synthesis kernel carries through unchanged.  With skin
// radiation (TdsModel::Options.radiationFromSkin): first the glottal-tone filter over section 25's
// stored pressures, added to the flows, in the output filter's loop (tone_output_run).
__global__ void __launch_bounds__(64) tree_output_kernel(const Tables *tab, double *lds_state, double *out,
                                                         int64_t out_stride, int64_t n, int B, const double *p25,
                                                         int64_t p25_stride, int skin,
                                                         const uint32_t *skip_claims, int64_t skip_cap) {
  const int u = blockIdx.x * 64 + threadIdx.x;
  if (u >= B) return;
  if (skip_claims && (int64_t)*skip_claims > skip_cap) return;  // (as the guarded K1 launch: TreeArgs)
  double *X = lds_state + (int64_t)u * X_TOTAL;
  double *o = out + (int64_t)u * out_stride;
  if (p25 && skin) tone_output_run(X, tab->consts, p25 + (int64_t)u * p25_stride, o, (int)n);
  else output_filter_run(X, tab->consts, o, (int)n);
}
// K6 of a ragged call: utterance u ends at sample row_hops[u] * hop of the call, so of this launch's n
// samples from s_begin it filters those K1 stored for it (TreeArgs::block_end) -- none once it has ended
__global__ void __launch_bounds__(64) tree_output_ragged_kernel(const Tables *tab, double *lds_state, double *out,
                                                                int64_t out_stride, int64_t n, int B, const double *p25,
                                                                int64_t p25_stride, int skin,
                                                                const uint32_t *skip_claims, int64_t skip_cap,
                                                                const int32_t *row_hops, int hop, int64_t s_begin) {
  const int u = blockIdx.x * 64 + threadIdx.x;
  if (u >= B) return;
  if (skip_claims && (int64_t)*skip_claims > skip_cap) return;
  const int64_t left = (int64_t)row_hops[u] * hop - s_begin;
  n = left < n ? left : n;
  if (n <= 0) return;
  double *X = lds_state + (int64_t)u * X_TOTAL;
  double *o = out + (int64_t)u * out_stride;
  // (tone_output_run / output_filter_run in instantiations of this kernel's own: tree_core.h FORM)
  if (p25 && skin) output_filter_run_t<true, 1>(X, tab->consts, o, (int)n, p25 + (int64_t)u * p25_stride);
  else output_filter_run_t<false, 1>(X, tab->consts, o, (int)n, nullptr);
}

// K6 of the _pcm calls: the same filters over the launch's flow window (flow[u * win_stride + i], read
// only; p25 likewise), the audio converted to int16 (sample_to_int16) on its way out to
// pcm[u * pcm_stride + i], i < n -- the fp64 audio is never stored.  Rows of pcm may sit at any 2-byte
// alignment (tree_core.h PcmPack).  Instantiations of the filter of their own (FORM 2, 3).
__global__ void __launch_bounds__(64) tree_output_pcm_kernel(const Tables *tab, double *lds_state, const double *flow,
                                                             int64_t win_stride, int64_t n, int B, const double *p25,
                                                             int skin, const uint32_t *skip_claims, int64_t skip_cap,
                                                             int16_t *pcm, int64_t pcm_stride) {
  const int u = blockIdx.x * 64 + threadIdx.x;
  if (u >= B) return;
  if (skip_claims && (int64_t)*skip_claims > skip_cap) return;
  double *X = lds_state + (int64_t)u * X_TOTAL;
  const double *f = flow + (int64_t)u * win_stride;
  int16_t *o = pcm + (int64_t)u * pcm_stride;
  if (p25 && skin) output_filter_run_pcm<true, 2>(X, tab->consts, f, (int)n, p25 + (int64_t)u * win_stride, o);
  else output_filter_run_pcm<false, 2>(X, tab->consts, f, (int)n, nullptr, o);
}
// ... of a ragged _pcm call (as tree_output_ragged_kernel)
__global__ void __launch_bounds__(64) tree_output_pcm_ragged_kernel(const Tables *tab, double *lds_state,
                                                                    const double *flow, int64_t win_stride, int64_t n,
                                                                    int B, const double *p25, int skin,
                                                                    const uint32_t *skip_claims, int64_t skip_cap,
                                                                    int16_t *pcm, int64_t pcm_stride,
                                                                    const int32_t *row_hops, int hop, int64_t s_begin) {
  const int u = blockIdx.x * 64 + threadIdx.x;
  if (u >= B) return;
  if (skip_claims && (int64_t)*skip_claims > skip_cap) return;
  const int64_t left = (int64_t)row_hops[u] * hop - s_begin;
  n = left < n ? left : n;
  if (n <= 0) return;
  double *X = lds_state + (int64_t)u * X_TOTAL;
  const double *f = flow + (int64_t)u * win_stride;
  int16_t *o = pcm + (int64_t)u * pcm_stride;
  if (p25 && skin) output_filter_run_pcm<true, 3>(X, tab->consts, f, (int)n, p25 + (int64_t)u * win_stride, o);
  else output_filter_run_pcm<false, 3>(X, tab->consts, f, (int)n, nullptr, o);
}

// K6 of the _f32 call: tree_output_pcm_kernel with the float32 sink (sample_to_f32, tree_core.h F32Pack):
// f32[u * f32_stride + i], i < n, rows at any 4-byte alignment.  FORM 4.
__global__ void __launch_bounds__(64) tree_output_f32_kernel(const Tables *tab, double *lds_state, const double *flow,
                                                             int64_t win_stride, int64_t n, int B, const double *p25,
                                                             int skin, const uint32_t *skip_claims, int64_t skip_cap,
                                                             float *f32, int64_t f32_stride) {
  const int u = blockIdx.x * 64 + threadIdx.x;
  if (u >= B) return;
  if (skip_claims && (int64_t)*skip_claims > skip_cap) return;
  double *X = lds_state + (int64_t)u * X_TOTAL;
  const double *f = flow + (int64_t)u * win_stride;
  float *o = f32 + (int64_t)u * f32_stride;
  if (p25 && skin) output_filter_run_f32<true, 4>(X, tab->consts, f, (int)n, p25 + (int64_t)u * win_stride, o);
  else output_filter_run_f32<false, 4>(X, tab->consts, f, (int)n, nullptr, o);
}
// K6 of the packed ragged calls: as tree_output_pcm_ragged_kernel, but utterance u's row of the call starts
// at sample row_base[u] of the caller's buffer (any order, any alignment of the sample type) instead of
// u * pcm_stride, so this launch's samples go to row_base[u] + s_begin + i, i < n.  FORM 5 (int16), 6 (float32).
__global__ void __launch_bounds__(64) tree_output_pcm_packed_kernel(const Tables *tab, double *lds_state,
                                                                    const double *flow, int64_t win_stride, int64_t n,
                                                                    int B, const double *p25, int skin,
                                                                    const uint32_t *skip_claims, int64_t skip_cap,
                                                                    int16_t *pcm, const int64_t *row_base,
                                                                    const int32_t *row_hops, int hop, int64_t s_begin) {
  const int u = blockIdx.x * 64 + threadIdx.x;
  if (u >= B) return;
  if (skip_claims && (int64_t)*skip_claims > skip_cap) return;
  const int64_t left = (int64_t)row_hops[u] * hop - s_begin;
  n = left < n ? left : n;
  if (n <= 0) return;
  double *X = lds_state + (int64_t)u * X_TOTAL;
  const double *f = flow + (int64_t)u * win_stride;
  int16_t *o = pcm + row_base[u] + s_begin;
  if (p25 && skin) output_filter_run_pcm<true, 5>(X, tab->consts, f, (int)n, p25 + (int64_t)u * win_stride, o);
  else output_filter_run_pcm<false, 5>(X, tab->consts, f, (int)n, nullptr, o);
}
// (a strided ragged float32 row is this kernel's with row_base[u] = u * stride)
__global__ void __launch_bounds__(64) tree_output_f32_packed_kernel(const Tables *tab, double *lds_state,
                                                                    const double *flow, int64_t win_stride, int64_t n,
                                                                    int B, const double *p25, int skin,
                                                                    const uint32_t *skip_claims, int64_t skip_cap,
                                                                    float *f32, const int64_t *row_base,
                                                                    const int32_t *row_hops, int hop, int64_t s_begin) {
  const int u = blockIdx.x * 64 + threadIdx.x;
  if (u >= B) return;
  if (skip_claims && (int64_t)*skip_claims > skip_cap) return;
  const int64_t left = (int64_t)row_hops[u] * hop - s_begin;
  n = left < n ? left : n;
  if (n <= 0) return;
  double *X = lds_state + (int64_t)u * X_TOTAL;
  const double *f = flow + (int64_t)u * win_stride;
  float *o = f32 + row_base[u] + s_begin;
  if (p25 && skin) output_filter_run_f32<true, 6>(X, tab->consts, f, (int)n, p25 + (int64_t)u * win_stride, o);
  else output_filter_run_f32<false, 6>(X, tab->consts, f, (int)n, nullptr, o);
}

// seeds == nullptr: utterance u is seeded u + 1 (afs.h)
template <int W>
__global__ void tree_reset_kernel(Lane<W> *lanes, double *lds, int B, const uint32_t *seeds) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)B * W) return;
  const int u = (int)(id / W), gl = (int)(id % W);
  Lane<W> R;
  reset_lane<W>(gl, R);
  lanes[id] = R;
  if (gl == 0) reset_lds(lds + (int64_t)u * X_TOTAL, seeds ? seeds[u] : (uint32_t)u + 1u);
}

__global__ void tree_nonfinite_kernel(const double *lds, int B, int32_t *count, uint8_t *flags) {
  int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= B) return;
  const bool nf = lds[(int64_t)u * X_TOTAL + X_NONFIN] != 0.0;
  if (flags) flags[u] = nf ? 1 : 0;
  if (nf) atomicAdd(count, 1);
}

__global__ void tree_draws_kernel(const double *lds, int B, int64_t *draws) {
  int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= B) return;
  draws[u] = (int64_t)*(const uint64_t *)(lds + (int64_t)u * X_TOTAL + X_NDRAW);
}

// Diagnostics (afs_tube_interpolate): the synthesis kernel's own frame_load + phase_interpolate,
// compiled in this file with its flags, for n (frame pair, ratio) samples; thread (i, gl) writes
// the pharynx/mouth sections of lane gl's slots.  X: a private stand-in of the LDS block's frame
// values (only X_FRAME .. X_FRAME + 3 are read).
__global__ void tree_interp_kernel(const Tables *tab, const afs_frame *fl, const afs_frame *fr, const double *ratio,
                                   int n, double *area, double *len) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)n * TW) return;
  const int i = (int)(id / TW), gl = (int)(id % TW);
  Lane<TW> R = Lane<TW>{};
  double X[X_FRAME + 16];
  for (int k = 0; k < X_FRAME + 16; ++k) X[k] = 0.0;
  frame_load<TW>(0, R, X, fl + i, fr + i);  // (lane 0's frame values for every thread)
  frame_load<TW>(gl, R, X, fl + i, fr + i);
  phase_interpolate<TW>(gl, R, X, tab->consts, ratio[i]);
#pragma unroll
  for (int j = 0; j < Shape<TW>::ND; ++j) {
    const int m = dyn_section(TW, j, gl) - S_PHARYNX0;
    if (m >= 0 && m < NPM) {
      area[(int64_t)i * NPM + m] = R.acur[j];
      len[(int64_t)i * NPM + m] = R.lcur[j];
    }
  }
}

// Diagnostics (afs_plan_hop_words): the synthesis kernel's per-sample plan words, plan_word_fast
// compiled here with its flags, for n (hop record, ratio) pairs: thread (i, w) writes word w.
__global__ void tree_hop_words_kernel(const tree::PlanHop *h, const double *ratio, int n, uint64_t *out) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)n * PLAN_WORDS) return;
  const int i = (int)(id / PLAN_WORDS), w = (int)(id % PLAN_WORDS);
  out[id] = plan_word_fast(h[i].kind[w], h[i].p[w], ratio[i]);
}

}  // namespace

hipError_t launch_tree_hop_words(const tree::PlanHop *h, const double *ratio, int n, uint64_t *out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int64_t t = (int64_t)n * PLAN_WORDS;
  hipLaunchKernelGGL(tree_hop_words_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, st, h, ratio, n, out);
  return hipGetLastError();
}

hipError_t launch_tree_interp(const Tables *tab, const afs_frame *fl, const afs_frame *fr, const double *ratio, int n,
                              double *area, double *len, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int64_t t = (int64_t)n * TW;
  hipLaunchKernelGGL(tree_interp_kernel, dim3((unsigned)((t + 127) / 128)), dim3(128), 0, st, tab, fl, fr, ratio, n,
                     area, len);
  return hipGetLastError();
}

hipError_t launch_tree_output(const Tables *tab, double *lds_state, double *out, int64_t out_stride, int64_t n, int B,
                              const double *p25, int64_t p25_stride, int skin, hipStream_t st,
                              const uint32_t *skip_claims, int64_t skip_cap, const int32_t *row_hops, int hop,
                              int64_t s_begin) {
  if (B <= 0 || n <= 0) return hipSuccess;
  if (row_hops)
    hipLaunchKernelGGL(tree_output_ragged_kernel, dim3((B + 63) / 64), dim3(64), 0, st, tab, lds_state, out, out_stride,
                       n, B, p25, p25_stride, skin, skip_claims, skip_cap, row_hops, hop, s_begin);
  else
    hipLaunchKernelGGL(tree_output_kernel, dim3((B + 63) / 64), dim3(64), 0, st, tab, lds_state, out, out_stride, n, B,
                       p25, p25_stride, skin, skip_claims, skip_cap);
  return hipGetLastError();
}

hipError_t launch_tree_output_samples(const Tables *tab, double *lds_state, const double *flow, int64_t win_stride,
                                      int64_t n, int B, const double *p25, int skin, int format, void *samples,
                                      int64_t stride, const int64_t *row_base, hipStream_t st,
                                      const uint32_t *skip_claims, int64_t skip_cap, const int32_t *row_hops, int hop,
                                      int64_t s_begin) {
  if (B <= 0 || n <= 0) return hipSuccess;
  const bool f32 = format == AFS_SAMPLE_F32;
  // (row_base belongs to a ragged launch; a ragged float32 launch has no strided kernel and needs one)
  if ((!f32 && format != AFS_SAMPLE_I16) || (row_base && !row_hops) || (f32 && row_hops && !row_base))
    return hipErrorInvalidValue;
  const dim3 grid((B + 63) / 64), block(64);
  int16_t *pcm = (int16_t *)samples;
  float *flt = (float *)samples;
  if (row_base && f32)
    hipLaunchKernelGGL(tree_output_f32_packed_kernel, grid, block, 0, st, tab, lds_state, flow, win_stride, n, B, p25,
                       skin, skip_claims, skip_cap, flt, row_base, row_hops, hop, s_begin);
  else if (row_base)
    hipLaunchKernelGGL(tree_output_pcm_packed_kernel, grid, block, 0, st, tab, lds_state, flow, win_stride, n, B, p25,
                       skin, skip_claims, skip_cap, pcm, row_base, row_hops, hop, s_begin);
  else if (f32)
    hipLaunchKernelGGL(tree_output_f32_kernel, grid, block, 0, st, tab, lds_state, flow, win_stride, n, B, p25, skin,
                       skip_claims, skip_cap, flt + s_begin, stride);
  else if (row_hops)
    hipLaunchKernelGGL(tree_output_pcm_ragged_kernel, grid, block, 0, st, tab, lds_state, flow, win_stride, n, B, p25,
                       skin, skip_claims, skip_cap, pcm + s_begin, stride, row_hops, hop, s_begin);
  else
    hipLaunchKernelGGL(tree_output_pcm_kernel, grid, block, 0, st, tab, lds_state, flow, win_stride, n, B, p25, skin,
                       skip_claims, skip_cap, pcm + s_begin, stride);
  return hipGetLastError();
}

int64_t tree_lane_bytes(int lanes) { return lanes == 64 ? (int64_t)sizeof(Lane<64>) : (int64_t)sizeof(Lane<TW>); }
int64_t tree_lds_doubles() { return X_TOTAL; }

hipError_t launch_tree_reset(void *lane_state, double *lds_state, int B, const uint32_t *seeds, int lanes,
                             hipStream_t st) {
  if (B <= 0) return hipSuccess;
  const int64_t n = (int64_t)B * lanes;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (lanes == 64)
    hipLaunchKernelGGL(tree_reset_kernel<64>, grid, block, 0, st, (Lane<64> *)lane_state, lds_state, B, seeds);
  else
    hipLaunchKernelGGL(tree_reset_kernel<TW>, grid, block, 0, st, (Lane<TW> *)lane_state, lds_state, B, seeds);
  return hipGetLastError();
}

// Run-time switches as template arguments: f(std::bool_constant<B>{}...) for the bools' values.
// (The order of the bools is the order the kernels are instantiated in, true first, the first bool
// outermost, and so their order in the code object: the callers keep the order the kernels always
// had, which keeps every kernel's pc-relative addresses, tools/kernel_meta.py --text.)
template <class F>
static void with_bools(F f) { f(); }
template <class F, class... Bs>
static void with_bools(F f, bool b, Bs... rest) {
  if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// One launch per (glottis model, plan mode): kernel(model, hops) names the kernel.
template <class K>
static void launch_model_hops(const TreeArgs &a, dim3 grid, dim3 block, hipStream_t st, K kernel) {
  with_bools([&](auto hops, auto two) {
    constexpr int MODEL = decltype(two)::value ? AFS_GLOTTIS_TWO_MASS : AFS_GLOTTIS_TRIANGULAR;
    hipLaunchKernelGGL(kernel(std::integral_constant<int, MODEL>{}, hops), grid, block, 0, st, a);
  }, a.hops != nullptr, a.uni.opt.glottis_model == AFS_GLOTTIS_TWO_MASS);
}

// kernel(model, hops) of a kernel family in launch_synth_w's form: NAME_ragged_kernel for a ragged
// call, NAME_kernel otherwise, of (model, hops, the arguments that follow)
#define AFS_TREE_KERNEL(NAME, ...)                                                                         \
  [](auto m, auto h) {                                                                                     \
    if constexpr (RAGGED) return NAME##_ragged_kernel<decltype(m)::value, decltype(h)::value, __VA_ARGS__>; \
    else return NAME##_kernel<decltype(m)::value, decltype(h)::value, __VA_ARGS__>;                        \
  }

template <int W, bool TAPS, bool RAGGED>
static void launch_synth_w(const TreeArgs &a, hipStream_t st) {
  constexpr int UPB_ = Geom<W>::UPB;
  const dim3 grid(a.grid_blocks > 0 ? a.grid_blocks : (a.B + UPB_ - 1) / UPB_), block(64 * Geom<W>::WPB);
#if AFS_PAIR
  if constexpr (W == TW) {  // (the one-wave kernel at 16 lanes is not instantiated in this build)
    static_assert(Geom<TW>::WPB == 2, "a wave pair per four utterances: 4 waves per 8-utterance block");
    return launch_model_hops(a, grid, dim3(256), st, AFS_TREE_KERNEL(tree_pair, TAPS));
  } else if constexpr (W == 64) {
    if (a.B <= TREE_PAIR64_MAX) return launch_model_hops(a, grid, dim3(128), st, AFS_TREE_KERNEL(tree_pair64, TAPS));
  }
#endif
  // the one-wave kernel (every phase on one wave)
  if constexpr (!AFS_PAIR || W != TW) launch_model_hops(a, grid, block, st, AFS_TREE_KERNEL(tree_synth, W, TAPS));
}
#undef AFS_TREE_KERNEL

hipError_t launch_tree_synth(const TreeArgs &a, int lanes, hipStream_t st) {
  if (a.B <= 0 || a.s_end <= a.s_begin) return hipSuccess;
  // (a ragged launch carries both arrays and a slot order with a block count: afs_ragged_order.h)
  const bool ragged = a.block_end || a.pad_standin;
  if (ragged && !(a.block_end && a.pad_standin && a.order && a.grid_blocks > 0)) return hipErrorInvalidValue;
  if (a.taps.n > 0 && (a.taps.n > AFS_MAX_TAPS || !a.tap_out)) return hipErrorInvalidValue;
  with_bools([&](auto taps, auto w64, auto rg) {
    launch_synth_w<decltype(w64)::value ? 64 : TW, decltype(taps)::value, decltype(rg)::value>(a, st);
  }, a.taps.n > 0, lanes == 64, ragged);
  return hipGetLastError();
}

hipError_t launch_tree_nonfinite(const double *lds_state, int B, int32_t *count, uint8_t *flags, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(tree_nonfinite_kernel, dim3((B + 63) / 64), dim3(64), 0, st, lds_state, B, count, flags);
  return hipGetLastError();
}

hipError_t launch_tree_draws(const double *lds_state, int B, int64_t *draws, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(tree_draws_kernel, dim3((B + 63) / 64), dim3(64), 0, st, lds_state, B, draws);
  return hipGetLastError();
}

// Loads this file's code object on the context's device now (HIP loads a code object at the first
// launch of one of its kernels otherwise: tens of milliseconds inside a real-time caller's first
// buffer).
template <class K> static hipError_t preload_one(K k) {
  hipFuncAttributes at;
  return hipFuncGetAttributes(&at, reinterpret_cast<const void *>(k));
}
hipError_t preload_tree_kernels() {
  hipError_t e = hipSuccess;
  for (hipError_t x : {
#if AFS_PAIR
                       preload_one(tree_pair_kernel<AFS_GLOTTIS_TRIANGULAR, true>),
                       preload_one(tree_pair_kernel<AFS_GLOTTIS_TRIANGULAR, false>),
                       preload_one(tree_pair_kernel<AFS_GLOTTIS_TWO_MASS, true>),
                       preload_one(tree_pair_kernel<AFS_GLOTTIS_TWO_MASS, false>),
                       preload_one(tree_pair64_kernel<AFS_GLOTTIS_TRIANGULAR, true>),
                       preload_one(tree_pair64_kernel<AFS_GLOTTIS_TRIANGULAR, false>),
                       preload_one(tree_pair64_kernel<AFS_GLOTTIS_TWO_MASS, true>),
                       preload_one(tree_pair64_kernel<AFS_GLOTTIS_TWO_MASS, false>),
#else
                       preload_one(tree_synth_kernel<AFS_GLOTTIS_TRIANGULAR, true, TW>),
                       preload_one(tree_synth_kernel<AFS_GLOTTIS_TRIANGULAR, false, TW>),
                       preload_one(tree_synth_kernel<AFS_GLOTTIS_TWO_MASS, true, TW>),
                       preload_one(tree_synth_kernel<AFS_GLOTTIS_TWO_MASS, false, TW>),
#endif
                       preload_one(tree_synth_kernel<AFS_GLOTTIS_TRIANGULAR, true, 64>),
                       preload_one(tree_synth_kernel<AFS_GLOTTIS_TRIANGULAR, false, 64>),
                       preload_one(tree_synth_kernel<AFS_GLOTTIS_TWO_MASS, true, 64>),
                       preload_one(tree_synth_kernel<AFS_GLOTTIS_TWO_MASS, false, 64>),
                       preload_one(tree_output_kernel), preload_one(tree_reset_kernel<TW>),
                       preload_one(tree_reset_kernel<64>), preload_one(tree_nonfinite_kernel),
                       preload_one(tree_draws_kernel), preload_one(tree_output_f32_kernel),
                       preload_one(tree_output_pcm_packed_kernel), preload_one(tree_output_f32_packed_kernel)})
    if (e == hipSuccess) e = x;
  return e;
}

}  // namespace afs
