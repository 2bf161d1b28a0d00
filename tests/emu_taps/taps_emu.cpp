// taps_emu.cpp -- TEST-ONLY host execution of the signal taps' device code (csrc/tree_core.h
// tap_publish, the TAPS form of sample_step_pair, and the read of TapSet::x after the sample's last
// barrier), over the executors of tests/emu (cpu_exec.h): the one-wave step with the lanes run one
// after another, or the wave-pair step with its two roles on two threads that meet at the step's
// barriers.  tests/test_taps_emu.py compares the traces with the oracle's state after every sample.
// Never part of the product.
#include <thread>
#include <vector>

#include "tree_core.h"

using namespace afs;
using namespace afs::tree;

#include "cpu_exec.h"

namespace {

// the library's TapSet of a tap list (afs_capi.cpp tap_set)
TapSet tap_set(const Tables &T, const int *kind, const int *index, int n) {
  TapSet t;
  t.n = n;
  for (int k = 0; k < n; ++k) {
    const bool cur = kind[k] == AFS_TAP_CURRENT;
    t.sec[k] = cur ? -1 : index[k];
    t.x[k] = cur ? T.tap_u[index[k]] : T.tap_p + k;
  }
  return t;
}

// the output stage K6 runs after a launch (tree_output_kernel), per hop
void output_stage(double *X, const Tables &T, const afs_options &opt, const double *p25, double *out, long total, int hop) {
  for (long t0 = 0; t0 < total; t0 += hop) {
    if (opt.radiation_from_skin) tone_output_run(X, T.consts, p25 + t0, out + t0, hop);
    else output_filter_run(X, T.consts, out + t0, hop);
  }
}

template <int W>
long run_one(const afs_frame *frames, int F, int hop, unsigned seed, double fs, const int *kind, const int *index, int n,
             double *out, double *taps) {
  const afs_options opt = afs::default_options();
  std::vector<Tables> tab(1);
  Tables &T = tab[0];
  build_tables(&T, fs, opt);
  if (T.n_rounds < 0) return -1;
  const TapSet tp = tap_set(T, kind, index, n);
  std::vector<Lane<W>> R(W);
  std::vector<double> X(X_STRIDE);  // (the taps' slots lie behind the saved image, in the stride's padding)
  for (int gl = 0; gl < W; ++gl) reset_lane<W>(gl, R[gl]);
  reset_lds(X.data(), seed);
  CpuExec<W, true> ex{R.data()};
  const long total = (long)(F - 1) * hop;
  std::vector<double> p25(total);
  long t = 0;
  for (int k = 1; k < F; ++k) {
    for (int gl = 0; gl < W; ++gl) frame_load<W>(gl, R[gl], X.data(), frames + k - 1, frames + k);
    for (int i = 0; i < hop; ++i, ++t) {
      const double ratio = (double)i / (double)hop;
      uint64_t w[PLAN_WORDS];
      plan_sample(frames + k - 1, frames + k, ratio, T.consts.sec, false, w);
      for (int gl = 0; gl < W; ++gl) R[gl].planw = w[gl % PLAN_WORDS];
      sample_step<W, AFS_GLOTTIS_TRIANGULAR, NZ_FULL>(ex, X.data(), T.uni, T.consts, ratio, true);
      out[t] = R[0].sample;
      p25[t] = R[2 % W].p[0];
      // tree_kernel.h tree_synth_run, TAPS: publish, fence, collect
      for (int gl = 0; gl < W; ++gl) tap_publish<W>(gl, R[gl], X.data(), tp);
      for (int q = 0; q < n; ++q) taps[q * total + t] = X[tp.x[q]];
    }
  }
  output_stage(X.data(), T, opt, p25.data(), out, total, hop);
  return total;
}

template <int W>
long run_pair(const afs_frame *frames, int F, int hop, unsigned seed, double fs, const int *kind, const int *index,
              int n, double *out, double *taps) {
  const afs_options opt = afs::default_options();
  std::vector<Tables> tab(1);
  Tables &T = tab[0];
  build_tables(&T, fs, opt);
  if (T.n_rounds < 0) return -1;
  const TapSet tp = tap_set(T, kind, index, n);
  std::vector<Lane<W>> RD(W), RS(W);
  for (int gl = 0; gl < W; ++gl) {
    reset_lane<W>(gl, RD[gl]);
    reset_lane<W>(gl, RS[gl]);
  }
  std::vector<double> X(X_STRIDE);
  reset_lds(X.data(), seed);
  {
    int32_t *hp = (int32_t *)(X.data() + X_RNGHP);
    hp[0] = RS[0].rhead;
    hp[1] = RS[0].rpend;
  }
  Barrier2 bar;
  CpuExec<W, true> exD{RD.data(), &bar}, exS{RS.data(), &bar};
  const long total = (long)(F - 1) * hop;
  std::vector<double> p25(total);
  auto dyn = [&] {
    long t = 0;
    for (int k = 1; k < F; ++k) {
      for (int gl = 0; gl < W; ++gl) frame_load<W>(gl, RD[gl], X.data(), frames + k - 1, frames + k);
      exD.bar();
      for (int i = 0; i < hop; ++i, ++t) {
        const double ratio = (double)i / (double)hop;
        sample_step_pair<W, AFS_GLOTTIS_TRIANGULAR, NZ_FULL, ROLE_DYN, true>(exD, X.data(), T.uni, T.consts, ratio,
                                                                             (int)(t & 1), &tp);
        // (tree_pair_run: the DYN wave collects after P4's barrier, before it meets STAT again)
        for (int q = 0; q < n; ++q) taps[q * total + t] = X[tp.x[q]];
        out[t] = RD[0].sample;
        p25[t] = RD[2 % W].p[0];
      }
    }
  };
  auto stat = [&] {
    long t = 0;
    for (int k = 1; k < F; ++k) {
      exS.bar();
      for (int i = 0; i < hop; ++i, ++t) {
        const double ratio = (double)i / (double)hop;
        uint64_t w[PLAN_WORDS];
        plan_sample(frames + k - 1, frames + k, ratio, T.consts.sec, false, w);
        for (int gl = 0; gl < W; ++gl) RS[gl].planw = w[gl % PLAN_WORDS];
        sample_step_pair<W, AFS_GLOTTIS_TRIANGULAR, NZ_FULL, ROLE_STAT, true>(exS, X.data(), T.uni, T.consts, ratio,
                                                                              (int)(t & 1), &tp);
      }
    }
  };
  std::thread th(stat);
  dyn();
  th.join();
  output_stage(X.data(), T, opt, p25.data(), out, total, hop);
  return total;
}

}  // namespace

// One utterance of frames[F] at `hop` samples per transition, W = 16 or 64 lanes, as the one-wave
// kernel (pair = 0) or the wave pairs (pair = 1), default options: the audio out[(F-1) hop] and tap
// q's trace taps[q][(F-1) hop] (kind: afs_tap_kind, index: the reference's numbering).
extern "C" long emu_taps_utterance(const afs_frame *frames, int F, int hop, unsigned seed, double fs, int W, int pair,
                                   const int *kind, const int *index, int n, double *out, double *taps) {
  if (n < 0 || n > AFS_MAX_TAPS) return -3;
  if (W == 16) return pair ? run_pair<16>(frames, F, hop, seed, fs, kind, index, n, out, taps)
                           : run_one<16>(frames, F, hop, seed, fs, kind, index, n, out, taps);
  if (W == 64) return pair ? run_pair<64>(frames, F, hop, seed, fs, kind, index, n, out, taps)
                           : run_one<64>(frames, F, hop, seed, fs, kind, index, n, out, taps);
  return -2;
}
