// afs_capi.cpp -- the C ABI of include/afs.h: contexts, sessions, staging, launches.
//
// Host-side orchestration only; all synthesis arithmetic runs in the HIP kernels.
// There is no CPU fallback: without a usable HIP device afs_create fails with
// AFS_ERR_NO_DEVICE.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "afs_af.h"
#include "afs_lane.h"
#include "afs_audio.h"
#include "afs_ctx.h"
#include "afs_device_math.h"
#include "afs_indexed.h"
#include "afs_model.h"
#include "afs_ragged_order.h"
#include "afs_session_kernels.h"
#include "afs_tree.h"
#include "afs_xcd_order.h"

static_assert(sizeof(afs_frame) == 1072, "afs_frame layout");

namespace afs {

afs_status fail(afs_ctx *c, afs_status s, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return s;
}

bool is_device_ptr(const void *p) {
  if (!p) return false;
  hipPointerAttribute_t at;
  hipError_t e = hipPointerGetAttributes(&at, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

// Lanes per utterance of the tree kernel for a batch of B: forced by AFS_LANES_16 / AFS_LANES_64,
// else the voice kernel (64 lanes, one utterance per wave: fewer instructions per sample on the
// chain) while the batch leaves SIMDs idle with 16 lanes per utterance (B <= the GPU's SIMDs), the
// throughput kernel (16 lanes, four utterances per wave) above.
int lanes_for(const afs_ctx *c, int64_t B) {
  if (c->cfg.flags & AFS_LANES_16) return TREE_W;
  if (c->cfg.flags & AFS_LANES_64) return TREE_VOICE_W;
  return B <= c->simds ? TREE_VOICE_W : TREE_W;
}

}  // namespace afs

using afs::fail;
using afs::is_device_ptr;
using afs::lanes_for;

namespace {

int64_t pad64(int64_t b) { return (b + 63) / 64 * 64; }

// bytes of one sample of an afs_sample_format
size_t sample_bytes(int format) { return format == AFS_SAMPLE_F32 ? sizeof(float) : sizeof(int16_t); }

bool solver_ok(int32_t s) { return s == AFS_SOLVER_CHOLESKY || s == AFS_SOLVER_TREE || s == AFS_SOLVER_SOR; }

// the cooperative kernel (noise-source plans from K5)
bool tree(const afs_ctx *c) { return c->cfg.solver == AFS_SOLVER_TREE; }


// Bytes of noise-source plans one call may hold (afs_ctx::plan_budget: 4 GiB, or
// AFS_PLAN_BUDGET_MB).  Hop mode keeps the hop records of the whole call and the dense records
// of its mixed hops within it (static vowels: 446 MB of records for 8192 utterances x 1 s) and
// runs launches of up to afs_ctx::launch_cap samples; the dense path (hops < 32, or past the
// budget) runs launches of at most plan_budget / (rows * 128 B) samples (4096 at 8192 rows).
// (Round 2 measured one launch per second with 46 GB of dense records no faster than 11
// launches; round 4's compact hop-mode plans make the one launch +0.1..0.5 %,
// profiles/r04h_launch_ab.txt.)
constexpr int64_t PLAN_BUDGET_DEFAULT = (int64_t)4 << 30;
// Hop mode: calls whose dense records fit this many bytes even with every hop listed skip the
// read-back of K5's claimed slots (run_hop_call).
constexpr int64_t SMALL_CALL_DENSE_BYTES = (int64_t)64 << 20;

// AFS_PROFILE: record an event on the context's stream (a pooled one; recording stops past
// the pool's cap until afs_kernel_times drains it).
hipEvent_t prof_event(afs_ctx *c) {
  if (!(c->cfg.flags & AFS_PROFILE)) return nullptr;
  constexpr size_t CAP = 1 << 14;
  if (c->pev_used == c->pev.size()) {
    hipEvent_t e = nullptr;
    if (c->pev.size() >= CAP || hipEventCreate(&e) != hipSuccess) {
      c->timed_overflow = true;
      return nullptr;
    }
    c->pev.push_back(e);
  }
  hipEvent_t e = c->pev[c->pev_used++];
  if (hipEventRecord(e, c->stream) != hipSuccess) return nullptr;
  return e;
}
void prof_pair(afs_ctx *c, hipEvent_t a, hipEvent_t b, int kind) {
  if (a && b) c->timed.push_back({a, b, kind});
}

// A call's slot order for K1 (shape_order): the order (null: the identity), the launch's blocks, and
// whether K1 may run the noise-phase variants (variants_dev: decided on the device, else `variants`).
struct SlotOrder {
  const int32_t *order = nullptr;
  int grid = 0;
  bool variants = true;
  const int32_t *variants_dev = nullptr;
};
// the slot order of a call without one (the voice kernel, sessions, target sequences, small batches)
SlotOrder plain_order(const afs_ctx *c) {
  SlotOrder so;
  so.variants = c->noise_variants != 0;
  return so;
}

// One synthesis call as the launch functions below see it: frame transitions 1 .. ntrans
// (frames[row * fstride + k], k = 0 the latched frame) of `rows` distinct frame rows (B, or the
// target sequences' trajectories: utterance u plays row frame_row[u]) at `hop` samples each, the
// audio to out[u * ostride + s], the state the launches carry between them (the context's or a
// session's), and K1's slot order.
struct SynthCall {
  const afs_frame *frames = nullptr;
  int64_t fstride = 0;
  int rows = 0, ntrans = 0, hop = 0;
  double *out = nullptr;
  int64_t ostride = 0;
  // the _pcm calls (out is null): the audio as int16 to pcm[u * pstride + s]; the flows of each launch
  // pass through the context's flow window instead of `out`
  // (the _f32 and packed calls as well: `format` says what pcm points at, AFS_SAMPLE_I16 or
  // AFS_SAMPLE_F32, and with row_base -- a device array of B row starts in samples, ragged calls only --
  // utterance u's row starts at pcm[row_base[u]] instead of pcm[u * pstride])
  void *pcm = nullptr;
  int64_t pstride = 0;
  int format = AFS_SAMPLE_I16;
  const int64_t *row_base = nullptr;
  void *ws = nullptr;
  int32_t *rng = nullptr;
  void *lanes = nullptr;
  int64_t bp = 0;
  int B = 0, width = 0;
  const int32_t *frame_row = nullptr;
  SlotOrder so;
  // the _taps calls: tap k of utterance u to out[(u * n_taps + k) * stride + s] (null: no taps)
  struct Taps {
    double *out = nullptr;
    int64_t stride = 0;
  } taps;
  // afs_synthesize_ragged (device arrays; null: every utterance plays all ntrans transitions):
  // utterance u plays row_hops[u] of them, ntrans the longest's; block_end and pad_standin belong to
  // the slot order so.order (afs_ragged_order.h)
  struct Ragged {
    const int32_t *row_hops = nullptr;
    const int64_t *block_end = nullptr;
    const int32_t *pad_standin = nullptr;
  } ragged;
};

// the context's tap list as K1 reads it: a current from the slot the solver leaves it in, a
// pressure from the slot its owner publishes it into (afs_model.h TapSet)
afs::TapSet tap_set(const afs_ctx *c) {
  afs::TapSet t;
  t.n = c->n_taps;
  for (int k = 0; k < c->n_taps; ++k) {
    const bool cur = c->taps[k].kind == AFS_TAP_CURRENT;
    t.sec[k] = cur ? -1 : c->taps[k].index;
    t.x[k] = cur ? c->host_tab.tap_u[c->taps[k].index] : c->host_tab.tap_p + k;
  }
  return t;
}

// The noise-source plans one K1 launch reads: the dense records, the hop records (hop mode; K1
// indexes them from the launch's first hop), and for the guarded launches of run_hop_call K5's count
// of claimed slots and how many there are (the launch does nothing when *skip > skip_cap).
struct LaunchPlans {
  const uint64_t *plan;
  int64_t plan_stride;
  const afs::tree::PlanHop *hops;
  int64_t hop_stride;
  const uint32_t *skip = nullptr;
  int64_t skip_cap = 0;
};

// K6's glottal-tone input: section 25's pressure per sample of a launch of `per` samples.  Laid out
// so that every utterance's row sits at the same position in its 128-byte lines as its output row
// (stride and base congruent to the output's modulo 16 doubles): K1 stores both through one
// line-aligned window (tree_kernel.h).
// A _pcm call keeps the flows in a window of the same shape (c->flow): rows of `per` rounded up to whole
// lines, the base on a line, so every row of both windows starts a 128-byte line whatever the caller's
// pcm looks like, and neither window grows with the call's length.
afs_status p25_for(afs_ctx *c, const SynthCall &call, int64_t per, int64_t *stride) {
  const int64_t ostride = call.pcm ? (per + 15) / 16 * 16 : call.ostride;
  *stride = per + ((ostride - per) % 16 + 16) % 16;
  HIP_TRY(c, c->p25.reserve(((size_t)call.B * (size_t)*stride + 32) * sizeof(double)));
  if (call.pcm) HIP_TRY(c, c->flow.reserve(((size_t)call.B * (size_t)*stride + 16) * sizeof(double)));
  return AFS_OK;
}
// the flow window's first row: the first 128-byte line of c->flow
double *flow_row0(const afs_ctx *c) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(c->flow.data());
  return reinterpret_cast<double *>((p + 127) & ~(uintptr_t)127);
}
// the p25 base for the launch whose outputs start at `out`
double *p25_row0(const afs_ctx *c, const double *out) {
  const int64_t want = (int64_t)((reinterpret_cast<uintptr_t>(out) >> 3) & 15);
  const int64_t have = (int64_t)((reinterpret_cast<uintptr_t>(c->p25.data()) >> 3) & 15);
  return c->p25.as<double>() + ((want - have) % 16 + 16) % 16;
}

// K5's arguments for samples [s0, s1) of the call's frame rows, dense records into `plan`
afs::PlanArgs plan_args(const afs_ctx *c, const afs_frame *frames, int64_t fstride, int rows, int hop, int64_t s0,
                        int64_t s1, uint64_t *plan, int64_t plan_stride) {
  afs::PlanArgs pa{};
  pa.tab = c->tab(), pa.uo = c->tab()->consts.sec;
  pa.frames = frames, pa.frame_stride = fstride;
  pa.rows = rows, pa.hop = hop;
  pa.s_begin = s0, pa.s_end = s1;
  pa.plan = plan, pa.plan_stride = plan_stride;
  pa.two_mass = c->cfg.options.glottis_model == AFS_GLOTTIS_TWO_MASS ? 1 : 0;
  return pa;
}

// K1 over samples [s0, s1) of the call, then K6 over them (both timed).  A _pcm call: K1's flows into
// the flow window (rows of p25_stride, as p25's), K6's PCM form from there to the caller's pcm -- or its
// float32 or packed form, by the call's format and row_base (afs_tree.h launch_tree_output_samples).
afs_status launch_synth_output(afs_ctx *c, const SynthCall &call, int64_t s0, int64_t s1, const LaunchPlans &lp,
                               int64_t p25_stride) {
  const SlotOrder &so = call.so;
  double *out = call.pcm ? flow_row0(c) : call.out + s0, *p25 = p25_row0(c, out);
  afs::TreeArgs a{};
  a.tab = c->tab(), a.uni = c->host_tab.uni;
  a.frames = call.frames, a.frame_stride = call.fstride, a.frame_row = call.frame_row;
  a.hop = call.hop, a.s_begin = s0, a.s_end = s1;
  a.out = out, a.out_stride = call.pcm ? p25_stride : call.ostride;
  a.plan = lp.plan, a.plan_stride = lp.plan_stride;
  a.hops = lp.hops, a.hop_stride = lp.hop_stride;
  a.skip_claims = lp.skip, a.skip_cap = lp.skip_cap;
  a.lane_state = call.lanes, a.lds_state = (double *)call.ws, a.B = call.B;
  a.p25 = p25, a.p25_stride = p25_stride;
  a.order = so.order, a.grid_blocks = so.grid;
  a.noise_variants = so.variants ? 1 : 0, a.variants_dev = so.variants_dev;
  {  // the pairs' STAT priority mode by the launch's rounds of workgroups per CU slot (two per CU):
     // mode 2 from two rounds, 0 below (profiles/r06_pair_ab.txt r06zh-r06zm)
    const int64_t blocks = so.grid > 0 ? so.grid : ((int64_t)call.B + afs::TREE_UPB - 1) / afs::TREE_UPB;
    const int64_t slots = std::max<int64_t>(1, c->simds / 2), rounds = (blocks + slots - 1) / slots;
    a.stat_prio = (call.width == afs::TREE_W && rounds >= 2) ? 2 : 0;
  }
  if (call.taps.out) {  // (every launch of the call carries the list: the rows go on where the last launch stopped)
    a.taps = tap_set(c);
    a.tap_out = call.taps.out + s0, a.tap_stride = call.taps.stride;
  }
  a.block_end = call.ragged.block_end, a.pad_standin = call.ragged.pad_standin;
  hipEvent_t e1 = prof_event(c);
  HIP_TRY(c, afs::launch_tree_synth(a, call.width, c->stream));
  hipEvent_t e2 = prof_event(c);
  prof_pair(c, e1, e2, 0);
  // K6: the glottal-tone filter and the output stage of the launch's samples
  if (call.pcm)
    HIP_TRY(c, afs::launch_tree_output_samples(c->tab(), (double *)call.ws, out, p25_stride, s1 - s0, call.B, p25,
                                               c->cfg.options.radiation_from_skin, call.format, call.pcm, call.pstride,
                                               call.row_base, c->stream, lp.skip, lp.skip_cap, call.ragged.row_hops,
                                               call.hop, s0));
  else
    HIP_TRY(c, afs::launch_tree_output(c->tab(), (double *)call.ws, out, call.ostride, s1 - s0, call.B, p25, p25_stride,
                                       c->cfg.options.radiation_from_skin, c->stream, lp.skip, lp.skip_cap,
                                       call.ragged.row_hops, call.hop, s0));
  prof_pair(c, e2, prof_event(c), 2);
  return AFS_OK;
}

// hop mode: hop records from K5 (tree solver, hops >= PLAN_HOP_MIN, not AFS_PLAN_DENSE=1)
bool hop_mode(const afs_ctx *c, int hop) { return !c->plan_dense && hop >= afs::tree::PLAN_HOP_MIN; }

// The hop records and K5's work list for `rows` rows of `hstride` hop slots.
afs_status ensure_hop_buffers(afs_ctx *c, int rows, int64_t hstride) {
  HIP_TRY(c, c->hops.reserve((size_t)rows * (size_t)hstride * sizeof(afs::tree::PlanHop)));
  HIP_TRY(c, c->plan_work.reserve((size_t)afs::plan_work_bytes(rows, hstride)));
  return AFS_OK;
}

// Hop mode's fast path: K5 decides every hop of the call first -- one record per (row, hop), the
// hops it cannot decide at once listed -- and K5's second stage decides the listed hops sample by
// sample, writing the dense records of the mixed ones (whose samples differ) into a compact array
// (one hop-long slot each, claimed from a counter).  K1 then runs the call in launches of up to
// 65536 samples, each hop's words evaluated from its record (or read from its dense slot).  One K1
// launch per second of 44.1 kHz audio instead of one per 4096 samples: no state save / restore and
// launch tail in between (+0.6 %, profiles/r04c_store_launch_ab.txt).
// *done = false: nothing ran that changed the state, and the caller runs the chunked path -- the
// call is not in hop mode, its hop records would exceed the plan budget, or its mixed hops
// overflowed the slots (below).
afs_status run_hop_call(afs_ctx *c, const SynthCall &call, bool *done) {
  *done = false;
  const int rows = call.rows, hop = call.hop;
  const int64_t S = (int64_t)call.ntrans * hop;
  const int64_t hstride = afs::plan_hop_slots(0, S, hop);  // (the hops of the call)
  const int64_t hbytes = (int64_t)rows * hstride * (int64_t)sizeof(afs::tree::PlanHop);
  if (!hop_mode(c, hop) || hbytes > c->plan_budget) return AFS_OK;
  afs_status st;
  if ((st = ensure_hop_buffers(c, rows, hstride)) != AFS_OK) return st;
  afs::tree::PlanHop *hbuf = c->hops.as<afs::tree::PlanHop>();
  uint32_t *work = c->plan_work.as<uint32_t>();
  afs::PlanArgs pa = plan_args(c, call.frames, call.fstride, rows, hop, 0, S, nullptr, 0);
  pa.hops = hbuf;
  pa.hop_stride = hstride;
  pa.work = work;
  pa.compact = true;
  pa.row_hops = call.ragged.row_hops;
  hipEvent_t e0 = prof_event(c);
  HIP_TRY(c, afs::launch_plan_hops_iv(pa, c->stream));
  // Slots for the mixed hops: one for every hop of the call when they fit the budget (small calls:
  // real-time sessions, short batches), else the budget's worth.  No host read-back before K1: the
  // launches are queued at once, guarded by the count of slots K5's second stage claimed (they do
  // nothing if it exceeds the slots); the host then waits for K5 alone -- the launches are already
  // queued behind it, so the device never idles for the host -- and, in the rare call whose mixed
  // hops overflowed the slots, queues the chunked path (most listed hops are not mixed: near-ties
  // decided alike by every sample; static vowels have none).
  const int64_t slot_bytes = (int64_t)hop * afs::PLAN_RECORD_BYTES;
  const int64_t every = (int64_t)rows * hstride;
  const bool small = every * slot_bytes <= std::min<int64_t>(c->plan_budget, SMALL_CALL_DENSE_BYTES);
  const int64_t cap = small ? every : std::min<int64_t>(every, std::max<int64_t>(1, c->plan_budget / slot_bytes));
  HIP_TRY(c, c->plan.reserve((size_t)(cap * slot_bytes)));
  pa.plan = c->plan.as<uint64_t>();
  pa.dense_cap = cap;
  HIP_TRY(c, afs::launch_plan_hops_wave(pa, c->stream));
  const bool guard = cap < every;
  if (guard) {
    HIP_TRY(c, hipMemcpyAsync(c->hcount.data(), work + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_k5, c->stream));
  }
  prof_pair(c, e0, prof_event(c), 1);
  const int64_t per = std::min<int64_t>(S, c->launch_cap);
  int64_t p25_stride = 0;
  if ((st = p25_for(c, call, per, &p25_stride)) != AFS_OK) return st;
  for (int64_t s0 = 0; s0 < S; s0 += per) {
    const LaunchPlans lp{c->plan.as<uint64_t>(), 0, hbuf + s0 / hop, hstride, guard ? work + 1 : nullptr, cap};
    if ((st = launch_synth_output(c, call, s0, std::min(S, s0 + per), lp, p25_stride)) != AFS_OK) return st;
  }
  if (guard) {
    HIP_TRY(c, hipEventSynchronize(c->ev_k5));
    // (overflow: the guarded launches did nothing, the state is still the call's initial state)
    if ((int64_t)*c->hcount.as<uint32_t>() > cap) return AFS_OK;
  }
  *done = true;
  return AFS_OK;
}

// The chunked path (hops < PLAN_HOP_MIN, AFS_PLAN_DENSE=1, or past the plan budget): launches of
// `per` samples, each K5 (the chunk's plans: dense records, or in hop mode the chunk's hop records
// with compact dense records) and then K1, on the one stream.  (K5 of the next chunk on a second
// stream beside K1 of this one was measured and not kept: +1.4 % in one run, K1 9 % slower beside
// it in others, profiles/r03m_kernel_stats.csv, AB_LOG.md.)
// Dense records: `per` samples per row.  Hop mode: the compact dense records of the chunk's
// listed hops, slot e of the work list holding `hop` records, and every hop the chunk spans may
// be listed -- rows x hstride slots of hop records, hstride = the chunk's hop slots + 1 (a chunk
// may start inside a hop).  Chunks of whole hops are sized so that this worst case fits the
// budget (at least one hop per chunk: past that the budget is exceeded, not the buffer).
afs_status run_chunked(afs_ctx *c, const SynthCall &call) {
  const int rows = call.rows, hop = call.hop;
  const int64_t S = (int64_t)call.ntrans * hop;
  const bool hops = hop_mode(c, hop);
  int64_t per = std::min<int64_t>(S, c->launch_cap);
  if (hops) {
    const int64_t slots_fit = c->plan_budget / ((int64_t)rows * hop * afs::PLAN_RECORD_BYTES) - 1;
    per = std::min<int64_t>(per, std::max<int64_t>(1, slots_fit) * hop);
  } else {
    per = std::min<int64_t>(per, c->plan_budget / ((int64_t)rows * afs::PLAN_RECORD_BYTES));
  }
  per = std::max<int64_t>(1, per);
  const int64_t hstride = afs::plan_hop_slots(0, per, hop) + 1;
  const size_t pbytes = (size_t)rows * (size_t)(hops ? hstride * hop : per) * afs::PLAN_RECORD_BYTES;
  afs_status st;
  HIP_TRY(c, c->plan.reserve(pbytes));
  if (hops && (st = ensure_hop_buffers(c, rows, hstride)) != AFS_OK) return st;
  int64_t p25_stride = 0;
  if ((st = p25_for(c, call, per, &p25_stride)) != AFS_OK) return st;
  afs::tree::PlanHop *hbuf = hops ? c->hops.as<afs::tree::PlanHop>() : nullptr;
  for (int64_t s0 = 0; s0 < S; s0 += per) {
    const int64_t s1 = std::min(S, s0 + per);
    afs::PlanArgs pa = plan_args(c, call.frames, call.fstride, rows, hop, s0, s1, c->plan.as<uint64_t>(), per);
    pa.hops = hbuf;
    pa.hop_stride = hstride;
    pa.work = hops ? c->plan_work.as<uint32_t>() : nullptr;
    pa.compact = hops;
    pa.dense_cap = (int64_t)rows * hstride;  // (hop mode: a slot for every hop of the chunk)
    pa.row_hops = call.ragged.row_hops;
    hipEvent_t e0 = prof_event(c);
    HIP_TRY(c, hops ? afs::launch_plan_hops(pa, c->stream) : afs::launch_plan(pa, c->stream));
    prof_pair(c, e0, prof_event(c), 1);
    const LaunchPlans lp{c->plan.as<uint64_t>(), per, hbuf, hstride};
    if ((st = launch_synth_output(c, call, s0, s1, lp, p25_stride)) != AFS_OK) return st;
  }
  return AFS_OK;
}

// The one-lane solvers: launches of at most 8192 samples, whole transitions each.
afs_status run_lane(afs_ctx *c, const SynthCall &call) {
  const int per = (int)std::max<int64_t>(1, 8192 / std::max(1, call.hop));
  for (int k = 1; k <= call.ntrans; k += per) {
    const int ke = std::min(call.ntrans + 1, k + per);
    afs::LaneArgs a{};
    a.tab = c->tab(), a.sor = c->cfg.solver == AFS_SOLVER_SOR ? 1 : 0;
    a.frames = call.frames, a.frame_stride = call.fstride, a.frame_row = call.frame_row;
    a.k_begin = k, a.k_end = ke, a.hop = call.hop;
    a.out = call.out + (int64_t)(k - 1) * call.hop, a.out_stride = call.ostride;
    a.ws = (double *)call.ws, a.rng = call.rng, a.bp = call.bp, a.B = call.B;
    hipEvent_t e0 = prof_event(c);
    HIP_TRY(c, afs::launch_lane_synth(a, c->stream));
    prof_pair(c, e0, prof_event(c), 0);
  }
  return AFS_OK;
}

// Queue the call's synthesis in launches that keep each kernel well below a second; the state is
// carried between launches.
afs_status run_call(afs_ctx *c, const SynthCall &call) {
  if (!tree(c)) return run_lane(c, call);
  bool done = false;
  const afs_status st = run_hop_call(c, call, &done);
  if (st != AFS_OK || done) return st;
  return run_chunked(c, call);
}

// bytes of the state buffers for B utterances
size_t ws_bytes_for(const afs_ctx *c, int64_t bp) {
  if (tree(c)) return (size_t)bp * afs::tree_lds_doubles() * sizeof(double);
  return (size_t)(afs::lane_ws_rows(c->host_tab) * bp) * sizeof(double);
}
size_t lanes_bytes_for(const afs_ctx *c, int64_t bp, int width) {
  return tree(c) ? (size_t)bp * (size_t)width * (size_t)afs::tree_lane_bytes(width) : 0;
}

afs_status reset_state(afs_ctx *c, void *ws, int32_t *rng, void *lanes, int64_t bp, int B, const uint32_t *seeds_dev,
                       int width) {
  if (tree(c))
    HIP_TRY(c, afs::launch_tree_reset(lanes, (double *)ws, B, seeds_dev, width, c->stream));
  else
    HIP_TRY(c, afs::launch_lane_reset((double *)ws, rng, bp, B, seeds_dev, c->stream));
  return AFS_OK;
}

// ---- call staging: the host-or-device arguments of the calls, the context's state, the report ----

// An argument of a call that may live on the host.  `dev` is what the kernels read or write: the
// caller's array `user` when that is device memory (or null), else (`host`) a buffer of the context
// sized to its bytes, which an input is uploaded to (`upload`) and an output is copied back from.
// An output whose kernels write only part of it is uploaded first as well: the rest is the caller's.
template <class T>
struct Staged {
  T *user = nullptr, *dev = nullptr;
  size_t bytes = 0;
  bool host = false;
  afs_status stage(afs_ctx *c, T *p, size_t n, afs::DeviceBuf &buf, bool upload = false) {
    user = dev = p;
    bytes = n;
    host = p && !is_device_ptr(p);
    if (!host) return AFS_OK;
    HIP_TRY(c, buf.reserve(n));
    dev = buf.as<T>();
    if (upload) HIP_TRY(c, hipMemcpyAsync(buf.data(), p, n, hipMemcpyHostToDevice, c->stream));
    return AFS_OK;
  }
  // queue the copy a host output is owed (to `to`, a pinned stand-in for the caller's array, when given)
  afs_status copy_back(afs_ctx *c, void *to = nullptr) const {
    if (host) HIP_TRY(c, hipMemcpyAsync(to ? to : user, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    return AFS_OK;
  }
};

// frames[n] on the device: a host array is uploaded through the context's staging buffer
using Frames = Staged<const afs_frame>;
afs_status frames_to_device(afs_ctx *c, const afs_frame *frames, size_t n, Frames *d) {
  return d->stage(c, frames, n * sizeof(afs_frame), c->stage_in, true);
}
// seeds[B] on the device likewise (null stays null: the reset kernels seed utterance u with u + 1)
using Seeds = Staged<const uint32_t>;
afs_status seeds_to_device(afs_ctx *c, const uint32_t *seeds, int B, Seeds *d) {
  return d->stage(c, seeds, (size_t)B * sizeof(uint32_t), c->stage_seeds, true);
}

// Per-utterance non-finite flags (into `flags`, a host or device array of B bytes, or nowhere)
// and their count (into the pinned c->hcount, read after the stream synchronises).  *host_sync
// is set when the flags go to host memory (the call must synchronise before returning).
afs_status nonfinite_report(afs_ctx *c, void *ws, int64_t bp, int B, uint8_t *flags, bool want_count,
                            bool *host_sync) {
  *host_sync = false;
  if (!flags && !want_count) return AFS_OK;
  Staged<uint8_t> f;
  afs_status s = f.stage(c, flags, (size_t)B, c->stage_nf);
  if (s != AFS_OK) return s;
  *host_sync = f.host;
  int32_t *dcount = c->dcount.as<int32_t>();
  HIP_TRY(c, hipMemsetAsync(dcount, 0, sizeof(int32_t), c->stream));
  if (tree(c))
    HIP_TRY(c, afs::launch_tree_nonfinite((const double *)ws, B, dcount, f.dev, c->stream));
  else
    HIP_TRY(c, afs::launch_lane_nonfinite((const double *)ws, bp, B, dcount, f.dev, c->stream));
  if ((s = f.copy_back(c)) != AFS_OK) return s;
  if (want_count) HIP_TRY(c, hipMemcpyAsync(c->hcount.data(), dcount, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  return AFS_OK;
}

// the context's state buffers for B utterances of `width` lanes, enlarged as needed and reset to the seeds
afs_status fresh_state(afs_ctx *c, int B, int width, const uint32_t *dseeds) {
  const int64_t bp = pad64(B);
  HIP_TRY(c, c->ws.reserve(ws_bytes_for(c, bp)));
  HIP_TRY(c, c->rng.reserve((size_t)(32 * bp) * sizeof(int32_t)));
  if (tree(c)) HIP_TRY(c, c->tree_lanes.reserve(lanes_bytes_for(c, bp, width)));
  return reset_state(c, c->ws.data(), c->rng.as<int32_t>(), c->tree_lanes.data(), bp, B, dseeds, width);
}

// the call on the context's state (fresh_state) for B utterances of `width` lanes
SynthCall context_call(const afs_ctx *c, int B, int width) {
  SynthCall call;
  call.ws = c->ws.data(), call.rng = c->rng.as<int32_t>(), call.lanes = c->tree_lanes.data();
  call.bp = pad64(B), call.B = B, call.width = width;
  call.so = plain_order(c);
  return call;
}

// the report of a call whose kernels ran between ev0 and ev1 (after the stream has synchronised)
afs_status fill_report(afs_ctx *c, afs_report *rep, int64_t samples) {
  if (!rep) return AFS_OK;
  float ms = 0.f;
  HIP_TRY(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
  rep->device_ms = ms;
  rep->samples = samples;
  rep->nonfinite_utterances = *c->hcount.as<int32_t>();
  rep->kernel = c->cfg.solver;
  return AFS_OK;
}

// The end of a whole-trajectory call on the context's state: the copy of staged taps to a host
// array, ev1, the non-finite flags and count, the copy of staged audio to a host `out`, then the wait
// and the report.  The call returns without a wait only when it is asynchronous (`async`) and nothing
// goes to host memory: no host `out` or taps, no report, no host flags.  `samples`: what the report
// counts.  (`out`: the audio as the call delivers it, doubles or the _pcm calls' int16.)
template <class T>
afs_status finish_call(afs_ctx *c, int B, int64_t samples, const Staged<T> &out, const Staged<double> &taps,
                       uint8_t *nonfinite, afs_report *rep, bool async) {
  afs_status s;
  if ((s = taps.copy_back(c)) != AFS_OK) return s;
  HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
  c->last_B = B;
  bool nf_sync = false;
  if ((s = nonfinite_report(c, c->ws.data(), pad64(B), B, nonfinite, rep != nullptr, &nf_sync)) != AFS_OK) return s;
  if ((s = out.copy_back(c)) != AFS_OK) return s;
  if (!async || out.host || taps.host || rep || nf_sync) HIP_TRY(c, hipStreamSynchronize(c->stream));
  return fill_report(c, rep, samples);
}

afs_status draws_of(afs_ctx *c, const void *ws, int B, int64_t *draws) {
  if (!tree(c)) return fail(c, AFS_ERR_UNSUPPORTED, "rand() call counts are kept by the tree solver only");
  afs::DeviceBuf tmp;
  Staged<int64_t> d;
  afs_status s;
  if ((s = d.stage(c, draws, (size_t)B * sizeof(int64_t), tmp)) != AFS_OK) return s;
  HIP_TRY(c, afs::launch_tree_draws((const double *)ws, B, d.dev, c->stream));
  if ((s = d.copy_back(c)) != AFS_OK) return s;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return AFS_OK;
}

}  // namespace

extern "C" {

int32_t afs_abi_version(void) { return AFS_ABI_VERSION; }

void afs_config_default(afs_config *cfg) {
  if (!cfg) return;
  std::memset(cfg, 0, sizeof *cfg);
  cfg->sampling_rate_hz = 22050.0;
  cfg->precision = AFS_FP64;
  cfg->solver = AFS_SOLVER_TREE;  // (the fastest kernel: DESIGN.md 4)
  cfg->device = 0;
  cfg->flags = 0;
  cfg->options = afs::default_options();
}

const char *afs_status_string(afs_status s) {
  switch (s) {
    case AFS_OK: return "ok";
    case AFS_ERR_INVALID_ARGUMENT: return "invalid argument";
    case AFS_ERR_NO_DEVICE: return "no HIP device";
    case AFS_ERR_HIP: return "HIP runtime error";
    case AFS_ERR_OUT_OF_MEMORY: return "out of device memory";
    case AFS_ERR_UNSUPPORTED: return "unsupported configuration";
  }
  return "unknown status";
}

afs_status afs_create(afs_ctx **out, const afs_config *cfg) {
  if (!out) return AFS_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  afs_config c;
  if (cfg) c = *cfg; else afs_config_default(&c);
  if (!(c.sampling_rate_hz > 0.0) || c.precision != AFS_FP64 || !solver_ok(c.solver) ||
      ((c.flags & AFS_LANES_16) && (c.flags & AFS_LANES_64)))
    return AFS_ERR_INVALID_ARGUMENT;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    return AFS_ERR_NO_DEVICE;
  }
  if (c.device < 0 || c.device >= n) return AFS_ERR_NO_DEVICE;
  if (hipSetDevice(c.device) != hipSuccess) return AFS_ERR_NO_DEVICE;
  afs_ctx *ctx = new afs_ctx();
  ctx->cfg = c;
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c.device) != hipSuccess || cus <= 0) cus = 256;
    ctx->simds = 4 * cus;  // (4 SIMDs per CU on CDNA)
  }
  afs::build_tables(&ctx->host_tab, c.sampling_rate_hz, c.options);
  if (ctx->host_tab.n_rounds <= 0) { afs_destroy(ctx); return AFS_ERR_UNSUPPORTED; }
  auto bail = [&](afs_status s) { afs_destroy(ctx); return s; };
  if (ctx->dev_tab.reserve(sizeof(afs::Tables)) != hipSuccess) return bail(AFS_ERR_OUT_OF_MEMORY);
  if (hipMemcpy(ctx->dev_tab.data(), &ctx->host_tab, sizeof(afs::Tables), hipMemcpyHostToDevice) != hipSuccess)
    return bail(AFS_ERR_HIP);
  if (ctx->dcount.reserve(sizeof(int32_t)) != hipSuccess) return bail(AFS_ERR_OUT_OF_MEMORY);
  if (ctx->hcount.reserve(sizeof(int32_t)) != hipSuccess) return bail(AFS_ERR_OUT_OF_MEMORY);
  *ctx->hcount.as<int32_t>() = 0;
  if (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) return bail(AFS_ERR_HIP);
  // the code objects of the kernels a synthesis call launches, loaded now rather than at their
  // first launch (which cost a real-time caller's first buffer ~35 ms)
  if (afs::preload_tree_kernels() != hipSuccess || afs::preload_plan_kernels() != hipSuccess ||
      afs::preload_audio_kernels() != hipSuccess || afs::preload_session_kernels() != hipSuccess)
    return bail(AFS_ERR_HIP);
  if (hipEventCreateWithFlags(&ctx->ev_k5, hipEventDisableTiming) != hipSuccess) return bail(AFS_ERR_HIP);
  if (const char *e = std::getenv("AFS_PLAN_DENSE")) ctx->plan_dense = std::atoi(e) != 0;
  if (const char *e = std::getenv("AFS_SHAPE_ORDER")) ctx->shape_order = std::atoi(e) != 0;
  if (const char *e = std::getenv("AFS_NOISE_VARIANTS")) ctx->noise_variants = std::atoi(e);
  if (const char *e = std::getenv("AFS_LAUNCH_SAMPLES")) {  // (A/B and latency studies: samples per K1 launch)
    const long long v = std::atoll(e);
    if (v > 0) ctx->launch_cap = std::min<int64_t>(v, 65536);
  }
  ctx->plan_budget = PLAN_BUDGET_DEFAULT;
  if (const char *e = std::getenv("AFS_PLAN_BUDGET_MB")) {
    const long long mb = std::atoll(e);
    if (mb > 0) ctx->plan_budget = (int64_t)mb << 20;
  }
  *out = ctx;
  return AFS_OK;
}

void afs_destroy(afs_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->cfg.device);
  for (hipEvent_t e : {c->ev_k5, c->ev_ragged, c->ev0, c->ev1})
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->pev) (void)hipEventDestroy(e);
  delete c;  // (its buffers go with it: afs_buf.h)
}

const char *afs_last_error(const afs_ctx *c) { return c ? c->err.c_str() : "null context"; }

afs_status afs_set_stream(afs_ctx *c, void *s) {
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  c->stream = (hipStream_t)s;
  return AFS_OK;
}

afs_status afs_synchronize(afs_ctx *c) {
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return AFS_OK;
}

}  // extern "C"

// Slot order of the 16-lane tree kernel for a batch of independent utterances: sorted by the shape
// key of their first frame (how narrow the tube is and where: launch_utterance_keys), so that the
// four utterances of a wave -- which run in lockstep and pay for the union of their branches
// (noise sources, the cutoff filter's exponential, mixed hops) -- and the blocks of a compute unit
// play alike shapes, the heaviest (narrowest constrictions) first.  Each utterance's audio is the
// same in any slot.  Config-4 shard: +2.7 % static vowels, +1.4 % fricatives against the call order
// (profiles/r04s_shape_order_ab.txt, r04v_shape_key_ab.txt).  Off for the voice kernel (one
// utterance per wave), batches of one block and AFS_SHAPE_ORDER=0.
//
// All on the device, with no host wait (the call's K1 is queued behind it while the previous call's
// K1 still runs): the key kernel, the variant rule and a stable radix sort of (key, utterance)
// (af_kernels.hip launch_slot_order).  The rule: the noise-phase variants pay when most waves are
// light, or when every SIMD runs many waves: at 8192 static vowels (61 % light, two waves per SIMD)
// +2.3 %, at 8192 fricatives (28 % light) -3 % -- the full-phase waves lose more to the light ones'
// copies of the kernel body in their CUs' instruction caches than the light ones gain -- but at 65536
// fricatives (16 waves per SIMD, the classes in long runs of the slot order) +0.7 %, at 32768 (8 per
// SIMD) +0.05 % (profiles/r05i_fricatives_variants_ab.txt, r05k_variant_rule_ab.txt,
// r05r_variant_rule_ab.txt).  Without them the class is left out of the sort (the class key alone
// measured -0.6 %, r05f_variant_order_ab.txt).  (Dealing the blocks of a class-major order to the XCDs
// on the host, one variant per XCD, cost a host wait and measured 311 M against 425 M samples/s:
// profiles/r05j_xcd_deal_static_ab.txt, AB_LOG.md.)
static afs_status shape_order(afs_ctx *c, const afs_frame *dframes, int64_t fstride, int B, int width, SlotOrder *so) {
  *so = plain_order(c);
  const int upb = afs::TREE_UPB;
  if (!tree(c) || !c->shape_order || width == afs::TREE_VOICE_W || B <= upb) return AFS_OK;
  const int nb = (B + upb - 1) / upb;
  // keys[B], sorted keys[B], indices[B], the variant flag
  const size_t kb = (size_t)B * (2 * sizeof(uint64_t) + sizeof(int32_t)) + 16;
  HIP_TRY(c, c->keys.reserve(kb));
  uint64_t *dkeys = c->keys.as<uint64_t>(), *dsorted = dkeys + B;
  int32_t *didx = (int32_t *)(dsorted + B), *dvar = didx + B;
  HIP_TRY(c, afs::launch_utterance_keys(dframes, fstride, B, dkeys, c->stream));
  const int64_t waves_per_simd = (int64_t)B / ((int64_t)(64 / afs::TREE_W) * std::max(1, c->simds));
  const int mode = c->noise_variants == 0 ? 0 : c->noise_variants == 1 ? 1 : 2;
  HIP_TRY(c, c->order_buf.reserve((size_t)nb * upb * sizeof(int32_t)));
  int32_t *dorder = c->order_buf.as<int32_t>();
  size_t tb = 0;  // (the first call asks for the sort's scratch size only)
  HIP_TRY(c, afs::launch_slot_order(dkeys, dsorted, didx, B, mode, waves_per_simd >= 16, dvar,
                                    dorder, nb * upb, nullptr, &tb, c->stream));
  HIP_TRY(c, c->sort_tmp.reserve(tb + 256));
  tb = c->sort_tmp.capacity();
  HIP_TRY(c, afs::launch_slot_order(dkeys, dsorted, didx, B, mode, waves_per_simd >= 16, dvar,
                                    dorder, nb * upb, c->sort_tmp.data(), &tb, c->stream));
  so->order = dorder;
  so->grid = nb;
  so->variants_dev = dvar;
  return AFS_OK;
}

// what a _taps call needs beside the plain call's arguments
static afs_status taps_check(afs_ctx *c, const char *fn, const double *taps_out) {
  if (!tree(c)) return fail(c, AFS_ERR_UNSUPPORTED, "%s: tree solver only", fn);
  if (c->n_taps <= 0) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: no taps set (afs_set_taps)", fn);
  if (!taps_out) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: taps_out is NULL", fn);
  return AFS_OK;
}

// The launch layout of a ragged call and its per-row hop counts on the device: built on the host from
// num_frames (afs_ragged_order.h), packed into the context's pinned buffer and uploaded on the stream
// -- no host wait, except for the previous ragged call's upload when that has not been read yet.
static afs_status ragged_layout(afs_ctx *c, const int32_t *num_frames, int B, int upb, int hop, SynthCall *call,
                                const int64_t *row_base = nullptr) {
  const afs::RaggedOrder ro = afs::ragged_order(num_frames, B, upb, hop);
  const size_t slots = ro.order.size();
  const size_t end_bytes = (size_t)ro.grid * sizeof(int64_t), slot_bytes = slots * sizeof(int32_t);
  // (a packed call's row starts ride behind the hop counts, on an 8-byte boundary)
  const size_t base0 = (end_bytes + 2 * slot_bytes + (size_t)B * sizeof(int32_t) + 7) / 8 * 8;
  const size_t bytes = base0 + (row_base ? (size_t)B * sizeof(int64_t) : 0);
  if (!c->ev_ragged) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_ragged, hipEventDisableTiming));
  else HIP_TRY(c, hipEventSynchronize(c->ev_ragged));
  HIP_TRY(c, c->ragged_host.reserve(bytes));
  HIP_TRY(c, c->ragged.reserve(bytes));
  char *h = c->ragged_host.as<char>(), *d = c->ragged.as<char>();
  std::memcpy(h, ro.block_end.data(), end_bytes);
  std::memcpy(h + end_bytes, ro.order.data(), slot_bytes);
  std::memcpy(h + end_bytes + slot_bytes, ro.standin.data(), slot_bytes);
  int32_t *hops = (int32_t *)(h + end_bytes + 2 * slot_bytes);
  for (int u = 0; u < B; ++u) hops[u] = num_frames[u] - 1;
  if (row_base) std::memcpy(h + base0, row_base, (size_t)B * sizeof(int64_t));
  HIP_TRY(c, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev_ragged, c->stream));
  call->row_base = row_base ? (const int64_t *)(d + base0) : nullptr;
  call->ragged.block_end = (const int64_t *)d;
  call->so.order = (const int32_t *)(d + end_bytes);
  call->so.grid = ro.grid;
  call->ragged.pad_standin = (const int32_t *)(d + end_bytes + slot_bytes);
  call->ragged.row_hops = (const int32_t *)(d + end_bytes + 2 * slot_bytes);
  return AFS_OK;
}

// A whole-trajectory call on fresh state of the context, as its entry point has validated it:
// afs_synthesize (with taps_out: afs_synthesize_taps), or with num_frames afs_synthesize_ragged, the
// same call for utterances of different lengths.
struct Trajectories {
  const afs_frame *frames = nullptr;  // frames[u * fstride + k]
  int64_t fstride = 0;
  const int32_t *num_frames = nullptr;  // ragged: the frames of each utterance (host); null: F each
  int32_t F = 0;                        // the frames of the longest utterance
  const uint32_t *seeds = nullptr;
  int32_t B = 0, hop = 0;
  double *out = nullptr;  // out[u * ostride + s]
  int64_t ostride = 0;
  double *taps_out = nullptr;  // the context's taps beside the audio, rows of ostride as well (null: none)
  void *pcm = nullptr;         // the _pcm calls, instead of out: pcm[u * pstride + s]
  int64_t pstride = 0;
  int format = AFS_SAMPLE_I16;  // ... its samples (the _f32 and packed calls: int16_t or float)
  // the packed calls: row u at pcm[row_base[u] + s] instead (a host array the entry point has validated
  // or built), and the samples the buffer spans, max(row_base[u] + T_u)
  const int64_t *row_base = nullptr;
  int64_t span = 0;
  int64_t samples = 0;         // what the report counts
  bool force_async = false;    // leave the stream running unless a host buffer needs a wait
  int lanes = 0;               // the tree kernel's lanes per utterance (0: chosen for B)
};

// Everything between an entry point's validation and finish_call.  The uniform call takes K1's slot
// order from shape_order.  The ragged call is one call of ntrans = the longest utterance's
// transitions: K1's blocks each hold one length and end their time loop there (ragged_layout), K5 and
// K6 stop at each row's own end; the slot order by shape inside a length group is left out
// (DESIGN.md 2.8).
static afs_status synth_core(afs_ctx *c, const Trajectories &t, uint8_t *nonfinite, afs_report *rep) {
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const int B = t.B;
  const bool ragged = t.num_frames != nullptr;
  const size_t out_bytes = (size_t)B * (size_t)t.ostride * sizeof(double), taps_bytes = out_bytes * (size_t)c->n_taps;
  afs_status s;
  Frames fr;
  Seeds seeds;
  Staged<double> out, taps;
  Staged<char> pcm;
  if ((s = frames_to_device(c, t.frames, (size_t)B * (size_t)t.fstride, &fr)) != AFS_OK) return s;
  if ((s = seeds_to_device(c, t.seeds, B, &seeds)) != AFS_OK) return s;
  // (a ragged call's host out and taps go up first and come back whole: what lies past each row's
  // end is the caller's)
  if ((s = out.stage(c, t.out, out_bytes, c->stage_out, ragged)) != AFS_OK) return s;
  // (a host pcm likewise when its rows have padding; it reaches to the end of the last row's samples)
  const int64_t Tmax = (int64_t)(t.F - 1) * t.hop;
  // (a packed host out as well: its gaps are the caller's)
  const size_t pcm_samples = t.row_base ? (size_t)t.span : (size_t)(B - 1) * (size_t)t.pstride + (size_t)Tmax;
  const size_t pcm_bytes = pcm_samples * sample_bytes(t.format);
  if ((s = pcm.stage(c, (char *)t.pcm, pcm_bytes, c->stage_pcm, ragged || t.pstride != Tmax)) != AFS_OK) return s;
  const int width = t.lanes > 0 ? t.lanes : lanes_for(c, B);
  if ((s = fresh_state(c, B, width, seeds.dev)) != AFS_OK) return s;
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  if ((s = taps.stage(c, t.taps_out, taps_bytes, c->stage_taps, ragged)) != AFS_OK) return s;
  SynthCall call = context_call(c, B, width);
  call.frames = fr.dev, call.fstride = t.fstride, call.rows = B;
  call.ntrans = t.F - 1, call.hop = t.hop;
  call.out = out.dev, call.ostride = t.ostride;
  call.pcm = pcm.dev, call.pstride = t.pstride, call.format = t.format;
  call.taps.out = taps.dev, call.taps.stride = t.ostride;
  s = ragged ? ragged_layout(c, t.num_frames, B, width == afs::TREE_VOICE_W ? 1 : afs::TREE_UPB, t.hop, &call, t.row_base)
             : shape_order(c, fr.dev, t.fstride, B, width, &call.so);
  if (s != AFS_OK) return s;
  if ((s = run_call(c, call)) != AFS_OK) return s;
  const bool async = t.force_async || (c->cfg.flags & AFS_ASYNC);
  if (t.pcm) return finish_call(c, B, t.samples, pcm, taps, nonfinite, rep, async);
  return finish_call(c, B, t.samples, out, taps, nonfinite, rep, async);
}

// afs_synthesize: every utterance F frames, rows of T = (F - 1) * hop samples
static afs_status synth_uniform(afs_ctx *c, const afs_frame *frames, const uint32_t *seeds, int32_t B, int32_t F,
                                int32_t hop, double *out, double *taps_out, uint8_t *nonfinite, afs_report *rep,
                                bool force_async, int lanes) {
  if (!frames || !out || B <= 0 || F < 2 || hop < 1)
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "afs_synthesize: need frames, out, batch>0, num_frames>=2, hop>=1");
  Trajectories t;
  t.frames = frames, t.fstride = t.F = F;
  t.seeds = seeds, t.B = B, t.hop = hop;
  t.out = out, t.ostride = (int64_t)(F - 1) * hop, t.taps_out = taps_out;
  t.samples = (int64_t)B * t.ostride;
  t.force_async = force_async, t.lanes = lanes;
  return synth_core(c, t, nonfinite, rep);
}

afs_status afs::synthesize_async(afs_ctx *c, const afs_frame *frames, const uint32_t *seeds, int32_t B, int32_t F,
                                 int32_t hop, double *out, uint8_t *nonfinite, int lanes) {
  if (lanes != 0 && lanes != afs::TREE_W && lanes != afs::TREE_VOICE_W)
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "synthesize: %d lanes per utterance", lanes);
  return synth_uniform(c, frames, seeds, B, F, hop, out, nullptr, nonfinite, nullptr, true, lanes);
}

extern "C" {

afs_status afs_synthesize(afs_ctx *c, const afs_frame *frames, const uint32_t *seeds, int32_t B,
                          int32_t F, int32_t hop, double *out, uint8_t *nonfinite, afs_report *rep) {
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  return synth_uniform(c, frames, seeds, B, F, hop, out, nullptr, nonfinite, rep, false, 0);
}

afs_status afs_set_taps(afs_ctx *c, const afs_tap *taps, int32_t n) {
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  if (!tree(c)) return fail(c, AFS_ERR_UNSUPPORTED, "afs_set_taps: tree solver only");
  if (n < 0 || n > AFS_MAX_TAPS || (n > 0 && !taps))
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "afs_set_taps: need 0 <= n <= %d taps", AFS_MAX_TAPS);
  for (int k = 0; k < n; ++k) {
    const int lim = taps[k].kind == AFS_TAP_PRESSURE ? afs::NS : taps[k].kind == AFS_TAP_CURRENT ? afs::NC : 0;
    if (taps[k].index < 0 || taps[k].index >= lim)
      return fail(c, AFS_ERR_INVALID_ARGUMENT, "afs_set_taps: tap %d: kind %d, index %d", k, taps[k].kind, taps[k].index);
  }
  for (int k = 0; k < n; ++k) c->taps[k] = taps[k];
  c->n_taps = n;
  return AFS_OK;
}

afs_status afs_synthesize_taps(afs_ctx *c, const afs_frame *frames, const uint32_t *seeds, int32_t B, int32_t F,
                               int32_t hop, double *out, double *taps_out, uint8_t *nonfinite, afs_report *rep) {
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  const afs_status s = taps_check(c, "afs_synthesize_taps", taps_out);
  if (s != AFS_OK) return s;
  return synth_uniform(c, frames, seeds, B, F, hop, out, taps_out, nonfinite, rep, false, 0);
}

afs_status afs_synthesize_ragged(afs_ctx *c, const afs_frame *frames, int64_t fstride, const int32_t *num_frames,
                                 const uint32_t *seeds, int32_t B, int32_t hop, double *out, int64_t ostride,
                                 double *taps_out, uint8_t *nonfinite, afs_report *rep) {
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  const char *fn = "afs_synthesize_ragged";
  if (!tree(c)) return fail(c, AFS_ERR_UNSUPPORTED, "%s: tree solver only", fn);
  if (!frames || !out || B <= 0 || hop < 1) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: need frames, out, batch>0, hop>=1", fn);
  if (!num_frames || is_device_ptr(num_frames))
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: num_frames is a host array of batch counts", fn);
  Trajectories t;
  for (int32_t u = 0; u < B; ++u) {
    const int32_t F = num_frames[u];
    if (F < 2 || F > fstride)
      return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: num_frames[%d] = %d outside 2..frame_stride = %lld", fn, u, F,
                  (long long)fstride);
    t.F = std::max(t.F, F);
    t.samples += (int64_t)(F - 1) * hop;
  }
  const int64_t Tmax = (int64_t)(t.F - 1) * hop;
  if (ostride < Tmax)
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: out_stride %lld below the longest utterance's %lld samples", fn,
                (long long)ostride, (long long)Tmax);
  if (taps_out && c->n_taps <= 0) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: no taps set (afs_set_taps)", fn);
  t.frames = frames, t.fstride = fstride, t.num_frames = num_frames;
  t.seeds = seeds, t.B = B, t.hop = hop;
  t.out = out, t.ostride = ostride, t.taps_out = taps_out;
  return synth_core(c, t, nonfinite, rep);
}

// what a _pcm call needs of its destination: the tree solver, rows of at least T int16 samples
static afs_status pcm_check(afs_ctx *c, const char *fn, const int16_t *pcm, int64_t pstride, int64_t T) {
  if (!tree(c)) return fail(c, AFS_ERR_UNSUPPORTED, "%s: tree solver only", fn);
  if (!pcm || (reinterpret_cast<uintptr_t>(pcm) & 1))
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: pcm is NULL or not int16-aligned", fn);
  if (pstride < T)
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: pcm_stride %lld below the longest utterance's %lld samples", fn,
                (long long)pstride, (long long)T);
  return AFS_OK;
}

afs_status afs_synthesize_pcm(afs_ctx *c, const afs_frame *frames, const uint32_t *seeds, int32_t B, int32_t F,
                              int32_t hop, int16_t *pcm, int64_t pstride, uint8_t *nonfinite, afs_report *rep) {
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  const char *fn = "afs_synthesize_pcm";
  if (!frames || B <= 0 || F < 2 || hop < 1)
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: need frames, batch>0, num_frames>=2, hop>=1", fn);
  Trajectories t;
  t.frames = frames, t.fstride = t.F = F;
  t.seeds = seeds, t.B = B, t.hop = hop;
  t.ostride = (int64_t)(F - 1) * hop;
  const afs_status s = pcm_check(c, fn, pcm, pstride, t.ostride);
  if (s != AFS_OK) return s;
  t.pcm = pcm, t.pstride = pstride;
  t.samples = (int64_t)B * t.ostride;
  return synth_core(c, t, nonfinite, rep);
}

afs_status afs_synthesize_ragged_pcm(afs_ctx *c, const afs_frame *frames, int64_t fstride, const int32_t *num_frames,
                                     const uint32_t *seeds, int32_t B, int32_t hop, int16_t *pcm, int64_t pstride,
                                     uint8_t *nonfinite, afs_report *rep) {
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  const char *fn = "afs_synthesize_ragged_pcm";
  if (!tree(c)) return fail(c, AFS_ERR_UNSUPPORTED, "%s: tree solver only", fn);
  if (!frames || B <= 0 || hop < 1) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: need frames, batch>0, hop>=1", fn);
  if (!num_frames || is_device_ptr(num_frames))
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: num_frames is a host array of batch counts", fn);
  Trajectories t;
  for (int32_t u = 0; u < B; ++u) {
    const int32_t F = num_frames[u];
    if (F < 2 || F > fstride)
      return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: num_frames[%d] = %d outside 2..frame_stride = %lld", fn, u, F,
                  (long long)fstride);
    t.F = std::max(t.F, F);
    t.samples += (int64_t)(F - 1) * hop;
  }
  t.ostride = (int64_t)(t.F - 1) * hop;
  const afs_status s = pcm_check(c, fn, pcm, pstride, t.ostride);
  if (s != AFS_OK) return s;
  t.frames = frames, t.fstride = fstride, t.num_frames = num_frames;
  t.seeds = seeds, t.B = B, t.hop = hop;
  t.pcm = pcm, t.pstride = pstride;
  return synth_core(c, t, nonfinite, rep);
}

}  // extern "C"

// The rows of a packed call, checked on the host before anything is queued: row u holds len[u] samples of
// `format` at out[offsets[u] ..] (offsets null: tight packing in order); a row with len[u] < 0 is absent
// (an idle voice: its offset is not looked at).  base[u]: the row's start (0 for an absent row), *span: the
// samples out reaches over.  Rows may abut and may not overlap; a row without samples overlaps nothing.
static afs_status packed_rows(afs_ctx *c, const char *fn, int32_t format, const void *out, const int64_t *offsets,
                              const std::vector<int64_t> &len, std::vector<int64_t> *base, int64_t *span) {
  if (format != AFS_SAMPLE_I16 && format != AFS_SAMPLE_F32)
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: format %d is neither AFS_SAMPLE_I16 nor AFS_SAMPLE_F32", fn, format);
  if (offsets && is_device_ptr(offsets)) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: offsets is a host array", fn);
  const size_t B = len.size();
  base->assign(B, 0);
  *span = 0;
  int64_t total = 0;
  std::vector<std::pair<int64_t, int64_t>> rows;  // (start, samples) of the rows that hold any
  for (size_t u = 0; u < B; ++u) {
    if (len[u] < 0) continue;
    const int64_t at = offsets ? offsets[u] : total;
    if (at < 0) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: offsets[%d] = %lld is negative", fn, (int)u, (long long)at);
    (*base)[u] = at;
    total += len[u];
    if (len[u] > 0) {
      rows.emplace_back(at, len[u]);
      *span = std::max(*span, at + len[u]);
    }
  }
  if (offsets) {
    std::sort(rows.begin(), rows.end());
    for (size_t i = 1; i < rows.size(); ++i)
      if (rows[i - 1].first + rows[i - 1].second > rows[i].first)
        return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: the rows at offsets %lld (%lld samples) and %lld overlap", fn,
                    (long long)rows[i - 1].first, (long long)rows[i - 1].second, (long long)rows[i].first);
  }
  if (total > 0 && (!out || (reinterpret_cast<uintptr_t>(out) & (sample_bytes(format) - 1))))
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: out is NULL or not aligned to its sample type", fn);
  return AFS_OK;
}

extern "C" {

afs_status afs_synthesize_f32(afs_ctx *c, const afs_frame *frames, const uint32_t *seeds, int32_t B, int32_t F,
                              int32_t hop, float *f32, int64_t fstride, uint8_t *nonfinite, afs_report *rep) {
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  const char *fn = "afs_synthesize_f32";
  if (!tree(c)) return fail(c, AFS_ERR_UNSUPPORTED, "%s: tree solver only", fn);
  if (!frames || B <= 0 || F < 2 || hop < 1)
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: need frames, batch>0, num_frames>=2, hop>=1", fn);
  Trajectories t;
  t.frames = frames, t.fstride = t.F = F;
  t.seeds = seeds, t.B = B, t.hop = hop;
  t.ostride = (int64_t)(F - 1) * hop;
  if (!f32 || (reinterpret_cast<uintptr_t>(f32) & 3))
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: f32 is NULL or not float-aligned", fn);
  if (fstride < t.ostride)
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: f32_stride %lld below the utterances' %lld samples", fn,
                (long long)fstride, (long long)t.ostride);
  t.pcm = f32, t.pstride = fstride, t.format = AFS_SAMPLE_F32;
  t.samples = (int64_t)B * t.ostride;
  return synth_core(c, t, nonfinite, rep);
}

afs_status afs_ragged_offsets(const int32_t *num_frames, int32_t B, int32_t hop, int64_t *offsets) {
  if ((!num_frames && B > 0) || !offsets || B < 0 || hop < 1) return AFS_ERR_INVALID_ARGUMENT;
  for (int32_t u = 0; u < B; ++u)
    if (num_frames[u] < 1) return AFS_ERR_INVALID_ARGUMENT;
  int64_t at = 0;
  for (int32_t u = 0; u < B; ++u) {
    offsets[u] = at;
    at += (int64_t)(num_frames[u] - 1) * hop;
  }
  offsets[B] = at;
  return AFS_OK;
}

afs_status afs_synthesize_ragged_packed(afs_ctx *c, const afs_frame *frames, int64_t fstride, const int32_t *num_frames,
                                        const uint32_t *seeds, int32_t B, int32_t hop, int32_t format, void *out,
                                        const int64_t *offsets, uint8_t *nonfinite, afs_report *rep) {
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  const char *fn = "afs_synthesize_ragged_packed";
  if (!tree(c)) return fail(c, AFS_ERR_UNSUPPORTED, "%s: tree solver only", fn);
  if (!frames || B <= 0 || hop < 1) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: need frames, batch>0, hop>=1", fn);
  if (!num_frames || is_device_ptr(num_frames))
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: num_frames is a host array of batch counts", fn);
  Trajectories t;
  std::vector<int64_t> len((size_t)B), base;
  for (int32_t u = 0; u < B; ++u) {
    const int32_t F = num_frames[u];
    if (F < 2 || F > fstride)
      return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: num_frames[%d] = %d outside 2..frame_stride = %lld", fn, u, F,
                  (long long)fstride);
    t.F = std::max(t.F, F);
    len[(size_t)u] = (int64_t)(F - 1) * hop;
    t.samples += len[(size_t)u];
  }
  const afs_status s = packed_rows(c, fn, format, out, offsets, len, &base, &t.span);
  if (s != AFS_OK) return s;
  t.ostride = (int64_t)(t.F - 1) * hop;
  t.frames = frames, t.fstride = fstride, t.num_frames = num_frames;
  t.seeds = seeds, t.B = B, t.hop = hop;
  t.pcm = out, t.pstride = 0, t.format = format, t.row_base = base.data();
  return synth_core(c, t, nonfinite, rep);
}

afs_status afs_memory_info_get(afs_ctx *c, afs_memory_info *info) {
  if (!c || !info) return AFS_ERR_INVALID_ARGUMENT;
  info->total_bytes = info->sample_buffer_bytes = 0;
  for (const afs::DeviceBuf *b : c->device_bufs()) info->total_bytes += (int64_t)b->capacity();
  for (const afs::DeviceBuf *b : c->sample_bufs()) info->sample_buffer_bytes += (int64_t)b->capacity();
  return AFS_OK;
}

afs_status afs_section_currents(int32_t section, int32_t *in, int32_t out[2]) {
  if (!in || !out || !afs::section_currents(section, in, out)) return AFS_ERR_INVALID_ARGUMENT;
  return AFS_OK;
}

int32_t afs_lanes_per_utterance(const afs_ctx *c, int32_t batch) {
  if (!c || c->cfg.solver != AFS_SOLVER_TREE || batch <= 0) return 1;
  return lanes_for(c, batch);
}

const char *afs_synthesis_kernel(const afs_ctx *c, int32_t batch) {
  if (!c || c->cfg.solver != AFS_SOLVER_TREE) return "lane_synth_kernel";
  const int lanes = afs_lanes_per_utterance(c, batch);
  if (AFS_PAIR && lanes == afs::TREE_W) return "tree_pair_kernel";
  if (AFS_PAIR && lanes == afs::TREE_VOICE_W && batch <= afs::TREE_PAIR64_MAX) return "tree_pair64_kernel";
  return "tree_synth_kernel";
}

afs_status afs_kernel_times_ex(afs_ctx *c, afs_kernel_timing *t) {
  if (!c || !t) return AFS_ERR_INVALID_ARGUMENT;
  if (!(c->cfg.flags & AFS_PROFILE)) return fail(c, AFS_ERR_INVALID_ARGUMENT, "afs_kernel_times: AFS_PROFILE is off");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  double ms[3] = {0.0, 0.0, 0.0};
  int32_t n[3] = {0, 0, 0};
  for (const auto &e : c->timed) {
    float x = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&x, e.a, e.b));
    ms[e.kind] += x;
    ++n[e.kind];
  }
  const bool overflow = c->timed_overflow;
  c->timed.clear();
  c->pev_used = 0;
  c->timed_overflow = false;
  t->synth_ms = ms[0];
  t->synth_launches = n[0];
  t->plan_ms = ms[1];
  t->plan_launches = n[1];
  t->output_ms = ms[2];
  t->output_launches = n[2];
  if (overflow) return fail(c, AFS_ERR_UNSUPPORTED, "afs_kernel_times: more launches than the event pool holds");
  return AFS_OK;
}

afs_status afs_kernel_times(afs_ctx *c, double *synth_ms, int32_t *synth_launches, double *plan_ms,
                            int32_t *plan_launches) {
  afs_kernel_timing t{};
  const afs_status s = afs_kernel_times_ex(c, &t);
  if (synth_ms) *synth_ms = t.synth_ms;
  if (synth_launches) *synth_launches = t.synth_launches;
  if (plan_ms) *plan_ms = t.plan_ms;
  if (plan_launches) *plan_launches = t.plan_launches;
  return s;
}

afs_status afs_rng_draws(afs_ctx *c, int32_t B, int64_t *draws) {
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  if (!draws || B <= 0 || B != c->last_B || !c->ws.data())
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "afs_rng_draws: need draws[B] with B = the last call's batch");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  return draws_of(c, c->ws.data(), B, draws);
}

afs_status afs_noise_plans(afs_ctx *c, const afs_frame *frames, int32_t rows, int32_t F, int32_t hop, int64_t s0,
                           int64_t s1, uint64_t *plans) {
  static_assert(AFS_PLAN_WORDS * 8 == afs::PLAN_RECORD_BYTES, "afs.h / tree_plan.h record size");
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  if (!tree(c)) return fail(c, AFS_ERR_UNSUPPORTED, "afs_noise_plans: tree solver only");
  if (!frames || !plans || rows <= 0 || F < 2 || hop < 1 || s0 < 0 || s1 <= s0 || s1 > (int64_t)(F - 1) * hop)
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "afs_noise_plans: need frames, plans, rows>0, num_frames>=2, hop>=1, "
                                             "0 <= s_begin < s_end <= (num_frames-1)*hop");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  afs_status s;
  Frames fr;
  if ((s = frames_to_device(c, frames, (size_t)rows * F, &fr)) != AFS_OK) return s;
  const int64_t n = s1 - s0;
  const size_t bytes = (size_t)rows * (size_t)n * afs::PLAN_RECORD_BYTES;
  Staged<uint64_t> out;
  if ((s = out.stage(c, plans, bytes, c->plan)) != AFS_OK) return s;
  HIP_TRY(c, afs::launch_plan(plan_args(c, fr.dev, F, rows, hop, s0, s1, out.dev, n), c->stream));
  if ((s = out.copy_back(c)) != AFS_OK) return s;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return AFS_OK;
}

afs_status afs_noise_plan_hops(afs_ctx *c, const afs_frame *frames, int32_t rows, int32_t F, int32_t hop, int64_t s0,
                               int64_t s1, uint8_t *hops, uint64_t *plans) {
  static_assert(AFS_PLAN_HOP_BYTES == sizeof(afs::tree::PlanHop), "afs.h / tree_plan.h hop record size");
  static_assert(AFS_PLAN_HOP_MIN == afs::tree::PLAN_HOP_MIN, "afs.h / tree_plan.h hop mode threshold");
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  if (c->cfg.solver != AFS_SOLVER_TREE || hop < AFS_PLAN_HOP_MIN)
    return fail(c, AFS_ERR_UNSUPPORTED, "afs_noise_plan_hops: tree solver and hop >= AFS_PLAN_HOP_MIN only");
  if (!frames || !hops || !plans || rows <= 0 || F < 2 || s0 < 0 || s1 <= s0 || s1 > (int64_t)(F - 1) * hop)
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "afs_noise_plan_hops: need frames, hops, plans, rows>0, num_frames>=2, "
                                             "0 <= s_begin < s_end <= (num_frames-1)*hop");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  afs_status s;
  Frames fr;
  if ((s = frames_to_device(c, frames, (size_t)rows * F, &fr)) != AFS_OK) return s;
  const int64_t n = s1 - s0, slots = afs::plan_hop_slots(s0, s1, hop);
  const size_t pbytes = (size_t)rows * (size_t)n * afs::PLAN_RECORD_BYTES;
  const size_t hbytes = (size_t)rows * (size_t)slots * sizeof(afs::tree::PlanHop);
  Staged<uint64_t> out_plans;
  Staged<uint8_t> out_hops;
  // (uploaded first: the records of the samples outside mixed hops are left as the caller passed them)
  if ((s = out_plans.stage(c, plans, pbytes, c->plan, true)) != AFS_OK) return s;
  if ((s = out_hops.stage(c, hops, hbytes, c->hops)) != AFS_OK) return s;
  HIP_TRY(c, c->plan_work.reserve((size_t)afs::plan_work_bytes(rows, slots)));
  afs::PlanArgs pa = plan_args(c, fr.dev, F, rows, hop, s0, s1, out_plans.dev, n);
  pa.hops = (afs::tree::PlanHop *)out_hops.dev;
  pa.hop_stride = slots;
  pa.work = c->plan_work.as<uint32_t>();
  HIP_TRY(c, afs::launch_plan_hops(pa, c->stream));
  if ((s = out_plans.copy_back(c)) != AFS_OK) return s;
  if ((s = out_hops.copy_back(c)) != AFS_OK) return s;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return AFS_OK;
}

afs_status afs_plan_hop_words(afs_ctx *c, const uint8_t *hops, const double *ratio, int32_t n, uint64_t *words) {
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  if (c->cfg.solver != AFS_SOLVER_TREE) return fail(c, AFS_ERR_UNSUPPORTED, "afs_plan_hop_words: tree solver only");
  if (!hops || !ratio || !words || n <= 0)
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "afs_plan_hop_words: need hops, ratio, words, n>0");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const size_t hb = (size_t)n * sizeof(afs::tree::PlanHop), rb = (size_t)n * 8, wb = (size_t)n * AFS_PLAN_WORDS * 8;
  afs::DeviceBuf tmp;
  HIP_TRY(c, tmp.reserve(hb + rb + wb));
  char *d = tmp.as<char>();
  HIP_TRY(c, hipMemcpyAsync(d, hops, hb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d + hb, ratio, rb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, afs::launch_tree_hop_words((const afs::tree::PlanHop *)d, (const double *)(d + hb), n,
                                        (uint64_t *)(d + hb + rb), c->stream));
  HIP_TRY(c, hipMemcpyAsync(words, d + hb + rb, wb, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return AFS_OK;
}

afs_status afs_tube_interpolate(afs_ctx *c, const afs_frame *fl, const afs_frame *fr, const double *ratio, int32_t n,
                                double *area, double *length) {
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  if (c->cfg.solver != AFS_SOLVER_TREE) return fail(c, AFS_ERR_UNSUPPORTED, "afs_tube_interpolate: tree solver only");
  if (!fl || !fr || !ratio || !area || !length || n <= 0)
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "afs_tube_interpolate: need left, right, ratio, area, length, n>0");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const size_t fb = (size_t)n * sizeof(afs_frame), rb = (size_t)n * 8, ob = (size_t)n * AFS_NUM_TUBE_SECTIONS * 8;
  afs::DeviceBuf tmp;
  HIP_TRY(c, tmp.reserve(2 * fb + rb + 2 * ob));
  char *d = tmp.as<char>();
  afs_frame *dl = (afs_frame *)d, *dr = (afs_frame *)(d + fb);
  double *dratio = (double *)(d + 2 * fb), *da = (double *)(d + 2 * fb + rb), *dlen = (double *)(d + 2 * fb + rb + ob);
  HIP_TRY(c, hipMemcpyAsync(dl, fl, fb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(dr, fr, fb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(dratio, ratio, rb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemsetAsync(da, 0, 2 * ob, c->stream));
  HIP_TRY(c, afs::launch_tree_interp(c->tab(), dl, dr, dratio, n, da, dlen, c->stream));
  HIP_TRY(c, hipMemcpyAsync(area, da, ob, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(length, dlen, ob, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return AFS_OK;
}

afs_status afs_device_math(afs_ctx *c, int32_t op, const double *a, const double *b, int64_t n, double *out) {
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  if (c->cfg.solver != AFS_SOLVER_TREE) return fail(c, AFS_ERR_UNSUPPORTED, "afs_device_math: tree solver only");
  if (op < 0 || op >= AFS_MATH_OP_COUNT || !a || !b || !out || n <= 0 || n > ((int64_t)1 << 31))
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "afs_device_math: need an afs_math_op, a, b, out, 0 < n <= 2^31");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const size_t nb = (size_t)n * 8;
  afs::DeviceBuf tmp;
  HIP_TRY(c, tmp.reserve(3 * nb));
  double *da = tmp.as<double>(), *db = da + n, *dout = db + n;
  HIP_TRY(c, hipMemcpyAsync(da, a, nb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(db, b, nb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, afs::launch_device_math(op, da, db, n, dout, c->stream));
  HIP_TRY(c, hipMemcpyAsync(out, dout, nb, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return AFS_OK;
}

afs_status afs_session_create(afs_ctx *c, int32_t B, const uint32_t *seeds, afs_session **out) {
  if (!c || !out || B <= 0) return c ? fail(c, AFS_ERR_INVALID_ARGUMENT, "afs_session_create: bad args") : AFS_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  afs_session *s = new afs_session();
  s->ctx = c;
  s->B = B;
  s->bp = pad64(B);
  s->lanes = lanes_for(c, B);  // (fixed for the session: the per-lane state layout depends on it)
  auto bail = [&](hipError_t e) {
    delete s;
    return fail(c, e == hipErrorOutOfMemory ? AFS_ERR_OUT_OF_MEMORY : AFS_ERR_HIP, "session alloc: %s", hipGetErrorString(e));
  };
  hipError_t e;
  if ((e = s->ws.reserve(ws_bytes_for(c, s->bp))) != hipSuccess) return bail(e);
  if ((e = s->rng.reserve((size_t)(32 * s->bp) * sizeof(int32_t))) != hipSuccess) return bail(e);
  if (tree(c) && (e = s->tree_lanes.reserve(lanes_bytes_for(c, s->bp, s->lanes))) != hipSuccess) return bail(e);
  if ((e = s->pair.reserve((size_t)B * 2 * sizeof(afs_frame))) != hipSuccess) return bail(e);
  if ((e = s->seeds.reserve((size_t)B * sizeof(uint32_t))) != hipSuccess) return bail(e);
  if ((e = s->hframes.reserve((size_t)B * sizeof(afs_frame))) != hipSuccess) return bail(e);
  *out = s;
  afs_status st = afs_session_reset(s, seeds);
  if (st != AFS_OK) {
    afs_session_destroy(s);
    *out = nullptr;
  }
  return st;
}

afs_status afs_session_reset(afs_session *s, const uint32_t *seeds) {
  if (!s) return AFS_ERR_INVALID_ARGUMENT;
  afs_ctx *c = s->ctx;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  if (seeds) {
    hipMemcpyKind k = is_device_ptr(seeds) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIP_TRY(c, hipMemcpyAsync(s->seeds.data(), seeds, (size_t)s->B * 4, k, c->stream));
  }
  // (no seeds: the reset kernels seed voice u with u + 1)
  afs_status st = reset_state(c, s->ws.data(), s->rng.as<int32_t>(), s->tree_lanes.data(), s->bp, s->B,
                              seeds ? s->seeds.as<uint32_t>() : nullptr, s->lanes);
  if (st != AFS_OK) return st;
  s->latch.assign((size_t)s->B, 0);
  s->seed_of.assign((size_t)s->B, 0);  // (device seeds: not known here)
  if (!seeds || !is_device_ptr(seeds))
    for (int u = 0; u < s->B; ++u) s->seed_of[(size_t)u] = seeds ? seeds[u] : (uint32_t)u + 1u;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return AFS_OK;
}

void afs_session_destroy(afs_session *s) {
  delete s;
}

}  // extern "C"

// afs_session_synthesize; taps_out: afs_session_synthesize_taps, else null; pcm (out null):
// afs_session_synthesize_pcm
static afs_status session_core(afs_session *s, const afs_frame *frames, int32_t n, double *out, double *taps_out,
                               int16_t *pcm, uint8_t *nonfinite, int32_t *produced, afs_report *rep) {
  if (!s || !frames) return AFS_ERR_INVALID_ARGUMENT;
  afs_ctx *c = s->ctx;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const int B = s->B;
  // (one latch state for all voices: everything these calls could see before the voices had lives of
  // their own; the pool calls and afs_session_reset take a session from any state)
  const bool latched = s->all_latched(true);
  if (!latched && !s->all_latched(false))
    return fail(c, AFS_ERR_INVALID_ARGUMENT,
                "afs_session_synthesize: the voices differ in latch state (afs_session_restart_voices, "
                "afs_session_synthesize_ragged): use afs_session_synthesize_ragged or afs_session_reset");
  // (the kinds of the caller's pointers are probed on every call: a freed buffer's address may come
  // back as memory of the other kind; one pointer query is ~1 us beside a ~6 ms call)
  const bool in_dev = is_device_ptr(frames);
  const afs_frame *src = frames;
  if (!in_dev) {  // host frames: through the session's pinned buffer
    std::memcpy(s->hframes.data(), frames, (size_t)B * sizeof(afs_frame));
    src = s->hframes.as<afs_frame>();
  }
  const hipMemcpyKind k = in_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  // frames[u] -> pair[u][slot]
  const int slot = latched ? 1 : 0;
  afs_frame *pair = s->pair.as<afs_frame>();
  HIP_TRY(c, hipMemcpy2DAsync(pair + slot, 2 * sizeof(afs_frame), src, sizeof(afs_frame),
                              sizeof(afs_frame), B, k, c->stream));
  if (!latched) {  // Synthesizer.cpp:522-532
    s->latch.assign((size_t)B, 1);
    if (produced) *produced = 0;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (rep) { std::memset(rep, 0, sizeof *rep); rep->kernel = c->cfg.solver; }
    return AFS_OK;
  }
  if (!out && !pcm) return fail(c, AFS_ERR_INVALID_ARGUMENT, "afs_session_synthesize: out is NULL");
  if (n < 1) n = 1;  // Synthesizer.cpp:543-546
  const size_t out_bytes = (size_t)B * (size_t)n * sizeof(double), pcm_bytes = (size_t)B * (size_t)n * sizeof(int16_t);
  Staged<double> dout, dtaps;
  Staged<int16_t> dpcm;
  afs_status st;
  if ((st = dout.stage(c, out, out_bytes, c->stage_out)) != AFS_OK) return st;
  if ((st = dpcm.stage(c, pcm, pcm_bytes, c->stage_pcm)) != AFS_OK) return st;
  // (back through the session's pinned buffer)
  if (dout.host || dpcm.host) HIP_TRY(c, s->hout.reserve(dout.host ? out_bytes : pcm_bytes));
  if ((st = dtaps.stage(c, taps_out, out_bytes * (size_t)c->n_taps, c->stage_taps)) != AFS_OK) return st;
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  SynthCall call;
  call.frames = pair, call.fstride = 2, call.rows = B;
  call.ntrans = 1, call.hop = n;
  call.out = dout.dev, call.ostride = n;
  call.pcm = dpcm.dev, call.pstride = n;
  call.taps.out = dtaps.dev, call.taps.stride = n;
  call.ws = s->ws.data(), call.rng = s->rng.as<int32_t>(), call.lanes = s->tree_lanes.data();
  call.bp = s->bp, call.B = B, call.width = s->lanes;
  call.so = plain_order(c);
  if ((st = run_call(c, call)) != AFS_OK) return st;
  HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
  // prevTube = *newTube (Synthesizer.cpp:633-637)
  HIP_TRY(c, hipMemcpy2DAsync(pair, 2 * sizeof(afs_frame), pair + 1, 2 * sizeof(afs_frame),
                              sizeof(afs_frame), B, hipMemcpyDeviceToDevice, c->stream));
  bool nf_sync = false;
  if ((st = nonfinite_report(c, s->ws.data(), s->bp, B, nonfinite, rep != nullptr, &nf_sync)) != AFS_OK) return st;
  if ((st = dout.copy_back(c, s->hout.data())) != AFS_OK) return st;
  if ((st = dpcm.copy_back(c, s->hout.data())) != AFS_OK) return st;
  if ((st = dtaps.copy_back(c)) != AFS_OK) return st;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (a session call always waits: its audio is due now)
  if (dout.host) std::memcpy(out, s->hout.data(), out_bytes);
  if (dpcm.host) std::memcpy(pcm, s->hout.data(), pcm_bytes);
  if (produced) *produced = n;
  return fill_report(c, rep, (int64_t)B * n);
}

// ---- the voice pool: per-voice frame counts, idle voices and restarts on a session ----

// The launch layout of a pool call and its per-voice arrays on the device, sent as ragged_layout sends
// a ragged call's (the context's pinned buffer, one upload on the stream, the event that guards its
// reuse): block_end, the slot order and stand-ins of afs::pool_order, the transitions each voice plays
// (K5's and K6's row_hops), then the frame counts and latch flags that launch_pool_rows reads; behind them
// a packed call's row starts and an indexed call's frame start indices (launch_pool_rows_indexed).
struct PoolArrays {
  const int32_t *count = nullptr, *latched = nullptr;
  const int64_t *start = nullptr;
};
static afs_status pool_layout(afs_ctx *c, const afs_session *s, const int32_t *num_frames, const int32_t *trans, int upb,
                              int hop, SynthCall *call, PoolArrays *pa, const int64_t *row_base = nullptr,
                              const int64_t *frame_start = nullptr) {
  const int B = s->B;
  const afs::RaggedOrder ro = afs::pool_order(trans, B, upb, hop);
  const size_t slots = ro.order.size();
  const size_t end_bytes = (size_t)ro.grid * sizeof(int64_t), slot_bytes = slots * sizeof(int32_t);
  const size_t row_bytes = (size_t)B * sizeof(int32_t);
  // (a packed call's row starts and an indexed call's frame starts ride behind the per-voice arrays, on
  // an 8-byte boundary)
  const size_t base0 = (end_bytes + 2 * slot_bytes + 3 * row_bytes + 7) / 8 * 8;
  const size_t start0 = base0 + (row_base ? (size_t)B * sizeof(int64_t) : 0);
  const size_t bytes = start0 + (frame_start ? (size_t)B * sizeof(int64_t) : 0);
  if (!c->ev_ragged) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_ragged, hipEventDisableTiming));
  else HIP_TRY(c, hipEventSynchronize(c->ev_ragged));
  HIP_TRY(c, c->ragged_host.reserve(bytes));
  HIP_TRY(c, c->ragged.reserve(bytes));
  char *h = c->ragged_host.as<char>(), *d = c->ragged.as<char>();
  std::memcpy(h, ro.block_end.data(), end_bytes);
  std::memcpy(h + end_bytes, ro.order.data(), slot_bytes);
  std::memcpy(h + end_bytes + slot_bytes, ro.standin.data(), slot_bytes);
  const size_t rows0 = end_bytes + 2 * slot_bytes;
  std::memcpy(h + rows0, trans, row_bytes);
  std::memcpy(h + rows0 + row_bytes, num_frames, row_bytes);
  int32_t *lat = (int32_t *)(h + rows0 + 2 * row_bytes);
  for (int u = 0; u < B; ++u) lat[u] = s->latch[(size_t)u] ? 1 : 0;
  if (row_base) std::memcpy(h + base0, row_base, (size_t)B * sizeof(int64_t));
  if (frame_start) std::memcpy(h + start0, frame_start, (size_t)B * sizeof(int64_t));
  HIP_TRY(c, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev_ragged, c->stream));
  call->row_base = row_base ? (const int64_t *)(d + base0) : nullptr;
  call->ragged.block_end = (const int64_t *)d;
  call->so.order = (const int32_t *)(d + end_bytes);
  call->so.grid = ro.grid;
  call->ragged.pad_standin = (const int32_t *)(d + end_bytes + slot_bytes);
  call->ragged.row_hops = (const int32_t *)(d + rows0);
  pa->count = (const int32_t *)(d + rows0 + row_bytes);
  pa->latched = (const int32_t *)(d + rows0 + 2 * row_bytes);
  pa->start = frame_start ? (const int64_t *)(d + start0) : nullptr;
  return AFS_OK;
}

// afs_session_synthesize_ragged (taps_out or null), afs_session_synthesize_ragged_pcm (pcm, out null),
// afs_session_synthesize_ragged_packed (packed: pcm holds samples of `format`, voice u's at offsets[u]).
// One SynthCall on the session's state over the call's frame rows (launch_pool_rows): voice u plays
// trans[u] transitions -- its count, less one while it is unlatched -- ntrans the largest; K1's blocks
// come from pool_order, so a voice without a transition is in no slot, K5 skips its row and K6 returns
// at once: nothing of it is read or written.
// afs_session_synthesize_indexed and _indexed_packed (index: the frame source is one flat array, voice u's
// frames at index->start[u]; fstride is not looked at, a row holds the largest count): only the gather of
// the rows differs (launch_pool_rows_indexed), everything behind it is the same call.
static afs_status pool_core(afs_session *s, const char *fn, const afs_frame *frames, int64_t fstride,
                            const int32_t *num_frames, int32_t hop, double *out, int64_t ostride, double *taps_out,
                            void *pcm, int64_t pstride, bool want_pcm, uint8_t *nonfinite, int32_t *produced,
                            afs_report *rep, int32_t format = AFS_SAMPLE_I16, bool packed = false,
                            const int64_t *offsets = nullptr, const afs::FrameIndex *index = nullptr) {
  if (!s) return AFS_ERR_INVALID_ARGUMENT;
  afs_ctx *c = s->ctx;
  if (!tree(c)) return fail(c, AFS_ERR_UNSUPPORTED, "%s: tree solver only", fn);
  if (hop < 1) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: need hop>=1", fn);
  if (fstride < 0) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: need frame_stride>=0", fn);
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  if (!num_frames || is_device_ptr(num_frames))
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: num_frames is a host array of batch counts", fn);
  if (taps_out && c->n_taps <= 0) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: no taps set (afs_set_taps)", fn);
  const int B = s->B;
  afs::IndexedSpans spans;
  if (index) {
    if (index->start && is_device_ptr(index->start))
      return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: frame_start is a host array of batch indices", fn);
    const afs::IndexedCheck ic = afs::indexed_check(index->start, num_frames, B, index->total);
    if (ic.fault == afs::INDEXED_TOTAL || ic.fault == afs::INDEXED_NULL)
      return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: need total_frames >= 0 and a frame_start array", fn);
    if (ic.fault != afs::INDEXED_OK)
      return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: voice %d: frames %lld .. +%d outside 0..total_frames = %lld", fn,
                  ic.voice, (long long)index->start[ic.voice], num_frames[ic.voice], (long long)index->total);
    spans = afs::indexed_spans(index->start, num_frames, B);
    fstride = spans.longest;  // (the frames a row holds besides the latch)
  }
  std::vector<int32_t> trans((size_t)B);
  int32_t ntrans = 0;
  int64_t samples = 0;
  bool any = false;
  for (int u = 0; u < B; ++u) {
    const int32_t n = num_frames[u];
    if (n < 0 || n > fstride)
      return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: num_frames[%d] = %d outside 0..frame_stride = %lld", fn, u, n,
                  (long long)fstride);
    trans[(size_t)u] = n == 0 ? 0 : (s->latch[(size_t)u] ? n : n - 1);
    ntrans = std::max(ntrans, trans[(size_t)u]);
    samples += (int64_t)trans[(size_t)u] * hop;
    any |= n > 0;
  }
  const int64_t Tmax = (int64_t)ntrans * hop;
  if (any && !frames) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: frames is NULL", fn);
  // (a packed call: the rows at the caller's offsets, or tight in voice order; an idle voice has no row)
  std::vector<int64_t> row_base;
  int64_t span = 0;
  if (packed) {
    std::vector<int64_t> len((size_t)B);
    for (int u = 0; u < B; ++u) len[(size_t)u] = num_frames[u] == 0 ? -1 : (int64_t)trans[(size_t)u] * hop;
    const afs_status ps = packed_rows(c, fn, format, pcm, offsets, len, &row_base, &span);
    if (ps != AFS_OK) return ps;
  } else if (want_pcm) {
    if (pstride < Tmax)
      return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: pcm_stride %lld below the %lld samples a voice produces", fn,
                  (long long)pstride, (long long)Tmax);
    if (Tmax > 0 && (!pcm || (reinterpret_cast<uintptr_t>(pcm) & 1)))
      return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: pcm is NULL or not int16-aligned", fn);
  } else {
    if (ostride < Tmax)
      return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: out_stride %lld below the %lld samples a voice produces", fn,
                  (long long)ostride, (long long)Tmax);
    if (Tmax > 0 && !out) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: out is NULL", fn);
  }
  auto done = [&](int64_t n) {
    for (int u = 0; u < B; ++u) {
      if (produced) produced[u] = (int32_t)((int64_t)trans[(size_t)u] * hop);
      if (num_frames[u] > 0) s->latch[(size_t)u] = 1;
    }
    return n;
  };
  if (!any) {  // every voice idle: nothing is queued
    done(0);
    if (rep) { std::memset(rep, 0, sizeof *rep); rep->kernel = c->cfg.solver; }
    return AFS_OK;
  }
  afs_status st;
  // the frames on the device, 16-byte aligned (a host array, or device memory at another alignment,
  // through the context's staging buffer)
  Frames fr;
  const size_t fbytes = (size_t)B * (size_t)fstride * sizeof(afs_frame);
  std::vector<int64_t> start;  // an indexed call: where the gather finds each voice's frames in fr.dev
  if (index) {
    start.resize((size_t)B);
    if (!is_device_ptr(frames)) {
      // a host corpus: the live spans alone, back to back through the session's pinned buffer, one upload
      const size_t live_bytes = (size_t)spans.sum * sizeof(afs_frame);
      HIP_TRY(c, s->hframes.reserve(live_bytes));
      HIP_TRY(c, c->stage_in.reserve(live_bytes));
      afs::indexed_compact(frames, index->start, num_frames, B, s->hframes.as<afs_frame>(), start.data());
      HIP_TRY(c, hipMemcpyAsync(c->stage_in.data(), s->hframes.data(), live_bytes, hipMemcpyHostToDevice, c->stream));
      fr.dev = c->stage_in.as<const afs_frame>();
    } else if (reinterpret_cast<uintptr_t>(frames) & 15) {
      // (device memory at another alignment: the hull of the live spans through the staging buffer)
      const size_t hull_bytes = (size_t)(spans.end - spans.first) * sizeof(afs_frame);
      HIP_TRY(c, c->stage_in.reserve(hull_bytes));
      HIP_TRY(c, hipMemcpyAsync(c->stage_in.data(), frames + spans.first, hull_bytes, hipMemcpyDeviceToDevice, c->stream));
      afs::indexed_rebase(index->start, num_frames, B, spans.first, start.data());
      fr.dev = c->stage_in.as<const afs_frame>();
    } else {  // read in place
      afs::indexed_rebase(index->start, num_frames, B, 0, start.data());
      fr.dev = frames;
    }
  } else if (is_device_ptr(frames) && (reinterpret_cast<uintptr_t>(frames) & 15)) {
    HIP_TRY(c, c->stage_in.reserve(fbytes));
    HIP_TRY(c, hipMemcpyAsync(c->stage_in.data(), frames, fbytes, hipMemcpyDeviceToDevice, c->stream));
    fr.dev = c->stage_in.as<const afs_frame>();
  } else if ((st = frames_to_device(c, frames, (size_t)B * (size_t)fstride, &fr)) != AFS_OK) {
    return st;
  }
  SynthCall call;
  PoolArrays pa;
  const int upb = s->lanes == afs::TREE_VOICE_W ? 1 : afs::TREE_UPB;
  call.so = plain_order(c);
  if ((st = pool_layout(c, s, num_frames, trans.data(), upb, hop, &call, &pa, packed ? row_base.data() : nullptr,
                        index ? start.data() : nullptr)) != AFS_OK)
    return st;
  const size_t had = c->pool_rows.capacity();
  HIP_TRY(c, c->pool_rows.reserve((size_t)B * (size_t)(fstride + 1) * sizeof(afs_frame)));
  // (a new block once, zeroed: K5 stages frame 0 of every row of a block's run, a voice's without a
  // transition included, and never uses it)
  if (c->pool_rows.capacity() != had) HIP_TRY(c, hipMemsetAsync(c->pool_rows.data(), 0, c->pool_rows.capacity(), c->stream));
  afs_frame *rows = c->pool_rows.as<afs_frame>();
  if (index)
    HIP_TRY(c, afs::launch_pool_rows_indexed(fr.dev, pa.start, fstride, pa.count, pa.latched, B, rows,
                                             s->pair.as<afs_frame>(), c->stream));
  else
    HIP_TRY(c, afs::launch_pool_rows(fr.dev, fstride, pa.count, pa.latched, B, rows, s->pair.as<afs_frame>(), c->stream));
  if (ntrans == 0) {  // the voices that got frames only latch: no synthesis kernel runs
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    done(0);
    if (rep) { std::memset(rep, 0, sizeof *rep); rep->kernel = c->cfg.solver; }
    return AFS_OK;
  }
  // (a host out, taps_out or pcm goes up first and comes back whole: what lies outside the samples a
  // voice produces is the caller's)
  Staged<double> dout, dtaps;
  Staged<char> dpcm;
  const size_t out_bytes = (size_t)B * (size_t)ostride * sizeof(double);
  if ((st = dout.stage(c, out, out_bytes, c->stage_out, true)) != AFS_OK) return st;
  if ((st = dtaps.stage(c, taps_out, out_bytes * (size_t)c->n_taps, c->stage_taps, true)) != AFS_OK) return st;
  const size_t pcm_samples = packed ? (size_t)span : (size_t)(B - 1) * (size_t)pstride + (size_t)Tmax;
  if ((st = dpcm.stage(c, (char *)pcm, pcm_samples * sample_bytes(format), c->stage_pcm, true)) != AFS_OK) return st;
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  call.frames = rows, call.fstride = fstride + 1, call.rows = B;
  call.ntrans = ntrans, call.hop = hop;
  call.out = dout.dev, call.ostride = ostride;
  call.pcm = dpcm.dev, call.pstride = pstride, call.format = format;
  call.taps.out = dtaps.dev, call.taps.stride = ostride;
  call.ws = s->ws.data(), call.rng = s->rng.as<int32_t>(), call.lanes = s->tree_lanes.data();
  call.bp = s->bp, call.B = B, call.width = s->lanes;
  if ((st = run_call(c, call)) != AFS_OK) return st;
  HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
  bool nf_sync = false;
  if ((st = nonfinite_report(c, s->ws.data(), s->bp, B, nonfinite, rep != nullptr, &nf_sync)) != AFS_OK) return st;
  if ((st = dout.copy_back(c)) != AFS_OK) return st;
  if ((st = dpcm.copy_back(c)) != AFS_OK) return st;
  if ((st = dtaps.copy_back(c)) != AFS_OK) return st;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (a session call always waits: its audio is due now)
  return fill_report(c, rep, done(samples));
}

// ---- voice records: a voice's state out of its slot, into another, or into many (afs_voice_state.h) ----

// the header of a record of this session: what every record loaded into it must carry, and with the
// voice's latch flag and seed what a saved one does
static afs::VoiceStateHeader voice_header(const afs_session *s, bool latched, uint32_t seed) {
  const afs::VoiceStateLayout L = afs::voice_state_layout_for(s->lanes);
  const afs_config &cfg = s->ctx->cfg;
  return afs::voice_state_header(s->lanes, L.bytes[0] / s->lanes, L.bytes[1] / (int64_t)sizeof(double),
                                 cfg.sampling_rate_hz, cfg.options, latched, seed);
}

static afs::VoiceStateBuffers voice_buffers(const afs_session *s) {
  return {s->tree_lanes.as<char>(), s->ws.as<char>(), s->pair.as<char>()};
}

// a host list of n voices of the session, each listed once when `distinct`
static afs_status voice_list_check(afs_ctx *c, const char *fn, const char *what, const afs_session *s,
                                   const int32_t *voices, int32_t n, bool distinct) {
  if (is_device_ptr(voices)) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: %s is a host array", fn, what);
  std::vector<uint8_t> listed((size_t)s->B, 0);
  for (int32_t i = 0; i < n; ++i) {
    const int32_t v = voices[i];
    if (v < 0 || v >= s->B)
      return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: %s[%d] = %d outside 0..%d", fn, what, i, v, s->B - 1);
    if (distinct && listed[(size_t)v]) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: voice %d listed twice in %s", fn, v, what);
    listed[(size_t)v] = 1;
  }
  return AFS_OK;
}

// The context's pinned buffer for a call's small host arrays (as pool_layout uses it): at least `bytes`,
// free to rewrite once the last upload from it has been read.  The caller records ev_ragged behind its
// own copies.
static afs_status pinned_lists(afs_ctx *c, size_t bytes, char **h) {
  if (!c->ev_ragged) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_ragged, hipEventDisableTiming));
  else HIP_TRY(c, hipEventSynchronize(c->ev_ragged));
  HIP_TRY(c, c->ragged_host.reserve(bytes));
  *h = c->ragged_host.as<char>();
  return AFS_OK;
}

// what save and load check before they touch anything (n == 0 passes: the caller then returns at once)
static afs_status voice_state_args(afs_session *s, const char *fn, const int32_t *voices, int32_t n, const void *state,
                                   bool *state_dev) {
  afs_ctx *c = s->ctx;
  if (!tree(c)) return fail(c, AFS_ERR_UNSUPPORTED, "%s: tree solver only", fn);
  if (n < 0 || (n > 0 && (!voices || !state)))
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: need n >= 0 voices and their records", fn);
  if (n == 0) return AFS_OK;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const afs_status st = voice_list_check(c, fn, "voices", s, voices, n, true);
  if (st != AFS_OK) return st;
  *state_dev = is_device_ptr(state);
  if (*state_dev && (reinterpret_cast<uintptr_t>(state) & 15))
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: device records are 16-byte aligned", fn);
  return AFS_OK;
}

extern "C" {

afs_status afs_session_synthesize(afs_session *s, const afs_frame *frames, int32_t n, double *out,
                                  uint8_t *nonfinite, int32_t *produced, afs_report *rep) {
  return session_core(s, frames, n, out, nullptr, nullptr, nonfinite, produced, rep);
}

// (one lane per utterance: no PCM form, as for the whole-trajectory calls; the latching first call
// writes nothing and does not look at pcm)
afs_status afs_session_synthesize_pcm(afs_session *s, const afs_frame *frames, int32_t n, int16_t *pcm,
                                      uint8_t *nonfinite, int32_t *produced, afs_report *rep) {
  if (!s) return AFS_ERR_INVALID_ARGUMENT;
  if (!tree(s->ctx)) return fail(s->ctx, AFS_ERR_UNSUPPORTED, "afs_session_synthesize_pcm: tree solver only");
  if (s->all_latched(true) && (!pcm || (reinterpret_cast<uintptr_t>(pcm) & 1)))
    return fail(s->ctx, AFS_ERR_INVALID_ARGUMENT, "afs_session_synthesize_pcm: pcm is NULL or not int16-aligned");
  return session_core(s, frames, n, nullptr, nullptr, pcm, nonfinite, produced, rep);
}

// (the latching first call produces no samples and leaves taps_out alone, as it leaves out)
afs_status afs_session_synthesize_taps(afs_session *s, const afs_frame *frames, int32_t n, double *out,
                                       double *taps_out, uint8_t *nonfinite, int32_t *produced, afs_report *rep) {
  if (!s) return AFS_ERR_INVALID_ARGUMENT;
  const afs_status st = taps_check(s->ctx, "afs_session_synthesize_taps", taps_out);
  if (st != AFS_OK) return st;
  return session_core(s, frames, n, out, taps_out, nullptr, nonfinite, produced, rep);
}

afs_status afs_session_rng_draws(afs_session *s, int64_t *draws) {
  if (!s || !draws) return AFS_ERR_INVALID_ARGUMENT;
  afs_ctx *c = s->ctx;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  return draws_of(c, s->ws.data(), s->B, draws);
}

afs_status afs_session_restart_voices(afs_session *s, const int32_t *voices, const uint32_t *seeds, int32_t n) {
  if (!s) return AFS_ERR_INVALID_ARGUMENT;
  afs_ctx *c = s->ctx;
  const char *fn = "afs_session_restart_voices";
  if (!tree(c)) return fail(c, AFS_ERR_UNSUPPORTED, "%s: tree solver only", fn);
  if (n < 0 || (n > 0 && !voices)) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: need n >= 0 voices", fn);
  if (n == 0) return AFS_OK;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  if (is_device_ptr(voices) || (seeds && is_device_ptr(seeds)))
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: voices and seeds are host arrays", fn);
  std::vector<uint8_t> listed((size_t)s->B, 0);
  for (int32_t i = 0; i < n; ++i) {
    const int32_t v = voices[i];
    if (v < 0 || v >= s->B) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: voices[%d] = %d outside 0..%d", fn, i, v, s->B - 1);
    if (listed[(size_t)v]) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: voice %d listed twice", fn, v);
    listed[(size_t)v] = 1;
  }
  // the two lists through the context's pinned buffer, as a pool call's arrays (pool_layout)
  const size_t lb = (size_t)n * sizeof(int32_t), bytes = seeds ? 2 * lb : lb;
  if (!c->ev_ragged) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_ragged, hipEventDisableTiming));
  else HIP_TRY(c, hipEventSynchronize(c->ev_ragged));
  HIP_TRY(c, c->ragged_host.reserve(bytes));
  HIP_TRY(c, c->pool_list.reserve(bytes));
  char *h = c->ragged_host.as<char>(), *d = c->pool_list.as<char>();
  std::memcpy(h, voices, lb);
  if (seeds) std::memcpy(h + lb, seeds, lb);
  HIP_TRY(c, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev_ragged, c->stream));
  HIP_TRY(c, afs::launch_voice_reset(s->tree_lanes.data(), s->ws.as<double>(), (const int32_t *)d,
                                     seeds ? (const uint32_t *)(d + lb) : nullptr, n, s->lanes, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int32_t i = 0; i < n; ++i) {
    s->latch[(size_t)voices[i]] = 0;
    s->seed_of[(size_t)voices[i]] = seeds ? seeds[i] : (uint32_t)voices[i] + 1u;
  }
  return AFS_OK;
}

afs_status afs_session_latched(afs_session *s, uint8_t *flags) {
  if (!s || !flags) return AFS_ERR_INVALID_ARGUMENT;
  for (int u = 0; u < s->B; ++u) flags[u] = s->latch[(size_t)u] ? 1 : 0;
  return AFS_OK;
}

int64_t afs_session_voice_state_bytes(const afs_session *s) {
  if (!s || !tree(s->ctx)) return 0;
  return afs::voice_state_layout_for(s->lanes).record_bytes;
}

// The headers are written here, into the pinned buffer behind the voice list, and copied to the front
// of each record; the gather fills in the payloads behind them.  A host `state` gets the records from
// the context's staging buffer, whole.
afs_status afs_session_save_voices(afs_session *s, const int32_t *voices, int32_t n, void *state) {
  if (!s) return AFS_ERR_INVALID_ARGUMENT;
  afs_ctx *c = s->ctx;
  const char *fn = "afs_session_save_voices";
  bool dev = false;
  afs_status st = voice_state_args(s, fn, voices, n, state, &dev);
  if (st != AFS_OK || n == 0) return st;
  const size_t rb = (size_t)afs::voice_state_layout_for(s->lanes).record_bytes;
  const size_t lb = (size_t)afs::voice_state_pad16((int64_t)n * 4), hb = (size_t)n * sizeof(afs::VoiceStateHeader);
  char *h = nullptr;
  if ((st = pinned_lists(c, lb + hb, &h)) != AFS_OK) return st;
  std::memcpy(h, voices, (size_t)n * sizeof(int32_t));
  for (int32_t i = 0; i < n; ++i) {
    const size_t v = (size_t)voices[i];
    const afs::VoiceStateHeader hdr = voice_header(s, s->latch[v] != 0, s->seed_of[v]);
    std::memcpy(h + lb + (size_t)i * sizeof hdr, &hdr, sizeof hdr);
  }
  HIP_TRY(c, c->pool_list.reserve(lb));
  char *records = static_cast<char *>(state);
  if (!dev) {
    HIP_TRY(c, c->voice_stage.reserve((size_t)n * rb));
    records = c->voice_stage.as<char>();
  }
  HIP_TRY(c, hipMemcpyAsync(c->pool_list.data(), h, lb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpy2DAsync(records, rb, h + lb, sizeof(afs::VoiceStateHeader), sizeof(afs::VoiceStateHeader),
                              (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev_ragged, c->stream));
  HIP_TRY(c, afs::launch_voice_gather(voice_buffers(s), c->pool_list.as<int32_t>(), n, s->lanes, records, c->stream));
  if (!dev) HIP_TRY(c, hipMemcpyAsync(state, records, (size_t)n * rb, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return AFS_OK;
}

// Every header is read (a device state's through the pinned buffer, with a wait) and checked against
// the session's own before anything is written; then the upload of host records and the scatter.
afs_status afs_session_load_voices(afs_session *s, const int32_t *voices, int32_t n, const void *state) {
  if (!s) return AFS_ERR_INVALID_ARGUMENT;
  afs_ctx *c = s->ctx;
  const char *fn = "afs_session_load_voices";
  bool dev = false;
  afs_status st = voice_state_args(s, fn, voices, n, state, &dev);
  if (st != AFS_OK || n == 0) return st;
  const size_t rb = (size_t)afs::voice_state_layout_for(s->lanes).record_bytes;
  const size_t lb = (size_t)afs::voice_state_pad16((int64_t)n * 4), hb = (size_t)n * sizeof(afs::VoiceStateHeader);
  char *h = nullptr;
  if ((st = pinned_lists(c, lb + hb, &h)) != AFS_OK) return st;
  std::vector<afs::VoiceStateHeader> hdr((size_t)n);
  if (dev) {
    HIP_TRY(c, hipMemcpy2DAsync(h + lb, sizeof(afs::VoiceStateHeader), state, rb, sizeof(afs::VoiceStateHeader),
                                (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::memcpy(hdr.data(), h + lb, hb);
  } else {
    for (int32_t i = 0; i < n; ++i)
      std::memcpy(&hdr[(size_t)i], static_cast<const char *>(state) + (size_t)i * rb, sizeof(afs::VoiceStateHeader));
  }
  const afs::VoiceStateHeader want = voice_header(s, false, 0);
  for (int32_t i = 0; i < n; ++i)
    if (const char *why = afs::voice_state_mismatch(hdr[(size_t)i], want))
      return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: record %d does not fit this session: %s", fn, i, why);
  std::memcpy(h, voices, (size_t)n * sizeof(int32_t));
  HIP_TRY(c, c->pool_list.reserve(lb));
  const char *records = static_cast<const char *>(state);
  if (!dev) {
    HIP_TRY(c, c->voice_stage.reserve((size_t)n * rb));
    HIP_TRY(c, hipMemcpyAsync(c->voice_stage.data(), state, (size_t)n * rb, hipMemcpyHostToDevice, c->stream));
    records = c->voice_stage.as<char>();
  }
  HIP_TRY(c, hipMemcpyAsync(c->pool_list.data(), h, lb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev_ragged, c->stream));
  HIP_TRY(c, afs::launch_voice_scatter(voice_buffers(s), c->pool_list.as<int32_t>(), n, s->lanes, records, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int32_t i = 0; i < n; ++i) {
    s->latch[(size_t)voices[i]] = hdr[(size_t)i].latched ? 1 : 0;
    s->seed_of[(size_t)voices[i]] = hdr[(size_t)i].seed;
  }
  return AFS_OK;
}

// A gather of the sources into the context's staging buffer, then a scatter into the destinations: on
// one stream, so every source is read before any destination is written (a swap on one session).
afs_status afs_session_copy_voices(afs_session *dst, const int32_t *dst_voices, afs_session *src,
                                   const int32_t *src_voices, int32_t n) {
  if (!dst || !src) return AFS_ERR_INVALID_ARGUMENT;
  afs_ctx *c = dst->ctx;
  const char *fn = "afs_session_copy_voices";
  if (!tree(c)) return fail(c, AFS_ERR_UNSUPPORTED, "%s: tree solver only", fn);
  if (src->ctx != c) return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: the sessions belong to different contexts", fn);
  if (src->lanes != dst->lanes)
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: the sessions differ in lane width (%d, %d)", fn, src->lanes, dst->lanes);
  if (n < 0 || (n > 0 && (!dst_voices || !src_voices)))
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "%s: need n >= 0 voices in both lists", fn);
  if (n == 0) return AFS_OK;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  afs_status st;
  if ((st = voice_list_check(c, fn, "dst_voices", dst, dst_voices, n, true)) != AFS_OK) return st;
  if ((st = voice_list_check(c, fn, "src_voices", src, src_voices, n, false)) != AFS_OK) return st;
  const size_t rb = (size_t)afs::voice_state_layout_for(dst->lanes).record_bytes;
  const size_t lb = (size_t)afs::voice_state_pad16((int64_t)n * 4);
  char *h = nullptr;
  if ((st = pinned_lists(c, 2 * lb, &h)) != AFS_OK) return st;
  std::memcpy(h, src_voices, (size_t)n * sizeof(int32_t));
  std::memcpy(h + lb, dst_voices, (size_t)n * sizeof(int32_t));
  HIP_TRY(c, c->pool_list.reserve(2 * lb));
  HIP_TRY(c, c->voice_stage.reserve((size_t)n * rb));
  char *d = c->pool_list.as<char>();
  HIP_TRY(c, hipMemcpyAsync(d, h, 2 * lb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev_ragged, c->stream));
  HIP_TRY(c, afs::launch_voice_gather(voice_buffers(src), (const int32_t *)d, n, src->lanes, c->voice_stage.data(), c->stream));
  HIP_TRY(c, afs::launch_voice_scatter(voice_buffers(dst), (const int32_t *)(d + lb), n, dst->lanes,
                                       c->voice_stage.data(), c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::vector<uint8_t> lat((size_t)n);
  std::vector<uint32_t> seed((size_t)n);
  for (int32_t i = 0; i < n; ++i) lat[(size_t)i] = src->latch[(size_t)src_voices[i]], seed[(size_t)i] = src->seed_of[(size_t)src_voices[i]];
  for (int32_t i = 0; i < n; ++i) dst->latch[(size_t)dst_voices[i]] = lat[(size_t)i], dst->seed_of[(size_t)dst_voices[i]] = seed[(size_t)i];
  return AFS_OK;
}

afs_status afs_session_synthesize_ragged(afs_session *s, const afs_frame *frames, int64_t frame_stride,
                                         const int32_t *num_frames, int32_t hop, double *out, int64_t out_stride,
                                         double *taps_out, uint8_t *nonfinite, int32_t *produced, afs_report *rep) {
  return pool_core(s, "afs_session_synthesize_ragged", frames, frame_stride, num_frames, hop, out, out_stride, taps_out,
                   nullptr, 0, false, nonfinite, produced, rep);
}

afs_status afs_session_synthesize_ragged_pcm(afs_session *s, const afs_frame *frames, int64_t frame_stride,
                                             const int32_t *num_frames, int32_t hop, int16_t *pcm, int64_t pcm_stride,
                                             uint8_t *nonfinite, int32_t *produced, afs_report *rep) {
  return pool_core(s, "afs_session_synthesize_ragged_pcm", frames, frame_stride, num_frames, hop, nullptr, 0, nullptr,
                   pcm, pcm_stride, true, nonfinite, produced, rep);
}

afs_status afs_session_synthesize_ragged_packed(afs_session *s, const afs_frame *frames, int64_t frame_stride,
                                                const int32_t *num_frames, int32_t hop, int32_t format, void *out,
                                                const int64_t *offsets, uint8_t *nonfinite, int32_t *produced,
                                                afs_report *rep) {
  return pool_core(s, "afs_session_synthesize_ragged_packed", frames, frame_stride, num_frames, hop, nullptr, 0, nullptr,
                   out, 0, true, nonfinite, produced, rep, format, true, offsets);
}

afs_status afs_session_synthesize_indexed(afs_session *s, const afs_frame *frames, int64_t total_frames,
                                          const int64_t *frame_start, const int32_t *num_frames, int32_t hop,
                                          double *out, int64_t out_stride, double *taps_out, uint8_t *nonfinite,
                                          int32_t *produced, afs_report *rep) {
  const afs::FrameIndex index{frame_start, total_frames};
  return pool_core(s, "afs_session_synthesize_indexed", frames, 0, num_frames, hop, out, out_stride, taps_out, nullptr, 0,
                   false, nonfinite, produced, rep, AFS_SAMPLE_I16, false, nullptr, &index);
}

afs_status afs_session_synthesize_indexed_packed(afs_session *s, const afs_frame *frames, int64_t total_frames,
                                                 const int64_t *frame_start, const int32_t *num_frames, int32_t hop,
                                                 int32_t format, void *out, const int64_t *offsets, uint8_t *nonfinite,
                                                 int32_t *produced, afs_report *rep) {
  const afs::FrameIndex index{frame_start, total_frames};
  return pool_core(s, "afs_session_synthesize_indexed_packed", frames, 0, num_frames, hop, nullptr, 0, nullptr, out, 0,
                   true, nonfinite, produced, rep, format, true, offsets, &index);
}

afs_status afs_af_to_frames(afs_ctx *c, const double *params, int64_t n, afs_frame *frames) {
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  if (!params || !frames || n <= 0) return fail(c, AFS_ERR_INVALID_ARGUMENT, "afs_af_to_frames: bad args");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  afs::DeviceBuf tmp_p, tmp_f;  // (freed on every return path)
  Staged<const double> dp;
  Staged<afs_frame> df;
  afs_status s;
  if ((s = dp.stage(c, params, (size_t)n * 16 * sizeof(double), tmp_p, true)) != AFS_OK) return s;
  // (uploaded first: what the kernel leaves alone of a frame stays the caller's)
  if ((s = df.stage(c, frames, (size_t)n * sizeof(afs_frame), tmp_f, true)) != AFS_OK) return s;
  HIP_TRY(c, afs::launch_af_to_frames(dp.dev, n, df.dev, c->stream));
  if ((s = df.copy_back(c)) != AFS_OK) return s;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return AFS_OK;
}

afs_status afs_to_int16(afs_ctx *c, const double *samples, int64_t n, int16_t *out) {
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AFS_OK;  // empty views may carry null pointers
  if (!samples || !out || n < 0) return fail(c, AFS_ERR_INVALID_ARGUMENT, "afs_to_int16: bad args");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  afs::DeviceBuf tmp_in, tmp_out;  // (freed on every return path)
  Staged<const double> din;
  Staged<int16_t> dout;
  afs_status s;
  if ((s = din.stage(c, samples, (size_t)n * sizeof(double), tmp_in, true)) != AFS_OK) return s;
  if ((s = dout.stage(c, out, (size_t)n * sizeof(int16_t), tmp_out)) != AFS_OK) return s;
  HIP_TRY(c, afs::launch_to_int16(din.dev, dout.dev, n, c->stream));
  if ((s = dout.copy_back(c)) != AFS_OK) return s;
  if (din.host || dout.host || !(c->cfg.flags & AFS_ASYNC)) HIP_TRY(c, hipStreamSynchronize(c->stream));
  return AFS_OK;
}

// ---- Synthesizer::playTargetSequence (Synthesizer.cpp:1299-1422) -------------------------

void afs_target_sequence_default(afs_target_sequence *ts) {
  if (!ts) return;
  static const double st[4] = {0.2, 0.05, 0.2, 0.1}, tr[3] = {0.05, 0.05, 0.05}, f0[4] = {100, 115, 105, 80};
  static const double g[6] = {120.0, 10000.0, 0.01, 0.01, 0.0, -40.0};
  std::memcpy(ts->stationary_s, st, sizeof st);
  std::memcpy(ts->transition_s, tr, sizeof tr);
  std::memcpy(ts->f0_hz, f0, sizeof f0);
  ts->lung_pressure_dpa = 8000.0;
  std::memcpy(ts->glottis, g, sizeof g);
}

static void target_bounds(const afs_target_sequence *ts, double *b) {  // :1318-1326, left to right
  const double *s = ts->stationary_s, *t = ts->transition_s;
  b[0] = s[0];
  b[1] = s[0] + t[0];
  b[2] = s[0] + t[0] + s[1];
  b[3] = s[0] + t[0] + s[1] + t[1];
  b[4] = s[0] + t[0] + s[1] + t[1] + s[2];
  b[5] = s[0] + t[0] + s[1] + t[1] + s[2] + t[2];
  b[6] = s[0] + t[0] + s[1] + t[1] + s[2] + t[2] + s[3];
}

int64_t afs_target_sequence_samples(const afs_target_sequence *ts, double fs) {
  if (!ts || !(fs > 0.0)) return -1;
  double b[7];
  target_bounds(ts, b);
  const double n = fs * b[6];
  if (!(n >= 0.0) || n >= 2147483647.0) return -1;
  return (int64_t)(int)n;  // int numSamples = SAMPLING_RATE * totalTime_s
}

afs_status afs_play_target_sequences(afs_ctx *c, const double *shapes, int32_t num_shapes, const int32_t *targets,
                                     const afs_target_sequence *ts, const uint32_t *seeds, int32_t B, double *out,
                                     uint8_t *nonfinite, afs_report *rep) {
  if (!c) return AFS_ERR_INVALID_ARGUMENT;
  if (!shapes || num_shapes <= 0 || !targets || !ts || B <= 0 || !out)
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "afs_play_target_sequences: need shapes, targets, timing, batch>0, out");
  if (is_device_ptr(shapes) || is_device_ptr(targets))
    return fail(c, AFS_ERR_INVALID_ARGUMENT, "afs_play_target_sequences: shapes and targets are host arrays");
  const double fs = c->cfg.sampling_rate_hz;
  const int64_t T = afs_target_sequence_samples(ts, fs);
  if (T < 0) return fail(c, AFS_ERR_INVALID_ARGUMENT, "afs_play_target_sequences: bad timing");
  for (int64_t k = 0; k < (int64_t)B * 4; ++k)
    if (targets[k] < 0 || targets[k] >= num_shapes)
      return fail(c, AFS_ERR_INVALID_ARGUMENT, "afs_play_target_sequences: target %lld out of range", (long long)k);
  if (rep) std::memset(rep, 0, sizeof *rep);
  if (T == 0) {
    if (nonfinite) {
      if (is_device_ptr(nonfinite)) HIP_TRY(c, hipMemset(nonfinite, 0, (size_t)B));
      else std::memset(nonfinite, 0, (size_t)B);
    }
    return AFS_OK;
  }
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  // one tube trajectory per distinct sequence of four shapes
  std::map<std::array<int32_t, 4>, int32_t> uniq;
  std::vector<int32_t> row((size_t)B);
  std::vector<double> seq;
  for (int32_t b = 0; b < B; ++b) {
    const std::array<int32_t, 4> key{targets[4 * b], targets[4 * b + 1], targets[4 * b + 2], targets[4 * b + 3]};
    auto it = uniq.find(key);
    if (it == uniq.end()) {
      it = uniq.emplace(key, (int32_t)uniq.size()).first;
      for (int j = 0; j < 4; ++j) seq.insert(seq.end(), shapes + 16 * (int64_t)key[j], shapes + 16 * (int64_t)key[j] + 16);
    }
    row[(size_t)b] = it->second;
  }
  const int Q = (int)uniq.size();
  afs::TargetPlan plan{};
  target_bounds(ts, plan.b);
  plan.fs = fs;
  std::memcpy(plan.f0, ts->f0_hz, sizeof plan.f0);
  plan.P = ts->lung_pressure_dpa;
  std::memcpy(plan.glottis, ts->glottis, sizeof plan.glottis);
  {  // the last sample below 0.1 fs: its fade-in value is held until the fade-out
    int64_t j = (int64_t)std::ceil((double)0.1 * fs);
    while (j >= 0 && !((double)j < (double)0.1 * fs)) --j;
    while ((double)(j + 1) < (double)0.1 * fs) ++j;
    plan.hold_j = j;
  }
  afs_status s;
  const int width = lanes_for(c, B);
  // tree solver: the XCD-aware slot order of the utterances by trajectory (xcd_order)
  std::vector<int32_t> order;
  if (tree(c)) {
    const int upb = width == afs::TREE_VOICE_W ? 1 : afs::TREE_UPB;
    // blocks the GPU holds at once: the voice kernel one wave (block) per SIMD, the throughput
    // kernel one wave per SIMD in blocks of TREE_WPB waves (4 / TREE_WPB blocks per CU, its LDS)
    const int conc = width == afs::TREE_VOICE_W ? c->simds : c->simds / afs::TREE_WPB;
    order = afs::xcd_order(row, B, upb, conc);
  }
  const size_t seq_bytes = seq.size() * sizeof(double);
  const size_t row_bytes = (size_t)B * sizeof(int32_t), ord_bytes = order.size() * sizeof(int32_t);
  HIP_TRY(c, c->tgt.reserve(seq_bytes + row_bytes + ord_bytes));
  double *dseq = c->tgt.as<double>();
  int32_t *drow = (int32_t *)(c->tgt.as<char>() + seq_bytes);
  int32_t *dord = order.empty() ? nullptr : (int32_t *)(c->tgt.as<char>() + seq_bytes + row_bytes);
  HIP_TRY(c, hipMemcpyAsync(dseq, seq.data(), seq_bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(drow, row.data(), row_bytes, hipMemcpyHostToDevice, c->stream));
  if (dord) HIP_TRY(c, hipMemcpyAsync(dord, order.data(), ord_bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the host vectors die with this call
  Seeds dseeds;
  Staged<double> dout;
  if ((s = seeds_to_device(c, seeds, B, &dseeds)) != AFS_OK) return s;
  if ((s = dout.stage(c, out, (size_t)B * (size_t)T * sizeof(double), c->stage_out)) != AFS_OK) return s;
  if ((s = fresh_state(c, B, width, dseeds.dev)) != AFS_OK) return s;
  // time chunks of Tc samples: Tc + 1 frames per sequence (the first repeats the previous
  // chunk's last), at most 1 GiB of frames
  const int64_t budget = (int64_t)1 << 30;
  const int64_t Tc = std::max<int64_t>(1, std::min<int64_t>({T, 65536, budget / ((int64_t)Q * (int64_t)sizeof(afs_frame)) - 1}));
  HIP_TRY(c, c->stage_in.reserve((size_t)Q * (size_t)(Tc + 1) * sizeof(afs_frame)));
  afs_frame *dframes = c->stage_in.as<afs_frame>();
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  for (int64_t k0 = 0; k0 < T; k0 += Tc) {
    const int nk = (int)std::min<int64_t>(Tc, T - k0);
    HIP_TRY(c, afs::launch_target_frames(dseq, Q, plan, k0, nk + 1, Tc + 1, dframes, c->stream));
    SynthCall call = context_call(c, B, width);
    call.frames = dframes, call.fstride = Tc + 1, call.rows = Q, call.frame_row = drow;
    call.ntrans = nk, call.hop = 1;
    call.out = dout.dev + k0, call.ostride = T;
    call.so.order = dord;
    if ((s = run_call(c, call)) != AFS_OK) return s;
  }
  return finish_call(c, B, (int64_t)B * T, dout, Staged<double>{}, nonfinite, rep, (c->cfg.flags & AFS_ASYNC) != 0);
}

}  // extern "C"
