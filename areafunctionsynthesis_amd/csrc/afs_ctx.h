// afs_ctx.h -- the library's internal context and session objects (afs_capi.cpp,
// afs_comm.cpp) and the host helpers they share.  Not part of the C ABI.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "afs_buf.h"
#include "afs_model.h"

struct afs_ctx {
  afs_config cfg{};
  int simds = 1024;  // SIMDs of the device (the voice kernel's batch limit, afs_capi.cpp lanes_for)
  hipStream_t stream = nullptr;
  afs::Tables host_tab{};
  afs::DeviceBuf dev_tab;  // afs::Tables (tab())
  const afs::Tables *tab() const { return dev_tab.as<afs::Tables>(); }
  std::string err;
  // The context's reusable buffers (afs_buf.h), each enlarged on demand and freed with the context.
  // the state of whole-trajectory calls
  afs::DeviceBuf ws;
  afs::DeviceBuf rng;         // int32_t
  afs::DeviceBuf tree_lanes;  // tree solver: per-lane register state
  afs::DeviceBuf stage_in, stage_out, stage_seeds;
  afs::DeviceBuf tgt;        // target sequences: shape rows [Q][4][16], frame_row [B], then the slot order
  afs::DeviceBuf plan;       // tree solver: noise-source plans of one launch (tree_plan.h)
  afs::DeviceBuf hops;       // tree solver, hops >= PLAN_HOP_MIN: hop records (tree_plan.h PlanHop)
  afs::DeviceBuf p25;        // tree solver: section 25's pressure per sample of a launch (K6's tone input)
  afs::DeviceBuf plan_work;  // hop mode: K5's work list (the hops decided sample by sample)
  // the _pcm calls: the radiated flows of one launch, [B][window stride] doubles between K1 and K6 (as
  // p25), and the staging of a host pcm (int16_t)
  afs::DeviceBuf flow, stage_pcm;
  // the environment's switches (afs_create; include/afs.h lists them)
  bool plan_dense = false;             // AFS_PLAN_DENSE=1: dense records at every hop (A/B, tests)
  int64_t launch_cap = 65536;          // samples per K1 launch at most (AFS_LAUNCH_SAMPLES lowers it)
  bool shape_order = true;             // AFS_SHAPE_ORDER=0: afs_synthesize's utterances in call order
  // AFS_NOISE_VARIANTS: 1 (default) K1's noise-phase variants for the calls whose slot order finds
  // at least half of the utterances in a light class (shape_order), 2 for every call, 0 never
  int noise_variants = 1;
  int64_t plan_budget = 0;  // bytes of plans one call may hold (AFS_PLAN_BUDGET_MB; afs_capi.cpp)
  afs::DeviceBuf keys;       // shape keys, sorted keys, utterance indices, the variant flag
  afs::DeviceBuf sort_tmp;   // the device radix sort's scratch
  afs::DeviceBuf order_buf;  // the slot order built from them
  hipEvent_t ev_k5 = nullptr;  // after K5 and the read-back of its claimed slots (run_hop_call's guarded launches)
  afs::DeviceBuf stage_nf;  // per-utterance non-finite flags staged for a host array
  // afs_multi_synthesize: this device's shard of float audio, its int16 audio, its flags, and
  // (device 0) the gathered int16 audio of the whole batch
  afs::DeviceBuf m_out, m_pcm, m_nf, m_root;
  // signal taps (afs_set_taps): the list the _taps calls collect, and the staging of a host taps_out
  afs_tap taps[AFS_MAX_TAPS] = {};
  int32_t n_taps = 0;
  afs::DeviceBuf stage_taps;
  // afs_synthesize_ragged: the call's launch layout (afs_ragged_order.h) and per-row hop counts on
  // the device, the pinned host copy they are uploaded from on the stream, and the event after that
  // upload (the next ragged call rewrites the host copy only once it has been read)
  afs::DeviceBuf ragged;
  afs::PinnedBuf ragged_host;
  hipEvent_t ev_ragged = nullptr;
  // afs_session_synthesize_ragged: the frame rows of one pool call, [B][frame_stride + 1] (session_kernels.hip;
  // the call's own, nothing in it outlives the call -- the latched frames stay in the session's pair), and
  // the voice and seed lists of afs_session_restart_voices
  afs::DeviceBuf pool_rows, pool_list;
  // voice records in flight (afs_voice_state.h): a host caller's records of afs_session_save_voices /
  // _load_voices, and what afs_session_copy_voices gathers before it scatters
  afs::DeviceBuf voice_stage;
  int32_t last_B = 0;        // batch of the last whole-trajectory call (afs_rng_draws)
  afs::DeviceBuf dcount;  // int32_t: the non-finite utterances of a call
  afs::PinnedBuf hcount;  // pinned host copy of dcount
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // AFS_PROFILE: an event pair around every kernel launch of the synthesis calls
  struct Timed { hipEvent_t a, b; int kind; };  // kind 0: synthesis kernel (K1), 1: noise-source plan (K5),
                                                // 2: output stage (K6)
  std::vector<hipEvent_t> pev;  // pool
  size_t pev_used = 0;
  std::vector<Timed> timed;
  bool timed_overflow = false;
  // afs_memory_info_get: every device buffer above, and those of them that hold one double per
  // utterance-sample (of a launch: the windows; of a call: staged fp64 audio and taps, a shard's audio)
  std::vector<const afs::DeviceBuf *> device_bufs() const {
    return {&dev_tab, &ws, &rng, &tree_lanes, &stage_in, &stage_out, &stage_seeds, &tgt, &plan, &hops, &p25,
            &plan_work, &flow, &stage_pcm, &keys, &sort_tmp, &order_buf, &stage_nf, &m_out, &m_pcm, &m_nf, &m_root,
            &stage_taps, &ragged, &dcount, &pool_rows, &pool_list, &voice_stage};
  }
  std::vector<const afs::DeviceBuf *> sample_bufs() const { return {&flow, &p25, &stage_out, &stage_taps, &m_out}; }
};

struct afs_session {
  afs_ctx *ctx = nullptr;
  int B = 0;
  int64_t bp = 0;
  afs::DeviceBuf ws;          // lane solver: SoA workspace; tree solver: per-utterance LDS blocks
  afs::DeviceBuf rng;         // lane solver: generator state (int32_t); tree solver: unused
  afs::DeviceBuf tree_lanes;  // tree solver: per-lane register state
  int lanes = 16;             // tree solver: lanes per utterance (fixed at creation)
  afs::DeviceBuf pair;        // afs_frame [B][2]: previous frame, new frame
  afs::DeviceBuf seeds;       // device copy (uint32_t)
  // per voice: whether pair[u][0] holds its latched frame (the first frame after create / reset /
  // afs_session_restart_voices only latches).  The lock-step calls need one state for all voices.
  std::vector<uint8_t> latch;
  // per voice: the seed it was last given (create / reset / restart, or with a loaded or copied state);
  // 0: not known (seeds given in device memory).  Goes into a saved record's header, nothing reads it.
  std::vector<uint32_t> seed_of;
  bool all_latched(bool v) const {
    for (uint8_t x : latch)
      if ((x != 0) != v) return false;
    return true;
  }
  // pinned staging of host frames (afs_frame) and host output (double): a real-time caller's
  // per-call copies go through these instead of pageable memory
  afs::PinnedBuf hframes, hout;
};

namespace afs {

afs_status fail(afs_ctx *c, afs_status s, const char *fmt, ...);
bool is_device_ptr(const void *p);
// afs_synthesize queued without a host wait (unless host buffers need one), with the tree solver's
// lanes per utterance fixed by the caller (lanes > 0; afs_multi_synthesize: the global batch's, so
// that a shard's audio does not depend on the GPU count) or chosen for B (lanes = 0)
afs_status synthesize_async(afs_ctx *c, const afs_frame *frames, const uint32_t *seeds, int32_t B, int32_t F,
                            int32_t hop, double *out, uint8_t *nonfinite, int lanes = 0);
// the lanes per utterance of the tree kernel for a batch of B (AFS_LANES_* or the library's choice)
int lanes_for(const afs_ctx *c, int64_t B);

}  // namespace afs

#define HIP_TRY(ctx, call)                                                                   \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return afs::fail((ctx), e_ == hipErrorOutOfMemory ? AFS_ERR_OUT_OF_MEMORY : AFS_ERR_HIP, \
                       "%s failed: %s", #call, hipGetErrorString(e_));                       \
  } while (0)
