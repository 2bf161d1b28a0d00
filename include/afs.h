/*
 * afs.h -- C ABI of the MI355X batched area-function synthesizer (libafs.so).
 *
 * This is the drop-in boundary for the reference's synthesis hot path.  The reference
 * has no FFI layer; its callers use the C++ class API, and every entry point below
 * names the reference interface it replaces:
 *
 *   afs_session_synthesize  <- Synthesizer::synthesizeSignalTds(Tube*, double*, int, double*)
 *                              src/Backend/Synthesizer.h:161-162, Synthesizer.cpp:515-639
 *                              (together with TdsModel::setTube / setFlowSource /
 *                              setPressureSource / proceedTimeStep, TdsModel.h:267-271, and
 *                              Glottis::calcGeometry / getTubeData / incTime, Glottis.h:77-82)
 *   afs_session_reset       <- Synthesizer::reset (Synthesizer.cpp:231-250: TdsModel::resetMotion,
 *                              TriangularGlottis::resetMotion, output filter reset) + srand(seed)
 *   afs_synthesize          <- the same driver run over whole trajectories: one latch call on
 *                              frame 0 then F-1 calls of `hop` samples each, as
 *                              Synthesizer::synthesizeSegment (Synthesizer.cpp:928-986) and
 *                              playTargetSequence (:1299-1422) drive it, for B utterances at once
 *   afs_af_to_frames        <- OneDimAreaFunction::calculateOneDimTubeFunction
 *                              (src/Backend/OneDimAreaFunction.cpp:75-138)
 *   afs_options             <- TdsModel::Options (src/Backend/TdsModel.h:83-95)
 *   afs_to_int16            <- the int16 audio ring of Synthesizer::synthesizeSegment
 *                              (Synthesizer.cpp:955-973, Signal16 = short, Signal.h:19)
 *   afs_play_target_sequences <- Synthesizer::playTargetSequence (Synthesizer.cpp:1299-1422)
 *                              with interpolateParameters (:1286-1294), for B utterances
 *   afs_multi_synthesize    <- the same whole-trajectory driver over several GPUs of one node,
 *   afs_comm_*, afs_gather_pcm  the int16 audio (Synthesizer.cpp:955-973) gathered to the first
 *                              GPU over RCCL (the reference has one Synthesizer per process and
 *                              no collectives; this is the only exchange the batch needs)
 *
 * Errors: the reference prints and continues (TdsModel.cpp:1832,1849,1898,2267); here every
 * call returns an afs_status and afs_last_error() holds a message.  Inputs are clamped exactly
 * as the reference clamps them (areas >= 0.001 cm^2, Tube.cpp:337/371/413).  Non-finite audio
 * (the reference's "matrix is not positive definite" path, TdsModel.cpp:2267) is reported per
 * utterance in the optional `nonfinite` flag array of the synthesis calls and counted in
 * afs_report.nonfinite_utterances.
 *
 * Seeds: srand() seed per utterance / voice; a NULL seed array seeds utterance u with u + 1.
 *
 * Memory: frames / seeds / out may be host or device (hipMalloc) pointers; the library
 * detects which.  Device state lives in the session.  One context per host thread.
 * All work is issued on the context's HIP stream (afs_set_stream) and the calls are
 * synchronous unless AFS_ASYNC is set in afs_config.flags.
 */
#ifndef AFS_H
#define AFS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AFS_ABI_VERSION 5
#define AFS_NUM_TUBE_SECTIONS 40   /* Tube::NUM_PHARYNX_MOUTH_SECTIONS (Tube.h:56-58) */
#define AFS_NUM_GLOTTIS_PARAMS 6   /* TriangularGlottis::NUM_CONTROL_PARAMS (TriangularGlottis.h:26-35) */
#define AFS_NUM_AF_PARAMS 16       /* OneDimAreaFunction::NUM_AF_PARAMS (OneDimAreaFunction.h:34-43) */

typedef enum afs_status {
  AFS_OK = 0,
  AFS_ERR_INVALID_ARGUMENT = 1,
  AFS_ERR_NO_DEVICE = 2,
  AFS_ERR_HIP = 3,
  AFS_ERR_OUT_OF_MEMORY = 4,
  AFS_ERR_UNSUPPORTED = 5
} afs_status;

/* Linear solver for the per-sample 97x97 SPD system. */
typedef enum afs_solver {
  AFS_SOLVER_CHOLESKY = 0, /* TdsModel::CHOLESKY_FACTORIZATION, same operation order (TdsModel.cpp:2231-2314):
                              one lane per utterance, the reference-order kernel (slow; for checks) */
  AFS_SOLVER_TREE = 1,     /* the default and the fastest: 16 lanes per utterance, the same system solved by an
                              LDL^T in arm order (tube tree, fewer flops), noise-source plans computed ahead */
  AFS_SOLVER_SOR = 2       /* TdsModel::SOR_GAUSS_SEIDEL, same sweep order (TdsModel.cpp:2105-2180), one lane
                              per utterance */
  /* 3 was AFS_SOLVER_SEG (a segment-aligned cooperative kernel, measured 42 % slower than TREE and
     withdrawn in ABI 5): afs_create rejects it with AFS_ERR_INVALID_ARGUMENT */
} afs_solver;

/* Glottis model driven by the synthesizer: the reference's Synthesizer uses TriangularGlottis
 * (Synthesizer.h:212-213); TwoMassModel (TwoMassModel.cpp) is the other Glottis subclass in its
 * sources.  Its six controls are f0, lung pressure, rest displacements 1/2, extra arytenoid
 * area and damping factor (afs_frame.glottis[5] is the damping factor; aspiration stays at
 * Glottis::DEFAULT_ASPIRATION_STRENGTH_DB = -40 dB). */
typedef enum afs_glottis_model {
  AFS_GLOTTIS_TRIANGULAR = 0,
  AFS_GLOTTIS_TWO_MASS = 1
} afs_glottis_model;

/* TdsModel::GlottisLossOptions (TdsModel.h:75-81). */
typedef enum afs_glottis_loss {
  AFS_ENTRANCE_LOSS_STANDARD = 0,     /* k_ent = 1 */
  AFS_ENTRANCE_LOSS_VAN_DEN_BERG = 1, /* k_ent = 1.375 */
  AFS_ENTRANCE_LOSS_VARIABLE = 2      /* Fulcher et al. 2011 (TdsModel.cpp:1019-1092) */
} afs_glottis_loss;

typedef enum afs_precision { AFS_FP64 = 0 } afs_precision;

/* Options of TdsModel (TdsModel.h:83-95), defaults of TdsModel.cpp:35-44. */
typedef struct afs_options {
  int32_t turbulence_losses;        /* 1 */
  int32_t soft_walls;               /* 1 */
  int32_t generate_noise_sources;   /* 1 */
  int32_t radiation_from_skin;      /* 1 */
  int32_t piriform_fossa;           /* 0 */
  int32_t inner_length_corrections; /* 1 */
  int32_t transvelar_coupling;      /* 0 */
  int32_t glottis_loss;             /* afs_glottis_loss, 0 */
  int32_t glottis_model;            /* afs_glottis_model, 0 (not a TdsModel option: the synthesizer's glottis) */
  double flow_separation_area_ratio; /* 1.0 */
} afs_options;

/* afs_synthesize, afs_play_target_sequences and afs_to_int16 return once their work is queued on the
 * context's stream.  These cases still wait on the host:
 *   - afs_play_target_sequences, once, early: for the upload of the trajectories' shape rows and slot
 *     order, which it builds in host memory of its own (the synthesis is queued after that wait);
 *   - a host `out` (the audio is copied back before the call returns), and host input or output
 *     of afs_to_int16;
 *   - a report (its device time and non-finite count are read when the work is done);
 *   - host `nonfinite` flags (device flags do not wait);
 *   - a large tree call whose mixed hops' noise plans may overflow the plan budget: it reads back how
 *     many plan slots K5 claimed, after its synthesis launches are queued (guarded on the device: they
 *     do nothing on an overflow, and the call then queues its chunked path).  That wait covers the
 *     work queued before K5, the previous call's synthesis included, but the device does not idle:
 *     this call's synthesis is queued behind K5.
 * The slot order is sorted on the device, with no read-back.  Sessions, the diagnostics and
 * afs_af_to_frames always wait. */
#define AFS_ASYNC 0x1u
/* Record an event pair around every kernel launch of the synthesis calls; afs_kernel_times
 * returns their summed durations (measurement only: a few microseconds per launch). */
#define AFS_PROFILE 0x2u
/* Tree solver, lanes per utterance.  By default the library picks per call (per session: at its
 * creation) from the batch: the voice kernel (64 lanes, two tube sections per lane, each utterance's
 * phases split over a pair of waves on two SIMDs: the shortest time per sample) while the batch is no
 * larger than the GPU's SIMD count, the throughput kernel (16 lanes, six sections per lane, four
 * utterances per pair of waves, two waves per SIMD) above.  These
 * flags force one of them (not both).  The two kernels evaluate the same operations per section but
 * are separate compilations: their audio agrees within the parity tolerances, not bit for bit. */
#define AFS_LANES_16 0x4u
#define AFS_LANES_64 0x8u

typedef struct afs_config {
  double sampling_rate_hz; /* reference: 22050 (Constants.h:22-26); any rate is accepted */
  int32_t precision;       /* afs_precision */
  int32_t solver;          /* afs_solver */
  int32_t device;          /* HIP device ordinal */
  uint32_t flags;          /* AFS_ASYNC | AFS_PROFILE | AFS_LANES_16 or AFS_LANES_64 */
  afs_options options;
} afs_config;

/* One frame = the arguments of one synthesizeSignalTds() call: the dynamic part of the
 * caller's Tube and the six glottis control parameters.  1072 bytes. */
typedef struct afs_frame {
  double area_cm2[AFS_NUM_TUBE_SECTIONS];   /* Tube::pharynxMouthSection[i].area_cm2 */
  double length_cm[AFS_NUM_TUBE_SECTIONS];  /* .length_cm */
  double laterality[AFS_NUM_TUBE_SECTIONS]; /* .laterality */
  double teeth_position_cm;                 /* Tube::teethPosition_cm */
  double velum_opening_cm2;                 /* argument of Tube::setVelumOpening */
  double glottis[AFS_NUM_GLOTTIS_PARAMS];   /* f0 Hz, lung pressure dPa, rest disp 1/2 cm, ary area cm^2, aspiration dB */
  uint8_t articulator[AFS_NUM_TUBE_SECTIONS]; /* Tube::Articulator (Tube.h:24-32) */
  uint8_t reserved[8];
} afs_frame;

typedef struct afs_report {
  double device_ms;              /* time of the synthesis kernels (HIP events) */
  int64_t samples;               /* audio samples produced (all utterances) */
  int32_t nonfinite_utterances;  /* utterances whose output contains NaN/Inf */
  int32_t kernel;                /* which kernel ran (implementation detail, for profiles) */
} afs_report;

typedef struct afs_ctx afs_ctx;
typedef struct afs_session afs_session;

void afs_config_default(afs_config *cfg);
const char *afs_status_string(afs_status s);
int32_t afs_abi_version(void);

/* Environment read by afs_create (studies and A/B runs; the defaults are the measured best):
 *   AFS_PLAN_DENSE=1        every hop reads K5's dense per-sample records (bit-exact plan, below)
 *   AFS_PLAN_BUDGET_MB=N    noise-plan memory per call (default 4096); past it the call runs in
 *                           launches of at most N MB of plans -- with one floor: a launch spans at
 *                           least one hop, so a hop-mode launch holds at least two hops of dense
 *                           records per row (2 x hop x 128 B x rows) even when that exceeds N MB
 *   AFS_LAUNCH_SAMPLES=N    samples per synthesis-kernel launch at most (default 65536; the state
 *                           crosses launches, the audio is the same bit for bit)
 *   AFS_SHAPE_ORDER=0      afs_synthesize's utterances in call order in the 16-lane kernel's
 *                           slots instead of sorted by the shape of their first frame (the audio
 *                           of each utterance is the same either way)
 *   AFS_NOISE_VARIANTS=0    the synthesis kernel always runs its full noise phases instead of the
 *                           lightest variant each launch's noise-source plans allow (same audio);
 *                           =2 the variants for every call (default: for calls whose batch is mostly
 *                           light or holds >= 16 waves per SIMD: DESIGN.md 2.5)
 * (Settled and no longer switches -- the XCD-aware slot order of shared trajectories, the noise
 * class's place in the shape key, the STAT waves' issue priority by the launch's rounds of workgroups,
 * K5 and K1 on one stream: profiles/AB_LOG.md.) */
afs_status afs_create(afs_ctx **ctx, const afs_config *cfg);
void afs_destroy(afs_ctx *ctx);
const char *afs_last_error(const afs_ctx *ctx);
/* Use this hipStream_t (passed as void*) for all work of the context; NULL = default stream. */
afs_status afs_set_stream(afs_ctx *ctx, void *hip_stream);
/* Lanes per utterance the tree solver uses for a batch of this size (AFS_LANES_*; 1 for the
 * one-lane solvers). */
int32_t afs_lanes_per_utterance(const afs_ctx *ctx, int32_t batch);
/* Name of the synthesis kernel a batch of this size runs ("tree_pair_kernel": 16 lanes per
 * utterance, two waves per SIMD; "tree_pair64_kernel": the 64-lane voice kernel as wave pairs, small
 * batches; "tree_synth_kernel": the 64-lane voice kernel one wave per utterance, or any batch of a
 * one-wave build; "lane_synth_kernel": the one-lane solvers) -- for matching profiler output.
 * Diagnostics; no reference counterpart. */
const char *afs_synthesis_kernel(const afs_ctx *ctx, int32_t batch);
afs_status afs_synchronize(afs_ctx *ctx);

/* Whole trajectories.  frames[batch][num_frames], seeds[batch] (srand() seed per utterance,
 * 0 behaves as 1 like glibc; NULL: u + 1), out[batch][(num_frames-1)*hop] doubles in [-1,1].
 * nonfinite: NULL or batch bytes (host or device), set to 1 for the utterances whose audio
 * holds a NaN or an infinity, else 0. */
afs_status afs_synthesize(afs_ctx *ctx, const afs_frame *frames, const uint32_t *seeds,
                          int32_t batch, int32_t num_frames, int32_t hop, double *out,
                          uint8_t *nonfinite, afs_report *report);
/* afs_synthesize for utterances of different lengths.  frames[batch][frame_stride]; utterance u plays
 * frames 0 .. num_frames[u]-1 and produces T_u = (num_frames[u]-1)*hop samples into
 * out[u*out_stride .. +T_u).  num_frames is a HOST array (the launch layout is built from it without a
 * read-back), 2 <= num_frames[u] <= frame_stride; out_stride >= max T_u.  Frames at or past
 * num_frames[u] are never read and samples at or past T_u are never written.  taps_out: NULL, or
 * [batch][n_taps][out_stride] with the context's tap list (afs_set_taps).  Row u, its tap rows, its
 * rand() count (afs_rng_draws) and its non-finite flag are bit for bit those of afs_synthesize /
 * afs_synthesize_taps called on utterance u alone with its own num_frames (same lane width).
 * report->samples = sum of T_u.  Tree solver only (else AFS_ERR_UNSUPPORTED).
 * frames, seeds, out, taps_out and nonfinite may be host or device memory and AFS_ASYNC treats them
 * as in afs_synthesize (a host out or taps_out is staged: uploaded, written up to each row's end and
 * copied back whole).  AFS_ERR_INVALID_ARGUMENT: a count outside 2..frame_stride, out_stride below
 * the longest T_u, a NULL num_frames, taps_out without a tap list.  Utterances of one length share
 * K1's workgroups; each distinct length costs at most one partly filled workgroup. */
afs_status afs_synthesize_ragged(afs_ctx *ctx, const afs_frame *frames, int64_t frame_stride,
                                 const int32_t *num_frames, const uint32_t *seeds, int32_t batch, int32_t hop,
                                 double *out, int64_t out_stride, double *taps_out,
                                 uint8_t *nonfinite, afs_report *report);
/* Diagnostics: the number of rand() calls (TdsModel.cpp:1690-1692) each utterance of the last
 * afs_synthesize / afs_play_target_sequences call made, draws[batch] (host or device).  A
 * count that differs from the reference's means a noise source switched on or off at a
 * different sample (TdsModel.cpp:1647-1666).  Tree solver only (else AFS_ERR_UNSUPPORTED). */
afs_status afs_rng_draws(afs_ctx *ctx, int32_t batch, int64_t *draws);
/* Diagnostics: the noise-source plan records the tree solver computes ahead of the time
 * loop (kernel K5; AFS_PLAN_WORDS u64 words per sample, layout in csrc/tree_plan.h) for samples
 * [s_begin, s_end) of frames[rows][num_frames] at this hop: plans[rows][s_end - s_begin]
 * [AFS_PLAN_WORDS] (host or device).  Everything calcNoiseSources decides from the geometry
 * (TdsModel.cpp:1188-1508); tests compare it bit for bit with the host restatement.  Other
 * solvers: AFS_ERR_UNSUPPORTED. */
#define AFS_PLAN_WORDS 16
/* Diagnostics: Tube::interpolate (Tube.cpp:438-505) of the pharynx/mouth areas and lengths as
 * the tree solver's synthesis kernel computes them, for n samples: frames left[n] and right[n]
 * at ratio[n] -> area[n][40], length[n][40] (host pointers).  The reference rounds each product
 * of r1 * a + ratio * b; so do the kernel and K5 (no fma contraction), which tests check bit for
 * bit.  Other solvers: AFS_ERR_UNSUPPORTED. */
afs_status afs_tube_interpolate(afs_ctx *ctx, const afs_frame *left, const afs_frame *right, const double *ratio,
                                int32_t n, double *area, double *length);
afs_status afs_noise_plans(afs_ctx *ctx, const afs_frame *frames, int32_t rows, int32_t num_frames, int32_t hop,
                           int64_t s_begin, int64_t s_end, uint64_t *plans);
/* Diagnostics: the tree solver's hop mode (hops >= AFS_PLAN_HOP_MIN): K5's hop records of the
 * hops samples [s_begin, s_end) span, hops[rows][(s_end - 1) / hop - s_begin / hop + 1]
 * [AFS_PLAN_HOP_BYTES] (layout: csrc/tree_plan.h PlanHop: per plan word its kind and inputs, the
 * mixed flag), and the dense records of the mixed hops' samples in plans (as afs_noise_plans;
 * the other samples' records are left as they were).  Host or device pointers.  Other solvers or
 * shorter hops: AFS_ERR_UNSUPPORTED. */
#define AFS_PLAN_HOP_BYTES 544
#define AFS_PLAN_HOP_MIN 32
afs_status afs_noise_plan_hops(afs_ctx *ctx, const afs_frame *frames, int32_t rows, int32_t num_frames, int32_t hop,
                               int64_t s_begin, int64_t s_end, uint8_t *hops, uint64_t *plans);
/* Diagnostics: the plan words the tree solver's synthesis kernel evaluates per sample from a hop
 * record (kernel K1's own evaluation, compiled with its flags) for n (record, ratio) pairs:
 * hops[n][AFS_PLAN_HOP_BYTES], ratio[n] -> words[n][AFS_PLAN_WORDS] (host pointers).  Outside
 * mixed hops, these words replace K5's dense records: the discrete words and sqrt(A) are the same
 * bits, the quotient words (1/A, 1/sqrt(4A/pi), the downstream factors N/D) come from a reciprocal
 * with one Newton step and a residual correction instead of an IEEE division -- within a few ulps
 * of the dense records (tests/test_plan_gpu.py measures it) -- and the downstream factors and the
 * glottis gain are hop-constant forms within 1e-12 / 1e-13 relative of the per-sample ones
 * (tests/test_plan_hops.py).  AFS_PLAN_DENSE=1 in the environment makes every hop read its dense
 * records (the per-sample plan bit for bit). */
afs_status afs_plan_hop_words(afs_ctx *ctx, const uint8_t *hops, const double *ratio, int32_t n, uint64_t *words);
/* Diagnostics: afs_device_math, the synthesis kernel's device-only arithmetic one operation at a time, is
 * declared in afs_device_math.h beside this header. */

/* Stateful sessions: B independent Synthesizer instances living on the device. */
afs_status afs_session_create(afs_ctx *ctx, int32_t batch, const uint32_t *seeds, afs_session **s);
/* One synthesizeSignalTds(newTube, glottisParams, num_samples, newSignal) call for every
 * utterance: frames[batch], out[batch][max(num_samples,1)].  The first call after create/reset
 * only latches the frames and produces no samples (*produced = 0). */
afs_status afs_session_synthesize(afs_session *s, const afs_frame *frames, int32_t num_samples,
                                  double *out, uint8_t *nonfinite, int32_t *produced, afs_report *report);
afs_status afs_session_reset(afs_session *s, const uint32_t *seeds);
/* rand() calls of every voice since the last reset (see afs_rng_draws). */
afs_status afs_session_rng_draws(afs_session *s, int64_t *draws);
void afs_session_destroy(afs_session *s);

/* ---- Voice pools: per-voice frame counts, idle voices and restarts on a session --------------
 * Continuous batching: keep the session's B voices busy, feed each a few frames per call, and when a
 * voice's utterance ends give that voice a fresh state and seed while the others carry on.  Memory is
 * bounded by voices x frames per call instead of corpus x length.  Tree solver only (else
 * AFS_ERR_UNSUPPORTED).
 *
 * afs_session_restart_voices: voices[n] (distinct, 0 <= v < batch) and seeds[n] are HOST arrays;
 * seeds == NULL seeds voice v with v + 1.  Each listed voice gets what afs_session_reset gives every
 * voice -- fresh lane state, a fresh output and tone filter state, non-finite flag, rand() state and
 * draw count -- and is unlatched.  No byte of any other voice's state changes.
 *
 * afs_session_synthesize_ragged: frames[batch][frame_stride] (host or device), num_frames[batch] a HOST
 * array, produced[batch] a host output (or NULL).  With c = num_frames[u], voice u
 *   c == 0 (idle)          no frame, no state and no output byte of voice u is read or written; 0 samples
 *   unlatched, c >= 1      frame 0 latches (Synthesizer.cpp:522-532), frames 1 .. c-1 play as transitions
 *                          of hop samples: (c-1)*hop samples
 *   latched, c >= 1        frames 0 .. c-1 play as c transitions from the latched frame: c*hop samples
 * and a voice with c >= 1 is afterwards latched on its last supplied frame.  Frames at or past c are
 * never read, samples at or past produced[u] in row out[u*out_stride ..] are never written (a host out,
 * taps_out or pcm is staged: uploaded, written and copied back whole).  taps_out: NULL, or
 * [batch][n_taps][out_stride] with the context's tap list.  nonfinite and report->samples (the sum of
 * produced) as afs_synthesize_ragged; hop may differ from call to call; the call waits for its audio as
 * every session call does.  A voice fed its utterance in pieces produces, bit for bit, the row, tap
 * rows, rand() count and non-finite flag of afs_synthesize on that utterance alone with its seed (same
 * lane width).  When no voice has a transition to play (all idle, or only latching) no synthesis kernel
 * is launched, produced is all 0 and the call returns AFS_OK.
 * afs_session_synthesize_ragged_pcm: the same with int16 rows pcm[u*pcm_stride ..] (as the _pcm calls
 * above the conversion of the fp64 row, bit for bit; no taps).
 * AFS_ERR_INVALID_ARGUMENT: a count outside 0..frame_stride, a NULL num_frames, hop < 1, out_stride or
 * pcm_stride below the largest produced, a NULL out / pcm (or an odd pcm) when a voice produces samples,
 * taps_out without a tap list, a voice index out of range or listed twice.
 *
 * afs_session_latched: flags[batch] host bytes, 1 for a latched voice.
 * afs_session_synthesize, _taps and _pcm keep their behaviour on a session whose voices share one latch
 * state and answer AFS_ERR_INVALID_ARGUMENT on a mixed one; afs_session_reset resets everything.  Both
 * kinds of call may alternate on one session (they keep the latched frame in the same place).
 * Not covered: afs_synthesizer.hpp, afs_multi_synthesize, target sequences, the one-lane solvers, a hop
 * per voice, num_frames in device memory. */
afs_status afs_session_restart_voices(afs_session *s, const int32_t *voices, const uint32_t *seeds, int32_t n);
afs_status afs_session_synthesize_ragged(afs_session *s, const afs_frame *frames, int64_t frame_stride,
                                         const int32_t *num_frames, int32_t hop, double *out, int64_t out_stride,
                                         double *taps_out, uint8_t *nonfinite, int32_t *produced,
                                         afs_report *report);
afs_status afs_session_latched(afs_session *s, uint8_t *flags);

/* ---- Voice snapshots: save, load and fork the voices of a session ---------------------------
 * A voice's state leaves its slot as a record of afs_session_voice_state_bytes bytes (a multiple of 16;
 * 0 for a session of a one-lane solver): a fixed header, then the voice's device state verbatim -- its
 * lane registers, its saved LDS image (output and tone filter state, non-finite flag, rand() ring and
 * draw count, sample position) and its latched frame, each part padded to 16 bytes.
 * The header carries a magic and layout version, the lane width, the sizes of the two state parts, the
 * sampling rate, the afs_options, the voice's latched flag and, for information, the seed it was given
 * (0: not known).  Tree solver only (else AFS_ERR_UNSUPPORTED).  voices, dst_voices and src_voices are
 * HOST arrays; state holds n records and is host memory, or device memory aligned to 16 bytes.  Like
 * every session call these wait for their work.
 *
 * afs_session_save_voices: record i receives voice voices[i] (distinct); no byte of the session changes.
 * afs_session_load_voices: voice voices[i] (distinct) gets the state of record i -- lane state, LDS
 * image, latched frame and latched flag; no byte of any other voice changes.  The slot, the session, its
 * batch size and the context may be others than the ones saved from, provided the context has the same
 * sampling rate, options and lane width: every header is checked before anything is written.
 * afs_session_copy_voices: voice src_voices[i] of src becomes voice dst_voices[i] of dst.  dst_voices
 * are distinct, src_voices may repeat (one voice into many: a fork), src == dst is allowed with
 * overlapping lists (a swap): every source is read before any destination is written.  Both sessions
 * belong to one context and have one lane width.
 * After a load or a copy the voice continues, bit for bit, as the saved or source voice would have:
 * rows, tap rows, afs_session_rng_draws, the non-finite flag and afs_session_latched, under every later
 * call.  A voice saved unlatched loads unlatched; the lock-step calls keep their rule on mixed latch
 * state.
 * AFS_ERR_INVALID_ARGUMENT: a NULL pointer with n > 0, n < 0, a voice out of range, a destination or a
 * saved voice listed twice, a misaligned device state, a record whose header does not fit the session
 * (magic, version, lane width, state sizes, rate, options), sessions of different contexts or lane
 * widths in a copy.  n == 0 is AFS_OK and does nothing.
 * Not covered: conversion between the 16- and 64-lane layouts, the one-lane solvers,
 * afs_synthesizer.hpp, records across library versions beyond the header check. */
int64_t afs_session_voice_state_bytes(const afs_session *s);
afs_status afs_session_save_voices(afs_session *s, const int32_t *voices, int32_t n, void *state);
afs_status afs_session_load_voices(afs_session *s, const int32_t *voices, int32_t n, const void *state);
afs_status afs_session_copy_voices(afs_session *dst, const int32_t *dst_voices, afs_session *src,
                                   const int32_t *src_voices, int32_t n);

/* ---- Signal taps: section pressures and branch currents beside the audio -----------------
 * TdsModel::getSectionPressure / getSectionFlow (TdsModel.cpp:1715-1734) for whole batches: up to
 * AFS_MAX_TAPS quantities of the tube's state, one value per audio sample.  Value t of a tap is the
 * state after sample t's proceedTimeStep, which is what the reference's getters return at that moment.
 * Sections and currents keep the reference's numbering (Tube.h:53-82; TdsModel.cpp:93-131: current c
 * flows into section c for c < 93, 93/94 leave the mouth, 95/96 the nostrils).
 * Tree solver only (the one-lane solvers: AFS_ERR_UNSUPPORTED).  afs_set_taps validates the list
 * (AFS_ERR_INVALID_ARGUMENT: n outside 0..AFS_MAX_TAPS, an unknown kind, an index outside its range)
 * and keeps it in the context until it is set again; n = 0 clears it.  The _taps calls are
 * afs_synthesize / afs_session_synthesize with one more output, taps_out[batch][n_taps][T] doubles
 * (host or device; T the call's samples per utterance, as for out); without a list they answer
 * AFS_ERR_INVALID_ARGUMENT.  Their audio is the plain calls' bit for bit, AFS_ASYNC treats taps_out as
 * it treats out (a device taps_out does not wait), and an utterance that goes non-finite carries the
 * NaN in its tap rows as in its audio.  afs_synthesize and afs_session_synthesize ignore the list.
 * afs_play_target_sequences and afs_multi_synthesize have no _taps form. */
#define AFS_MAX_TAPS 8
typedef enum afs_tap_kind {
  AFS_TAP_PRESSURE = 0, /* tubeSection[index].pressure (dPa),         index 0..92 */
  AFS_TAP_CURRENT = 1   /* branchCurrent[index].magnitude (cm^3/s),   index 0..96 */
} afs_tap_kind;
typedef struct afs_tap {
  int32_t kind;  /* afs_tap_kind */
  int32_t index;
} afs_tap;
afs_status afs_set_taps(afs_ctx *ctx, const afs_tap *taps, int32_t n);
afs_status afs_synthesize_taps(afs_ctx *ctx, const afs_frame *frames, const uint32_t *seeds, int32_t batch,
                               int32_t num_frames, int32_t hop, double *out, double *taps_out,
                               uint8_t *nonfinite, afs_report *report);
afs_status afs_session_synthesize_taps(afs_session *s, const afs_frame *frames, int32_t num_samples, double *out,
                                       double *taps_out, uint8_t *nonfinite, int32_t *produced,
                                       afs_report *report);
/* getCurrentIn / getCurrentOut's topology (TdsModel.cpp:139-203): the branch currents that flow into
 * and out of a section, -1 where there is none.  Needs no context. */
afs_status afs_section_currents(int32_t section, int32_t *in, int32_t out[2]);

/* Area-function model -> tube frames (pharynx/mouth part, teeth).  params[n][16] in
 * OneDimAreaFunction::ParamIndex order; velum and glottis fields of frames are left unchanged. */
afs_status afs_af_to_frames(afs_ctx *ctx, const double *params, int64_t n, afs_frame *frames);

/* Output format stage: out[i] = short(x * 32767) truncated towards zero, x > 1 -> 32767,
 * x < -1 -> -32768, NaN -> 0 (Synthesizer.cpp:955-973).  Host or device pointers. */
afs_status afs_to_int16(afs_ctx *ctx, const double *samples, int64_t n, int16_t *out);

/* ---- PCM output calls: the int16 audio without a call-long fp64 buffer ----------------------
 * afs_synthesize, afs_synthesize_ragged and afs_session_synthesize delivering what
 * Synthesizer::synthesizeSegment stores (Synthesizer.cpp:955-973): row u of pcm, pcm[u*pcm_stride + s],
 * is bit for bit afs_to_int16 of the row the fp64 call returns for the same arguments, context and
 * lane width (a NaN sample is 0); nonfinite, afs_rng_draws / afs_session_rng_draws and report->samples
 * are the fp64 call's as well.  pcm is host or device memory at any int16 alignment, pcm_stride >= T
 * (ragged: the longest T_u) in samples, and it reaches to the end of the last row's samples,
 * (batch-1)*pcm_stride + T; nothing is written outside [u*pcm_stride, u*pcm_stride + T_u).  The session
 * call takes pcm[batch][max(num_samples,1)]; its latching first call produces 0 samples and writes
 * nothing.  PCM and fp64 calls may alternate on one session.
 * The output stage converts each sample on its way out: the fp64 audio is never stored.  Between the
 * synthesis kernel and the output stage the radiated flows cross a window of one launch's samples
 * (batch x min(T, AFS_LAUNCH_SAMPLES, default 65536) doubles, next to the section-25 pressures' window
 * of the same shape) that does not grow with T.  Still allocated per T: the frames (a host array's
 * staging), the hop records of the call (544 B per utterance and hop) and, for a host pcm, its int16
 * staging (2 B per sample; a host pcm with pcm_stride > T is uploaded first and copied back whole).  A
 * device pcm does not wait under AFS_ASYNC.
 * Tree solver only (AFS_ERR_UNSUPPORTED otherwise).  AFS_ERR_INVALID_ARGUMENT: a NULL or odd pcm,
 * pcm_stride below T, and what the fp64 call refuses.  There is no _taps form. */
afs_status afs_synthesize_pcm(afs_ctx *ctx, const afs_frame *frames, const uint32_t *seeds, int32_t batch,
                              int32_t num_frames, int32_t hop, int16_t *pcm, int64_t pcm_stride,
                              uint8_t *nonfinite, afs_report *report);
afs_status afs_synthesize_ragged_pcm(afs_ctx *ctx, const afs_frame *frames, int64_t frame_stride,
                                     const int32_t *num_frames, const uint32_t *seeds, int32_t batch, int32_t hop,
                                     int16_t *pcm, int64_t pcm_stride, uint8_t *nonfinite, afs_report *report);
afs_status afs_session_synthesize_pcm(afs_session *s, const afs_frame *frames, int32_t num_samples, int16_t *pcm,
                                      uint8_t *nonfinite, int32_t *produced, afs_report *report);
/* (the voice pool's call, see afs_session_synthesize_ragged) */
afs_status afs_session_synthesize_ragged_pcm(afs_session *s, const afs_frame *frames, int64_t frame_stride,
                                             const int32_t *num_frames, int32_t hop, int16_t *pcm,
                                             int64_t pcm_stride, uint8_t *nonfinite, int32_t *produced,
                                             afs_report *report);
/* ---- Packed ragged output and float32 samples ----------------------------------------------
 * The _pcm calls with two more freedoms: a row of the destination may start at an offset of its own
 * instead of u*stride (no padding to the longest utterance), and the samples may be float32.
 *
 * afs_synthesize_f32: afs_synthesize_pcm with rows of float, f32[u*f32_stride + s] = (float)x of the
 * fp64 call's sample x (round to nearest even; a NaN stays a NaN and an infinity an infinity, where
 * the int16 form stores 0 and the clipped value).  f32 at any float alignment, f32_stride >= T.
 *
 * afs_synthesize_ragged_packed: afs_synthesize_ragged_pcm with row u at out[offsets[u] ..
 * offsets[u] + T_u), T_u = (num_frames[u]-1)*hop.  format: AFS_SAMPLE_I16 (out is int16_t *, the
 * _pcm calls' samples) or AFS_SAMPLE_F32 (float *, afs_synthesize_f32's).  out is host or device
 * memory aligned to its sample type; offsets is a HOST array of batch row starts in samples, in any
 * order and with any gaps, or NULL: tight packing in call order, row u at the sum of the T_v before it
 * (afs_ragged_offsets).  Nothing outside the rows is written.  A host out spans max(offsets[u] + T_u)
 * samples; it is uploaded first and copied back whole (the gaps are the caller's), through a staging
 * buffer of that size.  A device out does not wait under AFS_ASYNC.  nonfinite, afs_rng_draws and
 * report->samples are the strided call's.
 *
 * afs_ragged_offsets: offsets[batch + 1] = the exclusive prefix sum of (num_frames[u]-1)*hop, the
 * total in the last entry: the tight layout, and the samples a packed buffer holds.  Needs no context
 * (AFS_ERR_INVALID_ARGUMENT: a NULL array, batch < 0, hop < 1, a count below 1).
 *
 * afs_session_synthesize_ragged_packed: the voice pool's call (afs_session_synthesize_ragged_pcm) with
 * voice u's produced[u] samples at out[offsets[u] ..].  An idle voice (count 0) writes nothing and its
 * offset is not looked at; offsets == NULL packs the produced lengths tightly in voice order.  Packed,
 * strided, int16, float32 and fp64 calls may alternate on one session.
 *
 * Every check is made on the host before anything is queued, and a refused call writes nothing.
 * AFS_ERR_INVALID_ARGUMENT: an unknown format, a NULL or misaligned out when there are samples to
 * write, a negative offset, two rows that overlap (rows may abut; rows without samples overlap
 * nothing), offsets in device memory, and what the strided call refuses.  Tree solver only
 * (AFS_ERR_UNSUPPORTED otherwise).
 * Not covered: a packed fp64 form (the fp64 calls' rows are written by the synthesis kernel itself,
 * not by the output stage), float32 or packed taps and the _taps calls, afs_multi_synthesize, target
 * sequences, afs_synthesizer.hpp, a float32 afs_session_synthesize. */
typedef enum afs_sample_format {
  AFS_SAMPLE_I16 = 0, /* int16_t: afs_to_int16 of the fp64 sample */
  AFS_SAMPLE_F32 = 1  /* float: (float) of the fp64 sample */
} afs_sample_format;
afs_status afs_synthesize_f32(afs_ctx *ctx, const afs_frame *frames, const uint32_t *seeds, int32_t batch,
                              int32_t num_frames, int32_t hop, float *f32, int64_t f32_stride,
                              uint8_t *nonfinite, afs_report *report);
afs_status afs_synthesize_ragged_packed(afs_ctx *ctx, const afs_frame *frames, int64_t frame_stride,
                                        const int32_t *num_frames, const uint32_t *seeds, int32_t batch,
                                        int32_t hop, int32_t format, void *out, const int64_t *offsets,
                                        uint8_t *nonfinite, afs_report *report);
afs_status afs_ragged_offsets(const int32_t *num_frames, int32_t batch, int32_t hop, int64_t *offsets);
afs_status afs_session_synthesize_ragged_packed(afs_session *s, const afs_frame *frames, int64_t frame_stride,
                                                const int32_t *num_frames, int32_t hop, int32_t format, void *out,
                                                const int64_t *offsets, uint8_t *nonfinite, int32_t *produced,
                                                afs_report *report);
/* ---- Indexed voice pools: frames read in place from a flat corpus ---------------------------
 * The voice pool's calls with the frames taken from one flat array instead of a rectangle: the packed
 * sequence form the audio already has (afs_session_synthesize_ragged_packed), on the input side.  A
 * corpus lies once in memory, frames[total_frames], and a step costs the host three integers per voice:
 * where its next frames start, how many it plays, where its audio goes.  No frame moves on the host.
 *
 * afs_session_synthesize_indexed: afs_session_synthesize_ragged with voice u playing
 * frames[frame_start[u] .. frame_start[u] + num_frames[u]).  frame_start and num_frames are HOST arrays
 * of batch entries; frames is host or device memory.  Everything else is the ragged pool call's, word
 * for word: the latch rule and the idle voice (c == 0: nothing of the voice is read or written, and its
 * frame_start is not looked at), produced, nonfinite, report, taps_out, out_stride, and the alternation
 * with every other session call on the same session.  A voice fed its utterance in pieces by these calls
 * produces, bit for bit, the row, tap rows, rand() count and non-finite flag of afs_synthesize on that
 * utterance alone with its seed (same lane width).  The spans of different voices may overlap or
 * coincide (candidates that share a stretch, one utterance under two seeds): frames is only read, and no
 * frame outside a live voice's span is ever read.
 * afs_session_synthesize_indexed_packed: afs_session_synthesize_ragged_packed likewise -- format, out,
 * offsets and their rules are that call's.
 *
 * Device frames aligned to 16 bytes are read in place by the gather of the call's frame rows: nothing of
 * size total_frames is allocated or copied.  A device array at another alignment takes the ragged pool
 * call's fallback, a copy to the staging buffer, restricted to the hull of the live spans (from the
 * lowest frame_start to the highest end of a live voice).  Of a host array the library copies the live
 * spans alone, back to back in voice order, into the session's pinned buffer, uploads that once and
 * hands the gather the staging's own start indices: the bytes staged follow the sum of the counts, not
 * total_frames (a span that two voices share is staged once for each).
 *
 * Every check is made on the host before anything is queued, and a refused call writes nothing.
 * AFS_ERR_INVALID_ARGUMENT: total_frames < 0, a NULL frame_start or num_frames, a count below 0, a live
 * voice with frame_start[u] < 0 or frame_start[u] + num_frames[u] > total_frames (compared without
 * forming a sum that could overflow), frame_start in device memory, and everything the ragged pool calls
 * refuse.  Tree solver only (AFS_ERR_UNSUPPORTED otherwise).
 * Not covered: packed frame input for the one-shot afs_synthesize_ragged (the synthesis and plan kernels
 * address frames by row x stride), frame_start in device memory, a hop per voice, afs_multi_synthesize,
 * afs_synthesizer.hpp, the one-lane solvers, asynchronous session calls. */
afs_status afs_session_synthesize_indexed(afs_session *s, const afs_frame *frames, int64_t total_frames,
                                          const int64_t *frame_start, const int32_t *num_frames, int32_t hop,
                                          double *out, int64_t out_stride, double *taps_out, uint8_t *nonfinite,
                                          int32_t *produced, afs_report *report);
afs_status afs_session_synthesize_indexed_packed(afs_session *s, const afs_frame *frames, int64_t total_frames,
                                                 const int64_t *frame_start, const int32_t *num_frames, int32_t hop,
                                                 int32_t format, void *out, const int64_t *offsets,
                                                 uint8_t *nonfinite, int32_t *produced, afs_report *report);
/* Diagnostics: the device memory the context holds now (its buffers grow on demand and are kept).
 * total_bytes: all of it; sample_buffer_bytes: the part that holds one fp64 value per
 * utterance-sample -- the flow and section-25 windows of a launch, a staged fp64 out or taps of a host
 * caller, a shard's fp64 audio (afs_multi_synthesize).  A context that has only run PCM calls holds
 * the two windows alone.  total_bytes counts the frame rows of a pool call
 * (afs_session_synthesize_ragged: batch x (frame_stride + 1) frames, kept by the context) and the
 * staging of voice records (afs_session_copy_voices, host records of _save_voices / _load_voices: n
 * records, grown on demand and kept); neither is a sample buffer.  It also counts what a packed or
 * float32 call adds: the row starts on the device (8 B per utterance, beside the ragged layout) and the
 * staging of a host destination (its span in samples of its format, in the int16 staging's buffer).  An
 * indexed pool call (afs_session_synthesize_indexed) adds the frame start indices on the device (8 B per
 * voice, beside the same layout) and nothing that grows with total_frames: its frame rows are batch x
 * (the largest count + 1) frames, and only a host or misaligned corpus is staged (the live spans, or
 * their hull, in the frames' staging buffer). */
typedef struct afs_memory_info {
  int64_t total_bytes;
  int64_t sample_buffer_bytes;
} afs_memory_info;
afs_status afs_memory_info_get(afs_ctx *ctx, afs_memory_info *info);

/* Synthesizer::playTargetSequence(targetShape, stationary_s, transition_s)
 * (Synthesizer.cpp:1299-1422).  The reference hard-codes f0_hz {100, 115, 105, 80} (:1311), the
 * 8000 dPa lung pressure of sensorDataToGlottisParams (:903) and takes the other glottis controls
 * from TriangularGlottis' control parameters after reset() (f0 120 Hz, 10000 dPa, rest
 * displacements 0.01 cm, arytenoid area 0, aspiration -40 dB; TriangularGlottis.cpp:19-24,
 * Synthesizer.cpp:244); afs_target_sequence_default() sets those and the SURVEY config-3
 * timing (stationary 0.2/0.05/0.2/0.1 s, transitions 0.05 s). */
typedef struct afs_target_sequence {
  double stationary_s[4];
  double transition_s[3];
  double f0_hz[4];
  double lung_pressure_dpa;
  double glottis[AFS_NUM_GLOTTIS_PARAMS];  /* init() latch; [2..5] also for every sample */
} afs_target_sequence;

void afs_target_sequence_default(afs_target_sequence *ts);
/* int numSamples = SAMPLING_RATE * totalTime_s (:1328), with the context's rate. */
int64_t afs_target_sequence_samples(const afs_target_sequence *ts, double sampling_rate_hz);

/* B utterances, utterance b playing the four shapes targets[4 b .. 4 b + 3] of the shape
 * table shapes[num_shapes][16] (host pointers) with one timing for the batch.  Semantics of the
 * reference per utterance: reset + srand(seeds[b]) (NULL: b + 1), init() latches the schwa
 * tube, then one synthesizeSignalTds(tube_i, glottis_i, 1) per sample, where tube_i comes from
 * the area-function model at the cosine-interpolated parameters of sample i (teeth at xin).
 * out[B][afs_target_sequence_samples()] doubles, host or device.  Tube trajectories are built
 * on the GPU once per distinct target sequence and streamed in time chunks. */
afs_status afs_play_target_sequences(afs_ctx *ctx, const double *shapes, int32_t num_shapes,
                                     const int32_t *targets, const afs_target_sequence *ts,
                                     const uint32_t *seeds, int32_t B, double *out, uint8_t *nonfinite,
                                     afs_report *report);

/* AFS_PROFILE contexts: summed device time and count of the synthesis-kernel launches (K1), of
 * the noise-source plan launches (tree solver, K5) and of the output-stage launches (tree solver,
 * K6: glottal-tone filter, dU/dt, Chebyshev low-pass) since the previous call (waits for the
 * stream; the next call starts from zero).  afs_kernel_times is the same without K6; any pointer
 * may be NULL. */
typedef struct afs_kernel_timing {
  double synth_ms;
  int32_t synth_launches;
  double plan_ms;
  int32_t plan_launches;
  double output_ms;
  int32_t output_launches;
} afs_kernel_timing;
afs_status afs_kernel_times_ex(afs_ctx *ctx, afs_kernel_timing *timing);
afs_status afs_kernel_times(afs_ctx *ctx, double *synth_ms, int32_t *synth_launches, double *plan_ms,
                            int32_t *plan_launches);

/* ---- Several GPUs: utterance shards, the int16 audio gathered over RCCL (xGMI) ----------
 * Utterances are independent: shard r of `world` synthesizes a contiguous block with no
 * exchange; the only collective is the gather of the finished audio to rank 0.  RCCL
 * (librccl.so.1 of the ROCm installation) is loaded on first use. */
#define AFS_COMM_ID_BYTES 128 /* NCCL_UNIQUE_ID_BYTES */
typedef struct afs_comm afs_comm;

/* Block of `rank`: utterances [*first, *first + *count) of `total` over `world` ranks (the first
 * total % world ranks take one more). */
void afs_shard_range(int64_t total, int32_t world, int32_t rank, int64_t *first, int64_t *count);
/* One process per GPU: rank 0 creates the id (ncclGetUniqueId) and hands it to the other
 * ranks over any channel; every rank then joins with its context (device, stream). */
afs_status afs_comm_unique_id(uint8_t id[AFS_COMM_ID_BYTES]);
afs_status afs_comm_create(afs_ctx *ctx, const uint8_t id[AFS_COMM_ID_BYTES], int32_t rank, int32_t world,
                           afs_comm **comm);
/* One process, n GPUs: comms[i] = rank i on ctxs[i]'s device (ncclCommInitAll). */
afs_status afs_comm_create_all(afs_ctx *const *ctxs, int32_t n, afs_comm **comms);
void afs_comm_destroy(afs_comm *comm);
/* Gather `count` int16 samples (device memory of this rank's context) to rank 0's root_out
 * (device memory): rank r's block lands at the sum of the counts of ranks < r.  root_counts
 * (rank 0, world entries; NULL = every rank sends `count`).  The transfer runs on the comm's own
 * stream after the work queued so far on the context's stream, so the next synthesis overlaps
 * it; afs_comm_fence makes the context's stream wait for it (before local or root_out is
 * written again), afs_comm_synchronize waits on the host. */
afs_status afs_gather_pcm(afs_comm *comm, const int16_t *local, int64_t count, int16_t *root_out,
                          const int64_t *root_counts);
afs_status afs_comm_fence(afs_comm *comm);
afs_status afs_comm_synchronize(afs_comm *comm);
/* Device time of this rank's gathers since the previous call (HIP events on the comm's stream
 * around each afs_gather_pcm, from the moment its input is ready to the end of its sends /
 * receives) and their count; waits for the comm's stream.  Either pointer may be NULL. */
afs_status afs_comm_gather_times(afs_comm *comm, double *ms, int32_t *count);
/* The whole node from one host thread: `batch` utterances sharded over the n contexts of comms
 * (afs_comm_create_all) with afs_shard_range; each shard runs afs_synthesize on its GPU (seeds
 * keep the global index: NULL = u + 1), is converted to int16 on its GPU (afs_to_int16) and
 * gathered to ctxs[0]'s GPU.  frames[batch][num_frames] and seeds are host arrays; pcm_out
 * [batch][(num_frames-1)*hop] is host memory or device memory of ctxs[0]; nonfinite (host,
 * batch bytes) and report may be NULL.  Returns when pcm_out is complete. */
afs_status afs_multi_synthesize(afs_ctx *const *ctxs, afs_comm *const *comms, int32_t n, const afs_frame *frames,
                                const uint32_t *seeds, int32_t batch, int32_t num_frames, int32_t hop,
                                int16_t *pcm_out, uint8_t *nonfinite, afs_report *report);

#ifdef __cplusplus
}
#endif
#endif /* AFS_H */
