// afs_session_kernels.h -- the per-voice lifecycle of a session's voice pool (session_kernels.hip;
// afs_session_restart_voices, afs_session_synthesize_ragged, afs_session_save_voices and its kin): the
// reset of listed voices, the frame rows of a pool call, and voice records in and out of a session.  The
// synthesis kernels themselves (tds_tree.hip, tds_plan.hip) know nothing of it.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

#include "afs_model.h"
#include "afs_voice_state.h"

namespace afs {

// tree_reset_kernel (tds_tree.hip) over a list: voice voices[i] (n distinct voices of the session's
// state, `lanes` lanes each) gets fresh lane state and a fresh LDS image seeded seeds[i], or
// voices[i] + 1 when seeds is null.  One thread per (listed voice, lane); nothing else is touched.
hipError_t launch_voice_reset(void *lane_state, double *lds_state, const int32_t *voices, const uint32_t *seeds, int n,
                              int lanes, hipStream_t st);

// The frame rows of a pool call.  Voice u was given count[u] frames, frames[u * frame_stride + k], and
// is latched on pair[u * 2] when latched[u] != 0.  Its row, rows[u * (frame_stride + 1) + j], becomes
//   latched:   [latch, f_0 .. f_{c-1}]      unlatched:   [f_0 .. f_{c-1}]
// and pair[u * 2] the new latch f_{c-1} (the old one is read before it is overwritten: by the same
// wave, load before store).  count[u] == 0: nothing of voice u is read or written.  No frame at or past
// count[u] is read.  One wave per frame of a row, its 67 16-byte vectors spread over the lanes;
// frames, rows and pair are 16-byte aligned.
hipError_t launch_pool_rows(const afs_frame *frames, int64_t frame_stride, const int32_t *count,
                            const int32_t *latched, int B, afs_frame *rows, afs_frame *pair, hipStream_t st);
// The indexed form (afs_session_synthesize_indexed): the same rows and latches, voice u's frames being
// frames[start[u] + k] of one flat array, start a device array of B indices, and a row holding
// longest + 1 frames (longest: the largest count).  Spans may overlap: frames is only read.  The start of
// a voice with count[u] == 0 is not loaded.  The same kernel body, one wave per frame of a row.
hipError_t launch_pool_rows_indexed(const afs_frame *frames, const int64_t *start, int64_t longest, const int32_t *count,
                                    const int32_t *latched, int B, afs_frame *rows, afs_frame *pair, hipStream_t st);

// Voice records (afs_voice_state.h; afs_session_save_voices, _load_voices, _copy_voices).  The session's
// three buffers that hold a voice: the lane registers, the saved LDS images, the frame pairs.
struct VoiceStateBuffers {
  char *lanes, *lds, *pair;
};
// the record layout of a session of `lanes` lanes per utterance (Lane<lanes>, X_TOTAL, afs_frame)
VoiceStateLayout voice_state_layout_for(int lanes);
// Gather: the payload of record i of records[n] (device, 16-byte aligned) becomes a copy of the state of
// voice voices[i] (a device list; a voice may repeat), bit for bit; the records' headers and the session
// are not touched.  Scatter: voice voices[i] (distinct) gets the payload of record i; no byte of another
// voice, and none of pair[u][1], is written.  One 16-byte vector per thread, a record over 7 (16
// lanes) or 11 (64 lanes) blocks of four waves.
hipError_t launch_voice_gather(const VoiceStateBuffers &s, const int32_t *voices, int n, int lanes, void *records,
                               hipStream_t st);
hipError_t launch_voice_scatter(const VoiceStateBuffers &s, const int32_t *voices, int n, int lanes, const void *records,
                                hipStream_t st);

// load the code object on the current device (afs_create; see afs_tree.h)
hipError_t preload_session_kernels();

}  // namespace afs
