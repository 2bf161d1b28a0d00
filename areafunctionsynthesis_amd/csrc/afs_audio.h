// afs_audio.h -- output format stage: the int16 conversion (host and device: audio_kernels.hip's K3,
// tree_core.h's PCM form of K6, tests/cpp/pcm_pack_main.cpp), the float32 conversion (tree_core.h's
// float32 form of K6, tests/cpp/f32_pack_main.cpp) and K3's launch (audio_kernels.hip).
#pragma once

#include <cstdint>

#include "afs_model.h"

namespace afs {

// Synthesizer::synthesizeSegment (Synthesizer.cpp:955-973): short(x * SHRT_MAX), truncated towards
// zero, x > 1 -> SHRT_MAX, x < -1 -> SHRT_MIN; a NaN (undefined in C++, 0 on the reference's x86
// build) -> 0.
AFS_HD inline int16_t sample_to_int16(double x) {
  if (x > 1.0) return 32767;
  if (x < -1.0) return -32768;
  if (!(x == x)) return 0;
  return (int16_t)(int)(x * 32767.0);  // |x| <= 1: fits; truncation towards zero
}

// The float32 sample of the _f32 and packed calls: (float)x, round to nearest even; a NaN stays a NaN
// and an infinity an infinity (the int16 form above has no way to carry them, this one has).
AFS_HD inline float sample_to_f32(double x) { return (float)x; }

}  // namespace afs

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace afs {

hipError_t launch_to_int16(const double *in, int16_t *out, int64_t n, hipStream_t st);
// load the code object on the current device (afs_create; see afs_tree.h)
hipError_t preload_audio_kernels();

}  // namespace afs
#endif
