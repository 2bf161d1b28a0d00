// afs_device_math.h -- host-side interface of the arithmetic probe (device_math.hip).  A header of its
// own: afs_tree.h is part of what the synthesis kernel's object is built from (build.py kernel_digest).
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../include/afs_device_math.h"

namespace afs {

// diagnostics (afs_device_math): out[k] = op(a[k], b[k]), k < n, with tree_core.h's device forms;
// device pointers; op: an afs_math_op (else hipErrorInvalidValue)
hipError_t launch_device_math(int op, const double *a, const double *b, int64_t n, double *out, hipStream_t st);

}  // namespace afs
