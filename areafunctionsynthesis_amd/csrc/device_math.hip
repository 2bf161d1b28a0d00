// device_math.hip -- diagnostics (afs_device_math): the device-only arithmetic of tree_core.h, one
// operation per launch over arrays of operands.  This file holds no copy of those functions: it
// includes the header the synthesis kernel includes and is compiled with that kernel's flags
// (build.py TREE_FLAGS), so what a test measures here is the code the time loop runs
// (tests/test_device_math_gpu.py).  The CPU emulator compiles the header's host branch -- plain
// division, sqrt and comparisons -- and never sees these forms.
#include <hip/hip_runtime.h>

#include "afs_device_math.h"
#include "tree_core.h"

namespace afs {

using namespace tree;

namespace {

template <int OP>
__device__ __forceinline__ double math_op(double a, double b) {
  if constexpr (OP == AFS_MATH_RCP) return pivot_recip(a);
  else if constexpr (OP == AFS_MATH_SQRT) return fast_sqrt(a);
  else if constexpr (OP == AFS_MATH_DIV) return fast_div(a, b);
  else if constexpr (OP == AFS_MATH_HOP_RATIO) {
    // dhop and inv_hop as the synthesis kernels obtain them, on the device, from the launch's integer
    // hop: `const double dhop = (double)hop, inv_hop = 1.0 / dhop;` (tree_kernel.h tree_synth_run and
    // tree_pair_run, ahead of their time loops)
    const int hop = (int)b;
    const double dhop = (double)hop, inv_hop = 1.0 / dhop;
    return hop_ratio((int)a, dhop, inv_hop);
  } else if constexpr (OP == AFS_MATH_AT_LEAST) return at_least(a, b);
  else if constexpr (OP == AFS_MATH_AT_MOST) return at_most(a, b);
  else if constexpr (OP == AFS_MATH_NONNEG) return nonneg(a);
  else if constexpr (OP == AFS_MATH_DIPOLE_GAIN) return glottis_dipole_gain(a);
  else if constexpr (OP == AFS_MATH_NOISE_COEF) return exp(-2.0 * PI * (a * b));  // as tree_core.h phase_noise writes it
  // The weakened forms (afs_device_math.h): they exist here only.
  else if constexpr (OP == AFS_MATH_RCP_SEED) return __builtin_amdgcn_rcp(a);
  else if constexpr (OP == AFS_MATH_DIV_UNCORRECTED) return a * pivot_recip(b);
  else {
    static_assert(OP == AFS_MATH_SQRT_SHORT, "an afs_math_op");
    // fast_sqrt's sequence up to its first residual step
    const double y = __builtin_amdgcn_rsq(a);
    double g = a * y, h = 0.5 * y;
    const double r = fma(-h, g, 0.5);
    g = fma(g, r, g);
    h = fma(h, r, h);
    const double d = fma(-g, g, a);
    return fma(d, h, g);
  }
}

template <int OP>
__global__ void __launch_bounds__(256) device_math_kernel(const double *a, const double *b, int64_t n, double *out) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  out[k] = math_op<OP>(a[k], b[k]);
}

template <int OP>
hipError_t launch_op(int op, const double *a, const double *b, int64_t n, double *out, hipStream_t st) {
  if constexpr (OP < AFS_MATH_OP_COUNT) {
    if (op != OP) return launch_op<OP + 1>(op, a, b, n, out, st);
    hipLaunchKernelGGL(device_math_kernel<OP>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, b, n, out);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t launch_device_math(int op, const double *a, const double *b, int64_t n, double *out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (op < 0 || n > ((int64_t)1 << 31)) return hipErrorInvalidValue;
  return launch_op<0>(op, a, b, n, out, st);
}

}  // namespace afs
