/* afs_device_math.h -- diagnostics of libafs.so: the tree solver's device-only arithmetic, one
 * operation at a time.
 *
 * The synthesis kernel does not take the compiler's division, square root and compare-and-select on
 * its hot path: csrc/tree_core.h has shorter device forms of them (pivot_recip / fast_rcp, fast_sqrt,
 * fast_div, hop_ratio, at_least / at_most / nonneg) which the CPU emulator of the kernel never
 * compiles.  afs_device_math runs these functions themselves -- the header's, compiled as device code
 * with the synthesis kernel's compiler flags (csrc/device_math.hip) -- over arrays of operands, so
 * that a test can hold each to an IEEE reference (tests/test_device_math_gpu.py).
 *
 * The declaration has a header of its own because include/afs.h is part of what the synthesis
 * kernel's object is built from (build.py kernel_digest: the committed counter summaries are keyed by
 * it), and a diagnostic must not change that key. */
#ifndef AFS_DEVICE_MATH_H
#define AFS_DEVICE_MATH_H

#include "afs.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum afs_math_op {
  AFS_MATH_RCP = 0,          /* pivot_recip(a) (fast_rcp is the same function) */
  AFS_MATH_SQRT = 1,         /* fast_sqrt(a) */
  AFS_MATH_DIV = 2,          /* fast_div(a, b) */
  AFS_MATH_HOP_RATIO = 3,    /* hop_ratio((int)a, hop, 1 / hop), hop = (double)(int)b: sample a of a hop of b */
  AFS_MATH_AT_LEAST = 4,     /* at_least(a, b) */
  AFS_MATH_AT_MOST = 5,      /* at_most(a, b) */
  AFS_MATH_NONNEG = 6,       /* nonneg(a) */
  AFS_MATH_DIPOLE_GAIN = 7,  /* glottis_dipole_gain(a): a = aspiration strength in dB */
  AFS_MATH_NOISE_COEF = 8,   /* exp(-2 pi (a b)): a = cut-off frequency in Hz, b = the sampling period */
  /* Deliberately weakened forms, which no kernel uses: a test of the forms above shows with them
   * that its operands would expose a missing step. */
  AFS_MATH_RCP_SEED = 9,         /* the hardware reciprocal estimate alone (pivot_recip without its Newton step) */
  AFS_MATH_DIV_UNCORRECTED = 10, /* a * pivot_recip(b) (fast_div without its residual correction) */
  AFS_MATH_SQRT_SHORT = 11,      /* fast_sqrt without its last residual step */
  AFS_MATH_OP_COUNT = 12
} afs_math_op;

/* out[k] = op(a[k], b[k]) for k < n, evaluated on the device; a, b and out are host arrays of n
 * doubles (b is read by the two-operand ops only, but is never NULL).  Tree solver only (else
 * AFS_ERR_UNSUPPORTED).  AFS_ERR_INVALID_ARGUMENT: an op outside afs_math_op, a NULL pointer,
 * n <= 0 or n > 2^31. */
afs_status afs_device_math(afs_ctx *ctx, int32_t op, const double *a, const double *b, int64_t n, double *out);

#ifdef __cplusplus
}
#endif

#endif /* AFS_DEVICE_MATH_H */
