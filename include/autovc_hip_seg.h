/* autovc_hip_seg.h -- per-segment moments and AdaIN of libautovc_hip.so: what a batch of AdaIN
 * conversions needs.  The AdaIN variants (AutoVC2 / MetaConv2 / MetaPool2) take [x.mean(), x.std()] and
 * (x - x.mean()) / x.std() * sigma + mu over the WHOLE tensor, which at B = 1 -- how util/evaluate.py
 * converts -- is the one utterance in flight.  A batch x of B contiguous segments of n floats (a
 * frame-major (B*T, C) tensor with ld == C: n = T*C) gets the moments, and the AdaIN, of each segment
 * alone here, which makes segment b of a batched forward the B = 1 forward of utterance b.
 * Forward only.
 *
 * A sixth header of the same library: the symbols were added without a change to autovc_hip.h,
 * autovc_hip_dv.h, autovc_hip_audio.h, autovc_hip_resample.h, autovc_hip_eval.h or AVC_ABI_VERSION (a
 * library that has them still reports the same version; a binding that needs them looks them up and
 * fails if they are missing).
 *
 * Conventions are those of autovc_hip.h: 0 on success, -1 with avc_last_error() set otherwise; every
 * argument is checked on the host BEFORE any launch; `stream` is a hipStream_t.  One launch, one
 * 256-thread workgroup per segment; workgroups do not synchronise with each other, spin or use atomics,
 * no workspace, and every sum has a fixed order, so a segment's result does not depend on the other
 * segments of the batch (bit for bit) and is the same from run to run.
 */
#ifndef AUTOVC_HIP_SEG_H
#define AUTOVC_HIP_SEG_H

#include "autovc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Segments of at most this many floats stay in LDS between the passes (64 KiB, the most a workgroup
 * takes without opting in, less 64 bytes of reduction slots: 16368 floats; the conversion shape
 * 176 x 80 = 14080 fits); a longer segment is re-read from global memory. */
#define AVC_SEG_MOMENTS_LDS_FLOATS 16368

/* out[b] = [mean, unbiased std] of x[b*n .. b*n + n), b < B: torch.mean / torch.std of that segment.
 * The sums are fp64 and the variance is taken about the mean (sum (x - mean)^2 / (n - 1)), never as
 * E[x^2] - E[x]^2.  n = 1 gives a NaN std, as torch.std and avc_moments do.
 *   x    fp32 [B*n], contiguous;   out  fp32 [B][2]
 * float4 accesses when n % 4 == 0 and x is 16-byte aligned, a scalar path otherwise.
 * Refused: a null x / out, B < 1, n < 1. */
int avc_seg_moments(const float* x, int B, long long n, float* out, void* stream);

/* y[b*n + i] = (x[b*n + i] - mean_b) / std_b * sigma[b] + mu[b], mean_b / std_b the moments above of
 * segment b, computed inside the same launch (no second kernel, no workspace).
 *   mu, sigma  fp32 [B];   y  fp32 [B*n], may alias x
 * float4 accesses when n % 4 == 0 and x and y are 16-byte aligned.  Only y[0 .. B*n) is written.
 * Refused: a null x / mu / sigma / y, B < 1, n < 1. */
int avc_adain_seg(const float* x, int B, long long n, const float* mu, const float* sigma, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif
