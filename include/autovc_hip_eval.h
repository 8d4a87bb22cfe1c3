/* autovc_hip_eval.h -- per-utterance BatchNorm of libautovc_hip.so: the normalisation a batch of
 * train-mode conversions needs (util/evaluate.py converts with the model in train mode at B = 1, so
 * every BatchNorm1d uses the statistics of the one utterance in flight).  A frame-major batch
 * y [B*T][C] is B segments of T rows; each (segment, channel) is normalised with the mean and the
 * biased variance of its own T values, which makes row block b of a batched forward the B = 1 forward
 * of utterance b.  Forward only.
 *
 * A fifth header of the same library: the symbol was added without a change to autovc_hip.h,
 * autovc_hip_dv.h, autovc_hip_audio.h, autovc_hip_resample.h or AVC_ABI_VERSION (a library that has it
 * still reports the same version; a binding that needs it looks it up and fails if it is missing).
 *
 * Conventions are those of autovc_hip.h: 0 on success, -1 with avc_last_error() set otherwise;
 * every argument is checked on the host BEFORE any launch; `stream` is a hipStream_t.  One launch,
 * one workgroup per (segment, 64-channel tile); workgroups do not synchronise with each other, spin
 * or use atomics, and every sum has a fixed order, so a segment's result does not depend on the
 * other segments of the batch (bit for bit).
 */
#ifndef AUTOVC_HIP_EVAL_H
#define AUTOVC_HIP_EVAL_H

#include "autovc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Segments of at most this many rows stay in LDS between the statistics passes and the apply pass
 * (a T x 64 fp32 tile: 60 KiB at 240 rows); a longer segment is re-read from global memory. */
#define AVC_BN_SEG_LDS_ROWS 240

/* For segment b < B and channel c < C, over rows r = b*T .. b*T + T - 1 of y (fp32, `ld` floats apart):
 *   mean[b][c] = sum_r y[r][c] / T
 *   var        = sum_r (y[r][c] - mean)^2 / T          (biased; about the mean, never E[y^2] - E[y]^2)
 *   rstd[b][c] = 1 / sqrt(var + eps)
 *   o[r][c]    = act(gamma[c] (y[r][c] - mean) rstd + beta[c]) (+ residual[r][c])
 * i.e. F.batch_norm(training=True) of each utterance alone, then the AVC_ACT_* activation.
 *   out       fp32 [B*T][ld] or NULL;  out_bf16  bf16 [B*T][ld] or NULL (at least one of the two)
 *   residual  fp32 [B*T][ld] or NULL, added after the activation
 *   mean, rstd   fp32 [B][C] or NULL (the statistics, for a caller that wants them)
 * out may alias y.  Only rows [0, B*T) and columns [0, C) of out / out_bf16 are written.
 * Refused: T < 2 (one value per channel has no variance, as torch refuses it in training), B < 1,
 * C < 1, ld < C, a null y / gamma / beta, neither out nor out_bf16, eps < 0 or not finite, an act
 * outside AVC_ACT_*, y_dtype other than AVC_F32 (the statistics are not taken from rounded values),
 * more than 2^31 - 1 workgroups. */
int avc_bn_seg_apply(const void* y, int y_dtype, long long ld, int B, int T, int C, const float* gamma,
                     const float* beta, float eps, int act, const float* residual, float* out, void* out_bf16,
                     float* mean, float* rstd, void* stream);

#ifdef __cplusplus
}
#endif
#endif
