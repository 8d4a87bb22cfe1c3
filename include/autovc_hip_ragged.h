/* autovc_hip_ragged.h -- the ragged-batch entry points of libautovc_hip.so: what a batch of whole
 * utterances of DIFFERENT lengths needs so that row block b of a batched forward is the B = 1 forward
 * of utterance b at its own length.  A frame-major batch [B*T][C] holds utterance b in rows
 * b*T .. b*T + lens[b] - 1; the rows lens[b] .. T - 1 of its block are padding.  The invariant the three
 * kernels keep: every activation that feeds a convolution is exactly 0.0 in the padding rows, so a
 * 5-tap 'same' convolution sees past an utterance's end what it sees at B = 1 -- zero padding.
 * Forward only.
 *
 * A seventh header of the same library: the symbols were added without a change to autovc_hip.h,
 * autovc_hip_dv.h, autovc_hip_audio.h, autovc_hip_resample.h, autovc_hip_eval.h, autovc_hip_seg.h or
 * AVC_ABI_VERSION (a library that has them still reports the same version; a binding that needs them
 * looks them up and fails if one is missing).
 *
 * Conventions are those of autovc_hip.h: 0 on success, -1 with avc_last_error() set otherwise;
 * every argument is checked on the host BEFORE any launch; `stream` is a hipStream_t.  Every entry
 * point is one launch whose workgroups do not synchronise with each other, spin or use atomics, and
 * every sum has a fixed order: an utterance's result does not depend on the other utterances of the
 * batch (bit for bit).
 *
 * Lengths travel twice, as in autovc_hip_audio.h: `lens` on the host (checked there: B ints, each in
 * 2..T) and `lens_dev`, the same ints on the device (read by the kernel).  The caller keeps the pair
 * equal.
 */
#ifndef AUTOVC_HIP_RAGGED_H
#define AUTOVC_HIP_RAGGED_H

#include "autovc_hip_eval.h"

#ifdef __cplusplus
extern "C" {
#endif

/* avc_bn_seg_apply (autovc_hip_eval.h) with a length per segment.  For segment b < B and channel
 * c < C, over the rows r = b*T .. b*T + lens[b] - 1 of y (fp32, `ld` floats apart), n = lens[b]:
 *   mean[b][c] = sum_r y[r][c] / n
 *   var        = sum_r (y[r][c] - mean)^2 / n          (biased, about the mean)
 *   rstd[b][c] = 1 / sqrt(var + eps)
 *   o[r][c]    = act(gamma[c] (y[r][c] - mean) rstd + beta[c]) (+ residual[r][c])
 * and o[r][c] = 0.0 exactly for the padding rows r = b*T + lens[b] .. b*T + T - 1, in out and in
 * out_bf16, whichever are given.  y's padding rows are never read.  The sums are those of
 * avc_bn_seg_apply in the same order (pivoted on the segment's first row, rows ascending per wave,
 * then waves 0..3): with lens[b] = T for every b the outputs are bit-identical to it.  A segment of
 * at most AVC_BN_SEG_LDS_ROWS rows stays in LDS between the passes, a longer one is re-read; the
 * decision is taken per segment from its own length, so both forms may run in one launch.
 * Arguments and refusals as avc_bn_seg_apply, and: null lens / lens_dev, lens[b] outside 2..T. */
int avc_bn_seg_ragged(const void* y, int y_dtype, long long ld, int B, int T, int C, const int* lens,
                      const int* lens_dev, const float* gamma, const float* beta, float eps, int act,
                      const float* residual, float* out, void* out_bf16, float* mean, float* rstd, void* stream);

/* In place: x[b*T + t][c] = 0.0 for t >= lens[b], c < C, in the fp32 tensor x (rows `ld` floats apart)
 * and / or its bf16 twin x_bf16 (rows `ld` elements apart); at least one of the two.  Nothing else is
 * written: rows t < lens[b] and columns c >= C keep their bits.  16-byte (fp32) / 8-byte (bf16) stores
 * when C, ld and the base addresses allow, scalar stores otherwise.
 * Refused: both pointers null, null lens / lens_dev, lens[b] outside 2..T, B < 1, T < 2, C < 1, ld < C,
 * more than 2^31 - 1 workgroups. */
int avc_row_mask(float* x, void* x_bf16, long long ld, int B, int T, int C, const int* lens, const int* lens_dev,
                 void* stream);

/* One bidirectional LSTM layer over a ragged batch, forward only, nothing kept for a backward.
 *   xproj  fp32 [B*T][2*4H]: W_ih x + b_ih + b_hh, direction d in columns d*4H .. d*4H + 4H - 1, gate
 *          order i, f, g, o -- the layout avc_lstm_fwd takes with dirs = 2
 *   w_hh   fp32 [2][4H][H]
 *   h      fp32 [B*T][2H] or NULL;  h_bf16  bf16 [B*T][2H] or NULL (at least one of the two)
 * For utterance b the forward direction runs t = 0 .. lens[b] - 1 and the backward direction runs
 * t = lens[b] - 1 .. 0, both from h = c = 0; h is written as 0.0 in the rows t >= lens[b].  xproj's
 * padding rows are never read.  compute = AVC_BF16 takes the fast exp / rcp activations of
 * avc_lstm_fwd's small-H path, AVC_F32 the IEEE library forms; weights and state are fp32 either way.
 * One workgroup per (utterance, direction).
 * Refused: null xproj / w_hh / lens / lens_dev, neither h nor h_bf16, H outside 1..64, B < 1, T < 2,
 * lens[b] outside 2..T, a compute other than AVC_F32 / AVC_BF16. */
int avc_bilstm_ragged_fwd(const float* xproj, const float* w_hh, const int* lens, const int* lens_dev, int B, int T,
                          int H, float* h, void* h_bf16, int compute, void* stream);

#ifdef __cplusplus
}
#endif
#endif
