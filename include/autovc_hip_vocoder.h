/* autovc_hip_vocoder.h -- the ragged-batch entry points of the MelGAN generator in libautovc_hip.so:
 * the three glue kernels of csrc/melgan.hip that look ACROSS rows (the reflect gather, the LeakyReLU
 * twin in front of a transposed conv, the output layer) in a form that takes a length per utterance, so
 * that row block b of a batched generator forward is the B = 1 forward of utterance b at its own length.
 *
 * Layout: frame-major, as everywhere.  A stage of the generator whose cumulative upsampling is `scale`
 * (1, 8, 64, 128, 256) holds a batch as [B * Tmax*scale][C]; utterance b occupies the first
 * lens[b]*scale rows of its block of Tmax*scale rows, the rest of the block is padding.  `lens` are
 * MEL-FRAME counts, the same B ints at every stage: the kernels multiply by `scale` themselves.
 *
 * The invariant the three kernels keep (DESIGN "Vocoder over ragged batches"):
 *   - a valid output row reads valid input rows only: reflection is about row 0 and about row
 *     lens[b]*scale - 1 of the utterance's OWN block, never about the block edge;
 *   - every padding row a kernel of this header writes is exactly 0.0 (so the zero-padded 3-tap window of
 *     a transposed conv sees after an utterance's last frame what it sees at B = 1);
 *   - no padding row of an input is ever read: it may hold NaN.
 * Padding rows of the tensors BETWEEN these kernels (GEMM outputs) hold finite values the GEMMs computed
 * from those zeros; no valid row reads them.
 *
 * An eighth header of the same library: the symbols were added without a change to autovc_hip.h,
 * autovc_hip_dv.h, autovc_hip_audio.h, autovc_hip_resample.h, autovc_hip_eval.h, autovc_hip_seg.h,
 * autovc_hip_ragged.h or AVC_ABI_VERSION (a library that has them still reports the same version; a
 * binding that needs them looks them up and fails if one is missing).
 *
 * Conventions are those of autovc_hip.h: 0 on success, -1 with avc_last_error() set otherwise; every
 * argument is checked on the host BEFORE any launch; `stream` is a hipStream_t.  Every entry point is one
 * launch without atomics or inter-workgroup waits; every sum has a fixed order: a batch is bit-identical
 * from run to run and an utterance's result does not depend on the other utterances of the batch.
 *
 * Lengths travel twice, as in autovc_hip_ragged.h: `lens` on the host (checked there) and `lens_dev`, the
 * same ints on the device (read by the kernels, clamped to the block so that a pair that disagrees cannot
 * move an access out of the tensors).  The caller keeps the pair equal.
 *
 * Common refusals: a null x / out / lens / lens_dev, B outside 1..65535, Tmax < 1, scale < 1,
 * Tmax*scale above 2^30, C < 4 or C % 4 != 0 (the kernels move 4 channels per access), a base address
 * that is not aligned to 4 elements, lens[b] outside 1..Tmax.
 */
#ifndef AUTOVC_HIP_VOCODER_H
#define AUTOVC_HIP_VOCODER_H

#include "autovc_hip_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

/* avc_mg_gather (reflect = 1) of a 'same' dilated conv with a length per utterance.  With
 * L = Tmax*scale and n_b = lens[b]*scale, for b < B, t < L, k < taps, c < C:
 *   out[b*L + t][k*C + c] = act(x[b*L + r(t + k*dil - pad)][c])    t <  n_b
 *                         = 0.0                                     t >= n_b
 *   r(s) = -s for s < 0,  2 (n_b - 1) - s for s >= n_b,  s otherwise     (nn.ReflectionPad1d)
 * act != 0: LeakyReLU with `slope` (one fp32 multiply); x and out are fp32 or bf16 (AVC_F32 / AVC_BF16), a
 * bf16 out is the fp32 value rounded once.  With lens[b] = Tmax for every b the output is bit-identical to
 * avc_mg_gather(x, ., B, L, C, taps, dil, pad, 1, act, slope, ...).
 * Refused besides the common list: taps < 1, dil < 1, 2*pad != dil*(taps - 1) (the generator's convs all
 * keep the length), pad >= lens[b]*scale for any b (one reflection must land inside the utterance). */
int avc_mg_gather_ragged(const void* x, int x_dtype, int B, int Tmax, int C, int taps, int dil, int pad, int act,
                         float slope, const int* lens, const int* lens_dev, int scale, void* out, int out_dtype,
                         void* stream);

/* avc_mg_act over [B * Tmax*scale][C] fp32 with a length per utterance: LeakyReLU of the rows
 * t < lens[b]*scale of every block, exact zeros in the rows t >= lens[b]*scale, into out (fp32) and / or
 * out_bf16 (at least one of the two; the bf16 copy is the fp32 result rounded once).
 * Refused besides the common list: neither out nor out_bf16. */
int avc_mg_act_ragged(const float* x, int B, int Tmax, int C, float slope, const int* lens, const int* lens_dev,
                      int scale, float* out, void* out_bf16, void* stream);

/* avc_mg_conv_out with a length per utterance: with L = Tmax*scale, n_b = lens[b]*scale,
 *   out[b*L + t] = tanh(bias[0] + sum_k sum_c w[k][c] * lrelu(x[b*L + r(t + k - 3)][c]))    t <  n_b
 *                = 0.0                                                                       t >= n_b
 * r as above (reflection about n_b - 1), sums in avc_mg_conv_out's order: with lens[b] = Tmax for every b
 * the output is bit-identical to avc_mg_conv_out(x, B, L, C, ...).  x fp32 [B*L][C], w fp32 [7][C].
 * Refused besides the common list: null w / bias, taps != 7, lens[b]*scale <= 3 for any b. */
int avc_mg_conv_out_ragged(const float* x, int B, int Tmax, int C, int taps, const float* w, const float* bias,
                           float slope, const int* lens, const int* lens_dev, int scale, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
