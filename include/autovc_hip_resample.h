/* autovc_hip_resample.h -- the band-limited sample-rate converter of libautovc_hip.so
 * (make_data/make_spec.ipynb: librosa.resample(x, fs, 22050) with the notebook-era
 * res_type='kaiser_best', i.e. resampy's Kaiser-windowed sinc interpolator), as an exact polyphase
 * FIR: for a reduced rate pair fs_out / fs_in = L / M the interpolator's weights depend only on
 * t mod L, so the host tabulates them once (fp64, rounded once to fp32) and the kernel applies them.
 *
 * A fourth header of the same library: the symbols were added without a change to autovc_hip.h,
 * autovc_hip_dv.h, autovc_hip_audio.h or AVC_ABI_VERSION (a library that has them still reports the
 * same version; a binding that needs them looks them up and fails if they are missing).
 *
 * Conventions are those of autovc_hip.h: 0 on success, -1 with avc_last_error() set otherwise;
 * every argument is checked on the host BEFORE any launch; `stream` is a hipStream_t.  The kernel
 * is one launch, does not synchronise between workgroups, spin or use atomics: every sum has a
 * fixed order (taps ascending, one fp32 FMA each).
 *
 * Values that the host checks travel twice, as in autovc_hip_audio.h: `lens` / `tab` on the host
 * and `lens_dev` / `tab_dev`, the same ints on the device (read by the kernel).  The caller keeps
 * each pair equal.
 */
#ifndef AUTOVC_HIP_RESAMPLE_H
#define AUTOVC_HIP_RESAMPLE_H

#include "autovc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AVC_RESAMPLE_MAX_WEIGHTS 131072 /* taps * L of the largest table taken (96000 -> 22050 has 82173) */

/* Per utterance b of lens[b] = N samples (fp32, row b of x, `stride` floats apart), output sample
 * t = j L + r (0 <= r < L):
 *   y[t] = sum_{k = first_r}^{first_r + count_r - 1} weights[k L + r] * x_b[j M + offset_r + k]
 *          with x_b = 0 outside [0, N), for t <  floor(N L / M)
 *   y[t] = 0.0                            for t >= floor(N L / M), up to out_stride
 * Every element of out (B rows, out_stride floats apart) is written: the pad sample of
 * ceil(N L / M) and the padding of a shorter row are zeros, so the caller needs no memset.
 *   weights  device, taps * L floats, tap-major: weights[k][r], consecutive residues adjacent
 *   tab / tab_dev   3 * L ints: offset_r, first_r, count_r for r = 0 .. L - 1; checked on the host:
 *            first_r >= 0, count_r >= 0, first_r + count_r <= taps, and the inputs one period reaches,
 *            max_r (offset_r + first_r + count_r) - min_r (offset_r + first_r), at most M + taps
 * Refused: null pointers, L or M < 1, taps < 1, n_weights != taps * L or above
 * AVC_RESAMPLE_MAX_WEIGHTS, lens[b] < 1, lens[b] > stride, lens[b] > 2^30,
 * out_stride < max_b ceil(lens[b] L / M), B outside 1..65535, and a pair whose M and taps leave no
 * room for one tile in the kernel's LDS budget (avc_resample_tile reports it). */
int avc_resample(const float* x, long long stride, const int* lens, const int* lens_dev, int B, const float* weights,
                 int n_weights, const int* tab, const int* tab_dev, int L, int M, int taps, float* out,
                 long long out_stride, void* stream);

/* Output samples one workgroup of avc_resample produces for this L, M, taps (a multiple of L), or -1
 * with the error set when no tile fits.  Host arithmetic only. */
int avc_resample_tile(int L, int M, int taps);

#ifdef __cplusplus
}
#endif
#endif
