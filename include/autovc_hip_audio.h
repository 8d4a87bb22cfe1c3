/* autovc_hip_audio.h -- the waveform -> log-mel entry point of libautovc_hip.so
 * (melgan/modules.py Audio2Mel, make_data/make_spec.ipynb mel_gan_handler: reflect pad, STFT with a
 * periodic Hann window, magnitude, mel filterbank, log10 of the clamped result).
 *
 * A third header of the same library: the symbol was added without a change to autovc_hip.h,
 * autovc_hip_dv.h or AVC_ABI_VERSION (a library that has it still reports the same version; a
 * binding that needs it looks the symbol up and fails if it is missing).
 *
 * Conventions are those of autovc_hip.h: 0 on success, -1 with avc_last_error() set otherwise;
 * every argument is checked on the host BEFORE any launch; `stream` is a hipStream_t.  The kernel
 * is one launch, does not synchronise between workgroups, spin or use atomics: every sum has a
 * fixed order.
 *
 * Values that the host checks travel twice, as in autovc_hip_dv.h: `lens` / `filt` on the host and
 * `lens_dev` / `filt_dev`, the same ints on the device (read by the kernel).  The caller keeps
 * each pair equal.
 */
#ifndef AUTOVC_HIP_AUDIO_H
#define AUTOVC_HIP_AUDIO_H

#include "autovc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AVC_MEL_FRAME_MAJOR 0   /* out[b][t][m], (B, Tmax, n_mel) */
#define AVC_MEL_CHANNEL_MAJOR 1 /* out[b][m][t], (B, n_mel, Tmax) */
#define AVC_MEL_MAX_WEIGHTS 8192 /* compact filterbank weights that fit the kernel's LDS budget */

/* Per utterance b of lens[b] = L samples (fp32, row b of audio, `stride` floats apart), p = 384:
 *   x'      = reflect_pad(scale[b] * x_b, p, p)          (i < 0 -> -i, i >= L -> 2(L-1) - i)
 *   frame_t = x'[256 t : 256 t + 1024] * window           t = 0 .. T_b - 1, T_b = (L + 2p - 1024)/256 + 1
 *   mag     = |rfft(frame_t)|                             513 bins, fp32 FFT
 *   mel[m]  = sum_{i < count_m} weights[offset_m + i] * mag[start_m + i]
 *   out     = log10(max(mel, floor))                      frames t >= T_b are written as 0.0
 * Every element of out is written.  n_fft = win = 1024 and hop = 256 are the only supported values.
 *   scale    device, B floats, nullable (= 1)
 *   window   device, 1024 floats
 *   twiddle  device, 513 (cos, -sin) pairs of the angles 2 pi m / 1024, m = 0 .. 512
 *   filt / filt_dev   3 * n_mel ints: start_m, count_m, offset_m for m = 0 .. n_mel - 1; checked on the
 *            host: start_m + count_m <= 513, offset_m + count_m <= n_weights
 *   weights  device, n_weights <= AVC_MEL_MAX_WEIGHTS floats
 * Refused: null pointers, lens[b] <= 384 (the reflection needs pad < length), lens[b] > stride,
 * Tmax < max T_b, n_mel outside 1..128, an unknown layout, other n_fft / win / hop. */
int avc_audio2mel(const float* audio, long long stride, const int* lens, const int* lens_dev, const float* scale, int B,
                  const float* window, const float* twiddle, const int* filt, const int* filt_dev, const float* weights,
                  int n_weights, int n_mel, int n_fft, int win, int hop, float floor, float* out, int Tmax, int layout,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif
