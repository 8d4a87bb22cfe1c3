/* autovc_hip_dv.h -- the MetaDV speaker-classifier entry points of libautovc_hip.so
 * (factory/MetaDV.py: LSTM(80 -> E) -> S random W-frame windows, each read as a Conv1d input with
 * the window frames as channels -> MLP-Mixer -> one output channel -> mean -> two linears).
 *
 * A second header of the same library: these symbols were added without a change to
 * autovc_hip.h or to AVC_ABI_VERSION (a library that has them still reports the same version;
 * a binding that needs them looks the symbols up and fails if one is missing).
 *
 * Conventions are those of autovc_hip.h: every function returns 0 on success and -1 with
 * avc_last_error() set otherwise; every argument is checked on the host BEFORE any launch;
 * `stream` is a hipStream_t; dtypes are AVC_F32 / AVC_BF16.  None of the kernels synchronises
 * between workgroups, spins or uses atomics: every sum has a fixed order.
 *
 * Window starts travel twice: `left` on the host (S*B ints, checked here against the frame counts)
 * and `left_dev`, the same values on the device (read by the kernel).  Entry s*B + b is the first
 * frame of crop s of utterance b.  The caller keeps the two equal.
 */
#ifndef AUTOVC_HIP_DV_H
#define AUTOVC_HIP_DV_H

#include "autovc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* X[(s*B + b)*E + l][c] = h[b][left[s*B + b] + c][l]   (0 <= c < W, 0 <= l < E)
 * h (B, T, E) of h_dtype, X (S*B*E, W) of x_dtype (fp32 h may be written as bf16; bf16 h as fp32 is
 * refused: nothing needs it).  lens (host, nullable = all T): frames of utterance b; every start
 * must satisfy 0 <= left <= lens[b] - W. */
int avc_crop_windows(const void* h, int h_dtype, const int* left, const int* left_dev, const int* lens, int B, int T,
                     int E, int W, int S, void* X, int x_dtype, void* stream);

/* dh[b][t][l] = sum over crops s with left <= t < left + W of dX[(s*B + b)*E + l][t - left]
 *               + (t == last[b] ? de1[b][l] : 0)
 * dX (S*B*E, W) fp32, dh (B, T, E) fp32 -- every element is written (zeros outside all windows).
 * de1 (B, E) nullable.  last / last_dev (host / device, B ints in 0..T-1; both null = T - 1). */
int avc_crop_windows_bwd(const float* dX, const float* de1, const int* left, const int* left_dev, const int* last,
                         const int* last_dev, int B, int T, int E, int W, int S, float* dh, void* stream);

/* e2[b][l] = (1/S) sum_s Y[(s*B + b)*E + l][O - 1],  Y (S*B*E, O) fp32, e2 (B, E) fp32 */
int avc_chan_mean(const float* Y, int S, int B, int E, int O, float* e2, void* stream);

/* dY (S*B*E, O), all of it: g[b][l] / S in column O - 1, zero elsewhere */
int avc_chan_mean_bwd(const float* g, int S, int B, int E, int O, float* dY, void* stream);

/* The forward-only head, one launch, fp32:
 *   e2  = the avc_chan_mean of Y (S crops, O channels)
 *   emb = W_dv . cat(e1[b], e2[b]) + b_dv        W_dv (D, 2E), b_dv (D) nullable
 *   d_vec[b] = emb / ||emb||_2                    (B, D)
 *   pred[b]  = W_out . emb + b_out                W_out (C, D), b_out (C) nullable, pred (B, C)
 * E a multiple of 4; (2E + D) floats of LDS. */
int avc_metadv_head(const float* e1, const float* Y, int S, int O, const float* w_dv, const float* b_dv,
                    const float* w_out, const float* b_out, int B, int E, int D, int C, float* pred, float* d_vec,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
