/* autovc_hip_ge2e.h -- the GE2E loss (Wan et al. 2018, softmax form) of libautovc_hip.so: what trains the
 * LstmDV speaker embedder.  For e (N, M, D) fp32 -- N speakers, M utterances each, row-major, rows of any
 * norm -- and a scalar w, with cos = cosine_similarity(.., eps = 1e-8):
 *
 *   c[k]       = mean_i e[k, i]                                   the inclusive centroids
 *   c_ex[j, i] = (sum_i' e[j, i'] - e[j, i]) / (M - 1)            own centroid without the utterance itself
 *   S[j, i, k] = cos(e[j, i], c[k])  (k != j),   S[j, i, j] = cos(e[j, i], c_ex[j, i])
 *   L          = mean over the N*M rows of  -log softmax_k(w * S[j, i, :])[j]
 *
 * The usual additive bias b is left out: cross-entropy does not change when a constant is added to a row, so
 * L does not depend on b and its gradient is identically zero.
 *
 * A ninth header of the same library: the symbols were added without a change to autovc_hip.h, the other
 * headers or AVC_ABI_VERSION (a library that has them still reports the same version; a binding that needs
 * them looks them up and fails if they are missing).
 *
 * Conventions are those of autovc_hip.h: 0 on success, -1 with avc_last_error() set otherwise; every
 * argument is checked on the host BEFORE any launch; `stream` is a hipStream_t.  fp32 throughout.  Three
 * launches (two without the gradients), 256-thread workgroups: per-speaker sums; one workgroup per row for
 * the similarity row, softmax, loss partial and the row's own gradient terms; one workgroup per speaker for
 * the centroid terms, the assembly of de and the final sums.  Workgroups do not synchronise with each other,
 * spin or use atomics; every sum has a fixed order, so two calls on the same input are bit-identical.
 */
#ifndef AUTOVC_HIP_GE2E_H
#define AUTOVC_HIP_GE2E_H

#include <stddef.h>

#include "autovc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Upper limits, from the LDS layout: a row workgroup keeps its row and one D-vector of partial results plus
 * two N-vectors, a speaker workgroup one N*M-vector (its column of coefficients) plus one D-vector. */
#define AVC_GE2E_MAX_N 1024
#define AVC_GE2E_MAX_M 1024
#define AVC_GE2E_MAX_D 2048
#define AVC_GE2E_MAX_ROWS 8192 /* N * M */

/* Bytes of workspace avc_ge2e needs for (N, M, D); 0 for a shape it refuses. */
size_t avc_ge2e_ws(int N, int M, int D);

/* L (and, where de and dw are given, dL/de and dL/dw for an upstream gradient of 1).
 *   e   fp32 [N][M][D], contiguous;   w  fp32 [1] on the device
 *   L   fp32 [1];   de  fp32 [N][M][D] or null;   dw  fp32 [1] or null (de and dw: both or neither)
 *   ws  avc_ge2e_ws(N, M, D) bytes, 16-byte aligned; its contents afterwards are unspecified
 * float4 accesses when D % 4 == 0 and e (and de) are 16-byte aligned, single elements otherwise.
 * Only L, de, dw and ws[0 .. avc_ge2e_ws) are written; de must not alias e.
 * A norm below eps = 1e-8 is clamped to eps and then counts as a constant (torch's cosine_similarity).
 * Refused: a null e / w / L / ws, exactly one of de / dw, ws not 16-byte aligned, N < 2, M < 2, D < 1,
 * N > AVC_GE2E_MAX_N, M > AVC_GE2E_MAX_M, D > AVC_GE2E_MAX_D, N * M > AVC_GE2E_MAX_ROWS. */
int avc_ge2e(const float* e, int N, int M, int D, const float* w, float* L, float* de, float* dw, void* ws,
             void* stream);

#ifdef __cplusplus
}
#endif
#endif
