/* autovc_hip_xent.h -- softmax cross-entropy of libautovc_hip.so with its gradient and the top-1 count: what
 * trains the MetaDV speaker classifier.  For logits x (B, C) fp32, labels (B) and a label smoothing s, with
 * y_b = (1 - s) * onehot(label_b) + s / C:
 *
 *   L        = mean_b ( logsumexp(x_b) - sum_c y_bc x_bc )       torch's F.cross_entropy(label_smoothing = s)
 *   dlogits  = (softmax(x_b) - y_b) / B                          dL/dx for an upstream gradient of 1
 *   correct  = the number of rows whose largest logit is at label_b (the lowest index wins an exact tie)
 *
 * A tenth header of the same library: the symbols were added without a change to autovc_hip.h, the other
 * headers or AVC_ABI_VERSION (a library that has them still reports the same version; a binding that needs
 * them looks them up and fails if they are missing).
 *
 * Conventions are those of autovc_hip.h: 0 on success, -1 with avc_last_error() set otherwise; every
 * argument is checked on the host BEFORE any launch; `stream` is a hipStream_t.  fp32 throughout.  Two
 * launches of 256-thread workgroups: one workgroup per row (the row maximum first, then the sums of the
 * shifted row, then the row of dlogits), and one finishing workgroup that adds the B row losses and row
 * hits in index order.  Workgroups do not synchronise with each other, spin or use atomics; every sum has
 * a fixed order, so two calls on the same input are bit-identical.
 */
#ifndef AUTOVC_HIP_XENT_H
#define AUTOVC_HIP_XENT_H

#include <stddef.h>

#include "autovc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Upper limits.  A row of AVC_XENT_MAX_C floats is 64 KB: a row workgroup reads its row three times, and
 * the second and third reading are meant to come from the cache; B is one workgroup per row in a
 * one-dimensional grid and one partial per row for the finishing workgroup. */
#define AVC_XENT_MAX_B 65536
#define AVC_XENT_MAX_C 16384

/* Bytes of workspace avc_xent needs for (B, C); 0 for a shape it refuses. */
size_t avc_xent_ws(int B, int C);

/* L, and where they are given dlogits and correct.
 *   logits   fp32 [B][ld], ld >= C;   labels  int32 [B] on the device;   smooth  in [0, 1)
 *   L        fp32 [1];   dlogits  fp32 [B][ldd], ldd >= C, or null;   correct  int32 [1] or null
 *   ws       avc_xent_ws(B, C) bytes, 16-byte aligned; its contents afterwards are unspecified
 * float4 accesses when C, ld (and ldd) are multiples of 4 and logits (and dlogits) are 16-byte aligned,
 * single elements otherwise.  Only L, dlogits[b][0 .. C), correct and ws[0 .. avc_xent_ws) are written:
 * columns C .. ldd of dlogits keep their bits.  dlogits must not alias logits.
 * A label is never used as an address: the target logit is found by comparing column indices.  A label
 * outside [0, C) matches no column; its row reads and writes nothing outside itself, counts as not
 * correct, and makes L NaN so that the error is visible.  (kernels.Labels checks labels on the host.)
 * Refused: a null logits / labels / L / ws, ws not 16-byte aligned, B < 1, C < 1, ld < C, ldd < C with
 * dlogits given, smooth outside [0, 1), B > AVC_XENT_MAX_B, C > AVC_XENT_MAX_C. */
int avc_xent(const float* logits, int ld, int B, int C, const int* labels, float smooth, float* L,
             float* dlogits, int ldd, int* correct, void* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif
