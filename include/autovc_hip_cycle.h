/* autovc_hip_cycle.h -- the loss tail of the StarGAN trainer's cycle step (train_with_stargan.py:162-188) of
 * libautovc_hip.so: the two cosine embedding losses (the classifier's style of the converted mel against the
 * target style, of the reconstructed mel against the source style), the discriminator's two BCE terms, the cycle
 * MSE between the source mel and its reconstruction, their weighted sum and its addition to the VC loss, and the
 * gradients of all of it.  For e1, t1, e2, t2 (B, E), p_real (n_r), p_fake (n_f), x, y (n_x), all fp32:
 *
 *   c_trans   = F.cosine_embedding_loss(e1, t1, ones(B))        c_reconst = F.cosine_embedding_loss(e2, t2, ones(B))
 *   d_loss    = nn.BCELoss()(p_real, 1) + nn.BCELoss()(p_fake, 0)                 (both as autovc_hip_critic.h)
 *   cycle     = mean_i (y_i - x_i)^2                             F.mse_loss(x, y)
 *   extra     = lambda_cls (c_trans + c_reconst) + lambda_dis d_loss + lambda_cycle cycle
 *   total     = base + extra                                     (extra without a base)
 *
 * A twelfth header of the same library: the symbols were added without a change to autovc_hip.h, the other
 * headers or AVC_ABI_VERSION (a library that has them still reports the same version; a binding that needs
 * them looks them up and fails if they are missing).
 *
 * Conventions are those of autovc_hip_critic.h: 0 on success, -1 with avc_last_error() set otherwise; every
 * argument is checked on the host BEFORE any launch; `stream` is a hipStream_t.  fp32 throughout, one launch per
 * entry point, no memset, no workgroup waits on another, every output element written exactly once, every sum
 * in a fixed order: two calls on the same input are bit-identical.  The float4 form (rows: E and the four row
 * strides multiples of 4 and the four bases 16-byte aligned; x, y, dy: n_x a multiple of 4 and the bases 16-byte
 * aligned) and the single-element form give the same bits: a thread owns the same four elements per group in
 * both and adds them in the same order.  c_trans and d_loss carry the bits avc_critic_loss gives for (e1, t1,
 * p_real, p_fake), de1, dp_real and dp_fake the bits of avc_critic_loss_grad for the same g_c and g_d.
 */
#ifndef AUTOVC_HIP_CYCLE_H
#define AUTOVC_HIP_CYCLE_H

#include <stddef.h>

#include "autovc_hip_critic.h"

#ifdef __cplusplus
extern "C" {
#endif

/* B, E, n_r, n_f: the limits of autovc_hip_critic.h.  n_x: 1 .. 2^31 - 1. */
#define AVC_CYCLE_MAX_NX 2147483647LL
/* The forward's grid cap: min(256, ceil(ceil(n_x / 4) / 256)) workgroups of 256 threads. */
#define AVC_CYCLE_GRID 256

/* Bytes of workspace: (dot, m1, m2) per row of both pairs, three handed-over scalars and one partial per
 * workgroup of the forward, rounded up to 16; 0 for a B or an n_x the calls refuse. */
size_t avc_cycle_loss_ws(int B, long long n_x);

/* out[0..5] = (c_trans, c_reconst, d_loss, cycle, extra, total).  One launch: a capped grid reads x and y with
 * grid-stride float4 loads (group g of four elements belongs to thread g mod (256 grid) of the grid), each
 * workgroup hands its partial over with a write-through store, the last one to arrive adds the partials in
 * workgroup order; workgroup 0 also computes the rows and the probabilities, in avc_critic_loss's order.
 *   e1, t1, e2, t2   fp32 [B][ld], each ld >= E
 *   p_real  fp32 [n_r] in [0, 1];   p_fake  fp32 [n_f] in [0, 1];   x, y  fp32 [n_x]
 *   base    fp32 [1] on the device, or null (total = extra)
 *   out     fp32 [6];   ws  avc_cycle_loss_ws(B, n_x) bytes, read by the gradient
 * Refused: a null e1 / t1 / e2 / t2 / p_real / p_fake / x / y / out / ws, B or E outside 1..4096, n_r or n_f
 * outside 1..65536, n_x outside 1..2^31 - 1, a row stride below E. */
int avc_cycle_loss(const float* e1, int lde1, const float* t1, int ldt1, const float* e2, int lde2, const float* t2,
                   int ldt2, int B, int E, const float* p_real, int n_r, const float* p_fake, int n_f, const float* x,
                   const float* y, long long n_x, const float* base, float lambda_cls, float lambda_dis,
                   float lambda_cycle, float* out, void* ws, void* stream);

/* The gradients for upstream gradients g_ctrans, g_creconst, g_dloss, g_cycle, g_extra, g_total of out[0..5]:
 * device scalars, null meaning absent (zero).  With g_s = g_extra + g_total:
 *   de1      avc_critic_loss_grad's de for g_c = lambda_cls g_s + g_ctrans           [B][ldde1], ldde1 >= E
 *   de2      the same for (e2, t2) and g_c = lambda_cls g_s + g_creconst             [B][ldde2], ldde2 >= E
 *   dp_real, dp_fake   avc_critic_loss_grad's for g_d = lambda_dis g_s + g_dloss
 *   dy       = (lambda_cycle g_s + g_cycle) 2 (y - x) / n_x                           [n_x]
 * Each output may be null (not computed).  t1, t2 and x are data and have no gradient.  One launch: workgroups
 * 0 .. B - 1 take one row of de1 each, the next B one row of de2, the ones after them 256 elements each of
 * dp_real, then of dp_fake, the rest 1024 elements of dy each.  Only de[b][0 .. E), dp_real[0 .. n_r),
 * dp_fake[0 .. n_f) and dy[0 .. n_x) are written: columns E .. ldde keep their bits.
 *   ws       what avc_cycle_loss left for the same inputs
 * Refused: what avc_cycle_loss refuses (out aside), and ldde1 < E with de1 given, ldde2 < E with de2 given.
 * With no output: no launch. */
int avc_cycle_loss_grad(const float* e1, int lde1, const float* t1, int ldt1, const float* e2, int lde2,
                        const float* t2, int ldt2, int B, int E, const float* p_real, int n_r, const float* p_fake,
                        int n_f, const float* x, const float* y, long long n_x, float lambda_cls, float lambda_dis,
                        float lambda_cycle, const void* ws, const float* g_ctrans, const float* g_creconst,
                        const float* g_dloss, const float* g_cycle, const float* g_extra, const float* g_total,
                        float* de1, int ldde1, float* de2, int ldde2, float* dp_real, float* dp_fake, float* dy,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
