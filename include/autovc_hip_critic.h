/* autovc_hip_critic.h -- the loss tail of the GAN trainer's critic step (train_with_gan_ver1.py:149-166) of
 * libautovc_hip.so: the cosine embedding loss between the classifier's style of the converted mel and the target
 * style, the discriminator's two BCE terms, their weighted sum and its addition to the VC loss, and the
 * gradients of all of it.  For e, t (B, E), p_real (n_r), p_fake (n_f), all fp32:
 *
 *   dot_b = sum_k e_bk t_bk    m1_b = sum_k e_bk^2 + 1e-12    m2_b = sum_k t_bk^2 + 1e-12
 *   c_loss = mean_b (1 - dot_b / sqrt(m1_b m2_b))               F.cosine_embedding_loss(e, t, ones(B))
 *   d_loss = mean_i -max(log p_real_i, -100) + mean_i -max(log(1 - p_fake_i), -100)
 *                                                               nn.BCELoss()(p_real, 1) + nn.BCELoss()(p_fake, 0)
 *   extra  = lambda_cls c_loss + lambda_dis d_loss              total = base + extra  (extra without a base)
 *
 * An eleventh header of the same library: the symbols were added without a change to autovc_hip.h, the other
 * headers or AVC_ABI_VERSION (a library that has them still reports the same version; a binding that needs
 * them looks them up and fails if they are missing).
 *
 * Conventions are those of autovc_hip.h: 0 on success, -1 with avc_last_error() set otherwise; every
 * argument is checked on the host BEFORE any launch; `stream` is a hipStream_t.  fp32 throughout, one launch
 * per entry point, no atomics, no workgroup waits on another, no memset, every output element written exactly
 * once, every sum in a fixed order: two calls on the same input are bit-identical.  Rows are read with float4
 * accesses when E and the row strides are multiples of 4 and the bases are 16-byte aligned, single elements
 * otherwise; a lane adds the same elements in the same order in both forms, so both give the same bits.
 */
#ifndef AUTOVC_HIP_CRITIC_H
#define AUTOVC_HIP_CRITIC_H

#include <stddef.h>

#include "autovc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Upper limits.  The forward is ONE workgroup, so these are safety limits, not a working range: the training
 * shape is B <= 64 rows of E = 256 (64 KB per operand) and n_r = n_f = B. */
#define AVC_CRITIC_MAX_B 4096
#define AVC_CRITIC_MAX_E 4096
#define AVC_CRITIC_MAX_N 65536

/* Bytes of workspace for B rows (12 per row, rounded up to 16); 0 for a B the calls refuse. */
size_t avc_critic_loss_ws(int B);

/* out[0..3] = (c_loss, d_loss, extra, total).  One launch of one 256-thread workgroup.
 *   e        fp32 [B][lde], lde >= E;   t  fp32 [B][ldt], ldt >= E
 *   p_real   fp32 [n_r] in [0, 1];   p_fake  fp32 [n_f] in [0, 1]
 *   base     fp32 [1] on the device, or null (total = extra)
 *   out      fp32 [4];   ws  avc_critic_loss_ws(B) bytes: (dot_b, m1_b, m2_b) per row, read by the gradient
 * Refused: a null e / t / p_real / p_fake / out / ws, B or E outside 1..4096, n_r or n_f outside 1..65536,
 * lde < E, ldt < E. */
int avc_critic_loss(const float* e, int lde, const float* t, int ldt, int B, int E, const float* p_real, int n_r,
                    const float* p_fake, int n_f, const float* base, float lambda_cls, float lambda_dis, float* out,
                    void* ws, void* stream);

/* The gradients for upstream gradients g_closs, g_dloss, g_extra, g_total of out[0..3]: device scalars, null
 * meaning absent (zero).  With g_c = lambda_cls (g_extra + g_total) + g_closs and g_d = lambda_dis (g_extra +
 * g_total) + g_dloss:
 *   de_b     = -(g_c / B) (t_b / sqrt(m1_b m2_b) - (dot_b / sqrt(m1_b m2_b)) e_b / m1_b)     [B][ldde], ldde >= E
 *   dp_real  = g_d (p - 1) / max(p (1 - p), 1e-12) / n_r       dp_fake = g_d p / max(p (1 - p), 1e-12) / n_f
 * Each output may be null (not computed).  t is data and has no gradient.  One launch: workgroups 0 .. B - 1
 * take one row of de each, the ones after them 256 elements each of dp_real, then of dp_fake.  Only
 * de[b][0 .. E), dp_real[0 .. n_r) and dp_fake[0 .. n_f) are written: columns E .. ldde keep their bits.
 *   ws       what avc_critic_loss left for the same e, t
 * Refused: what avc_critic_loss refuses (out aside), and ldde < E with de given.  With no output: no launch. */
int avc_critic_loss_grad(const float* e, int lde, const float* t, int ldt, int B, int E, const float* p_real,
                         int n_r, const float* p_fake, int n_f, float lambda_cls, float lambda_dis, const void* ws,
                         const float* g_closs, const float* g_dloss, const float* g_extra, const float* g_total,
                         float* de, int ldde, float* dp_real, float* dp_fake, void* stream);

#ifdef __cplusplus
}
#endif
#endif
