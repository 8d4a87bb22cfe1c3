// The loss tail of the GAN trainer's critic step (include/autovc_hip_critic.h), fp32, deterministic: the cosine
// embedding loss of (e, t), the two BCE terms of the discriminator, the weighted sum and its addition to the VC
// loss in one launch; the gradients of all of it in a second.
//
//   dot = sum e t, m1 = sum e^2 + 1e-12, m2 = sum t^2 + 1e-12, cos = dot / sqrt(m1 m2)      (ATen's formula)
//   c_loss = mean_b (1 - cos_b)
//   d_loss = mean -max(log p_real, -100) + mean -max(log1p(-p_fake), -100)
//   de_b   = -(g_c / B) (t_b / sqrt(m1 m2) - (dot / sqrt(m1 m2)) e_b / m1)
//   dp     = g_d (p - y) / max(p (1 - p), 1e-12) / n
//
// Forward: ONE 256-thread workgroup.  Wave w takes rows w, w + 4, ...; lane l of it takes the column groups
// 4u .. 4u + 3, u = l, l + 64, ..., and adds their products in ascending column order with fmaf -- as one
// float4 load per operand where the layout allows it, as single loads otherwise: the same additions in the
// same order, hence the same bits in both forms.  A 64-wide shuffle butterfly ends the row; (dot, m1, m2) go
// to the workspace for the gradient, 1 - cos to the wave's partial in row order.  Thread i takes the
// probabilities i, i + 256, ...; a butterfly per wave, then the four waves' partials through LDS, added in
// wave order by thread 0.  Backward: one workgroup per row of de, then one per 256 probabilities; elementwise.
// The launch is latency, not arithmetic: the training shape is B <= 64, E = 256, n = B.
#include "../../include/autovc_hip_critic.h"
#include "critic_internal.h"

namespace {
using namespace critic;  // the rows, the sums and their gradients: shared with cycle_loss.hip, one order for both

template <bool VEC>
__global__ void __launch_bounds__(THREADS)
    critic_loss_kernel(const float* __restrict__ e, int lde, const float* __restrict__ t, int ldt, int B, int E,
                       const float* __restrict__ p_real, int n_r, const float* __restrict__ p_fake, int n_f,
                       const float* __restrict__ base, float lambda_cls, float lambda_dis, float* __restrict__ out,
                       float* __restrict__ ws) {
  __shared__ float red[3][WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float cpart = cos_rows<VEC>(e, lde, t, ldt, B, E, ws, lane, wave);
  const float rpart = real_sum(p_real, n_r, tid), fpart = fake_sum(p_fake, n_f, tid);
  if (lane == 0) {
    red[0][wave] = cpart;
    red[1][wave] = rpart;
    red[2][wave] = fpart;
  }
  __syncthreads();
  if (tid == 0) {
    const float c = sum4(red[0]) / (float)B;
    const float r = sum4(red[1]) / (float)n_r;
    const float f = sum4(red[2]) / (float)n_f;
    const float d = r + f;
    const float extra = fmaf(lambda_dis, d, lambda_cls * c);
    out[0] = c;
    out[1] = d;
    out[2] = extra;
    out[3] = base ? base[0] + extra : extra;
  }
}

template <bool VEC>
__global__ void __launch_bounds__(THREADS)
    critic_grad_kernel(const float* __restrict__ e, int lde, const float* __restrict__ t, int ldt, int B, int E,
                       const float* __restrict__ p_real, int n_r, const float* __restrict__ p_fake, int n_f,
                       float lambda_cls, float lambda_dis, const float* __restrict__ ws,
                       const float* __restrict__ g_closs, const float* __restrict__ g_dloss,
                       const float* __restrict__ g_extra, const float* __restrict__ g_total, float* __restrict__ de,
                       int ldde, float* __restrict__ dp_real, float* __restrict__ dp_fake, int row_blocks,
                       int real_blocks) {
  const int tid = threadIdx.x;
  int blk = blockIdx.x;
  const float g_sum = (g_extra ? g_extra[0] : 0.f) + (g_total ? g_total[0] : 0.f);
  if (blk < row_blocks) {  // row blk of de
    const float g_c = fmaf(lambda_cls, g_sum, g_closs ? g_closs[0] : 0.f);
    de_row<VEC>(e, lde, t, ldt, B, E, ws, g_c, de, ldde, blk, tid);
    return;
  }
  blk -= row_blocks;
  const float g_d = fmaf(lambda_dis, g_sum, g_dloss ? g_dloss[0] : 0.f);
  const bool real = blk < real_blocks;
  if (!real) blk -= real_blocks;
  const int i = blk * THREADS + tid;
  if (real)
    dp_elem(p_real, dp_real, n_r, i, 1.f, g_d);
  else
    dp_elem(p_fake, dp_fake, n_f, i, 0.f, g_d);
}

bool b_ok(int B) { return B >= 1 && B <= AVC_CRITIC_MAX_B; }

// the checks both entry points share; `who` names the caller in the message
int check_inputs(const char* who, const void* e, int lde, const void* t, int ldt, int B, int E, const void* p_real,
                 int n_r, const void* p_fake, int n_f, const void* ws) {
  AVC_CHECK_ARG(e && t && p_real && p_fake && ws, "%s: null pointer (e, t, p_real, p_fake and ws are required)", who);
  AVC_CHECK_ARG(b_ok(B) && E >= 1 && E <= AVC_CRITIC_MAX_E,
                "%s: bad shape B = %d, E = %d (1 <= B <= %d, 1 <= E <= %d)", who, B, E, AVC_CRITIC_MAX_B,
                AVC_CRITIC_MAX_E);
  AVC_CHECK_ARG(n_r >= 1 && n_r <= AVC_CRITIC_MAX_N && n_f >= 1 && n_f <= AVC_CRITIC_MAX_N,
                "%s: bad counts n_r = %d, n_f = %d (1 <= n <= %d)", who, n_r, n_f, AVC_CRITIC_MAX_N);
  AVC_CHECK_ARG(lde >= E, "%s: lde = %d is below E = %d", who, lde, E);
  AVC_CHECK_ARG(ldt >= E, "%s: ldt = %d is below E = %d", who, ldt, E);
  return 0;
}
}  // namespace

extern "C" size_t avc_critic_loss_ws(int B) {
  return b_ok(B) ? (((size_t)B * 3 * sizeof(float)) + 15) & ~(size_t)15 : 0;
}

extern "C" int avc_critic_loss(const float* e, int lde, const float* t, int ldt, int B, int E, const float* p_real,
                               int n_r, const float* p_fake, int n_f, const float* base, float lambda_cls,
                               float lambda_dis, float* out, void* ws, void* stream) {
  if (check_inputs("avc_critic_loss", e, lde, t, ldt, B, E, p_real, n_r, p_fake, n_f, ws)) return -1;
  AVC_CHECK_ARG(out, "avc_critic_loss: null pointer (out is required)");
  const bool vec = E % 4 == 0 && lde % 4 == 0 && ldt % 4 == 0 && (((uintptr_t)e | (uintptr_t)t) & 15) == 0;
  hipStream_t s = as_stream(stream);
  float* w = static_cast<float*>(ws);
  if (vec)
    critic_loss_kernel<true><<<dim3(1), dim3(THREADS), 0, s>>>(e, lde, t, ldt, B, E, p_real, n_r, p_fake, n_f, base,
                                                               lambda_cls, lambda_dis, out, w);
  else
    critic_loss_kernel<false><<<dim3(1), dim3(THREADS), 0, s>>>(e, lde, t, ldt, B, E, p_real, n_r, p_fake, n_f, base,
                                                                lambda_cls, lambda_dis, out, w);
  return avc_check_launch("avc_critic_loss");
}

extern "C" int avc_critic_loss_grad(const float* e, int lde, const float* t, int ldt, int B, int E,
                                    const float* p_real, int n_r, const float* p_fake, int n_f, float lambda_cls,
                                    float lambda_dis, const void* ws, const float* g_closs, const float* g_dloss,
                                    const float* g_extra, const float* g_total, float* de, int ldde, float* dp_real,
                                    float* dp_fake, void* stream) {
  if (check_inputs("avc_critic_loss_grad", e, lde, t, ldt, B, E, p_real, n_r, p_fake, n_f, ws)) return -1;
  AVC_CHECK_ARG(!de || ldde >= E, "avc_critic_loss_grad: ldde = %d is below E = %d", ldde, E);
  const int row_blocks = de ? B : 0;
  const int real_blocks = dp_real ? cdiv(n_r, THREADS) : 0, fake_blocks = dp_fake ? cdiv(n_f, THREADS) : 0;
  const int grid = row_blocks + real_blocks + fake_blocks;
  if (grid == 0) return 0;
  const bool vec = E % 4 == 0 && lde % 4 == 0 && ldt % 4 == 0 && (!de || ldde % 4 == 0) &&
                   (((uintptr_t)e | (uintptr_t)t | (uintptr_t)de) & 15) == 0;
  hipStream_t s = as_stream(stream);
  const float* w = static_cast<const float*>(ws);
  if (vec)
    critic_grad_kernel<true><<<dim3(grid), dim3(THREADS), 0, s>>>(e, lde, t, ldt, B, E, p_real, n_r, p_fake, n_f,
                                                                  lambda_cls, lambda_dis, w, g_closs, g_dloss, g_extra,
                                                                  g_total, de, ldde, dp_real, dp_fake, row_blocks,
                                                                  real_blocks);
  else
    critic_grad_kernel<false><<<dim3(grid), dim3(THREADS), 0, s>>>(e, lde, t, ldt, B, E, p_real, n_r, p_fake, n_f,
                                                                   lambda_cls, lambda_dis, w, g_closs, g_dloss,
                                                                   g_extra, g_total, de, ldde, dp_real, dp_fake,
                                                                   row_blocks, real_blocks);
  return avc_check_launch("avc_critic_loss_grad");
}
