// The loss tail of the StarGAN trainer's cycle step (include/autovc_hip_cycle.h), fp32, deterministic: two cosine
// embedding losses, the discriminator's two BCE terms, the cycle MSE, the weighted sum and its addition to the VC
// loss in one launch; the gradients of all of it in a second.
//
//   c_trans, c_reconst, d_loss: critic_internal.h, in critic_loss.hip's order (the same bits)
//   cycle = mean (y - x)^2        dy = (lambda_cycle g_s + g_cycle) 2 (y - x) / n_x
//
// Forward: the MSE reads 2 n_x floats (2 x 3.6 MB at B = 64, T = 176), so it cannot be one workgroup as
// critic_loss.hip's forward is.  A grid of min(256, ceil(G / 256)) workgroups over the G = ceil(n_x / 4) groups of
// four elements: thread i of the grid owns the groups i, i + 256 grid, ..., and adds their squared differences
// in ascending element order with fmaf -- one float4 load per operand where the layout allows it, single loads
// otherwise (what lies past n_x reads as zero and adds +0): the same additions in the same order.  A butterfly
// per wave, the four waves in wave order, and the workgroup's partial goes to the workspace with a write-through
// store (st_sc1); the workgroup that arrives last at the counter (arrive_last) reads all partials (ld_sc1) and
// adds them in workgroup order.  No workgroup waits on another.  Workgroup 0 also computes the rows and the
// probabilities -- 2 B rows of E floats and n_r + n_f probabilities, small beside its share of the MSE -- and
// hands c_trans, c_reconst and d_loss over the same way.
// Backward: one launch; workgroups 0 .. B - 1 one row of de1 each, the next B one row of de2, then 256
// probabilities each, then 256 groups of dy each; elementwise, every element written once.
#include "../../include/autovc_hip_cycle.h"
#include "critic_internal.h"

namespace {
using namespace critic;
constexpr int GRID_CAP = AVC_CYCLE_GRID;
static_assert(GRID_CAP <= THREADS, "the last workgroup loads one partial per thread");

// the workspace, in floats: [0, 3B) (dot, m1, m2) of pair 1, [3B, 6B) of pair 2, then 4 handed-over scalars
// (c_trans, c_reconst, d_loss, unused), then one partial per workgroup
__host__ __device__ inline size_t hand_at(int B) { return (size_t)6 * B; }
__host__ __device__ inline size_t part_at(int B) { return (size_t)6 * B + 4; }

// elements 4g .. 4g + 3 of v[0 .. n); the scalar form leaves what lies past n at zero
__device__ __forceinline__ f32x4 load_x(const float* __restrict__ v, long long g, long long n, bool vec) {
  if (vec) return reinterpret_cast<const f32x4*>(v)[g];
  f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (4 * g + k < n) r[k] = v[4 * g + k];
  return r;
}

struct Rows {  // both pairs of rows
  const float *e1, *t1, *e2, *t2;
  int lde1, ldt1, lde2, ldt2;
};

template <bool VEC>
__global__ void __launch_bounds__(THREADS)
    cycle_loss_kernel(Rows r, int B, int E, const float* __restrict__ p_real, int n_r,
                      const float* __restrict__ p_fake, int n_f, const float* __restrict__ x,
                      const float* __restrict__ y, long long n_x, int vecx, const float* __restrict__ base,
                      float lambda_cls, float lambda_dis, float lambda_cycle, float* __restrict__ out,
                      float* __restrict__ ws, unsigned* cnt) {
  __shared__ float red[5][WAVES];
  __shared__ float parts[GRID_CAP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* hand = ws + hand_at(B);
  float* part = ws + part_at(B);

  const long long G = (n_x + 3) >> 2, stride = (long long)gridDim.x * THREADS;
  float s = 0.f;
  for (long long g = (long long)blockIdx.x * THREADS + tid; g < G; g += stride) {
    const f32x4 a = load_x(x, g, n_x, vecx), b = load_x(y, g, n_x, vecx);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = b[k] - a[k];
      s = fmaf(d, d, s);
    }
  }
  s = warp_sum(s);
  if (lane == 0) red[4][wave] = s;
  if (blockIdx.x == 0) {
    const float c1 = cos_rows<VEC>(r.e1, r.lde1, r.t1, r.ldt1, B, E, ws, lane, wave);
    const float c2 = cos_rows<VEC>(r.e2, r.lde2, r.t2, r.ldt2, B, E, ws + 3 * (size_t)B, lane, wave);
    const float rpart = real_sum(p_real, n_r, tid), fpart = fake_sum(p_fake, n_f, tid);
    if (lane == 0) {
      red[0][wave] = c1;
      red[1][wave] = rpart;
      red[2][wave] = fpart;
      red[3][wave] = c2;
    }
  }
  __syncthreads();
  if (tid == 0) {
    st_sc1(part + blockIdx.x, sum4(red[4]));
    if (blockIdx.x == 0) {
      const float rm = sum4(red[1]) / (float)n_r, fm = sum4(red[2]) / (float)n_f;
      st_sc1(hand + 0, sum4(red[0]) / (float)B);
      st_sc1(hand + 1, sum4(red[3]) / (float)B);
      st_sc1(hand + 2, rm + fm);
    }
  }
  if (!arrive_last(cnt, gridDim.x)) return;
  // thread t loads workgroup t's partial (all loads in flight at once), thread 0 adds them in workgroup order
  if (tid < (int)gridDim.x) parts[tid] = ld_sc1(part + tid);
  __syncthreads();
  if (tid == 0) {
    float tot = 0.f;
    for (int i = 0; i < (int)gridDim.x; ++i) tot += parts[i];
    const float c1 = ld_sc1(hand + 0), c2 = ld_sc1(hand + 1), d = ld_sc1(hand + 2);
    const float cyc = tot / (float)n_x;
    const float extra = fmaf(lambda_cycle, cyc, fmaf(lambda_dis, d, lambda_cls * (c1 + c2)));
    out[0] = c1;
    out[1] = c2;
    out[2] = d;
    out[3] = cyc;
    out[4] = extra;
    out[5] = base ? base[0] + extra : extra;
  }
}

struct Ups {  // the upstream gradients of out[0..5], null = absent
  const float *ctrans, *creconst, *dloss, *cycle, *extra, *total;
};
__device__ __forceinline__ float dval(const float* p) { return p ? p[0] : 0.f; }

template <bool VEC>
__global__ void __launch_bounds__(THREADS)
    cycle_grad_kernel(Rows r, int B, int E, const float* __restrict__ p_real, int n_r,
                      const float* __restrict__ p_fake, int n_f, const float* __restrict__ x,
                      const float* __restrict__ y, long long n_x, int vecx, float lambda_cls, float lambda_dis,
                      float lambda_cycle, const float* __restrict__ ws, Ups g, float* __restrict__ de1, int ldde1,
                      float* __restrict__ de2, int ldde2, float* __restrict__ dp_real, float* __restrict__ dp_fake,
                      float* __restrict__ dy, int row1_blocks, int row2_blocks, int real_blocks, int fake_blocks) {
  const int tid = threadIdx.x;
  long long blk = blockIdx.x;
  const float g_sum = dval(g.extra) + dval(g.total);
  if (blk < row1_blocks) {
    de_row<VEC>(r.e1, r.lde1, r.t1, r.ldt1, B, E, ws, fmaf(lambda_cls, g_sum, dval(g.ctrans)), de1, ldde1, (int)blk,
                tid);
    return;
  }
  blk -= row1_blocks;
  if (blk < row2_blocks) {
    de_row<VEC>(r.e2, r.lde2, r.t2, r.ldt2, B, E, ws + 3 * (size_t)B, fmaf(lambda_cls, g_sum, dval(g.creconst)), de2,
                ldde2, (int)blk, tid);
    return;
  }
  blk -= row2_blocks;
  if (blk < real_blocks + fake_blocks) {
    const float g_d = fmaf(lambda_dis, g_sum, dval(g.dloss));
    if (blk < real_blocks)
      dp_elem(p_real, dp_real, n_r, (int)blk * THREADS + tid, 1.f, g_d);
    else
      dp_elem(p_fake, dp_fake, n_f, (int)(blk - real_blocks) * THREADS + tid, 0.f, g_d);
    return;
  }
  blk -= real_blocks + fake_blocks;
  const long long G = (n_x + 3) >> 2, gi = blk * THREADS + tid;
  if (gi >= G) return;
  const float coef = fmaf(lambda_cycle, g_sum, dval(g.cycle));
  const f32x4 a = load_x(x, gi, n_x, vecx), b = load_x(y, gi, n_x, vecx);
  f32x4 v;
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = coef * 2.f * (b[k] - a[k]) / (float)n_x;
  if (vecx) {
    reinterpret_cast<f32x4*>(dy)[gi] = v;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (4 * gi + k < n_x) dy[4 * gi + k] = v[k];
  }
}

bool b_ok(int B) { return B >= 1 && B <= AVC_CRITIC_MAX_B; }
bool nx_ok(long long n_x) { return n_x >= 1 && n_x <= AVC_CYCLE_MAX_NX; }
bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the checks both entry points share; `who` names the caller in the message
int check_inputs(const char* who, const Rows& r, int B, int E, const void* p_real, int n_r, const void* p_fake, int n_f,
                 const void* x, const void* y, long long n_x, const void* ws) {
  AVC_CHECK_ARG(r.e1 && r.t1 && r.e2 && r.t2 && p_real && p_fake && x && y && ws,
                "%s: null pointer (e1, t1, e2, t2, p_real, p_fake, x, y and ws are required)", who);
  AVC_CHECK_ARG(b_ok(B) && E >= 1 && E <= AVC_CRITIC_MAX_E,
                "%s: bad shape B = %d, E = %d (1 <= B <= %d, 1 <= E <= %d)", who, B, E, AVC_CRITIC_MAX_B,
                AVC_CRITIC_MAX_E);
  AVC_CHECK_ARG(n_r >= 1 && n_r <= AVC_CRITIC_MAX_N && n_f >= 1 && n_f <= AVC_CRITIC_MAX_N,
                "%s: bad counts n_r = %d, n_f = %d (1 <= n <= %d)", who, n_r, n_f, AVC_CRITIC_MAX_N);
  AVC_CHECK_ARG(nx_ok(n_x), "%s: bad count n_x = %lld (1 <= n_x <= %lld)", who, n_x, AVC_CYCLE_MAX_NX);
  AVC_CHECK_ARG(r.lde1 >= E, "%s: lde1 = %d is below E = %d", who, r.lde1, E);
  AVC_CHECK_ARG(r.ldt1 >= E, "%s: ldt1 = %d is below E = %d", who, r.ldt1, E);
  AVC_CHECK_ARG(r.lde2 >= E, "%s: lde2 = %d is below E = %d", who, r.lde2, E);
  AVC_CHECK_ARG(r.ldt2 >= E, "%s: ldt2 = %d is below E = %d", who, r.ldt2, E);
  return 0;
}

bool rows_vec(const Rows& r, int E) {
  return E % 4 == 0 && r.lde1 % 4 == 0 && r.ldt1 % 4 == 0 && r.lde2 % 4 == 0 && r.ldt2 % 4 == 0 && al16(r.e1) &&
         al16(r.t1) && al16(r.e2) && al16(r.t2);
}
}  // namespace

extern "C" size_t avc_cycle_loss_ws(int B, long long n_x) {
  if (!b_ok(B) || !nx_ok(n_x)) return 0;
  return ((part_at(B) + GRID_CAP) * sizeof(float) + 15) & ~(size_t)15;
}

extern "C" int avc_cycle_loss(const float* e1, int lde1, const float* t1, int ldt1, const float* e2, int lde2,
                              const float* t2, int ldt2, int B, int E, const float* p_real, int n_r,
                              const float* p_fake, int n_f, const float* x, const float* y, long long n_x,
                              const float* base, float lambda_cls, float lambda_dis, float lambda_cycle, float* out,
                              void* ws, void* stream) {
  const Rows r = {e1, t1, e2, t2, lde1, ldt1, lde2, ldt2};
  if (check_inputs("avc_cycle_loss", r, B, E, p_real, n_r, p_fake, n_f, x, y, n_x, ws)) return -1;
  AVC_CHECK_ARG(out, "avc_cycle_loss: null pointer (out is required)");
  hipStream_t s = as_stream(stream);
  unsigned* cnt = avc_counter_slots(1, s);
  if (!cnt) return -1;
  const long long G = (n_x + 3) / 4;
  const int grid = (int)((G + THREADS - 1) / THREADS < GRID_CAP ? (G + THREADS - 1) / THREADS : GRID_CAP);
  const int vecx = n_x % 4 == 0 && al16(x) && al16(y);
  float* w = static_cast<float*>(ws);
  if (rows_vec(r, E))
    cycle_loss_kernel<true><<<dim3(grid), dim3(THREADS), 0, s>>>(r, B, E, p_real, n_r, p_fake, n_f, x, y, n_x, vecx,
                                                                 base, lambda_cls, lambda_dis, lambda_cycle, out, w,
                                                                 cnt);
  else
    cycle_loss_kernel<false><<<dim3(grid), dim3(THREADS), 0, s>>>(r, B, E, p_real, n_r, p_fake, n_f, x, y, n_x, vecx,
                                                                  base, lambda_cls, lambda_dis, lambda_cycle, out, w,
                                                                  cnt);
  return avc_check_launch("avc_cycle_loss");
}

extern "C" int avc_cycle_loss_grad(const float* e1, int lde1, const float* t1, int ldt1, const float* e2, int lde2,
                                   const float* t2, int ldt2, int B, int E, const float* p_real, int n_r,
                                   const float* p_fake, int n_f, const float* x, const float* y, long long n_x,
                                   float lambda_cls, float lambda_dis, float lambda_cycle, const void* ws,
                                   const float* g_ctrans, const float* g_creconst, const float* g_dloss,
                                   const float* g_cycle, const float* g_extra, const float* g_total, float* de1,
                                   int ldde1, float* de2, int ldde2, float* dp_real, float* dp_fake, float* dy,
                                   void* stream) {
  const Rows r = {e1, t1, e2, t2, lde1, ldt1, lde2, ldt2};
  if (check_inputs("avc_cycle_loss_grad", r, B, E, p_real, n_r, p_fake, n_f, x, y, n_x, ws)) return -1;
  AVC_CHECK_ARG(!de1 || ldde1 >= E, "avc_cycle_loss_grad: ldde1 = %d is below E = %d", ldde1, E);
  AVC_CHECK_ARG(!de2 || ldde2 >= E, "avc_cycle_loss_grad: ldde2 = %d is below E = %d", ldde2, E);
  const int row1_blocks = de1 ? B : 0, row2_blocks = de2 ? B : 0;
  const int real_blocks = dp_real ? cdiv(n_r, THREADS) : 0, fake_blocks = dp_fake ? cdiv(n_f, THREADS) : 0;
  const long long G = (n_x + 3) / 4;
  const int dy_blocks = dy ? (int)((G + THREADS - 1) / THREADS) : 0;  // at most 2^21
  const int grid = row1_blocks + row2_blocks + real_blocks + fake_blocks + dy_blocks;
  if (grid == 0) return 0;
  const bool vec = rows_vec(r, E) && (!de1 || (ldde1 % 4 == 0 && al16(de1))) && (!de2 || (ldde2 % 4 == 0 && al16(de2)));
  const int vecx = n_x % 4 == 0 && al16(x) && al16(y) && al16(dy);
  const Ups g = {g_ctrans, g_creconst, g_dloss, g_cycle, g_extra, g_total};
  hipStream_t s = as_stream(stream);
  const float* w = static_cast<const float*>(ws);
  if (vec)
    cycle_grad_kernel<true><<<dim3(grid), dim3(THREADS), 0, s>>>(
        r, B, E, p_real, n_r, p_fake, n_f, x, y, n_x, vecx, lambda_cls, lambda_dis, lambda_cycle, w, g, de1, ldde1, de2,
        ldde2, dp_real, dp_fake, dy, row1_blocks, row2_blocks, real_blocks, fake_blocks);
  else
    cycle_grad_kernel<false><<<dim3(grid), dim3(THREADS), 0, s>>>(
        r, B, E, p_real, n_r, p_fake, n_f, x, y, n_x, vecx, lambda_cls, lambda_dis, lambda_cycle, w, g, de1, ldde1, de2,
        ldde2, dp_real, dp_fake, dy, row1_blocks, row2_blocks, real_blocks, fake_blocks);
  return avc_check_launch("avc_cycle_loss_grad");
}
