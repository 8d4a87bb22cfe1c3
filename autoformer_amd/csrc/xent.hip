// Softmax cross-entropy with label smoothing, its gradient and the top-1 count (include/autovc_hip_xent.h),
// fp32, deterministic.
//
// With m = max_c x_c, v_c = x_c - m, se = sum_c exp(v_c), keep = 1 - s and y_c = keep [c == label] + s / C
// (the y_c sum to one, so the shift by m drops out of the loss):
//
//   L_b      = log(se) - keep v_label - (s / C) sum_c v_c
//   dlogits  = ((exp(v_c) / se - s / C) - keep [c == label]) / B
//   hit_b    = [the first c with v_c == 0 is the label]
//
// Two launches: xent_rows (one 256-thread workgroup per row: the maximum, then se, sum v, v_label and the first
// index of the maximum in one pass over the shifted row, then the row of dlogits; L_b and hit_b go to the
// workspace), xent_finish (one workgroup: L = sum_b L_b / B and correct = sum_b hit_b).  The row is read from
// global memory each time (three times with the gradient): it is 64 KB at most and 1 KB at the training shape,
// so the second and third reading come from the cache.  The label is compared with column indices and never
// used as an address; a row whose label matches no column gets L_b = NaN.  Every sum has a fixed order: ascending
// per thread (four lanes of a float4 apart, then (0 + 1) + (2 + 3)), a shuffle butterfly per wave, the waves in
// index order.  No atomics, no workgroup waits on another.
#include <limits.h>
#include <math.h>

#include "../../include/autovc_hip_xent.h"
#include "common.h"

namespace {
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;

static inline size_t r4(size_t v) { return (v + 3) & ~(size_t)3; }

template <typename V>
struct Width;
template <>
struct Width<float> {
  static constexpr int W = 1;
};
template <>
struct Width<f32x4> {
  static constexpr int W = 4;
};
__device__ __forceinline__ float at(const float& v, int) { return v; }
__device__ __forceinline__ float at(const f32x4& v, int k) { return v[k]; }
__device__ __forceinline__ void put(float& v, int, float s) { v = s; }
__device__ __forceinline__ void put(f32x4& v, int k, float s) { v[k] = s; }
__device__ __forceinline__ float hsum(float v) { return v; }
__device__ __forceinline__ float hsum(const f32x4& v) { return (v[0] + v[1]) + (v[2] + v[3]); }

__device__ __forceinline__ float warp_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int warp_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int warp_sumi(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// d == nullptr: the loss and hit partials only
template <typename V>
__global__ void __launch_bounds__(THREADS)
    xent_rows(const float* __restrict__ x, int ld, int C, const int* __restrict__ labels, float smooth, float invB,
              float* __restrict__ lossp, int* __restrict__ hitp, float* __restrict__ d, int ldd) {
  __shared__ float redf[WAVES][4];
  __shared__ int redi[WAVES][2];
  constexpr int W = Width<V>::W;
  const int U = C / W, t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.x;
  const V* xr = reinterpret_cast<const V*>(x + (size_t)b * ld);
  const int label = labels[b];  // a value to compare column indices with, never an index

  float m = -INFINITY;
  for (int u = t; u < U; u += THREADS) {
    const V v = xr[u];
#pragma unroll
    for (int k = 0; k < W; ++k) m = fmaxf(m, at(v, k));
  }
  m = warp_max(m);
  if (lane == 0) redf[wave][0] = m;
  __syncthreads();
  m = fmaxf(fmaxf(redf[0][0], redf[1][0]), fmaxf(redf[2][0], redf[3][0]));
  __syncthreads();  // redf is reused below

  V sev{}, sxv{};
  float xt = 0.f;
  int found = 0, first = INT_MAX;
  for (int u = t; u < U; u += THREADS) {
    const V v = xr[u] - m;
    V e;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const int c = u * W + k;
      const float vk = at(v, k);
      put(e, k, expf(vk));
      if (c == label) {
        xt = vk;
        found = 1;
      }
      if (vk == 0.f) first = min(first, c);
    }
    sev += e;
    sxv += v;
  }
  float se = warp_sum(hsum(sev)), sx = warp_sum(hsum(sxv));
  xt = warp_sum(xt);  // one thread of the row holds it, the others 0
  found = warp_sumi(found);
  first = warp_min(first);
  if (lane == 0) {
    redf[wave][0] = se;
    redf[wave][1] = sx;
    redf[wave][2] = xt;
    redi[wave][0] = found;
    redi[wave][1] = first;
  }
  __syncthreads();
  se = (redf[0][0] + redf[1][0]) + (redf[2][0] + redf[3][0]);
  sx = (redf[0][1] + redf[1][1]) + (redf[2][1] + redf[3][1]);
  xt = (redf[0][2] + redf[1][2]) + (redf[2][2] + redf[3][2]);
  found = (redi[0][0] + redi[1][0]) + (redi[2][0] + redi[3][0]);
  first = min(min(redi[0][1], redi[1][1]), min(redi[2][1], redi[3][1]));

  const float keep = 1.f - smooth, sC = smooth / (float)C;
  if (t == 0) {
    float Lb = logf(se) - keep * xt;
    if (smooth > 0.f) Lb -= sC * sx;
    lossp[b] = found ? Lb : NAN;
    hitp[b] = (found && first == label) ? 1 : 0;
  }
  if (d == nullptr) return;

  const float inv = 1.f / se;
  V* dr = reinterpret_cast<V*>(d + (size_t)b * ldd);
  for (int u = t; u < U; u += THREADS) {
    const V v = xr[u] - m;
    V g;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const int c = u * W + k;
      const float p = expf(at(v, k)) * inv;
      put(g, k, ((p - sC) - (c == label ? keep : 0.f)) * invB);
    }
    dr[u] = g;
  }
}

__global__ void __launch_bounds__(THREADS)
    xent_finish(const float* __restrict__ lossp, const int* __restrict__ hitp, int B, float* __restrict__ L,
                int* __restrict__ correct) {
  __shared__ float redf[WAVES];
  __shared__ int redi[WAVES];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float l = 0.f;
  int h = 0;
  for (int r = t; r < B; r += THREADS) {
    l += lossp[r];
    h += hitp[r];
  }
  l = warp_sum(l);
  h = warp_sumi(h);
  if (lane == 0) {
    redf[wave] = l;
    redi[wave] = h;
  }
  __syncthreads();
  if (t == 0) {
    L[0] = ((redf[0] + redf[1]) + (redf[2] + redf[3])) / (float)B;
    if (correct) correct[0] = (redi[0] + redi[1]) + (redi[2] + redi[3]);
  }
}

bool shape_ok(int B, int C) { return B >= 1 && C >= 1 && B <= AVC_XENT_MAX_B && C <= AVC_XENT_MAX_C; }

template <typename V>
int run(const float* x, int ld, int B, int C, const int* labels, float smooth, float* L, float* d, int ldd,
        int* correct, void* ws, hipStream_t s) {
  float* lossp = static_cast<float*>(ws);              // [B]
  int* hitp = reinterpret_cast<int*>(lossp + r4(B));   // [B]
  xent_rows<V><<<dim3(B), dim3(THREADS), 0, s>>>(x, ld, C, labels, smooth, 1.f / (float)B, lossp, hitp, d, ldd);
  if (avc_check_launch("avc_xent (rows)")) return -1;
  xent_finish<<<dim3(1), dim3(THREADS), 0, s>>>(lossp, hitp, B, L, correct);
  return avc_check_launch("avc_xent (finish)");
}
}  // namespace

extern "C" size_t avc_xent_ws(int B, int C) { return shape_ok(B, C) ? 2 * r4(B) * sizeof(float) : 0; }

extern "C" int avc_xent(const float* logits, int ld, int B, int C, const int* labels, float smooth, float* L,
                        float* dlogits, int ldd, int* correct, void* ws, void* stream) {
  AVC_CHECK_ARG(logits && labels && L && ws, "avc_xent: null pointer (logits, labels, L and ws are required)");
  AVC_CHECK_ARG(((uintptr_t)ws & 15) == 0, "avc_xent: ws must be 16-byte aligned");
  AVC_CHECK_ARG(B >= 1 && C >= 1, "avc_xent: bad shape B = %d, C = %d (B >= 1, C >= 1)", B, C);
  AVC_CHECK_ARG(shape_ok(B, C), "avc_xent: B = %d, C = %d is past the limits (B <= %d, C <= %d)", B, C,
                AVC_XENT_MAX_B, AVC_XENT_MAX_C);
  AVC_CHECK_ARG(ld >= C, "avc_xent: ld = %d is below C = %d", ld, C);
  AVC_CHECK_ARG(!dlogits || ldd >= C, "avc_xent: ldd = %d is below C = %d", ldd, C);
  AVC_CHECK_ARG(smooth >= 0.f && smooth < 1.f, "avc_xent: smooth = %g outside [0, 1)", (double)smooth);
  if (dlogits) {
    const float* xe = logits + (size_t)(B - 1) * ld + C;
    const float* de = dlogits + (size_t)(B - 1) * ldd + C;
    AVC_CHECK_ARG(de <= logits || xe <= dlogits, "avc_xent: dlogits must not alias logits");
  }
  const bool vec = C % 4 == 0 && ld % 4 == 0 && (!dlogits || ldd % 4 == 0) &&
                   (((uintptr_t)logits | (uintptr_t)dlogits) & 15) == 0;
  hipStream_t s = as_stream(stream);
  return vec ? run<f32x4>(logits, ld, B, C, labels, smooth, L, dlogits, ldd, correct, ws, s)
             : run<float>(logits, ld, B, C, labels, smooth, L, dlogits, ldd, correct, ws, s);
}
