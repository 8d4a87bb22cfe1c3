// What critic_loss.hip and cycle_loss.hip share: the cosine rows, the BCE sums and their gradients, each in ONE
// fixed order, so that both files give the same bits on the same inputs (c_loss / c_trans, d_loss, de, dp).
//
//   dot = sum e t, m1 = sum e^2 + 1e-12, m2 = sum t^2 + 1e-12, cos = dot / sqrt(m1 m2)      (ATen's formula)
//   de_b = -(g_c / B) (t_b / sqrt(m1 m2) - (dot / sqrt(m1 m2)) e_b / m1)
//   dp   = g_d (p - y) / max(p (1 - p), 1e-12) / n
//
// A 256-thread workgroup: wave w takes rows w, w + 4, ...; lane l of it takes the column groups 4u .. 4u + 3,
// u = l, l + 64, ..., and adds their products in ascending column order with fmaf -- as one float4 load per
// operand where the layout allows it, as single loads otherwise: the same additions in the same order, hence the
// same bits in both forms.  A 64-wide shuffle butterfly ends the row.  Thread i takes the probabilities i,
// i + 256, ...; a butterfly per wave.  The four wave partials are added in wave order (sum4).
#pragma once
#include <math.h>

#include "common.h"

namespace critic {
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr float COS_EPS = 1e-12f;    // ATen's EPSILON of cosine_embedding_loss, and of BCE's backward
constexpr float LOG_FLOOR = -100.f;  // nn.BCELoss clamps its logarithms here

// columns 4u .. 4u + 3 of a row of E floats; the scalar form leaves what lies past E at zero (never added)
template <bool VEC>
__device__ __forceinline__ f32x4 load_group(const float* __restrict__ row, int u, int E) {
  if (VEC) return *reinterpret_cast<const f32x4*>(row + 4 * u);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (4 * u + k < E) v[k] = row[4 * u + k];
  return v;
}

// the calling wave's sum of 1 - cos over its rows, in row order; (dot, m1, m2) of each row to ws3[3 b ..]
template <bool VEC>
__device__ __forceinline__ float cos_rows(const float* __restrict__ e, int lde, const float* __restrict__ t, int ldt,
                                          int B, int E, float* __restrict__ ws3, int lane, int wave) {
  const int U = (E + 3) >> 2;
  float cpart = 0.f;
  for (int b = wave; b < B; b += WAVES) {
    const float* er = e + (size_t)b * lde;
    const float* tr = t + (size_t)b * ldt;
    float dot = 0.f, se = 0.f, st = 0.f;
    for (int u = lane; u < U; u += 64) {
      const f32x4 ev = load_group<VEC>(er, u, E), tv = load_group<VEC>(tr, u, E);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (VEC || 4 * u + k < E) {
          dot = fmaf(ev[k], tv[k], dot);
          se = fmaf(ev[k], ev[k], se);
          st = fmaf(tv[k], tv[k], st);
        }
      }
    }
    dot = warp_sum(dot);
    const float m1 = warp_sum(se) + COS_EPS, m2 = warp_sum(st) + COS_EPS;
    if (lane == 0) {
      ws3[3 * b + 0] = dot;
      ws3[3 * b + 1] = m1;
      ws3[3 * b + 2] = m2;
    }
    cpart += 1.f - dot / sqrtf(m1 * m2);
  }
  return cpart;
}

// the calling wave's sums of -max(log p, -100) and of -max(log(1 - p), -100)
__device__ __forceinline__ float real_sum(const float* __restrict__ p_real, int n_r, int tid) {
  float rpart = 0.f;
  for (int i = tid; i < n_r; i += THREADS) rpart -= fmaxf(logf(p_real[i]), LOG_FLOOR);
  return warp_sum(rpart);
}
__device__ __forceinline__ float fake_sum(const float* __restrict__ p_fake, int n_f, int tid) {
  float fpart = 0.f;
  for (int i = tid; i < n_f; i += THREADS) fpart -= fmaxf(log1pf(-p_fake[i]), LOG_FLOOR);
  return warp_sum(fpart);
}

// the four wave partials, in wave order
__device__ __forceinline__ float sum4(const float* r) { return ((r[0] + r[1]) + r[2]) + r[3]; }

// row b of de for the upstream gradient g_c of the mean, by the whole workgroup
template <bool VEC>
__device__ __forceinline__ void de_row(const float* __restrict__ e, int lde, const float* __restrict__ t, int ldt, int B,
                                       int E, const float* __restrict__ ws3, float g_c, float* __restrict__ de,
                                       int ldde, int b, int tid) {
  const float dot = ws3[3 * b + 0], m1 = ws3[3 * b + 1], m2 = ws3[3 * b + 2];
  const float denom = sqrtf(m1 * m2), s = -(g_c / (float)B);
  const float ct = s / denom, ce = s * (dot / denom) / m1;
  const float* er = e + (size_t)b * lde;
  const float* tr = t + (size_t)b * ldt;
  float* dr = de + (size_t)b * ldde;
  const int U = (E + 3) >> 2;
  for (int u = tid; u < U; u += THREADS) {
    const f32x4 ev = load_group<VEC>(er, u, E), tv = load_group<VEC>(tr, u, E);
    f32x4 g;
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = fmaf(ct, tv[k], -(ce * ev[k]));
    if (VEC) {
      *reinterpret_cast<f32x4*>(dr + 4 * u) = g;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * u + k < E) dr[4 * u + k] = g[k];
    }
  }
}

// element i of dp for the label y (1 real, 0 fake)
__device__ __forceinline__ void dp_elem(const float* __restrict__ p, float* __restrict__ dp, int n, int i, float y,
                                        float g_d) {
  if (i < n) {
    const float v = p[i];
    dp[i] = g_d * (v - y) / fmaxf(v * (1.f - v), COS_EPS) / (float)n;
  }
}
}  // namespace critic
