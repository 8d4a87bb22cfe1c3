// The GE2E loss and its gradients (include/autovc_hip_ge2e.h), fp32, deterministic.
//
// With s_k = sum_i e[k,i] (so c_k = s_k / M and c_ex[j,i] = (s_j - e[j,i]) / (M - 1)), a = e[j,i] one row r,
// n(.) = max(||.||, eps), and g_k = dL/dS[r,k] = w (p_k - [k == j]) / (N M) from the row's softmax p:
//
//   de[r]  =  sum_{k != j} g_k / (n(a) n(c_k)) c_k  +  g_j / (n(a) n(u)) u  -  (sum_k g_k S_k) / n(a)^2 a     (direct)
//          +  (sum_{i'} G[j,i'] - G[r]) / (M - 1),   G[r] = g_j (a / (n(a) n(u)) - S_j u / n(u)^2)             (via c_ex)
//          +  H_j / M,   H_k = sum_{r': j' != k} g_{r'k} / (n(a') n(c_k)) a'  -  (sum_{r'} g_{r'k} S_{r'k}) / n(c_k)^2 c_k   (via c)
//   dw     =  sum_r sum_k (p_k - [k == j]) / (N M) S[r,k]
//
// where u = c_ex[r].  c_ex and its norm are formed from s_j - a element by element (never from ||s_j||^2 -
// 2 a.s_j + ||a||^2, which cancels when one row dominates its speaker's sum).
//
// Three launches: ge2e_sums (one workgroup per speaker: s_k, ||s_k||), ge2e_rows (one per row: S[r,:], softmax,
// loss and dw partials, the coefficients alpha[r,k] = g_k / (n(a) n(c_k)) and q[r,k] = g_k S_k for k != j, the
// direct part of de[r], G[r]), ge2e_speakers (one per speaker: H_k, the assembly of its M rows of de; workgroup
// 0 also the final sums L and dw).  The two N x (N M) x D products (S and the direct part; H) are sums over
// rows weighted by an LDS-resident coefficient vector (weighted_rows).  Every sum has a fixed order: ascending
// per thread, a shuffle butterfly per wave, waves / row groups in index order.  No atomics, no workgroup
// waits on another.
#include <math.h>

#include "../../include/autovc_hip_ge2e.h"
#include "common.h"

namespace {
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr float EPS = 1e-8f;
constexpr int RED_BYTES = THREADS * (int)sizeof(f32x4);  // weighted_rows' partials, first in LDS: 16-byte aligned

static inline size_t r4(size_t v) { return (v + 3) & ~(size_t)3; }

// the workspace, in floats; every region starts on a multiple of 4 floats (float4 accesses to sums and G)
struct Layout {
  size_t sums, snorm, alpha, q, G, lossp, dwp, total;
};
Layout layout(int N, int M, int D) {
  const size_t R = (size_t)N * M;
  Layout l;
  l.sums = 0;                              // [N][D]  s_k
  l.snorm = l.sums + r4((size_t)N * D);    // [N]     ||s_k||
  l.alpha = l.snorm + r4(N);               // [R][N]  g_k / (n(a) n(c_k)), 0 at k == j
  l.q = l.alpha + r4(R * N);               // [R][N]  g_k S_k, 0 at k == j
  l.G = l.q + r4(R * N);                   // [R][D]  dL/dc_ex[r]
  l.lossp = l.G + r4(R * D);               // [R]
  l.dwp = l.lossp + r4(R);                 // [R]
  l.total = l.dwp + r4(R);
  return l;
}

__device__ __forceinline__ float dot(float a, float b) { return a * b; }
__device__ __forceinline__ float dot(const f32x4& a, const f32x4& b) {
  return fmaf(a[3], b[3], fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])));
}
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

__device__ __forceinline__ float warp_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// sum over the workgroup, returned to every thread.  The leading barrier lets `slot` be reused by the
// next call (and orders the caller's LDS writes before whatever follows).
__device__ __forceinline__ float block_sum(float* slot, float v) {
  v = warp_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  return (slot[0] + slot[1]) + (slot[2] + slot[3]);
}

// dst[u] = sum_{r < R} coef[r] * X[r][u], u < U units of V (X global, row-major [R][U]; coef, red, dst in
// LDS; red holds THREADS units).  With U < THREADS the rows are dealt to G = THREADS / U groups of U threads
// (row r to group r % G) and the G partials are added in group order; otherwise a thread owns units
// t, t + THREADS, ...  Every thread of the workgroup calls it; dst is complete (barrier) on return.
template <typename V>
__device__ __forceinline__ void weighted_rows(const V* __restrict__ X, int R, int U, const float* coef, V* red,
                                              V* dst) {
  const int t = threadIdx.x;
  if (U < THREADS) {
    const int G = THREADS / U, g = t / U, u = t - g * U;
    V acc{};
    if (g < G)
      for (int r = g; r < R; r += G) acc += coef[r] * X[(size_t)r * U + u];
    red[t] = acc;
    __syncthreads();
    if (t < U) {
      V tot = red[t];
      for (int gg = 1; gg < G; ++gg) tot += red[gg * U + t];
      dst[t] = tot;
    }
  } else {
    for (int u = t; u < U; u += THREADS) {
      V acc{};
      for (int r = 0; r < R; ++r) acc += coef[r] * X[(size_t)r * U + u];
      dst[u] = acc;
    }
  }
  __syncthreads();
}

template <typename V>
__global__ void __launch_bounds__(THREADS)
    ge2e_sums(const float* __restrict__ e, int M, int D, float* __restrict__ sums, float* __restrict__ snorm) {
  __shared__ float slots[WAVES];
  const int U = D / Width<V>::W, k = blockIdx.x;
  const V* ek = reinterpret_cast<const V*>(e + (size_t)k * M * D);
  V* sk = reinterpret_cast<V*>(sums + (size_t)k * D);
  float sq = 0.f;
  for (int u = threadIdx.x; u < U; u += THREADS) {
    V acc{};
    for (int i = 0; i < M; ++i) acc += ek[(size_t)i * U + u];
    sk[u] = acc;
    sq += dot(acc, acc);
  }
  sq = block_sum(slots, sq);
  if (threadIdx.x == 0) snorm[k] = sqrtf(sq);
}

// de == nullptr: the loss and dw partials only
template <typename V>
__global__ void __launch_bounds__(THREADS)
    ge2e_rows(const float* __restrict__ e, int N, int M, int D, const float* __restrict__ w,
              const float* __restrict__ sums, const float* __restrict__ snorm, float* __restrict__ alpha,
              float* __restrict__ q, float* __restrict__ G, float* __restrict__ lossp, float* __restrict__ dwp,
              float* __restrict__ de) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ge2e_smem[];
  const int D4 = (D + 3) & ~3, N4 = (N + 3) & ~3;
  V* red = reinterpret_cast<V*>(ge2e_smem);                     // [THREADS]
  float* As = reinterpret_cast<float*>(ge2e_smem + RED_BYTES);  // [D4]  the row
  float* Ds = As + D4;                                          // [D4]  sum_k Al[k] s_k
  float* Ss = Ds + D4;                                          // [N4]  S[r, :]
  float* Al = Ss + N4;                                          // [N4]  alpha[r, :] / M
  float* slots = Al + N4;                                       // [8]
  float* sc = slots + 8;                                        // [8]   row scalars
  constexpr int W = Width<V>::W;
  const int U = D / W, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = blockIdx.x, j = r / M;
  const bool grads = de != nullptr;
  const float invM = 1.f / (float)M, invM1 = 1.f / (float)(M - 1);
  const V* er = reinterpret_cast<const V*>(e + (size_t)r * D);
  V* Av = reinterpret_cast<V*>(As);

  float sq = 0.f;
  for (int u = t; u < U; u += THREADS) {
    const V v = er[u];
    Av[u] = v;
    sq += dot(v, v);
  }
  const float na_raw = sqrtf(block_sum(slots, sq));
  const float na = fmaxf(na_raw, EPS);

  // S[r, k]: wave `wave` takes k = wave, wave + WAVES, ... (k is wave-uniform)
  for (int k = wave; k < N; k += WAVES) {
    const V* sk = reinterpret_cast<const V*>(sums + (size_t)k * D);
    if (k != j) {
      float acc = 0.f;
      for (int u = lane; u < U; u += 64) acc += dot(Av[u], sk[u]);
      acc = warp_sum(acc);
      if (lane == 0) Ss[k] = (acc * invM) / (na * fmaxf(snorm[k] * invM, EPS));
    } else {
      float d = 0.f, n2 = 0.f;
      for (int u = lane; u < U; u += 64) {
        const V a = Av[u], uu = (sk[u] - a) * invM1;
        d += dot(a, uu);
        n2 += dot(uu, uu);
      }
      d = warp_sum(d);
      n2 = warp_sum(n2);
      if (lane == 0) {
        const float nex_raw = sqrtf(n2), nex = fmaxf(nex_raw, EPS);
        Ss[k] = d / (na * nex);
        sc[0] = nex;
        sc[1] = nex_raw >= EPS ? 1.f : 0.f;
      }
    }
  }
  __syncthreads();

  if (wave == 0) {
    const float wv = w[0], invR = 1.f / ((float)N * (float)M);
    float m = -INFINITY;
    for (int k = lane; k < N; k += 64) m = fmaxf(m, wv * Ss[k]);
    m = warp_max(m);
    const float zj = wv * Ss[j], pj_un = expf(zj - m);
    float so = 0.f;  // the other columns' share: 1 - p_j without cancellation
    for (int k = lane; k < N; k += 64)
      if (k != j) so += expf(wv * Ss[k] - m);
    so = warp_sum(so);
    const float invs = 1.f / (so + pj_un);
    // sum_k dz_k S_k as sum_{k != j} dz_k (S_k - S_j): the dz sum to zero, and the differences do not cancel
    // against each other when every S is close to 1 (embeddings that have not separated yet)
    const float Sj = Ss[j];
    float dwr = 0.f;
    for (int k = lane; k < N; k += 64) {
      const float S = Ss[k];
      const float dz = (k == j ? -so * invs : expf(wv * S - m) * invs) * invR;
      dwr += dz * (S - Sj);
      if (grads) {
        const float g = wv * dz;
        const float al = k == j ? 0.f : g / (na * fmaxf(snorm[k] * invM, EPS));
        alpha[(size_t)r * N + k] = al;
        q[(size_t)r * N + k] = k == j ? 0.f : g * S;
        Al[k] = al * invM;
      }
    }
    dwr = warp_sum(dwr);
    if (lane == 0) {
      lossp[r] = m + logf(so + pj_un) - zj;
      dwp[r] = dwr;
      if (grads) {
        const float nex = sc[0], gj = wv * (-so * invs) * invR;
        sc[2] = gj / (na * nex);                                  // on u in de, on a in G
        sc[3] = na_raw >= EPS ? (wv * dwr) / (na * na) : 0.f;     // sum_k g_k S_k / n(a)^2
        sc[4] = sc[1] * gj * Ss[j] / (nex * nex);                 // on u in G
      }
    }
  }
  if (!grads) return;
  __syncthreads();

  weighted_rows<V>(reinterpret_cast<const V*>(sums), N, U, Al, red, reinterpret_cast<V*>(Ds));
  const float cU = sc[2], cA = sc[3], cG = sc[4];
  const V* sj = reinterpret_cast<const V*>(sums + (size_t)j * D);
  const V* Dv = reinterpret_cast<const V*>(Ds);
  V* der = reinterpret_cast<V*>(de + (size_t)r * D);
  V* Gr = reinterpret_cast<V*>(G + (size_t)r * D);
  for (int u = t; u < U; u += THREADS) {
    const V a = Av[u], uu = (sj[u] - a) * invM1;
    der[u] = Dv[u] + cU * uu - cA * a;
    Gr[u] = cU * a - cG * uu;
  }
}

// grads == 0: one workgroup, the final sums only
template <typename V>
__global__ void __launch_bounds__(THREADS)
    ge2e_speakers(const float* __restrict__ e, int N, int M, int D, const float* __restrict__ sums,
                  const float* __restrict__ snorm, const float* __restrict__ alpha, const float* __restrict__ q,
                  const float* __restrict__ G, const float* __restrict__ lossp, const float* __restrict__ dwp,
                  float* __restrict__ de, float* __restrict__ L, float* __restrict__ dw, int grads) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ge2e_smem[];
  const int D4 = (D + 3) & ~3, R = N * M, R4 = (R + 3) & ~3;
  V* red = reinterpret_cast<V*>(ge2e_smem);                     // [THREADS]
  float* Hs = reinterpret_cast<float*>(ge2e_smem + RED_BYTES);  // [D4]  sum_r alpha[r, k] e[r]
  float* Ac = Hs + D4;                                          // [R4]  alpha[:, k]   (grads only)
  float* slots = Ac + (grads ? R4 : 0);                         // [8]
  constexpr int W = Width<V>::W;
  const int U = D / W, t = threadIdx.x, k = blockIdx.x;

  if (k == 0) {
    float l = 0.f, d = 0.f;
    for (int r = t; r < R; r += THREADS) {
      l += lossp[r];
      d += dwp[r];
    }
    l = block_sum(slots, l);
    d = block_sum(slots, d);
    if (t == 0) {
      L[0] = l / (float)R;
      if (dw) dw[0] = d;
    }
  }
  if (!grads) return;

  float qs = 0.f;
  for (int r = t; r < R; r += THREADS) {
    Ac[r] = alpha[(size_t)r * N + k];
    qs += q[(size_t)r * N + k];
  }
  qs = block_sum(slots, qs);
  const float invM = 1.f / (float)M, invM1 = 1.f / (float)(M - 1);
  const float nk_raw = snorm[k] * invM, nk = fmaxf(nk_raw, EPS);
  const float cc = nk_raw >= EPS ? (qs / (nk * nk)) * invM : 0.f;  // on s_k: beta_k c_k = beta_k / M s_k

  weighted_rows<V>(reinterpret_cast<const V*>(e), R, U, Ac, red, reinterpret_cast<V*>(Hs));
  const V* Hv = reinterpret_cast<const V*>(Hs);
  const V* sk = reinterpret_cast<const V*>(sums + (size_t)k * D);
  const V* Gk = reinterpret_cast<const V*>(G + (size_t)k * M * D);
  V* dek = reinterpret_cast<V*>(de + (size_t)k * M * D);
  for (int u = t; u < U; u += THREADS) {
    const V h = (Hv[u] - cc * sk[u]) * invM;
    V gsum{};
    for (int i = 0; i < M; ++i) gsum += Gk[(size_t)i * U + u];
    for (int i = 0; i < M; ++i) {
      const size_t idx = (size_t)i * U + u;
      dek[idx] = dek[idx] + h + (gsum - Gk[idx]) * invM1;
    }
  }
}

bool shape_ok(int N, int M, int D) {
  return N >= 2 && M >= 2 && D >= 1 && N <= AVC_GE2E_MAX_N && M <= AVC_GE2E_MAX_M && D <= AVC_GE2E_MAX_D &&
         (long long)N * M <= AVC_GE2E_MAX_ROWS;
}

template <typename V>
int run(const float* e, int N, int M, int D, const float* w, float* L, float* de, float* dw, float* ws,
        hipStream_t s) {
  const Layout l = layout(N, M, D);
  const int R = N * M, grads = de != nullptr;
  const size_t lds_rows = RED_BYTES + sizeof(float) * (2 * r4(D) + 2 * r4(N) + 16);
  const size_t lds_spk = RED_BYTES + sizeof(float) * (r4(D) + (grads ? r4(R) : 0) + 8);
  ge2e_sums<V><<<dim3(N), dim3(THREADS), 0, s>>>(e, M, D, ws + l.sums, ws + l.snorm);
  if (avc_check_launch("avc_ge2e (sums)")) return -1;
  ge2e_rows<V><<<dim3(R), dim3(THREADS), lds_rows, s>>>(e, N, M, D, w, ws + l.sums, ws + l.snorm, ws + l.alpha,
                                                        ws + l.q, ws + l.G, ws + l.lossp, ws + l.dwp, de);
  if (avc_check_launch("avc_ge2e (rows)")) return -1;
  ge2e_speakers<V><<<dim3(grads ? N : 1), dim3(THREADS), lds_spk, s>>>(e, N, M, D, ws + l.sums, ws + l.snorm,
                                                                      ws + l.alpha, ws + l.q, ws + l.G,
                                                                      ws + l.lossp, ws + l.dwp, de, L, dw, grads);
  return avc_check_launch("avc_ge2e (speakers)");
}
}  // namespace

extern "C" size_t avc_ge2e_ws(int N, int M, int D) {
  return shape_ok(N, M, D) ? layout(N, M, D).total * sizeof(float) : 0;
}

extern "C" int avc_ge2e(const float* e, int N, int M, int D, const float* w, float* L, float* de, float* dw,
                        void* ws, void* stream) {
  AVC_CHECK_ARG(e && w && L && ws, "avc_ge2e: null pointer (e, w, L and ws are required)");
  AVC_CHECK_ARG((de != nullptr) == (dw != nullptr), "avc_ge2e: de and dw go together (both or neither)");
  AVC_CHECK_ARG(((uintptr_t)ws & 15) == 0, "avc_ge2e: ws must be 16-byte aligned");
  AVC_CHECK_ARG(N >= 2 && M >= 2 && D >= 1, "avc_ge2e: bad shape N = %d, M = %d, D = %d (N >= 2, M >= 2, D >= 1)", N,
                M, D);
  AVC_CHECK_ARG(shape_ok(N, M, D), "avc_ge2e: N = %d, M = %d, D = %d is past the LDS layout (N <= %d, M <= %d, "
                "D <= %d, N * M <= %d)", N, M, D, AVC_GE2E_MAX_N, AVC_GE2E_MAX_M, AVC_GE2E_MAX_D, AVC_GE2E_MAX_ROWS);
  AVC_CHECK_ARG(de != e, "avc_ge2e: de must not alias e");
  const bool vec = D % 4 == 0 && (((uintptr_t)e | (uintptr_t)de) & 15) == 0;
  hipStream_t s = as_stream(stream);
  float* wsf = static_cast<float*>(ws);
  return vec ? run<f32x4>(e, N, M, D, w, L, de, dw, wsf, s) : run<float>(e, N, M, D, w, L, de, dw, wsf, s);
}
