// Per-segment moments and AdaIN (include/autovc_hip_seg.h): [mean, unbiased std] of each of B contiguous
// n-float segments, and (x - mean) / std * sigma[b] + mu[b] with the segment's own moments, in one launch.
//
// One 256-thread workgroup owns one segment.  Thread t takes units t, t + 256, ... of it (a unit is a
// float4 when n % 4 == 0 and the pointers are 16-byte aligned, a float otherwise: a wave reads 1 KiB
// resp. 256 B of consecutive memory per instruction).  Up to three passes over the segment: sum -> mean,
// squares about the mean -> std, apply.  A thread touches the same units in all three, so the copy kept
// in LDS needs no barrier of its own; the barriers are those of the two block reductions.  A segment of
// more than AVC_SEG_MOMENTS_LDS_FLOATS floats does not fit and is re-read from global memory.
// The sums are fp64 (55 elements per thread at the conversion shape: the fp64 adds are free beside the
// loads) and have a fixed order: units ascending per thread, a shuffle tree per wave, then waves 0..3.
#include <math.h>

#include "../../include/autovc_hip_seg.h"
#include "common.h"

namespace {
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int RED_BYTES = 2 * WAVES * (int)sizeof(double);  // one slot row per reduction: 64 bytes
static_assert(RED_BYTES % 16 == 0, "the LDS copy behind the reduction slots stays 16-byte aligned");
static_assert(RED_BYTES + AVC_SEG_MOMENTS_LDS_FLOATS * sizeof(float) <= 64 * 1024, "LDS without opting in");
static_assert(AVC_SEG_MOMENTS_LDS_FLOATS % 4 == 0, "a float4 path segment fills whole float4 units");

// sum over the workgroup, returned to every thread; `slot` is this reduction's own row of WAVES doubles
__device__ __forceinline__ double block_sum(double* slot, double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  return (slot[0] + slot[1]) + (slot[2] + slot[3]);
}

template <typename V>
struct Unit;
template <>
struct Unit<float> {
  static constexpr int W = 1;
  static __device__ __forceinline__ float get(const float& v, int) { return v; }
  static __device__ __forceinline__ void set(float& v, int, float e) { v = e; }
};
template <>
struct Unit<f32x4> {
  static constexpr int W = 4;
  static __device__ __forceinline__ float get(const f32x4& v, int k) { return v[k]; }
  static __device__ __forceinline__ void set(f32x4& v, int k, float e) { v[k] = e; }
};

// y == nullptr: moments only.  x and y are not __restrict__: y may alias x (a thread reads a unit
// before it writes it, and no other thread touches that unit).
template <bool RESIDENT, typename V>
__global__ void __launch_bounds__(THREADS)
    seg_moments_kernel(const float* x, long long n, const float* __restrict__ mu, const float* __restrict__ sigma,
                       float* __restrict__ out, float* y) {
  extern __shared__ __attribute__((aligned(16))) unsigned char seg_smem[];
  double* red = reinterpret_cast<double*>(seg_smem);      // [2][WAVES]
  V* tile = reinterpret_cast<V*>(seg_smem + RED_BYTES);   // [n / W] when RESIDENT
  constexpr int W = Unit<V>::W;
  const long long b = blockIdx.x;
  const V* xb = reinterpret_cast<const V*>(x + b * n);
  const long long units = n / W;  // (the float4 path is taken only when n % 4 == 0)

  double s = 0.0;
  for (long long i = threadIdx.x; i < units; i += THREADS) {
    const V v = xb[i];
    if (RESIDENT) tile[i] = v;
#pragma unroll
    for (int k = 0; k < W; ++k) s += (double)Unit<V>::get(v, k);
  }
  const double mean = block_sum(red, s) / (double)n;

  double q = 0.0;
  for (long long i = threadIdx.x; i < units; i += THREADS) {
    const V v = RESIDENT ? tile[i] : xb[i];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const double d = (double)Unit<V>::get(v, k) - mean;
      q = fma(d, d, q);
    }
  }
  // n = 1: 0 / 0 = NaN, torch.std's answer
  const float sd = (float)sqrt(block_sum(red + WAVES, q) / (double)(n - 1));
  if (out && threadIdx.x == 0) {
    out[2 * b] = (float)mean;
    out[2 * b + 1] = sd;
  }
  if (!y) return;
  const float a = sigma[b] / sd, c = mu[b];
  V* yb = reinterpret_cast<V*>(y + b * n);
  for (long long i = threadIdx.x; i < units; i += THREADS) {
    const V v = RESIDENT ? tile[i] : xb[i];
    V r;
#pragma unroll
    for (int k = 0; k < W; ++k) Unit<V>::set(r, k, fmaf((float)((double)Unit<V>::get(v, k) - mean), a, c));
    yb[i] = r;
  }
}

int launch(const char* what, const float* x, int B, long long n, const float* mu, const float* sigma, float* out,
           float* y, void* stream) {
  AVC_CHECK_ARG(B >= 1 && n >= 1, "%s: bad shape B = %d, n = %lld", what, B, n);
  hipStream_t s = as_stream(stream);
  const bool vec = n % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
  const bool resident = n <= AVC_SEG_MOMENTS_LDS_FLOATS;
  const dim3 grid((unsigned)B), block(THREADS);
  const size_t lds = RED_BYTES + (resident ? sizeof(float) * (size_t)n : 0);
  if (resident && vec)
    seg_moments_kernel<true, f32x4><<<grid, block, lds, s>>>(x, n, mu, sigma, out, y);
  else if (resident)
    seg_moments_kernel<true, float><<<grid, block, lds, s>>>(x, n, mu, sigma, out, y);
  else if (vec)
    seg_moments_kernel<false, f32x4><<<grid, block, lds, s>>>(x, n, mu, sigma, out, y);
  else
    seg_moments_kernel<false, float><<<grid, block, lds, s>>>(x, n, mu, sigma, out, y);
  return avc_check_launch(what);
}
}  // namespace

extern "C" int avc_seg_moments(const float* x, int B, long long n, float* out, void* stream) {
  AVC_CHECK_ARG(x && out, "avc_seg_moments: null pointer (x and out are required)");
  return launch("avc_seg_moments", x, B, n, nullptr, nullptr, out, nullptr, stream);
}

extern "C" int avc_adain_seg(const float* x, int B, long long n, const float* mu, const float* sigma, float* y,
                             void* stream) {
  AVC_CHECK_ARG(x && mu && sigma && y, "avc_adain_seg: null pointer (x, mu, sigma and y are required)");
  return launch("avc_adain_seg", x, B, n, mu, sigma, nullptr, y, stream);
}
