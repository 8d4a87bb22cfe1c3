// Per-utterance BatchNorm (include/autovc_hip_eval.h): statistics over each T-row segment of a
// frame-major batch, then the affine + activation (+ residual) apply, in one launch.
//
// One 256-thread workgroup owns one (segment, 64-channel tile): lane tx = thread & 63 is the channel
// (a wave reads 64 consecutive floats of a row, 256 B), the four waves take rows ty, ty + 4, ...
// Three passes over the segment's tile: sum (of y - first row) -> mean, centred squares -> variance,
// apply.  A thread touches the same (row, channel) elements in all three, so the tile kept in LDS needs
// no barrier of its own; the barriers are those of the two 4-way reductions.  A segment of more than
// AVC_BN_SEG_LDS_ROWS rows does not fit and is re-read from global memory (L2-resident: 64 channels
// x T rows).  Every sum has a fixed order (rows ascending per wave, then waves 0..3).
#include <math.h>

#include "../../include/autovc_hip_eval.h"
#include "common.h"

namespace {
constexpr int TILE_C = 64;
constexpr int ROW_GROUPS = 4;

// sum of the four row groups' values of channel tx; all 256 threads call it
__device__ __forceinline__ float group_sum(float* red, int ty, int tx, float v) {
  __syncthreads();  // the previous reduction's reads are done
  red[ty * TILE_C + tx] = v;
  __syncthreads();
  return (red[tx] + red[TILE_C + tx]) + (red[2 * TILE_C + tx] + red[3 * TILE_C + tx]);
}

template <bool RESIDENT>
__global__ void __launch_bounds__(TILE_C* ROW_GROUPS)
    bn_seg_kernel(const float* y, long long ld, int T, int C, int ctiles, const float* __restrict__ gamma,
                  const float* __restrict__ beta, float eps, int act, const float* res, float* out, bf16* out16,
                  float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  extern __shared__ float smem[];
  float* red = smem;                          // [ROW_GROUPS][TILE_C]
  float* tile = smem + ROW_GROUPS * TILE_C;   // [T][TILE_C] when RESIDENT
  const int tx = threadIdx.x & (TILE_C - 1), ty = threadIdx.x >> 6;
  const int b = blockIdx.x / ctiles, ct = blockIdx.x - b * ctiles;
  const int c = ct * TILE_C + tx;
  const bool cv = c < C;
  const long long base = (long long)b * T * ld + c;  // element (row 0 of the segment, channel c)

  // the sum is taken of y - pivot (the segment's first value of the channel): a channel with a large
  // mean and a small spread then adds small numbers, and the mean keeps the precision of one value
  const float pivot = cv ? y[base] : 0.f;
  float s = 0.f;
  if (cv)
    for (int r = ty; r < T; r += ROW_GROUPS) {
      const float v = y[base + (long long)r * ld];
      if (RESIDENT) tile[r * TILE_C + tx] = v;
      s += v - pivot;
    }
  const float mean = pivot + group_sum(red, ty, tx, s) / (float)T;

  float q = 0.f;
  if (cv)
    for (int r = ty; r < T; r += ROW_GROUPS) {
      const float d = (RESIDENT ? tile[r * TILE_C + tx] : y[base + (long long)r * ld]) - mean;
      q = fmaf(d, d, q);
    }
  const float var = group_sum(red, ty, tx, q) / (float)T;
  const float rstd = 1.f / sqrtf(var + eps);
  if (!cv) return;  // (after the last barrier)
  if (ty == 0) {
    if (mean_out) mean_out[(long long)b * C + c] = mean;
    if (rstd_out) rstd_out[(long long)b * C + c] = rstd;
  }
  const float g = gamma[c] * rstd, be = beta[c];
  for (int r = ty; r < T; r += ROW_GROUPS) {
    const long long e = base + (long long)r * ld;
    const float v = RESIDENT ? tile[r * TILE_C + tx] : y[e];
    float o = act_fwd(fmaf(v - mean, g, be), act);
    if (res) o += res[e];
    if (out) out[e] = o;
    if (out16) out16[e] = (bf16)o;
  }
}
}  // namespace

extern "C" int avc_bn_seg_apply(const void* y, int y_dtype, long long ld, int B, int T, int C, const float* gamma,
                                const float* beta, float eps, int act, const float* residual, float* out,
                                void* out_bf16, float* mean, float* rstd, void* stream) {
  AVC_CHECK_ARG(y && gamma && beta, "avc_bn_seg_apply: null pointer (y, gamma and beta are required)");
  AVC_CHECK_ARG(out || out_bf16, "avc_bn_seg_apply: null pointer (neither out nor out_bf16 given)");
  AVC_CHECK_ARG(y_dtype == AVC_F32,
                "avc_bn_seg_apply: y_dtype = %d: the statistics are taken from fp32 values only", y_dtype);
  AVC_CHECK_ARG(act >= AVC_ACT_NONE && act <= AVC_ACT_SIGMOID, "avc_bn_seg_apply: unknown act %d", act);
  AVC_CHECK_ARG(B >= 1 && C >= 1, "avc_bn_seg_apply: bad shape B = %d, C = %d", B, C);
  AVC_CHECK_ARG(T >= 2, "avc_bn_seg_apply: T = %d: a segment needs more than one value per channel", T);
  AVC_CHECK_ARG(ld >= C, "avc_bn_seg_apply: ld = %lld is below C = %d", ld, C);
  AVC_CHECK_ARG(eps >= 0.f && isfinite(eps), "avc_bn_seg_apply: eps = %g", (double)eps);
  const int ctiles = cdiv(C, TILE_C);
  AVC_CHECK_ARG((long long)B * ctiles <= 2147483647ll, "avc_bn_seg_apply: %lld workgroups", (long long)B * ctiles);
  hipStream_t s = as_stream(stream);
  const float* yp = static_cast<const float*>(y);
  bf16* o16 = reinterpret_cast<bf16*>(out_bf16);
  const dim3 grid((unsigned)(B * ctiles)), block(TILE_C * ROW_GROUPS);
  const size_t red_bytes = sizeof(float) * ROW_GROUPS * TILE_C;
  if (T <= AVC_BN_SEG_LDS_ROWS)
    bn_seg_kernel<true><<<grid, block, red_bytes + sizeof(float) * (size_t)T * TILE_C, s>>>(
        yp, ld, T, C, ctiles, gamma, beta, eps, act, residual, out, o16, mean, rstd);
  else
    bn_seg_kernel<false><<<grid, block, red_bytes, s>>>(yp, ld, T, C, ctiles, gamma, beta, eps, act, residual, out,
                                                        o16, mean, rstd);
  return avc_check_launch("avc_bn_seg_apply");
}
