// ragged.hip — a batch of whole utterances of different lengths (include/autovc_hip_ragged.h): the
// per-utterance BatchNorm of bn_seg.hip with a length per segment, the row mask that keeps padding
// rows at exactly 0.0, and the encoder BiLSTM whose backward direction starts at each utterance's own
// last frame.  Forward only; no workgroup waits on another.
#include <math.h>

#include "../../include/autovc_hip_ragged.h"
#include "lstm_internal.h"

namespace {
using namespace avcl;

// host check shared by the three entry points: B lengths, each in 2..T; the longest comes back
int check_lens(const char* who, const int* lens, const int* lens_dev, int B, int T, int* longest) {
  AVC_CHECK_ARG(lens && lens_dev, "%s: null pointer (lens and lens_dev are both required)", who);
  int mx = 0;
  for (int b = 0; b < B; ++b) {
    AVC_CHECK_ARG(lens[b] >= 2 && lens[b] <= T, "%s: lens[%d] = %d outside 2..T = %d", who, b, lens[b], T);
    mx = lens[b] > mx ? lens[b] : mx;
  }
  *longest = mx;
  return 0;
}

// =============================================================== per-utterance BatchNorm, ragged
// bn_seg.hip's workgroup: one (segment, 64-channel tile), lane tx the channel, the four waves rows
// ty, ty + 4, ...; three passes (pivoted sum, centred squares, apply) over the segment's OWN rows
// 0 .. L-1, every sum in that kernel's order.  L <= AVC_BN_SEG_LDS_ROWS keeps the tile in LDS; a longer
// segment is re-read (64 channels x L rows: L2-resident), four rows of loads in flight per thread --
// the adds stay in row order, so the form does not change a bit of the result.
constexpr int TILE_C = 64;
constexpr int ROW_GROUPS = 4;

__device__ __forceinline__ float group_sum(float* red, int ty, int tx, float v) {
  __syncthreads();  // the previous reduction's reads are done
  red[ty * TILE_C + tx] = v;
  __syncthreads();
  return (red[tx] + red[TILE_C + tx]) + (red[2 * TILE_C + tx] + red[3 * TILE_C + tx]);
}

template <bool RESIDENT>
__device__ __forceinline__ void bn_segment(float* red, float* tile, const float* y, long long ld, int L, int T, int b,
                                           int C, int c, bool cv, long long base, int tx, int ty,
                                           const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                           int act, const float* res, float* out, bf16* out16,
                                           float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  constexpr int RG = ROW_GROUPS;
  const float pivot = cv ? y[base] : 0.f;
  float s = 0.f;
  if (cv) {
    int r = ty;
    if (!RESIDENT)
      for (; r + 3 * RG < L; r += 4 * RG) {
        const float v0 = y[base + (long long)r * ld], v1 = y[base + (long long)(r + RG) * ld];
        const float v2 = y[base + (long long)(r + 2 * RG) * ld], v3 = y[base + (long long)(r + 3 * RG) * ld];
        s += v0 - pivot;
        s += v1 - pivot;
        s += v2 - pivot;
        s += v3 - pivot;
      }
    for (; r < L; r += RG) {
      const float v = y[base + (long long)r * ld];
      if (RESIDENT) tile[r * TILE_C + tx] = v;
      s += v - pivot;
    }
  }
  const float mean = pivot + group_sum(red, ty, tx, s) / (float)L;

  float q = 0.f;
  if (cv) {
    int r = ty;
    if (!RESIDENT)
      for (; r + 3 * RG < L; r += 4 * RG) {
        const float d0 = y[base + (long long)r * ld] - mean, d1 = y[base + (long long)(r + RG) * ld] - mean;
        const float d2 = y[base + (long long)(r + 2 * RG) * ld] - mean;
        const float d3 = y[base + (long long)(r + 3 * RG) * ld] - mean;
        q = fmaf(d0, d0, q);
        q = fmaf(d1, d1, q);
        q = fmaf(d2, d2, q);
        q = fmaf(d3, d3, q);
      }
    for (; r < L; r += RG) {
      const float d = (RESIDENT ? tile[r * TILE_C + tx] : y[base + (long long)r * ld]) - mean;
      q = fmaf(d, d, q);
    }
  }
  const float var = group_sum(red, ty, tx, q) / (float)L;
  const float rstd = 1.f / sqrtf(var + eps);
  if (!cv) return;  // (after the last barrier)
  if (ty == 0) {
    if (mean_out) mean_out[(long long)b * C + c] = mean;
    if (rstd_out) rstd_out[(long long)b * C + c] = rstd;
  }
  const float g = gamma[c] * rstd, be = beta[c];
  for (int r = ty; r < L; r += RG) {
    const long long e = base + (long long)r * ld;
    const float v = RESIDENT ? tile[r * TILE_C + tx] : y[e];
    float o = act_fwd(fmaf(v - mean, g, be), act);
    if (res) o += res[e];
    if (out) out[e] = o;
    if (out16) out16[e] = (bf16)o;
  }
  // the padding rows: exact zeros (no activation of beta, no residual)
  for (int r = L + ty; r < T; r += RG) {
    const long long e = base + (long long)r * ld;
    if (out) out[e] = 0.f;
    if (out16) out16[e] = (bf16)0.f;
  }
}

__global__ void __launch_bounds__(TILE_C* ROW_GROUPS)
    bn_seg_ragged_kernel(const float* y, long long ld, int T, int C, int ctiles, const int* __restrict__ lens,
                         const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int act,
                         const float* res, float* out, bf16* out16, float* __restrict__ mean_out,
                         float* __restrict__ rstd_out) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* red = smem;                         // [ROW_GROUPS][TILE_C]
  float* tile = smem + ROW_GROUPS * TILE_C;  // [min(longest, AVC_BN_SEG_LDS_ROWS)][TILE_C]
  const int tx = threadIdx.x & (TILE_C - 1), ty = threadIdx.x >> 6;
  const int b = blockIdx.x / ctiles, ct = blockIdx.x - b * ctiles;
  const int c = ct * TILE_C + tx;
  const bool cv = c < C;
  const long long base = (long long)b * T * ld + c;  // element (row 0 of the segment, channel c)
  const int L = min(max(lens[b], 2), T);             // (checked on the host; clamped so no row leaves the block)
  if (L <= AVC_BN_SEG_LDS_ROWS)
    bn_segment<true>(red, tile, y, ld, L, T, b, C, c, cv, base, tx, ty, gamma, beta, eps, act, res, out, out16,
                     mean_out, rstd_out);
  else
    bn_segment<false>(red, tile, y, ld, L, T, b, C, c, cv, base, tx, ty, gamma, beta, eps, act, res, out, out16,
                      mean_out, rstd_out);
}

// =============================================================== row mask
// One workgroup per (utterance, chunk of MASK_ROWS padding rows); an utterance with fewer padding rows
// leaves its surplus workgroups idle.  VEC: four columns per store (16 B fp32, 8 B bf16).
constexpr int MASK_ROWS = 16;

template <bool VEC>
__global__ void __launch_bounds__(256) row_mask_kernel(float* x, bf16* x16, long long ld, int T, int C, int chunks,
                                                       const int* __restrict__ lens) {
  const int b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;
  const int L = min(max(lens[b], 0), T);
  const int r0 = L + ch * MASK_ROWS, r1 = min(r0 + MASK_ROWS, T);
  if (r0 >= T) return;
  const int W = VEC ? C / 4 : C;  // stores per row
  const int n = (r1 - r0) * W;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int r = r0 + i / W, k = i - (i / W) * W;
    const long long e = ((long long)b * T + r) * ld + (VEC ? 4 * k : k);
    if (VEC) {
      if (x) *reinterpret_cast<f32x4*>(x + e) = f32x4{0.f, 0.f, 0.f, 0.f};
      if (x16) *reinterpret_cast<u32x2_t*>(x16 + e) = u32x2_t{0u, 0u};
    } else {
      if (x) x[e] = 0.f;
      if (x16) x16[e] = (bf16)0.f;
    }
  }
}

// =============================================================== encoder BiLSTM, ragged, forward only
// lstm_small.hip's packed-FMA recurrence (its step helpers: lstm_internal.h) without its outputs for a
// backward: one workgroup of 4*HM threads
// = one (utterance, direction), lane (j, q) = (tid >> 2, tid & 3) owns gate q of hidden unit j with
// its W_hh row in registers, h_{s-1} in LDS, the x-projection element SD steps ahead in a register
// ring (clamped, unconditional loads).  Only h leaves: lane (j, 0) stores it -- fp32 and / or bf16 --
// as the step ends (a store is never waited for: the ring's loads are older than any store that could
// still be in flight when they are consumed).  The direction's first step is the utterance's own:
// t = 0 forward, t = L - 1 backward.
constexpr int SD = 4;  // input lead, steps

template <int HM, bool FAST>
__global__ void __launch_bounds__(4 * HM) bilstm_ragged_kernel(const float* __restrict__ xproj,
                                                               const float* __restrict__ whh, int T, int H,
                                                               const int* __restrict__ lens, float* __restrict__ hout,
                                                               bf16* __restrict__ hout16) {
  const int b = blockIdx.x, d = blockIdx.y, tid = threadIdx.x;
  const int G = 4 * H;
  __shared__ __attribute__((aligned(16))) float hs[2][HM];
  const long long ldx = 2ll * G, ldh = 2ll * H;
  const int L = min(max(lens[b], 1), T);
  const int t0 = d ? L - 1 : 0, dt = d ? -1 : 1;
  const int j = tid >> 2, q = tid & 3, row = q * H + j;
  const bool act = j < H;

  f32x2 wv[HM / 2];
  {
    const float* W = whh + (long long)d * G * H + (long long)min(row, G - 1) * H;
#pragma unroll
    for (int k = 0; k < HM / 2; ++k)
      wv[k] = f32x2{(act && 2 * k < H) ? W[2 * k] : 0.f, (act && 2 * k + 1 < H) ? W[2 * k + 1] : 0.f};
  }
  if (tid < 2 * HM) hs[tid / HM][tid % HM] = 0.f;
  const float* xl = xproj + (long long)b * T * ldx + d * G + min(row, G - 1);
  auto xload = [&](int sn) { return xl[(long long)(t0 + dt * min(sn, L - 1)) * ldx]; };
  float ring[SD];
#pragma unroll
  for (int r = 0; r < SD; ++r) ring[r] = xload(r);
  float c = 0.f;
  __syncthreads();

  // L rounded up to a multiple of SD: the ghost steps run on clamped inputs and store nothing
  for (int s0 = 0; s0 < L; s0 += SD) {
#pragma unroll
    for (int i = 0; i < SD; ++i) {
      const int s = s0 + i;
      const float xv = ring[i];
      ring[i] = xload(s + SD);
      f32x4 hv[HM / 4];
      {
        const f32x4* v4 = reinterpret_cast<const f32x4*>(hs[s & 1]);
#pragma unroll
        for (int kk = 0; kk < HM / 4; ++kk) hv[kk] = v4[kk];
      }
      const float pre = (act ? xv : 0.f) + dot_regs<HM>(hv, wv);
      float gv;
      if (FAST) {  // tanh(x) = 2 sig(2x) - 1: one exp + rcp for all four gate lanes
        const float sg = fsig((q == 2 ? 2.f : 1.f) * pre);
        gv = q == 2 ? 2.f * sg - 1.f : sg;
      } else {
        gv = q == 2 ? act_tanh<FAST>(pre) : act_sig<FAST>(pre);
      }
      const float ig = quad_bcast<0>(gv), fg = quad_bcast<1>(gv), gg = quad_bcast<2>(gv), og = quad_bcast<3>(gv);
      c = fg * c + ig * gg;
      const float h = og * act_tanh<FAST>(c);
      if (act && q == 0) {
        hs[(s + 1) & 1][j] = h;
        if (s < L) {
          const long long o = ((long long)b * T + t0 + dt * s) * ldh + d * H + j;
          if (hout) hout[o] = h;
          if (hout16) hout16[o] = (bf16)h;
        }
      }
      __syncthreads();
    }
  }
  // the padding rows of this direction's half: zeros
  for (int i = tid; i < (T - L) * H; i += 4 * HM) {
    const int r = L + i / H, u = i - (i / H) * H;
    const long long o = ((long long)b * T + r) * ldh + d * H + u;
    if (hout) hout[o] = 0.f;
    if (hout16) hout16[o] = (bf16)0.f;
  }
}

template <int HM>
void launch_bilstm(dim3 g, hipStream_t s, bool fast, const float* x, const float* w, int T, int H, const int* lens,
                   float* h, bf16* h16) {
  if (fast) bilstm_ragged_kernel<HM, true><<<g, 4 * HM, 0, s>>>(x, w, T, H, lens, h, h16);
  else bilstm_ragged_kernel<HM, false><<<g, 4 * HM, 0, s>>>(x, w, T, H, lens, h, h16);
}

}  // namespace

extern "C" int avc_bn_seg_ragged(const void* y, int y_dtype, long long ld, int B, int T, int C, const int* lens,
                                 const int* lens_dev, const float* gamma, const float* beta, float eps, int act,
                                 const float* residual, float* out, void* out_bf16, float* mean, float* rstd,
                                 void* stream) {
  AVC_CHECK_ARG(y && gamma && beta, "avc_bn_seg_ragged: null pointer (y, gamma and beta are required)");
  AVC_CHECK_ARG(out || out_bf16, "avc_bn_seg_ragged: null pointer (neither out nor out_bf16 given)");
  AVC_CHECK_ARG(y_dtype == AVC_F32,
                "avc_bn_seg_ragged: y_dtype = %d: the statistics are taken from fp32 values only", y_dtype);
  AVC_CHECK_ARG(act >= AVC_ACT_NONE && act <= AVC_ACT_SIGMOID, "avc_bn_seg_ragged: unknown act %d", act);
  AVC_CHECK_ARG(B >= 1 && C >= 1, "avc_bn_seg_ragged: bad shape B = %d, C = %d", B, C);
  AVC_CHECK_ARG(T >= 2, "avc_bn_seg_ragged: T = %d: a segment needs more than one value per channel", T);
  AVC_CHECK_ARG(ld >= C, "avc_bn_seg_ragged: ld = %lld is below C = %d", ld, C);
  AVC_CHECK_ARG(eps >= 0.f && isfinite(eps), "avc_bn_seg_ragged: eps = %g", (double)eps);
  int longest = 0;
  if (check_lens("avc_bn_seg_ragged", lens, lens_dev, B, T, &longest)) return -1;
  const int ctiles = cdiv(C, TILE_C);
  AVC_CHECK_ARG((long long)B * ctiles <= 2147483647ll, "avc_bn_seg_ragged: %lld workgroups", (long long)B * ctiles);
  const int tile_rows = longest < AVC_BN_SEG_LDS_ROWS ? longest : AVC_BN_SEG_LDS_ROWS;
  const size_t lds = sizeof(float) * ((size_t)ROW_GROUPS * TILE_C + (size_t)tile_rows * TILE_C);
  bn_seg_ragged_kernel<<<dim3((unsigned)(B * ctiles)), dim3(TILE_C * ROW_GROUPS), lds, as_stream(stream)>>>(
      static_cast<const float*>(y), ld, T, C, ctiles, lens_dev, gamma, beta, eps, act, residual, out,
      reinterpret_cast<bf16*>(out_bf16), mean, rstd);
  return avc_check_launch("avc_bn_seg_ragged");
}

extern "C" int avc_row_mask(float* x, void* x_bf16, long long ld, int B, int T, int C, const int* lens,
                            const int* lens_dev, void* stream) {
  AVC_CHECK_ARG(x || x_bf16, "avc_row_mask: null pointer (neither x nor x_bf16 given)");
  AVC_CHECK_ARG(B >= 1 && C >= 1 && T >= 2, "avc_row_mask: bad shape B = %d, T = %d, C = %d", B, T, C);
  AVC_CHECK_ARG(ld >= C, "avc_row_mask: ld = %lld is below C = %d", ld, C);
  int longest = 0;
  if (check_lens("avc_row_mask", lens, lens_dev, B, T, &longest)) return -1;
  int shortest = T;
  for (int b = 0; b < B; ++b) shortest = lens[b] < shortest ? lens[b] : shortest;
  if (shortest == T) return 0;  // no padding row anywhere: nothing to write
  const int chunks = cdiv(T - shortest, MASK_ROWS);
  AVC_CHECK_ARG((long long)B * chunks <= 2147483647ll, "avc_row_mask: %lld workgroups", (long long)B * chunks);
  const bool vec = C % 4 == 0 && ld % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)x_bf16 & 7) == 0;
  const dim3 grid((unsigned)(B * chunks));
  bf16* x16 = reinterpret_cast<bf16*>(x_bf16);
  if (vec) row_mask_kernel<true><<<grid, 256, 0, as_stream(stream)>>>(x, x16, ld, T, C, chunks, lens_dev);
  else row_mask_kernel<false><<<grid, 256, 0, as_stream(stream)>>>(x, x16, ld, T, C, chunks, lens_dev);
  return avc_check_launch("avc_row_mask");
}

extern "C" int avc_bilstm_ragged_fwd(const float* xproj, const float* w_hh, const int* lens, const int* lens_dev,
                                     int B, int T, int H, float* h, void* h_bf16, int compute, void* stream) {
  AVC_CHECK_ARG(xproj && w_hh, "avc_bilstm_ragged_fwd: null pointer (xproj and w_hh are required)");
  AVC_CHECK_ARG(h || h_bf16, "avc_bilstm_ragged_fwd: null pointer (neither h nor h_bf16 given)");
  AVC_CHECK_ARG(B >= 1 && T >= 2, "avc_bilstm_ragged_fwd: bad shape B = %d, T = %d", B, T);
  AVC_CHECK_ARG(H >= 1 && H <= 64, "avc_bilstm_ragged_fwd: H = %d outside 1..64 (the encoder's small-H recurrence)", H);
  AVC_CHECK_ARG(compute == AVC_F32 || compute == AVC_BF16, "avc_bilstm_ragged_fwd: unknown compute %d", compute);
  int longest = 0;
  if (check_lens("avc_bilstm_ragged_fwd", lens, lens_dev, B, T, &longest)) return -1;
  const dim3 g((unsigned)B, 2);
  hipStream_t s = as_stream(stream);
  const bool fast = compute == AVC_BF16;
  bf16* h16 = reinterpret_cast<bf16*>(h_bf16);
  if (H <= 32) launch_bilstm<32>(g, s, fast, xproj, w_hh, T, H, lens_dev, h, h16);
  else if (H <= 48) launch_bilstm<48>(g, s, fast, xproj, w_hh, T, H, lens_dev, h, h16);
  else launch_bilstm<64>(g, s, fast, xproj, w_hh, T, H, lens_dev, h, h16);
  return avc_check_launch("avc_bilstm_ragged_fwd");
}
