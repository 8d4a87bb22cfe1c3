// melgan_ragged.hip — the MelGAN generator over a batch of utterances of DIFFERENT lengths
// (include/autovc_hip_vocoder.h).  The generator is fully convolutional and its GEMMs are row-wise, so a
// ragged batch needs a length only where a kernel looks across rows: the reflect gather in front of a
// dilated conv, the LeakyReLU twin in front of a transposed conv (whose 3-tap window operand zero-pads at
// the block edge and must see zeros after a short utterance's last frame too) and the output layer.
//
// Invariant (stated once, kept by all three kernels): at a stage of cumulative upsampling `scale`,
// utterance b owns rows 0 .. n_b - 1, n_b = lens[b]*scale, of its block of L = Tmax*scale rows.
//   * A valid output row reads valid input rows only (reflection about 0 and n_b - 1).
//   * Every padding row written here is exactly 0.0; no padding row of an input is read (it may be NaN).
//   * Padding rows of the GEMM outputs in between hold finite values (bias plus products of those zeros
//     and of each other through the row-wise 1x1 / shortcut GEMMs); no valid row ever reads them, and the
//     next kernel of this file that writes a padding row writes 0.0 over whatever they led to.
//
// Index maths: the grid's y axis is the utterance, so n_b is one uniform load per workgroup and there is
// no division by L.  A thread owns (row, lane): `lpr` lanes (a power of two chosen from C / 4 on the host)
// sweep the 4-channel quads of one row, 256 / lpr rows per workgroup per sweep; the row's reflected source
// indices are computed once per row and tap, the per-element work is one 16-byte (fp32) or 8-byte (bf16)
// load, at most one multiply per channel and one store.  No LDS (but the output layer's weights), no
// atomics, one fixed order.
#include <algorithm>

#include "../../include/autovc_hip_vocoder.h"
#include "melgan_internal.h"

namespace {
using namespace avmg;

constexpr int THREADS = 256;

// rows of block b that belong to the utterance; the clamp keeps every access inside the block should
// lens_dev disagree with the host ints that were checked
__device__ __forceinline__ int valid_rows(const int* __restrict__ lens, int b, int scale, int Tmax) {
  return min(max(lens[b], 0), Tmax) * scale;
}

// out[(b*L + t)][k*C + c] = act(x[b*L + reflect_n(t + k*dil - pad)][c]) for t < n_b, 0 for t >= n_b.
// TAPS > 0: the tap loop unrolled (its loads independent and in flight together); TAPS = 0: `taps` at run time.
template <typename TI, typename TO, int TAPS>
__global__ void __launch_bounds__(THREADS)
    mg_gather_ragged_kernel(const TI* __restrict__ x, int Tmax, int L, int C, int taps_rt, int dil, int pad,
                            int lpr_shift, int act, float slope, const int* __restrict__ lens, int scale,
                            TO* __restrict__ out) {
  const int taps = TAPS ? TAPS : taps_rt;
  const int b = blockIdx.y;
  const int n = valid_rows(lens, b, scale, Tmax);
  const int lpr = 1 << lpr_shift, lane = threadIdx.x & (lpr - 1), rpb = THREADS >> lpr_shift;
  const int C4 = C >> 2;
  const long long row0 = (long long)b * L;
  const long long ldo = (long long)taps * C;
  for (int t = blockIdx.x * rpb + (threadIdx.x >> lpr_shift); t < L; t += gridDim.x * rpb) {
    TO* orow = out + (row0 + t) * ldo;
    if (t >= n) {  // a padding row: exact zeros, nothing read
      for (int k = 0; k < taps; ++k)
        for (int c4 = lane; c4 < C4; c4 += lpr) st4(orow + (long long)k * C + 4 * c4, f32x4{0.f, 0.f, 0.f, 0.f});
      continue;
    }
#pragma unroll
    for (int k = 0; k < taps; ++k) {
      int s = t + k * dil - pad;
      s = s < 0 ? -s : (s >= n ? 2 * (n - 1) - s : s);
      s = min(max(s, 0), n - 1);  // (pad < n is checked on the host: one reflection lands inside)
      const TI* xrow = x + (row0 + s) * C;
      for (int c4 = lane; c4 < C4; c4 += lpr) {
        f32x4 v = ld4(xrow + 4 * c4);
        if (act) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = lrelu(v[e], slope);
        }
        st4(orow + (long long)k * C + 4 * c4, v);
      }
    }
  }
}

// LeakyReLU of the valid rows, zeros in the padding rows, into the fp32 and / or the bf16 copy
__global__ void __launch_bounds__(THREADS)
    mg_act_ragged_kernel(const float* __restrict__ x, int Tmax, int L, int C, int lpr_shift, float slope,
                         const int* __restrict__ lens, int scale, float* __restrict__ out, bf16* __restrict__ out16) {
  const int b = blockIdx.y;
  const int n = valid_rows(lens, b, scale, Tmax);
  const int lpr = 1 << lpr_shift, lane = threadIdx.x & (lpr - 1), rpb = THREADS >> lpr_shift;
  const int C4 = C >> 2;
  for (int t = blockIdx.x * rpb + (threadIdx.x >> lpr_shift); t < L; t += gridDim.x * rpb) {
    const long long base = ((long long)b * L + t) * C;
    const bool valid = t < n;
    for (int c4 = lane; c4 < C4; c4 += lpr) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (valid) {
        v = ld4(x + base + 4 * c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = lrelu(v[e], slope);
      }
      if (out) st4(out + base + 4 * c4, v);
      if (out16) st4(out16 + base + 4 * c4, v);
    }
  }
}

// audio[b][t] = tanh(bias + sum_k sum_c w[k][c] * lrelu(x[b][reflect_n(t + k - 3)][c])), 0 for t >= n_b:
// melgan.hip's mg_conv_out_kernel (same sums, same order) with the utterance on the grid's y axis
template <int TAPS>
__global__ void __launch_bounds__(THREADS)
    mg_conv_out_ragged_kernel(const float* __restrict__ x, int Tmax, int L, int C, const float* __restrict__ w,
                              const float* __restrict__ bias, float slope, const int* __restrict__ lens, int scale,
                              float* __restrict__ out) {
  extern __shared__ float ws[];  // [TAPS][C]
  for (int i = threadIdx.x; i < TAPS * C; i += blockDim.x) ws[i] = w[i];
  __syncthreads();
  const int b = blockIdx.y;
  const int n = valid_rows(lens, b, scale, Tmax);
  const int t = blockIdx.x * THREADS + threadIdx.x;
  if (t >= L) return;
  const long long m = (long long)b * L + t;
  if (t >= n) {
    out[m] = 0.f;
    return;
  }
  float acc = bias[0];
#pragma unroll
  for (int k = 0; k < TAPS; ++k) {
    const int s = min(max(src_frame(t + k - TAPS / 2, n, 1), 0), n - 1);  // (n > 3 is checked on the host)
    const float* row = x + ((long long)b * L + s) * C;
    for (int c = 0; c < C; c += 4) {
      const f32x4 v = ld4(row + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc += ws[k * C + c + e] * lrelu(v[e], slope);
    }
  }
  out[m] = tanhf(acc);
}

// ------------------------------------------------------------------------------------------ host
// The checks the three entry points share; L = Tmax*scale comes back.
int check_common(const char* who, int B, int Tmax, int C, const int* lens, const int* lens_dev, int scale, int* L) {
  AVC_CHECK_ARG(lens && lens_dev, "%s: null pointer (lens and lens_dev are both required)", who);
  AVC_CHECK_ARG(B >= 1 && B <= 65535, "%s: B = %d outside 1..65535 (the utterance is the grid's y axis)", who, B);
  AVC_CHECK_ARG(Tmax >= 1 && scale >= 1, "%s: bad shape Tmax = %d, scale = %d", who, Tmax, scale);
  // (2^30: a row index plus a pad below it, and the grid-stride step, stay inside an int)
  AVC_CHECK_ARG((long long)Tmax * scale <= (1ll << 30), "%s: Tmax*scale = %lld rows per utterance exceed 2^30", who,
                (long long)Tmax * scale);
  AVC_CHECK_ARG(C >= 4 && C % 4 == 0, "%s: C = %d must be a positive multiple of 4 (4 channels per access)", who, C);
  for (int b = 0; b < B; ++b)
    AVC_CHECK_ARG(lens[b] >= 1 && lens[b] <= Tmax, "%s: lens[%d] = %d outside 1..Tmax = %d", who, b, lens[b], Tmax);
  *L = Tmax * scale;
  return 0;
}

bool aligned4(const void* p, int dtype) { return ((uintptr_t)p & (dtype == AVC_BF16 ? 7u : 15u)) == 0; }

// lanes per row: the largest power of two <= 64 that keeps at least 4 of 5 lanes busy over C4 quads
int lpr_shift_for(int C4) {
  for (int sh = 6; sh > 0; --sh) {
    const int p = 1 << sh;
    if (5 * C4 >= 4 * (cdiv(C4, p) * p)) return sh;
  }
  return 0;
}

// x blocks per utterance: every row once, capped so that the whole grid stays near 8192 workgroups
unsigned grid_x(int L, int rpb, int B) { return (unsigned)std::max(1, std::min(cdiv(L, rpb), cdiv(8192, B))); }

template <typename TI, typename TO>
void launch_gather(dim3 g, hipStream_t s, const void* x, int Tmax, int L, int C, int taps, int dil, int pad, int sh,
                   int act, float slope, const int* lens_dev, int scale, void* out) {
  const TI* xi = static_cast<const TI*>(x);
  TO* o = static_cast<TO*>(out);
  if (taps == 3)
    mg_gather_ragged_kernel<TI, TO, 3><<<g, THREADS, 0, s>>>(xi, Tmax, L, C, taps, dil, pad, sh, act, slope, lens_dev,
                                                              scale, o);
  else if (taps == 7)
    mg_gather_ragged_kernel<TI, TO, 7><<<g, THREADS, 0, s>>>(xi, Tmax, L, C, taps, dil, pad, sh, act, slope, lens_dev,
                                                              scale, o);
  else
    mg_gather_ragged_kernel<TI, TO, 0><<<g, THREADS, 0, s>>>(xi, Tmax, L, C, taps, dil, pad, sh, act, slope, lens_dev,
                                                              scale, o);
}

}  // namespace

extern "C" int avc_mg_gather_ragged(const void* x, int x_dtype, int B, int Tmax, int C, int taps, int dil, int pad,
                                    int act, float slope, const int* lens, const int* lens_dev, int scale, void* out,
                                    int out_dtype, void* stream) {
  AVC_CHECK_ARG(x && out, "avc_mg_gather_ragged: null pointer (x and out are required)");
  AVC_CHECK_ARG((x_dtype == AVC_F32 || x_dtype == AVC_BF16) && (out_dtype == AVC_F32 || out_dtype == AVC_BF16),
                "avc_mg_gather_ragged: unknown dtype %d -> %d", x_dtype, out_dtype);
  int L = 0;
  if (check_common("avc_mg_gather_ragged", B, Tmax, C, lens, lens_dev, scale, &L)) return -1;
  AVC_CHECK_ARG(aligned4(x, x_dtype) && aligned4(out, out_dtype),
                "avc_mg_gather_ragged: x and out must be aligned to 4 elements");
  AVC_CHECK_ARG(taps >= 1 && dil >= 1 && pad >= 0 && (long long)dil * (taps - 1) == 2ll * pad,
                "avc_mg_gather_ragged: taps = %d, dil = %d, pad = %d is not a conv that keeps the length "
                "(2*pad = dil*(taps - 1))", taps, dil, pad);
  AVC_CHECK_ARG((long long)taps * C <= 2147483647ll, "avc_mg_gather_ragged: taps*C = %lld", (long long)taps * C);
  for (int b = 0; b < B; ++b)
    AVC_CHECK_ARG((long long)lens[b] * scale > pad,
                  "avc_mg_gather_ragged: reflection pad %d needs more than pad rows, lens[%d]*scale = %lld", pad, b,
                  (long long)lens[b] * scale);
  const int sh = lpr_shift_for(C / 4);
  const dim3 g(grid_x(L, THREADS >> sh, B), (unsigned)B);
  hipStream_t s = as_stream(stream);
  if (x_dtype == AVC_BF16) {
    if (out_dtype == AVC_BF16)
      launch_gather<bf16, bf16>(g, s, x, Tmax, L, C, taps, dil, pad, sh, act, slope, lens_dev, scale, out);
    else
      launch_gather<bf16, float>(g, s, x, Tmax, L, C, taps, dil, pad, sh, act, slope, lens_dev, scale, out);
  } else {
    if (out_dtype == AVC_BF16)
      launch_gather<float, bf16>(g, s, x, Tmax, L, C, taps, dil, pad, sh, act, slope, lens_dev, scale, out);
    else
      launch_gather<float, float>(g, s, x, Tmax, L, C, taps, dil, pad, sh, act, slope, lens_dev, scale, out);
  }
  return avc_check_launch("avc_mg_gather_ragged");
}

extern "C" int avc_mg_act_ragged(const float* x, int B, int Tmax, int C, float slope, const int* lens,
                                 const int* lens_dev, int scale, float* out, void* out_bf16, void* stream) {
  AVC_CHECK_ARG(x, "avc_mg_act_ragged: null pointer (x is required)");
  AVC_CHECK_ARG(out || out_bf16, "avc_mg_act_ragged: null pointer (neither out nor out_bf16 given)");
  int L = 0;
  if (check_common("avc_mg_act_ragged", B, Tmax, C, lens, lens_dev, scale, &L)) return -1;
  AVC_CHECK_ARG(aligned4(x, AVC_F32) && aligned4(out, AVC_F32) && aligned4(out_bf16, AVC_BF16),
                "avc_mg_act_ragged: x, out and out_bf16 must be aligned to 4 elements");
  const int sh = lpr_shift_for(C / 4);
  const dim3 g(grid_x(L, THREADS >> sh, B), (unsigned)B);
  mg_act_ragged_kernel<<<g, THREADS, 0, as_stream(stream)>>>(x, Tmax, L, C, sh, slope, lens_dev, scale, out,
                                                             reinterpret_cast<bf16*>(out_bf16));
  return avc_check_launch("avc_mg_act_ragged");
}

extern "C" int avc_mg_conv_out_ragged(const float* x, int B, int Tmax, int C, int taps, const float* w,
                                      const float* bias, float slope, const int* lens, const int* lens_dev, int scale,
                                      float* out, void* stream) {
  AVC_CHECK_ARG(x && w && bias && out, "avc_mg_conv_out_ragged: null pointer (x, w, bias and out are required)");
  AVC_CHECK_ARG(taps == 7, "avc_mg_conv_out_ragged: taps = %d (the output layer has 7)", taps);
  int L = 0;
  if (check_common("avc_mg_conv_out_ragged", B, Tmax, C, lens, lens_dev, scale, &L)) return -1;
  AVC_CHECK_ARG(aligned4(x, AVC_F32), "avc_mg_conv_out_ragged: x must be aligned to 4 elements");
  AVC_CHECK_ARG((size_t)taps * C * sizeof(float) <= 65536, "avc_mg_conv_out_ragged: C = %d: the weights exceed LDS", C);
  for (int b = 0; b < B; ++b)
    AVC_CHECK_ARG((long long)lens[b] * scale > taps / 2,
                  "avc_mg_conv_out_ragged: reflection pad %d needs more than pad rows, lens[%d]*scale = %lld", taps / 2,
                  b, (long long)lens[b] * scale);
  const dim3 g((unsigned)cdiv(L, THREADS), (unsigned)B);
  mg_conv_out_ragged_kernel<7><<<g, THREADS, taps * C * sizeof(float), as_stream(stream)>>>(
      x, Tmax, L, C, w, bias, slope, lens_dev, scale, out);
  return avc_check_launch("avc_mg_conv_out_ragged");
}
