// metadv.hip — the data movement around the heavy products of the MetaDV speaker classifier
// (factory/MetaDV.py; declared in include/autovc_hip_dv.h).  The LSTM, the window conv and the
// MLP-Mixer run on the existing recurrence / GEMM kernels; what is here is
//   * the batched crop-and-transpose that builds the conv operand of all S crops in one launch
//     (the reference reads the window h[:, left:left+W, :] as a Conv1d input with the W frames as
//     channels and the E hidden units as the length axis) and its gather-sum backward,
//   * the mean over crops of the one mixer output channel the model keeps, and its backward,
//   * the fused forward-only head (chan mean + Linear + L2 normalise + Linear).
// No kernel synchronises between workgroups, spins or uses atomics; every sum has a fixed order.
#include "common.h"

#include "../../include/autovc_hip_dv.h"

namespace {

constexpr int CT = 64;        // tile edge of the transposes
constexpr int CTHREADS = 256;

template <typename T>
struct Vec4;
template <>
struct Vec4<float> {
  typedef f32x4 type;
};
template <>
struct Vec4<bf16> {
  typedef bf16x4 type;
};

// One (s, b) crop, one CT x CT tile: rows of h (coalesced along E) -> LDS -> rows of X (coalesced
// along the window axis).  The tile is padded to CT + 1 floats per row: the four-wide vector
// phases touch banks (row + 4 * vec + i) mod 64 on either side, distinct across a wave.
// vin / vout: four-element vectors on the read / write side (E resp. W a multiple of 4 and an
// aligned base); otherwise that side moves single elements, which also covers the partial tiles
// of an E or W that is no multiple of CT (guards per element / per vector).
template <typename TI, typename TO>
__global__ void __launch_bounds__(CTHREADS) crop_windows_kernel(const TI* __restrict__ h, const int* __restrict__ left,
                                                                int B, int T, int E, int W, TO* __restrict__ X,
                                                                int vin, int vout) {
  __shared__ float tile[CT][CT + 1];  // [c][l]
  const int sb = blockIdx.z, b = sb % B, tid = threadIdx.x;
  const int l0 = blockIdx.x * CT, c0 = blockIdx.y * CT;
  const int lf = left[sb];
  const TI* src = h + ((long long)b * T + lf + c0) * E + l0;
  if (vin) {
    typedef typename Vec4<TI>::type VI;
    const int lv = (tid & 15) * 4;
    for (int c = tid >> 4; c < CT; c += CTHREADS / 16) {
      if (c0 + c < W && l0 + lv < E) {
        const VI v = *reinterpret_cast<const VI*>(src + (long long)c * E + lv);
#pragma unroll
        for (int i = 0; i < 4; ++i) tile[c][lv + i] = (float)v[i];
      }
    }
  } else {
    const int l = tid & 63;
    for (int c = tid >> 6; c < CT; c += CTHREADS / 64)
      if (c0 + c < W && l0 + l < E) tile[c][l] = (float)src[(long long)c * E + l];
  }
  __syncthreads();
  TO* dst = X + ((long long)sb * E + l0) * W + c0;
  if (vout) {
    typedef typename Vec4<TO>::type VO;
    const int cv = (tid & 15) * 4;
    for (int l = tid >> 4; l < CT; l += CTHREADS / 16) {
      if (l0 + l < E && c0 + cv < W) {
        VO v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (TO)tile[cv + i][l];
        *reinterpret_cast<VO*>(dst + (long long)l * W + cv) = v;
      }
    }
  } else {
    const int c = tid & 63;
    for (int l = tid >> 6; l < CT; l += CTHREADS / 64)
      if (l0 + l < E && c0 + c < W) dst[(long long)l * W + c] = (TO)tile[c][l];
  }
}

// dh tile (CT frames x CT units) of utterance b: per (l, t) the crops covering t are summed in
// crop order (reads coalesced along the window axis), the tile turns in LDS, and the write is
// coalesced along E; de1 joins at t = last[b].  Every element of dh is written.
__global__ void __launch_bounds__(CTHREADS) crop_windows_bwd_kernel(const float* __restrict__ dX,
                                                                    const float* __restrict__ de1,
                                                                    const int* __restrict__ left,
                                                                    const int* __restrict__ last, int B, int T, int E,
                                                                    int W, int S, float* __restrict__ dh) {
  __shared__ float tile[CT][CT + 1];  // [l][t]
  const int b = blockIdx.z, tid = threadIdx.x;
  const int l0 = blockIdx.x * CT, t0 = blockIdx.y * CT;
  {
    const int t = t0 + (tid & 63);
    for (int l = tid >> 6; l < CT; l += CTHREADS / 64) {
      float acc = 0.f;
      if (t < T && l0 + l < E) {
        for (int s = 0; s < S; ++s) {
          const int c = t - left[s * B + b];
          if (c >= 0 && c < W) acc += dX[((long long)(s * B + b) * E + l0 + l) * W + c];
        }
      }
      tile[l][tid & 63] = acc;
    }
  }
  __syncthreads();
  const int l = l0 + (tid & 63);
  const int tl = last ? last[b] : T - 1;
  for (int tt = tid >> 6; tt < CT; tt += CTHREADS / 64) {
    const int t = t0 + tt;
    if (t < T && l < E) {
      float v = tile[tid & 63][tt];
      if (de1 && t == tl) v += de1[(long long)b * E + l];
      dh[((long long)b * T + t) * E + l] = v;
    }
  }
}

__global__ void __launch_bounds__(256) chan_mean_kernel(const float* __restrict__ Y, int S, int B, int E, int O,
                                                        float* __restrict__ e2) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // b * E + l
  if (i >= B * E) return;
  const long long sstride = (long long)B * E * O;
  const float* p = Y + (long long)i * O + O - 1;
  float acc = 0.f;
  for (int s = 0; s < S; ++s) acc += p[s * sstride];
  e2[i] = acc / (float)S;
}

__global__ void __launch_bounds__(256) chan_mean_bwd_kernel(const float* __restrict__ g, int S, int B, int E, int O,
                                                            long long n, float* __restrict__ dY) {
  const long long step = (long long)gridDim.x * 256;
  const int BE = B * E;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
    const long long row = i / O;
    const int col = (int)(i - row * O);
    dY[i] = col == O - 1 ? g[(int)(row % BE)] / (float)S : 0.f;
  }
}

// The forward-only head, one workgroup of 16 waves per utterance (the shape of avc_dvec_head):
// cat(e1[b], e2[b]) is staged in LDS -- e2 straight from the mixer output, which folds the channel
// mean in -- each wave takes HD_U rows of W_dv at a time with a float4 per lane and row, the
// workgroup reduces ||emb||^2, writes d_vec, and the waves then take the class logits one row of
// W_out each.
constexpr int HD_THREADS = 1024, HD_U = 8;

__global__ void __launch_bounds__(HD_THREADS) metadv_head_kernel(const float* __restrict__ e1,
                                                                 const float* __restrict__ Y, int S, int O,
                                                                 const float* __restrict__ w_dv,
                                                                 const float* __restrict__ b_dv,
                                                                 const float* __restrict__ w_out,
                                                                 const float* __restrict__ b_out, int B, int E, int D,
                                                                 int C, float* __restrict__ pred,
                                                                 float* __restrict__ d_vec) {
  extern __shared__ __attribute__((aligned(16))) float hsm[];
  float* xs = hsm;          // [2E]
  float* ys = hsm + 2 * E;  // [D]
  __shared__ float red[HD_THREADS / 64];
  constexpr int NW = HD_THREADS / 64;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, H = 2 * E, H4 = H >> 2;
  const long long sstride = (long long)B * E * O;
  for (int l = tid; l < E; l += HD_THREADS) {
    xs[l] = e1[(long long)b * E + l];
    const float* p = Y + ((long long)b * E + l) * O + O - 1;
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc += p[s * sstride];
    xs[E + l] = acc / (float)S;
  }
  __syncthreads();
  const f32x4* xs4 = reinterpret_cast<const f32x4*>(xs);
  const f32x4* w4 = reinterpret_cast<const f32x4*>(w_dv);
  for (int e0 = wv * HD_U; e0 < D; e0 += NW * HD_U) {
    float acc[HD_U];
#pragma unroll
    for (int u = 0; u < HD_U; ++u) acc[u] = 0.f;
    for (int k = lane; k < H4; k += 64) {
      const f32x4 x = xs4[k];
#pragma unroll
      for (int u = 0; u < HD_U; ++u) {
        const f32x4 a = w4[(long long)min(e0 + u, D - 1) * H4 + k];  // rows past D repeat the last one
        acc[u] += a[0] * x[0] + a[1] * x[1] + a[2] * x[2] + a[3] * x[3];
      }
    }
#pragma unroll
    for (int u = 0; u < HD_U; ++u) {
      const float v = warp_sum(acc[u]);
      if (lane == 0 && e0 + u < D) ys[e0 + u] = v + (b_dv ? b_dv[e0 + u] : 0.f);
    }
  }
  __syncthreads();
  float ss = 0.f;
  for (int e = tid; e < D; e += HD_THREADS) ss += ys[e] * ys[e];
  ss = warp_sum(ss);
  if (lane == 0) red[wv] = ss;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) tot += red[i];
  const float nrm = sqrtf(tot);
  for (int e = tid; e < D; e += HD_THREADS) d_vec[(long long)b * D + e] = ys[e] / nrm;
  for (int c = wv; c < C; c += NW) {
    const float* wr = w_out + (long long)c * D;
    float acc = 0.f;
    for (int k = lane; k < D; k += 64) acc += wr[k] * ys[k];
    acc = warp_sum(acc);
    if (lane == 0) pred[(long long)b * C + c] = acc + (b_out ? b_out[c] : 0.f);
  }
}

// 0 <= left[s*B + b] <= len_b - W for every crop; returns 0 or -1 with the error recorded
int check_lefts(const char* who, const int* left, const int* lens, int B, int T, int W, int S) {
  for (int b = 0; b < B; ++b) {
    const int len = lens ? lens[b] : T;
    AVC_CHECK_ARG(len >= 1 && len <= T, "%s: lens[%d] = %d outside 1..T = %d", who, b, len, T);
    AVC_CHECK_ARG(W <= len, "%s: window W = %d longer than the %d frames of utterance %d", who, W, len, b);
    for (int s = 0; s < S; ++s) {
      const int lf = left[s * B + b];
      AVC_CHECK_ARG(lf >= 0 && lf <= len - W, "%s: left[%d][%d] = %d outside 0..%d", who, s, b, lf, len - W);
    }
  }
  return 0;
}

}  // namespace

extern "C" int avc_crop_windows(const void* h, int h_dtype, const int* left, const int* left_dev, const int* lens,
                                int B, int T, int E, int W, int S, void* X, int x_dtype, void* stream) {
  AVC_CHECK_ARG(h && left && left_dev && X, "avc_crop_windows: null pointer (h, left, left_dev and X are required)");
  AVC_CHECK_ARG(B > 0 && T > 0 && E > 0 && W > 0 && S > 0 && (long long)S * B <= 65535,
                "avc_crop_windows: bad shape B=%d T=%d E=%d W=%d S=%d (S*B <= 65535)", B, T, E, W, S);
  AVC_CHECK_ARG(W <= T, "avc_crop_windows: window W = %d longer than T = %d", W, T);
  AVC_CHECK_ARG((h_dtype == AVC_F32 || h_dtype == AVC_BF16) && (x_dtype == AVC_F32 || x_dtype == AVC_BF16) &&
                    !(h_dtype == AVC_BF16 && x_dtype == AVC_F32),
                "avc_crop_windows: dtypes h=%d X=%d (fp32 -> fp32 / bf16, bf16 -> bf16)", h_dtype, x_dtype);
  AVC_CHECK_ARG((long long)B * T * E < (1ll << 31) && (long long)S * B * E * W < (1ll << 31),
                "avc_crop_windows: more than 2^31 elements");
  if (check_lefts("avc_crop_windows", left, lens, B, T, W, S)) return -1;
  const int vin = E % 4 == 0 && ((uintptr_t)h & 15) == 0, vout = W % 4 == 0 && ((uintptr_t)X & 15) == 0;
  const dim3 grid(cdiv(E, CT), cdiv(W, CT), S * B);
  hipStream_t st = as_stream(stream);
  if (h_dtype == AVC_F32 && x_dtype == AVC_F32)
    crop_windows_kernel<float, float><<<grid, CTHREADS, 0, st>>>(reinterpret_cast<const float*>(h), left_dev, B, T, E,
                                                                 W, reinterpret_cast<float*>(X), vin, vout);
  else if (h_dtype == AVC_F32)
    crop_windows_kernel<float, bf16><<<grid, CTHREADS, 0, st>>>(reinterpret_cast<const float*>(h), left_dev, B, T, E, W,
                                                                reinterpret_cast<bf16*>(X), vin, vout);
  else
    crop_windows_kernel<bf16, bf16><<<grid, CTHREADS, 0, st>>>(reinterpret_cast<const bf16*>(h), left_dev, B, T, E, W,
                                                               reinterpret_cast<bf16*>(X), vin, vout);
  return avc_check_launch("avc_crop_windows");
}

extern "C" int avc_crop_windows_bwd(const float* dX, const float* de1, const int* left, const int* left_dev,
                                    const int* last, const int* last_dev, int B, int T, int E, int W, int S, float* dh,
                                    void* stream) {
  AVC_CHECK_ARG(dX && left && left_dev && dh,
                "avc_crop_windows_bwd: null pointer (dX, left, left_dev and dh are required)");
  AVC_CHECK_ARG((last == nullptr) == (last_dev == nullptr), "avc_crop_windows_bwd: last and last_dev go together");
  AVC_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && E > 0 && W > 0 && S > 0 && cdiv(T, CT) <= 65535,
                "avc_crop_windows_bwd: bad shape B=%d T=%d E=%d W=%d S=%d", B, T, E, W, S);
  AVC_CHECK_ARG(W <= T, "avc_crop_windows_bwd: window W = %d longer than T = %d", W, T);
  AVC_CHECK_ARG((long long)B * T * E < (1ll << 31) && (long long)S * B * E * W < (1ll << 31),
                "avc_crop_windows_bwd: more than 2^31 elements");
  if (check_lefts("avc_crop_windows_bwd", left, nullptr, B, T, W, S)) return -1;
  if (last)
    for (int b = 0; b < B; ++b)
      AVC_CHECK_ARG(last[b] >= 0 && last[b] < T, "avc_crop_windows_bwd: last[%d] = %d outside 0..%d", b, last[b], T - 1);
  const dim3 grid(cdiv(E, CT), cdiv(T, CT), B);
  crop_windows_bwd_kernel<<<grid, CTHREADS, 0, as_stream(stream)>>>(dX, de1, left_dev, last_dev, B, T, E, W, S, dh);
  return avc_check_launch("avc_crop_windows_bwd");
}

extern "C" int avc_chan_mean(const float* Y, int S, int B, int E, int O, float* e2, void* stream) {
  AVC_CHECK_ARG(Y && e2, "avc_chan_mean: null pointer");
  AVC_CHECK_ARG(S > 0 && B > 0 && E > 0 && O > 0 && (long long)S * B * E * O < (1ll << 31),
                "avc_chan_mean: bad shape S=%d B=%d E=%d O=%d", S, B, E, O);
  chan_mean_kernel<<<cdiv((long long)B * E, 256), 256, 0, as_stream(stream)>>>(Y, S, B, E, O, e2);
  return avc_check_launch("avc_chan_mean");
}

extern "C" int avc_chan_mean_bwd(const float* g, int S, int B, int E, int O, float* dY, void* stream) {
  AVC_CHECK_ARG(g && dY, "avc_chan_mean_bwd: null pointer");
  AVC_CHECK_ARG(S > 0 && B > 0 && E > 0 && O > 0 && (long long)S * B * E * O < (1ll << 31),
                "avc_chan_mean_bwd: bad shape S=%d B=%d E=%d O=%d", S, B, E, O);
  const long long n = (long long)S * B * E * O;
  const int blocks = (int)((n + 4 * 256 - 1) / (4 * 256));
  chan_mean_bwd_kernel<<<blocks, 256, 0, as_stream(stream)>>>(g, S, B, E, O, n, dY);
  return avc_check_launch("avc_chan_mean_bwd");
}

extern "C" int avc_metadv_head(const float* e1, const float* Y, int S, int O, const float* w_dv, const float* b_dv,
                               const float* w_out, const float* b_out, int B, int E, int D, int C, float* pred,
                               float* d_vec, void* stream) {
  AVC_CHECK_ARG(e1 && Y && w_dv && w_out && pred && d_vec, "avc_metadv_head: null pointer");
  AVC_CHECK_ARG(S > 0 && O > 0 && B > 0 && E > 0 && D > 0 && C > 0 && E % 4 == 0 &&
                    (size_t)(2 * E + D) * 4 <= 48 * 1024 && (long long)S * B * E * O < (1ll << 31),
                "avc_metadv_head: bad shape S=%d O=%d B=%d E=%d D=%d C=%d (E a multiple of 4, (2E + D) floats of LDS)",
                S, O, B, E, D, C);
  AVC_CHECK_ARG(((uintptr_t)w_dv & 15) == 0, "avc_metadv_head: w_dv must be 16-byte aligned");
  metadv_head_kernel<<<B, HD_THREADS, (size_t)(2 * E + D) * 4, as_stream(stream)>>>(e1, Y, S, O, w_dv, b_dv, w_out,
                                                                                    b_out, B, E, D, C, pred, d_vec);
  return avc_check_launch("avc_metadv_head");
}
