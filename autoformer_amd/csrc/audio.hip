// audio.hip — waveform -> log-mel in one launch (declared in include/autovc_hip_audio.h): the
// reference's Audio2Mel (melgan/modules.py:26-69) and the notebook's mel_gan_handler.
//
// A workgroup of 256 threads takes AU_FPW = 8 consecutive frames of one utterance.
//   1. The 7*256 + 1024 = 2816 samples the frames share are loaded once into LDS, scaled, with the
//      reflection done by index at the utterance's two ends (never a neighbour's samples).
//   2. Each frame's 1024-point real FFT is a 512-point complex FFT of z[n] = x[2n] + i x[2n+1] plus
//      the split step.  The FFT is a radix-2 Stockham autosort, fp32, nine passes; thread j owns
//      butterfly j of all eight frames, so a pass's twiddle is one register pair per thread, taken
//      before the first pass from the host's table (fp64 rounded to fp32; no sincosf here).
//      Pass 1 reads the windowed samples straight from the span.
//   3. The split step writes |X[k]|, k = 0..512, per frame.
//   4. Mel, filter-major: one lane per (filter, frame) runs over the filter's contiguous support
//      from the compact table in LDS, then log10(max(., floor)).
//   5. The 8 x n_mel tile turns in LDS and is stored in either layout; frames t >= T_b as 0.0.
//
// LDS layout.  Real and imaginary parts are separate float planes, [frame][512] each, so every
// access is a 4-byte one (32 banks, lane groups of 32).  A Stockham pass reads in[j] and
// in[j + 256] -- consecutive lanes, consecutive words, conflict-free at any stage, which is what the
// constant-geometry form buys over the in-place one, whose power-of-two strides collide -- and
// writes out[j0], out[j0 + Ns] with j0 = 2 (j - j % Ns) + j % Ns: 32 lanes cover 32 of 64
// consecutive words, at most 2 on a bank, which a 4-byte LDS store absorbs (its issue cost already
// covers two array cycles).  The price is the second buffer: 2 x 32 KiB, the sample span aliased
// onto the second one (dead after pass 1), the magnitudes as well (row stride 516 = 4 mod 32 words,
// so the eight frames of one filter sit on eight different banks), the output tile onto the first.
// With the default filterbank (1000 weights) that is 70 KiB: two workgroups per CU.
#include "common.h"

#include "../../include/autovc_hip_audio.h"

namespace {

constexpr int AU_NFFT = 1024, AU_HOP = 256, AU_PAD = (AU_NFFT - AU_HOP) / 2, AU_NB = AU_NFFT / 2 + 1;
constexpr int AU_H = AU_NFFT / 2;  // complex points
constexpr int AU_FPW = 8, AU_THREADS = 256;
constexpr int AU_SPAN = (AU_FPW - 1) * AU_HOP + AU_NFFT;
constexpr int AU_MS = 516;                   // magnitude row stride
constexpr int AU_BUF = 2 * AU_FPW * AU_H;    // floats of one ping-pong buffer (re plane, im plane)
constexpr int AU_MAX_MEL = 128;

static_assert(AU_THREADS == AU_H / 2, "one radix-2 butterfly per thread and frame");
static_assert(AU_SPAN <= AU_BUF && AU_FPW * AU_MS <= AU_BUF && AU_FPW * (AU_MAX_MEL + 1) <= AU_BUF, "aliases fit");

// One Stockham pass over all frames: butterfly j, sub-transform length NS going to 2 NS.
template <int NS>
__device__ __forceinline__ void au_pass(const float* __restrict__ in, float* __restrict__ out, int j, float2 tw) {
  const int k = j & (NS - 1), j0 = ((j - k) << 1) + k;
#pragma unroll
  for (int f = 0; f < AU_FPW; ++f) {
    const float* re = in + f * AU_H;
    const float* im = in + (AU_FPW + f) * AU_H;
    const float ar = re[j], ai = im[j], br = re[j + AU_H / 2], bi = im[j + AU_H / 2];
    const float cr = br * tw.x - bi * tw.y, ci = br * tw.y + bi * tw.x;
    float* ore = out + f * AU_H;
    float* oim = out + (AU_FPW + f) * AU_H;
    ore[j0] = ar + cr;
    oim[j0] = ai + ci;
    ore[j0 + NS] = ar - cr;
    oim[j0 + NS] = ai - ci;
  }
}

__global__ void __launch_bounds__(AU_THREADS) audio2mel_kernel(
    const float* __restrict__ audio, long long stride, const int* __restrict__ lens, const float* __restrict__ scale,
    const float* __restrict__ window, const float2* __restrict__ twiddle, const int* __restrict__ filt,
    const float* __restrict__ weights, int n_weights, int n_mel, float floor_, float* __restrict__ out, int Tmax,
    int layout) {
  extern __shared__ __attribute__((aligned(16))) float au_sm[];
  float* bufA = au_sm;
  float* bufB = au_sm + AU_BUF;
  float* span = bufB;  // pass 1 only
  float* mag = bufB;   // after the last pass
  float* tile = bufA;  // after the split step
  int* ftab = reinterpret_cast<int*>(au_sm + 2 * AU_BUF);  // [3 * n_mel]
  float* fw = au_sm + 2 * AU_BUF + 3 * n_mel;              // [n_weights]

  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * AU_FPW;
  const int L = lens[b];
  const int Tb = (L + 2 * AU_PAD - AU_NFFT) / AU_HOP + 1;
  const int TS = n_mel + 1;  // tile row stride

  if (t0 < Tb) {  // uniform over the workgroup
    // pass twiddles and window values of this thread's butterflies, in flight with the span
    float2 tw[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int ns = 2 << s;  // 2 .. 256
      tw[s] = twiddle[(tid & (ns - 1)) * (AU_H / ns)];
    }
    const float2 w0 = *reinterpret_cast<const float2*>(window + 2 * tid);
    const float2 w1 = *reinterpret_cast<const float2*>(window + 2 * tid + AU_H);
    for (int i = tid; i < 3 * n_mel; i += AU_THREADS) ftab[i] = filt[i];
    for (int i = tid; i < n_weights; i += AU_THREADS) fw[i] = weights[i];
    const float sc = scale ? scale[b] : 1.f;
    const float* x = audio + (long long)b * stride;
    const int g0 = t0 * AU_HOP - AU_PAD;
    for (int i = tid; i < AU_SPAN; i += AU_THREADS) {
      int g = g0 + i;
      float v = 0.f;
      if (g < L + AU_PAD) {  // past the padded signal only for frames >= Tb, which are not kept
        g = g < 0 ? -g : g;
        g = g >= L ? 2 * (L - 1) - g : g;
        v = x[g] * sc;
      }
      span[i] = v;
    }
    __syncthreads();
    // pass 1 (NS = 1, twiddle 1): z[n] = x[2n] w[2n] + i x[2n+1] w[2n+1] from the span
#pragma unroll
    for (int f = 0; f < AU_FPW; ++f) {
      const float2 a = *reinterpret_cast<const float2*>(span + f * AU_HOP + 2 * tid);
      const float2 c = *reinterpret_cast<const float2*>(span + f * AU_HOP + 2 * tid + AU_H);
      const float ar = a.x * w0.x, ai = a.y * w0.y, br = c.x * w1.x, bi = c.y * w1.y;
      float* ore = bufA + f * AU_H;
      float* oim = bufA + (AU_FPW + f) * AU_H;
      ore[2 * tid] = ar + br;
      oim[2 * tid] = ai + bi;
      ore[2 * tid + 1] = ar - br;
      oim[2 * tid + 1] = ai - bi;
    }
    __syncthreads();
    au_pass<2>(bufA, bufB, tid, tw[0]);
    __syncthreads();
    au_pass<4>(bufB, bufA, tid, tw[1]);
    __syncthreads();
    au_pass<8>(bufA, bufB, tid, tw[2]);
    __syncthreads();
    au_pass<16>(bufB, bufA, tid, tw[3]);
    __syncthreads();
    au_pass<32>(bufA, bufB, tid, tw[4]);
    __syncthreads();
    au_pass<64>(bufB, bufA, tid, tw[5]);
    __syncthreads();
    au_pass<128>(bufA, bufB, tid, tw[6]);
    __syncthreads();
    au_pass<256>(bufB, bufA, tid, tw[7]);
    __syncthreads();
    // split step: X[k] = E[k] + W^k O[k], E = (Z[k] + conj Z[512-k]) / 2, O = (Z[k] - conj Z[512-k]) / 2i
    for (int k = tid; k < AU_NB; k += AU_THREADS) {
      const float2 w = twiddle[k];
      const int k0 = k & (AU_H - 1), k1 = (AU_H - k) & (AU_H - 1);
#pragma unroll
      for (int f = 0; f < AU_FPW; ++f) {
        const float* re = bufA + f * AU_H;
        const float* im = bufA + (AU_FPW + f) * AU_H;
        const float a = re[k0], bb = im[k0], c = re[k1], d = im[k1];
        const float er = 0.5f * (a + c), ei = 0.5f * (bb - d), orr = 0.5f * (bb + d), oi = -0.5f * (a - c);
        const float xr = er + (w.x * orr - w.y * oi), xi = ei + (w.x * oi + w.y * orr);
        mag[f * AU_MS + k] = sqrtf(xr * xr + xi * xi);
      }
    }
    __syncthreads();
    // mel: lane (m, f) over filter m's support
    for (int p = tid; p < AU_FPW * n_mel; p += AU_THREADS) {
      const int f = p & (AU_FPW - 1), m = p / AU_FPW;
      const int st = ftab[3 * m], cnt = ftab[3 * m + 1], off = ftab[3 * m + 2];
      const float* mg = mag + f * AU_MS + st;
      const float* wp = fw + off;
      float acc = 0.f;
      for (int i = 0; i < cnt; ++i) acc += wp[i] * mg[i];
      tile[f * TS + m] = log10f(fmaxf(acc, floor_));
    }
  }
  __syncthreads();
  const int n = AU_FPW * n_mel;
  if (layout == AVC_MEL_FRAME_MAJOR) {
    float* dst = out + ((long long)b * Tmax + t0) * n_mel;
    for (int i = tid; i < n; i += AU_THREADS) {
      const int f = i / n_mel, m = i - f * n_mel, t = t0 + f;
      if (t < Tmax) dst[i] = t < Tb ? tile[f * TS + m] : 0.f;
    }
  } else {
    for (int i = tid; i < n; i += AU_THREADS) {
      const int f = i & (AU_FPW - 1), m = i / AU_FPW, t = t0 + f;
      if (t < Tmax) out[((long long)b * n_mel + m) * Tmax + t] = t < Tb ? tile[f * TS + m] : 0.f;
    }
  }
}

}  // namespace

extern "C" int avc_audio2mel(const float* audio, long long stride, const int* lens, const int* lens_dev,
                             const float* scale, int B, const float* window, const float* twiddle, const int* filt,
                             const int* filt_dev, const float* weights, int n_weights, int n_mel, int n_fft, int win,
                             int hop, float floor, float* out, int Tmax, int layout, void* stream) {
  AVC_CHECK_ARG(audio && lens && lens_dev && window && twiddle && filt && filt_dev && weights && out,
                "avc_audio2mel: null pointer (only scale may be null)");
  AVC_CHECK_ARG(n_fft == AU_NFFT && win == AU_NFFT && hop == AU_HOP,
                "avc_audio2mel: n_fft=%d win=%d hop=%d (only n_fft = win = 1024, hop = 256 are built)", n_fft, win,
                hop);
  AVC_CHECK_ARG(n_mel >= 1 && n_mel <= AU_MAX_MEL, "avc_audio2mel: n_mel = %d outside 1..%d", n_mel, AU_MAX_MEL);
  AVC_CHECK_ARG(layout == AVC_MEL_FRAME_MAJOR || layout == AVC_MEL_CHANNEL_MAJOR,
                "avc_audio2mel: unknown layout %d (0 frame-major, 1 channel-major)", layout);
  AVC_CHECK_ARG(B >= 1 && B <= 65535 && Tmax >= 1 && stride >= 1, "avc_audio2mel: bad shape B=%d Tmax=%d stride=%lld",
                B, Tmax, stride);
  AVC_CHECK_ARG(n_weights >= 1 && n_weights <= AVC_MEL_MAX_WEIGHTS,
                "avc_audio2mel: the compact mel basis has %d weights; at most %d fit the LDS budget (a basis with "
                "wide or dense filters is not supported)",
                n_weights, AVC_MEL_MAX_WEIGHTS);
  for (int b = 0; b < B; ++b) {
    const int L = lens[b];
    AVC_CHECK_ARG(L > AU_PAD, "avc_audio2mel: lens[%d] = %d: the reflection of %d samples needs a longer utterance", b,
                  L, AU_PAD);
    AVC_CHECK_ARG(L <= stride, "avc_audio2mel: lens[%d] = %d exceeds the row stride %lld", b, L, stride);
    const int Tb = (L + 2 * AU_PAD - AU_NFFT) / AU_HOP + 1;
    AVC_CHECK_ARG(Tb <= Tmax, "avc_audio2mel: utterance %d has %d frames, Tmax = %d", b, Tb, Tmax);
  }
  for (int m = 0; m < n_mel; ++m) {
    const int st = filt[3 * m], cnt = filt[3 * m + 1], off = filt[3 * m + 2];
    AVC_CHECK_ARG(st >= 0 && cnt >= 0 && off >= 0 && st + cnt <= AU_NB && off + cnt <= n_weights,
                  "avc_audio2mel: filter %d (start %d, count %d, offset %d) outside %d bins / %d weights", m, st, cnt,
                  off, AU_NB, n_weights);
  }
  AVC_CHECK_ARG((long long)B * Tmax * n_mel < (1ll << 31), "avc_audio2mel: more than 2^31 output elements");
  AVC_CHECK_ARG(((uintptr_t)window & 7) == 0 && ((uintptr_t)twiddle & 7) == 0,
                "avc_audio2mel: window and twiddle must be 8-byte aligned");
  const size_t lds = (size_t)(2 * AU_BUF + 3 * n_mel + n_weights) * sizeof(float);
  static bool attr = false;  // > 64 KiB of dynamic LDS must be opted into once per kernel (the largest table)
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&audio2mel_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)((2 * AU_BUF + 3 * AU_MAX_MEL + AVC_MEL_MAX_WEIGHTS) * sizeof(float)));
    attr = true;
  }
  const dim3 grid(cdiv(Tmax, AU_FPW), B);
  audio2mel_kernel<<<grid, AU_THREADS, lds, as_stream(stream)>>>(audio, stride, lens_dev, scale, window,
                                                                 reinterpret_cast<const float2*>(twiddle), filt_dev,
                                                                 weights, n_weights, n_mel, floor, out, Tmax, layout);
  return avc_check_launch("avc_audio2mel");
}
