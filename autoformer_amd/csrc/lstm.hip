// lstm.hip — LSTM recurrences (forward and backward) for the AutoVC path.
//
// Replaces the time loops inside nn.LSTM: encoder BiLSTM(512->44, 2 layers)
// (factory/AutoVC.py:43,54-55), decoder lstm1(344->512) (:77,103) and lstm2(512->1024,
// 2 layers) (:96,110).  Gate order i, f, g, o; h0 = c0 = 0; the input projection
// x W_ih^T + b_ih + b_hh is a separate GEMM over all frames (gemm.hip) and arrives here
// as `xproj`.
//
// This file: the avc_lstm_fwd / avc_lstm_bwd dispatch, the per-step kernels, and the process-wide
// host state of all LSTM files (fault word, spin bound, trace buffer, residency cache).  The
// designs, chosen by H (shared pieces in lstm_internal.h):
//  * small H (<= 64, the encoder): one workgroup owns its utterances for all T steps, no
//    inter-workgroup sync at all (lstm_small.hip).
//  * large H (multiple of 128, the decoder): one persistent launch per layer when it fits
//    (bf16, one direction, H in {512, 768, 1024}: lstm_persist.hip; the two stacked lstm2
//    layers in one launch: lstm2.hip), otherwise one fused kernel per time step (below).  Each
//    workgroup owns (16*MT utterances) x (8 hidden units, all 4 gates) [forward] or
//    (16*MT utterances) x (16 hidden units) [backward]; the recurrent product runs on
//    MFMA with K split over the 4 waves and operands loaded straight into registers;
//    the cell update is fused into the same kernel's epilogue.  Kernel boundaries are the
//    grid-wide sync (cheaper on gfx950 than a software grid barrier at 256 workgroups,
//    MI355X_MICROARCH.md rows "boundary" vs "barrier-xcd"); the host loop is
//    graph-capturable.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <mutex>

#include "lstm_internal.h"

namespace {
using namespace avcl;

// =============================================================== large H: per-step kernels
struct StepArgs {
  const float* xproj;  // (B,T,dirs*4H)
  const void* w;       // fwd: dirs x [4H][H]; bwd: dirs x [H][4H]
  float* hout;         // (B,T,dirs*H)
  float* call;         // (B,T,dirs*H)
  float* gall;         // (B,T,dirs*4H) activated gates
  void* hb;            // bf16 ping-pong [2][dirs][B][H] (fwd) / [2][dirs][B][4H] (bwd)
  const float* dhout;  // bwd
  float* dg;           // bwd (B,T,dirs*4H)
  float* dcb;          // bwd [dirs][B][H]
  int B, T, H, dirs, s;
};

template <bool BF, int MT>
__global__ void __launch_bounds__(256) lstm_step_fwd(StepArgs a) {
  const int H = a.H, G = 4 * H, T = a.T, B = a.B;
  const int d = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int j0 = blockIdx.x * 8, b0 = blockIdx.y * 16 * MT;
  const int t = d ? T - 1 - a.s : a.s;
  const int tp = d ? t + 1 : t - 1;
  const long long ldx = (long long)a.dirs * G, ldh = (long long)a.dirs * H;
  __shared__ float red[4][16 * MT][33];

  // prefetch the epilogue's inputs (independent of the GEMM)
  const int pr = tid >> 3, pj = tid & 7;
  const int pb = b0 + pr;
  const bool pv = pr < 16 * MT && pb < B;
  float px[4] = {0.f, 0.f, 0.f, 0.f}, pcp = 0.f;
  if (pv) {
    const long long ox = ((long long)pb * T + t) * ldx + d * G + j0 + pj;
#pragma unroll
    for (int q = 0; q < 4; ++q) px[q] = a.xproj[ox + q * H];
    if (a.s > 0) pcp = a.call[((long long)pb * T + tp) * ldh + d * H + j0 + pj];
  }

  f32x4 acc[MT][2];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m][0] = acc[m][1] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (a.s > 0) {
    const int kw = H / 4, kbeg = w * kw;
    const int r16 = lane & 15, kh = lane >> 4;
    if constexpr (BF) {
      const bf16* hp = reinterpret_cast<const bf16*>(a.hb) + ((long long)((a.s - 1) & 1) * a.dirs + d) * B * H;
      const bf16* W = reinterpret_cast<const bf16*>(a.w) + (long long)d * G * H;
      const bf16* arow[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        int b = b0 + m * 16 + r16;
        arow[m] = b < B ? hp + (long long)b * H : nullptr;
      }
      const bf16* brow[2];
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        int col = n * 16 + r16;
        brow[n] = W + (long long)((col >> 3) * H + j0 + (col & 7)) * H;
      }
      const bf16x8 z = {};
#pragma unroll 4
      for (int k0 = kbeg; k0 < kbeg + kw; k0 += 32) {
        const int ko = k0 + 8 * kh;
        bf16x8 af[MT], bfr[2];
#pragma unroll
        for (int m = 0; m < MT; ++m) af[m] = arow[m] ? *reinterpret_cast<const bf16x8*>(arow[m] + ko) : z;
#pragma unroll
        for (int n = 0; n < 2; ++n) bfr[n] = *reinterpret_cast<const bf16x8*>(brow[n] + ko);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[m], bfr[n], acc[m][n], 0, 0, 0);
      }
    } else {
      const float* W = reinterpret_cast<const float*>(a.w) + (long long)d * G * H;
      const float* arow[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        int b = b0 + m * 16 + r16;
        arow[m] = b < B ? a.hout + ((long long)b * T + tp) * ldh + d * H : nullptr;
      }
      const float* brow[2];
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        int col = n * 16 + r16;
        brow[n] = W + (long long)((col >> 3) * H + j0 + (col & 7)) * H;
      }
#pragma unroll 8
      for (int k0 = kbeg; k0 < kbeg + kw; k0 += 4) {
        float af[MT], bfr[2];
#pragma unroll
        for (int m = 0; m < MT; ++m) af[m] = arow[m] ? arow[m][k0 + kh] : 0.f;
#pragma unroll
        for (int n = 0; n < 2; ++n) bfr[n] = brow[n][k0 + kh];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[m], bfr[n], acc[m][n], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[w][m * 16 + 4 * (lane >> 4) + e][n * 16 + (lane & 15)] = acc[m][n][e];
  __syncthreads();
  if (pv) {
    float pre[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      pre[q] = px[q] + red[0][pr][q * 8 + pj] + red[1][pr][q * 8 + pj] + red[2][pr][q * 8 + pj] + red[3][pr][q * 8 + pj];
    const float ig = sigmoidf_(pre[0]), fg = sigmoidf_(pre[1]), gg = tanhf(pre[2]), og = sigmoidf_(pre[3]);
    const float c = fg * pcp + ig * gg;
    const float h = og * tanhf(c);
    const int j = j0 + pj;
    const long long oh = ((long long)pb * T + t) * ldh + d * H + j;
    a.hout[oh] = h;
    a.call[oh] = c;
    const long long og_ = ((long long)pb * T + t) * ldx + d * G + j;
    a.gall[og_] = ig;
    a.gall[og_ + H] = fg;
    a.gall[og_ + 2 * H] = gg;
    a.gall[og_ + 3 * H] = og;
    if constexpr (BF) {
      bf16* hn = reinterpret_cast<bf16*>(a.hb) + ((long long)(a.s & 1) * a.dirs + d) * B * H;
      hn[(long long)pb * H + j] = (bf16)h;
    }
  }
}

template <bool BF, int MT>
__global__ void __launch_bounds__(256) lstm_step_bwd(StepArgs a) {
  const int H = a.H, G = 4 * H, T = a.T, B = a.B;
  const int d = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int j0 = blockIdx.x * 16, b0 = blockIdx.y * 16 * MT;
  const int t = d ? a.s : T - 1 - a.s;
  const int tn = d ? t - 1 : t + 1;  // time handled by the previous backward step
  const int tp = d ? t + 1 : t - 1;  // forward's previous time step
  const long long ldg = (long long)a.dirs * G, ldh = (long long)a.dirs * H;
  __shared__ float red[4][16 * MT][17];
  constexpr int PPT = MT;  // (row, unit) pairs per thread: 16*MT*16 / 256

  float pdh[PPT], pc[PPT], pcp[PPT], pg[PPT][4], pdc[PPT];
  int prow[PPT], pjj[PPT];
  bool pv[PPT];
#pragma unroll
  for (int u = 0; u < PPT; ++u) {
    const int p = tid + 256 * u;
    prow[u] = p >> 4;
    pjj[u] = p & 15;
    const int b = b0 + prow[u];
    pv[u] = b < B;
    pdh[u] = pc[u] = pcp[u] = pdc[u] = 0.f;
    pg[u][0] = pg[u][1] = pg[u][2] = pg[u][3] = 0.f;
    if (pv[u]) {
      const int j = j0 + pjj[u];
      const long long oh = ((long long)b * T + t) * ldh + d * H + j;
      pdh[u] = a.dhout[oh];
      pc[u] = a.call[oh];
      if (tp >= 0 && tp < T) pcp[u] = a.call[((long long)b * T + tp) * ldh + d * H + j];
      const long long og_ = ((long long)b * T + t) * ldg + d * G + j;
#pragma unroll
      for (int q = 0; q < 4; ++q) pg[u][q] = a.gall[og_ + q * H];
      if (a.s > 0) pdc[u] = a.dcb[((long long)d * B + b) * H + j];
    }
  }

  f32x4 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (a.s > 0) {
    const int kw = G / 4, kbeg = w * kw;
    const int r16 = lane & 15, kh = lane >> 4;
    if constexpr (BF) {
      const bf16* gp = reinterpret_cast<const bf16*>(a.hb) + ((long long)((a.s - 1) & 1) * a.dirs + d) * B * G;
      const bf16* WT = reinterpret_cast<const bf16*>(a.w) + (long long)d * H * G;
      const bf16* arow[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        int b = b0 + m * 16 + r16;
        arow[m] = b < B ? gp + (long long)b * G : nullptr;
      }
      const bf16* brow = WT + (long long)(j0 + r16) * G;
      const bf16x8 z = {};
#pragma unroll 4
      for (int k0 = kbeg; k0 < kbeg + kw; k0 += 32) {
        const int ko = k0 + 8 * kh;
        bf16x8 bfr = *reinterpret_cast<const bf16x8*>(brow + ko);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          bf16x8 af = arow[m] ? *reinterpret_cast<const bf16x8*>(arow[m] + ko) : z;
          acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr, acc[m], 0, 0, 0);
        }
      }
    } else {
      const float* WT = reinterpret_cast<const float*>(a.w) + (long long)d * H * G;
      const float* arow[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        int b = b0 + m * 16 + r16;
        arow[m] = b < B ? a.dg + ((long long)b * T + tn) * ldg + d * G : nullptr;
      }
      const float* brow = WT + (long long)(j0 + r16) * G;
#pragma unroll 8
      for (int k0 = kbeg; k0 < kbeg + kw; k0 += 4) {
        float bfr = brow[k0 + kh];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          float af = arow[m] ? arow[m][k0 + kh] : 0.f;
          acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bfr, acc[m], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int e = 0; e < 4; ++e) red[w][m * 16 + 4 * (lane >> 4) + e][lane & 15] = acc[m][e];
  __syncthreads();
#pragma unroll
  for (int u = 0; u < PPT; ++u) {
    if (!pv[u]) continue;
    const int r = prow[u], jl = pjj[u], b = b0 + r, j = j0 + jl;
    const float dh = pdh[u] + red[0][r][jl] + red[1][r][jl] + red[2][r][jl] + red[3][r][jl];
    const float ig = pg[u][0], fg = pg[u][1], gg = pg[u][2], og = pg[u][3];
    const float tc = tanhf(pc[u]);
    const float do_ = dh * tc;
    const float dcs = pdc[u] + dh * og * (1.f - tc * tc);
    const float di = dcs * gg, dgg = dcs * ig, df = dcs * pcp[u];
    a.dcb[((long long)d * B + b) * H + j] = dcs * fg;
    const float v[4] = {di * ig * (1.f - ig), df * fg * (1.f - fg), dgg * (1.f - gg * gg), do_ * og * (1.f - og)};
    const long long og_ = ((long long)b * T + t) * ldg + d * G + j;
#pragma unroll
    for (int q = 0; q < 4; ++q) a.dg[og_ + q * H] = v[q];
    if constexpr (BF) {
      bf16* gn = reinterpret_cast<bf16*>(a.hb) + ((long long)(a.s & 1) * a.dirs + d) * B * G + (long long)b * G;
#pragma unroll
      for (int q = 0; q < 4; ++q) gn[q * H + j] = (bf16)v[q];
    }
  }
}


// ---------------------------------------------------------------- bf16 step kernels, H known
// Every operand fragment of a wave's K-slice is loaded before the first MFMA, so a step
// pays ONE L2/MALL round trip instead of one per k-step.
template <int H, int MT>
__global__ void __launch_bounds__(256) lstm_step_fwd_bf(StepArgs a) {
  constexpr int G = 4 * H, KW = H / 4, NK = KW / 32;
  const int T = a.T, B = a.B, d = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int j0 = blockIdx.x * 8, b0 = blockIdx.y * 16 * MT;
  const int t = d ? T - 1 - a.s : a.s;
  const int tp = d ? t + 1 : t - 1;
  const long long ldx = (long long)a.dirs * G, ldh = (long long)a.dirs * H;
  __shared__ float red[4][16 * MT][33];
  const int pr = tid >> 3, pj = tid & 7, pb = b0 + pr;
  const bool pv = pr < 16 * MT && pb < B;
  float px[4] = {0.f, 0.f, 0.f, 0.f}, pcp = 0.f;
  if (pv) {
    const long long ox = ((long long)pb * T + t) * ldx + d * G + j0 + pj;
#pragma unroll
    for (int q = 0; q < 4; ++q) px[q] = a.xproj[ox + q * H];
    if (a.s > 0) pcp = a.call[((long long)pb * T + tp) * ldh + d * H + j0 + pj];
  }
  f32x4 acc[MT][2];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m][0] = acc[m][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (a.s > 0) {
    const int r16 = lane & 15, ko = w * KW + 8 * (lane >> 4);
    const bf16* hp = reinterpret_cast<const bf16*>(a.hb) + ((long long)((a.s - 1) & 1) * a.dirs + d) * B * H;
    const bf16* W = reinterpret_cast<const bf16*>(a.w) + (long long)d * G * H;
    bf16x8 af[NK][MT], bw[NK][2];
    const bf16x8 z = {};
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int b = b0 + m * 16 + r16;
      const bf16* row = hp + (long long)(b < B ? b : 0) * H + ko;
#pragma unroll
      for (int k = 0; k < NK; ++k) af[k][m] = b < B ? *reinterpret_cast<const bf16x8*>(row + 32 * k) : z;
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int col = n * 16 + r16;
      const bf16* row = W + (long long)((col >> 3) * H + j0 + (col & 7)) * H + ko;
#pragma unroll
      for (int k = 0; k < NK; ++k) bw[k][n] = *reinterpret_cast<const bf16x8*>(row + 32 * k);
    }
#pragma unroll
    for (int k = 0; k < NK; ++k)
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[k][m], bw[k][n], acc[m][n], 0, 0, 0);
  }
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[w][m * 16 + 4 * (lane >> 4) + e][n * 16 + (lane & 15)] = acc[m][n][e];
  __syncthreads();
  if (pv) {
    float pre[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      pre[q] = px[q] + red[0][pr][q * 8 + pj] + red[1][pr][q * 8 + pj] + red[2][pr][q * 8 + pj] + red[3][pr][q * 8 + pj];
    const float ig = sigmoidf_(pre[0]), fg = sigmoidf_(pre[1]), gg = tanhf(pre[2]), og = sigmoidf_(pre[3]);
    const float c = fg * pcp + ig * gg;
    const float h = og * tanhf(c);
    const int j = j0 + pj;
    const long long oh = ((long long)pb * T + t) * ldh + d * H + j;
    a.hout[oh] = h;
    a.call[oh] = c;
    const long long og_ = ((long long)pb * T + t) * ldx + d * G + j;
    a.gall[og_] = ig;
    a.gall[og_ + H] = fg;
    a.gall[og_ + 2 * H] = gg;
    a.gall[og_ + 3 * H] = og;
    bf16* hn = reinterpret_cast<bf16*>(a.hb) + ((long long)(a.s & 1) * a.dirs + d) * B * H;
    hn[(long long)pb * H + j] = (bf16)h;
  }
}

// backward: 8 waves split K = 4H; tile 16 utterances x 16 hidden units.
template <int H>
__global__ void __launch_bounds__(512) lstm_step_bwd_bf(StepArgs a) {
  constexpr int G = 4 * H, KW = G / 8, NK = KW / 32;
  const int T = a.T, B = a.B, d = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int j0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
  const int t = d ? a.s : T - 1 - a.s;
  const int tp = d ? t + 1 : t - 1;
  const long long ldg = (long long)a.dirs * G, ldh = (long long)a.dirs * H;
  __shared__ float red[8][16][17];
  const int prow = tid >> 4, pjj = tid & 15, pb = b0 + prow;
  const bool pv = tid < 256 && pb < B;
  float pdh = 0.f, pc = 0.f, pcp = 0.f, pdc = 0.f, pg[4] = {0.f, 0.f, 0.f, 0.f};
  if (pv) {
    const int j = j0 + pjj;
    const long long oh = ((long long)pb * T + t) * ldh + d * H + j;
    pdh = a.dhout[oh];
    pc = a.call[oh];
    if (tp >= 0 && tp < T) pcp = a.call[((long long)pb * T + tp) * ldh + d * H + j];
    const long long og_ = ((long long)pb * T + t) * ldg + d * G + j;
#pragma unroll
    for (int q = 0; q < 4; ++q) pg[q] = a.gall[og_ + q * H];
    if (a.s > 0) pdc = a.dcb[((long long)d * B + pb) * H + j];
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (a.s > 0) {
    const int r16 = lane & 15, ko = w * KW + 8 * (lane >> 4);
    const bf16* gp = reinterpret_cast<const bf16*>(a.hb) + ((long long)((a.s - 1) & 1) * a.dirs + d) * B * G;
    const bf16* WT = reinterpret_cast<const bf16*>(a.w) + (long long)d * H * G;
    const int b = b0 + r16;
    const bf16* arow = gp + (long long)(b < B ? b : 0) * G + ko;
    const bf16* brow = WT + (long long)(j0 + r16) * G + ko;
    bf16x8 af[NK], bw[NK];
    const bf16x8 z = {};
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      af[k] = b < B ? *reinterpret_cast<const bf16x8*>(arow + 32 * k) : z;
      bw[k] = *reinterpret_cast<const bf16x8*>(brow + 32 * k);
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[k], bw[k], acc, 0, 0, 0);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[w][4 * (lane >> 4) + e][lane & 15] = acc[e];
  __syncthreads();
  if (pv) {
    const int j = j0 + pjj;
    float dh = pdh;
#pragma unroll
    for (int ww = 0; ww < 8; ++ww) dh += red[ww][prow][pjj];
    const float ig = pg[0], fg = pg[1], gg = pg[2], og = pg[3];
    const float tc = tanhf(pc);
    const float do_ = dh * tc;
    const float dcs = pdc + dh * og * (1.f - tc * tc);
    const float di = dcs * gg, dgg = dcs * ig, df = dcs * pcp;
    a.dcb[((long long)d * B + pb) * H + j] = dcs * fg;
    const float v[4] = {di * ig * (1.f - ig), df * fg * (1.f - fg), dgg * (1.f - gg * gg), do_ * og * (1.f - og)};
    const long long og_ = ((long long)pb * T + t) * ldg + d * G + j;
    bf16* gn = reinterpret_cast<bf16*>(a.hb) + ((long long)(a.s & 1) * a.dirs + d) * B * G + (long long)pb * G;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      a.dg[og_ + q * H] = v[q];
      gn[q * H + j] = (bf16)v[q];
    }
  }
}

// ---------------------------------------------------------------- host-side launch state
// (process-wide; declared in lstm_internal.h for the other LSTM files)
std::atomic<unsigned*> g_fault[MAXDEV];         // per-device fault word (avc_set_fault_word)
std::atomic<unsigned> g_spin{0};                // 0 = PSPIN (or AVC_LSTM_SPIN)
std::atomic<unsigned long long*> g_trace{nullptr};  // avc_lstm_trace

}  // namespace

int avcl::num_cus() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAXDEV) return 0;
  static std::once_flag once[MAXDEV];
  static int cus[MAXDEV];
  std::call_once(once[dev], [dev] {
    hipDeviceProp_t prop;
    cus[dev] = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 0;
  });
  return cus[dev];
}

unsigned* avcl::fault_word() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAXDEV) return nullptr;
  return g_fault[dev].load(std::memory_order_acquire);
}

unsigned long long* avcl::trace_ptr() { return g_trace.load(std::memory_order_relaxed); }

unsigned avcl::spin_bound() {
  static const unsigned env = [] {
    const char* v = getenv("AVC_LSTM_SPIN");
    return v ? (unsigned)strtoul(v, nullptr, 10) : 0u;
  }();
  const unsigned s = g_spin.load(std::memory_order_relaxed);
  if (s == ~0u) return 0;  // injected timeout: every wait fails at once (fault-path tests)
  return s ? s : env ? env : PSPIN;
}

bool avcl::fits_resident(const void* fn, int threads, size_t lds, int grid) {
  static std::mutex mu;
  struct Entry {
    const void* fn;
    int dev;
    int blocks;
  };
  static Entry cache[64];
  static int n = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  int blocks = -1;
  {
    std::lock_guard<std::mutex> g(mu);
    for (int i = 0; i < n; ++i)
      if (cache[i].fn == fn && cache[i].dev == dev) blocks = cache[i].blocks;
    if (blocks < 0) {
      int nb = 0;
      if (lds) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, threads, lds) != hipSuccess) nb = 0;
      (void)hipGetLastError();
      blocks = nb;
      if (n < 64) cache[n++] = Entry{fn, dev, nb};
    }
  }
  return (long long)blocks * num_cus() >= grid;
}

bool avcl::no_persist_env() {
  static const bool v = getenv("AVC_LSTM_NO_PERSIST") != nullptr;
  return v;
}

unsigned* avc_fault_ptr() { return fault_word(); }

extern "C" int avc_lstm_trace(void* buf) {
  g_trace.store(reinterpret_cast<unsigned long long*>(buf), std::memory_order_relaxed);
  return 0;
}

extern "C" int avc_set_fault_word(void* word) {
  int dev = 0;
  AVC_CHECK_ARG(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < MAXDEV, "avc_set_fault_word: no device");
  g_fault[dev].store(reinterpret_cast<unsigned*>(word), std::memory_order_release);
  return 0;
}

extern "C" int avc_lstm_set_spin(unsigned spins) {
  g_spin.store(spins, std::memory_order_relaxed);
  return 0;
}

extern "C" size_t avc_lstm_bwd_scratch_bytes(int B, int H, int dirs) {
  if (B <= 0 || H <= 0 || dirs <= 0) return 0;
  // per-step ping-pong (16 dirs B H), or the persistent backward's control words + its [2][B][4H]
  // bf16 payload (16 B H; sized 32 B H, twice that, since the retired granule form of the payload)
  return std::max((size_t)16 * dirs * B * H, (size_t)32 * B * H + 8192);
}

extern "C" int avc_lstm_fwd(const float* xproj, const void* w_hh, int wdtype, int B, int T, int H, int dirs, float* h,
                            void* h_bf16, float* c, float* gates, void* hbuf, int compute, void* stream) {
  AVC_CHECK_ARG(xproj && w_hh && h && c && gates && B > 0 && T > 0 && H > 0 && (dirs == 1 || dirs == 2),
                "avc_lstm_fwd: bad args");
  hipStream_t s = as_stream(stream);
  if (H <= 64) {
    AVC_CHECK_ARG(wdtype == AVC_F32, "avc_lstm_fwd: small-H path takes fp32 W_hh");
    // fp32 weights and state either way; fast activations in bf16 mode
    return small_fwd(xproj, (const float*)w_hh, B, T, H, dirs, h, reinterpret_cast<bf16*>(h_bf16), c, gates,
                     compute == AVC_BF16, s);
  }
  AVC_CHECK_ARG(H % 128 == 0, "avc_lstm_fwd: H must be <= 64 or a multiple of 128 (got %d)", H);
  const bool bf = compute == AVC_BF16;
  AVC_CHECK_ARG(!bf || (wdtype == AVC_BF16 && hbuf), "avc_lstm_fwd: bf16 compute needs bf16 W_hh and hbuf");
  AVC_CHECK_ARG(bf || wdtype == AVC_F32, "avc_lstm_fwd: fp32 compute needs fp32 W_hh");
  StepArgs a = {};
  a.xproj = xproj;
  a.w = w_hh;
  a.hout = h;
  a.call = c;
  a.gall = gates;
  a.hb = hbuf;
  a.B = B;
  a.T = T;
  a.H = H;
  a.dirs = dirs;
  if (hbuf && persistent_path(B, H, dirs, bf, false))
    return persist_fwd(xproj, 1, w_hh, B, T, H, h, h_bf16, c, gates, hbuf, s, "avc_lstm_fwd(persistent)");
  AVC_CHECK_ARG(h_bf16 == nullptr, "avc_lstm_fwd: the bf16 h copy is produced by the persistent path only");
  const int mt = (H >= 1024 && B > 16) ? 2 : 1;  // 256 workgroups at B = 64
  dim3 g(H / 8, cdiv(B, 16 * mt), dirs);
  for (int st = 0; st < T; ++st) {
    a.s = st;
    if (bf && H == 1024) {
      if (mt == 2) lstm_step_fwd_bf<1024, 2><<<g, 256, 0, s>>>(a);
      else lstm_step_fwd_bf<1024, 1><<<g, 256, 0, s>>>(a);
    } else if (bf && H == 512) {
      if (mt == 2) lstm_step_fwd_bf<512, 2><<<g, 256, 0, s>>>(a);
      else lstm_step_fwd_bf<512, 1><<<g, 256, 0, s>>>(a);
    } else if (bf) {
      if (mt == 2) lstm_step_fwd<true, 2><<<g, 256, 0, s>>>(a);
      else lstm_step_fwd<true, 1><<<g, 256, 0, s>>>(a);
    } else {
      if (mt == 2) lstm_step_fwd<false, 2><<<g, 256, 0, s>>>(a);
      else lstm_step_fwd<false, 1><<<g, 256, 0, s>>>(a);
    }
  }
  return avc_check_launch("avc_lstm_fwd");
}

extern "C" int avc_lstm_bwd(const float* dh_out, const float* h, const float* c, const float* gates, const void* w_hh,
                            const void* w_hh_t, int wdtype, int B, int T, int H, int dirs, float* dgates,
                            void* dgates_bf16, float* dcbuf, void* gbuf, int compute, void* stream) {
  (void)h;
  AVC_CHECK_ARG(dh_out && c && gates && dgates && B > 0 && T > 0 && H > 0 && (dirs == 1 || dirs == 2),
                "avc_lstm_bwd: bad args");
  hipStream_t s = as_stream(stream);
  if (H <= 64) {
    AVC_CHECK_ARG(w_hh && wdtype == AVC_F32, "avc_lstm_bwd: small-H path takes fp32 W_hh");
    return small_bwd(dh_out, c, gates, (const float*)w_hh, B, T, H, dirs, dgates, reinterpret_cast<bf16*>(dgates_bf16),
                     compute == AVC_BF16, s);
  }
  AVC_CHECK_ARG(H % 128 == 0, "avc_lstm_bwd: H must be <= 64 or a multiple of 128 (got %d)", H);
  AVC_CHECK_ARG(w_hh_t && dcbuf, "avc_lstm_bwd: large-H path needs W_hh^T and dcbuf");
  const bool bf = compute == AVC_BF16;
  AVC_CHECK_ARG(!bf || (wdtype == AVC_BF16 && gbuf), "avc_lstm_bwd: bf16 compute needs bf16 W_hh^T and gbuf");
  if (persistent_path(B, H, dirs, bf, true))
    return persist_bwd(dh_out, c, gates, w_hh_t, B, T, H, dgates, dgates_bf16, nullptr, nullptr, 1, gbuf, s,
                       "avc_lstm_bwd(persistent)");
  AVC_CHECK_ARG(dgates_bf16 == nullptr, "avc_lstm_bwd: the bf16 dG twin is produced by the persistent path only");
  StepArgs a = {};
  a.w = w_hh_t;
  a.call = const_cast<float*>(c);
  a.gall = const_cast<float*>(gates);
  a.hb = gbuf;
  a.dhout = dh_out;
  a.dg = dgates;
  a.dcb = dcbuf;
  a.B = B;
  a.T = T;
  a.H = H;
  a.dirs = dirs;
  dim3 g(H / 16, cdiv(B, 16), dirs);
  for (int st = 0; st < T; ++st) {
    a.s = st;
    if (bf && H == 1024) lstm_step_bwd_bf<1024><<<g, 512, 0, s>>>(a);
    else if (bf && H == 512) lstm_step_bwd_bf<512><<<g, 512, 0, s>>>(a);
    else if (bf) lstm_step_bwd<true, 1><<<g, 256, 0, s>>>(a);
    else lstm_step_bwd<false, 1><<<g, 256, 0, s>>>(a);
  }
  return avc_check_launch("avc_lstm_bwd");
}
