// lstm_small.hip — the small-H LSTM recurrences (H <= 64: the encoder BiLSTM(512->44, 2 layers),
// factory/AutoVC.py:43,54-55).  Batch rows are independent in the recurrence, so a workgroup owns
// its utterances for all T steps and there is no inter-workgroup sync at all: W_hh in registers,
// h / gates in LDS.  The packed-FMA form is the default, the MFMA form selectable; avc_lstm_fwd /
// avc_lstm_bwd (lstm.hip) reach both through small_fwd / small_bwd.
#include <atomic>
#include <cstdlib>

#include "lstm_internal.h"

namespace {
using namespace avcl;

// =============================================================== packed FMA
// (quad_bcast, f32x2 and dot_regs are in lstm_internal.h: ragged.hip's forward-only BiLSTM shares them)
// sum over the lane quad (xor 1, then xor 2, as quad_perm)
__device__ __forceinline__ float quad_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false));
  return v;
}

// One workgroup = one (utterance, direction) for all T steps: 4 COMPUTE waves + 1 FLUSH wave.
// Compute lane (j, q) = (tid >> 2, tid & 3) owns gate q of hidden unit j.  Per step it
//  * takes its step inputs from a register ring it keeps SD steps ahead with its own global loads
//    (one x-projection element forward; dh, c, c_prev and the unit's four gates backward) -- the
//    loads are unconditional (clamped addresses), so the compiler's vmcnt bookkeeping waits only
//    for the slot being consumed, never for the loads still in flight;
//  * issues ALL its LDS reads of h_{s-1} / dG_{s-1} before the first FMA (one LDS latency per
//    step, not one per 4-wide slice) and runs the product as packed fp32 FMAs (v_pk_fma_f32);
//  * combines the quad's gates with DPP and writes its outputs into an LDS chunk buffer.
// The compute waves issue no stores at all: the flush wave writes each finished chunk of SC steps
// to HBM (fp32, plus an optional bf16 twin for the next GEMMs) while the next chunk runs, so no
// compute wave ever waits on a store.  One workgroup barrier per step orders everything.
constexpr int SNT = 320;  // 4 compute waves + 1 flush wave
constexpr int SD = 4;     // input lead, steps
constexpr int SC = 16;    // output chunk, steps

constexpr int OOB = 0x7FFFFFF0;  // buffer offset past every buffer here: the store is dropped

// sum_k w[k] * v[k] over HM/4 float4 LDS slices of v; every slice is read before the first FMA
template <int HM>
__device__ __forceinline__ float dot_lds(const float* __restrict__ v, const f32x2 (&w)[HM / 2]) {
  const f32x4* v4 = reinterpret_cast<const f32x4*>(v);
  f32x4 hv[HM / 4];
#pragma unroll
  for (int k = 0; k < HM / 4; ++k) hv[k] = v4[k];
  // four independent accumulation chains, so no packed FMA waits on its predecessor's result
  f32x2 a[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
  for (int k = 0; k < HM / 4; ++k) {
    a[(2 * k) & 3] = __builtin_elementwise_fma(f32x2{hv[k][0], hv[k][1]}, w[2 * k], a[(2 * k) & 3]);
    a[(2 * k + 1) & 3] = __builtin_elementwise_fma(f32x2{hv[k][2], hv[k][3]}, w[2 * k + 1], a[(2 * k + 1) & 3]);
  }
  const f32x2 t = (a[0] + a[1]) + (a[2] + a[3]);
  return t[0] + t[1];
}

// Forward.  T is padded to a multiple of SC with ghost steps that are never written out.
template <int HM, bool FAST, bool TRACE>
__global__ void __launch_bounds__(SNT) lstm_small_fwd(const float* __restrict__ xproj, const float* __restrict__ whh,
                                                      int T, int H, int dirs, float* __restrict__ hout,
                                                      bf16* __restrict__ hout16, float* __restrict__ cout,
                                                      float* __restrict__ gout, unsigned long long* tr) {
  constexpr int GM = 4 * HM;
  const int b = blockIdx.x, d = blockIdx.y, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int G = 4 * H;
  __shared__ __attribute__((aligned(16))) float hs[2][HM];
  __shared__ __attribute__((aligned(16))) float gst[2][SC][GM];  // output chunks
  __shared__ __attribute__((aligned(16))) float hst[2][SC][HM], cst[2][SC][HM];
  const long long ldx = (long long)dirs * G, ldh = (long long)dirs * H;
  const int t0 = d ? T - 1 : 0, dt = d ? -1 : 1;
  const int Tp = (T + SC - 1) / SC * SC;

  const int j = tid >> 2, q = tid & 3, row = q * H + j;
  const bool act = w < 4 && j < H;
  f32x2 wv[HM / 2];
  float c = 0.f, ring[SD];
  // this lane's x-projection element of step sn (clamped: the surplus lanes / steps load a valid
  // element that is never used)
  const float* xl = xproj + (long long)b * T * ldx + d * G + min(row, G - 1);
  auto xload = [&](int sn) { return xl[(long long)(t0 + dt * min(sn, T - 1)) * ldx]; };
  // flush chunk k (steps k*SC .. k*SC+SC-1) from buffer k & 1 (flush wave): fully unrolled,
  // branch-free buffer stores (gates as 16-B chunks)
  const __amdgpu_buffer_rsrc_t gr = brsrc_opt(gout, (long long)gridDim.x * T * ldx * 4);
  const __amdgpu_buffer_rsrc_t hr = brsrc_opt(hout, (long long)gridDim.x * T * ldh * 4);
  const __amdgpu_buffer_rsrc_t cr = brsrc_opt(cout, (long long)gridDim.x * T * ldh * 4);
  const __amdgpu_buffer_rsrc_t h16r = brsrc_opt(hout16, (long long)gridDim.x * T * ldh * 2);
  auto flush = [&](int k) {
    const int kb = k & 1;
#pragma unroll
    for (int it = 0; it < SC * GM / 4 / 64; ++it) {
      const int idx = it * 64 + lane, i = idx / (GM / 4), c4 = idx % (GM / 4), st = k * SC + i;
      const bool ok = 4 * c4 < G && st < T;
      const long long o = ((long long)b * T + t0 + dt * st) * ldx + d * G + 4 * c4;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, *reinterpret_cast<const f32x4*>(&gst[kb][i][4 * c4])),
                                             gr, ok ? (int)(o * 4) : OOB, 0, 0);
    }
    if (H % 4 == 0) {  // h, c as 16-B chunks, the bf16 h twin as 8-B chunks
#pragma unroll
      for (int it = 0; it < (SC * HM / 4 + 63) / 64; ++it) {
        const int idx = it * 64 + lane, i = min(idx / (HM / 4), SC - 1), u4 = idx % (HM / 4), st = k * SC + i;
        const bool ok = idx < SC * HM / 4 && 4 * u4 < H && st < T;
        const long long o = ((long long)b * T + t0 + dt * st) * ldh + d * H + 4 * u4;
        const f32x4 hv = *reinterpret_cast<const f32x4*>(&hst[kb][i][4 * u4]);
        const f32x4 cv = *reinterpret_cast<const f32x4*>(&cst[kb][i][4 * u4]);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, hv), hr, ok ? (int)(o * 4) : OOB, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, cv), cr, ok ? (int)(o * 4) : OOB, 0, 0);
        const bf16x4 h16 = {(bf16)hv[0], (bf16)hv[1], (bf16)hv[2], (bf16)hv[3]};
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_t, h16), h16r, ok ? (int)(o * 2) : OOB, 0, 0);
      }
    } else {
#pragma unroll
      for (int it = 0; it < SC * HM / 64; ++it) {
        const int idx = it * 64 + lane, i = idx / HM, u = idx % HM, st = k * SC + i;
        const bool ok = u < H && st < T;
        const long long o = ((long long)b * T + t0 + dt * st) * ldh + d * H + u;
        const float hv = hst[kb][i][u], cv = cst[kb][i][u];
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, hv), hr, ok ? (int)(o * 4) : OOB, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, cv), cr, ok ? (int)(o * 4) : OOB, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, (bf16)hv), h16r,
                                              ok ? (int)(o * 2) : OOB, 0, 0);
      }
    }
  };
  if (w < 4) {
    const float* W = whh + (long long)d * G * H + (long long)min(row, G - 1) * H;
#pragma unroll
    for (int k = 0; k < HM / 2; ++k)
      wv[k] = f32x2{(act && 2 * k < H) ? W[2 * k] : 0.f, (act && 2 * k + 1 < H) ? W[2 * k + 1] : 0.f};
    if (tid < 2 * HM) hs[tid / HM][tid % HM] = 0.f;
  }
#pragma unroll
  for (int r = 0; r < SD; ++r) ring[r] = xload(r);
  __syncthreads();

  // the chunk-buffer writes of step s (gates, h, c for the flush wave) are issued during step s + 1, after
  // that step's h reads: the barrier's LDS wait then covers the h_{s+1} write alone, and the deferred writes
  // complete under the next step's FMAs.  The flush of chunk k - 1 moves one step later accordingly.
  float pgv = 0.f, phv = 0.f, pcv = 0.f;
  for (int k = 0; k * SC < Tp; ++k) {
#pragma unroll
    for (int i = 0; i < SC; ++i) {
      const int s = k * SC + i;
      if (w == 4 && k > 0 && i == 1) flush(k - 1);
      // the ring advances in every wave (the flush wave's loads are harmless and unused): a ring
      // slot written only inside the role branch would need a copy at the branch join, and that
      // copy waits for the load just issued
      const float xv = ring[i % SD];
      ring[i % SD] = xload(s + SD);
      if (TRACE && w == 0) sstamp(tr, Tp, s, 0, 0.f);
      if (w < 4) {
        f32x4 hv[HM / 4];
        {
          const f32x4* v4 = reinterpret_cast<const f32x4*>(hs[s & 1]);
#pragma unroll
          for (int kk = 0; kk < HM / 4; ++kk) hv[kk] = v4[kk];
        }
        __builtin_amdgcn_sched_barrier(0);
        if (s > 0 && act) {  // step s - 1's chunk entries (buffer / row of that step)
          const int pb = i > 0 ? (k & 1) : ((k - 1) & 1), pi = i > 0 ? i - 1 : SC - 1;
          gst[pb][pi][row] = pgv;
          if (q == 0) hst[pb][pi][j] = phv;
          else if (q == 1) cst[pb][pi][j] = pcv;
        }
        __builtin_amdgcn_sched_barrier(0);
        const float pre = (act ? xv : 0.f) + dot_regs<HM>(hv, wv);
        if (TRACE && w == 0) sstamp(tr, Tp, s, 1, pre);
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
        if (TRACE && w == 0) sstamp(tr, Tp, s, 2, h);
        if (act && q == 0) hs[(s + 1) & 1][j] = h;
        pgv = gv;
        phv = h;
        pcv = c;
      }
      if (TRACE && w < 4) sstamp(tr, Tp, s, w == 0 ? 3 : 4 + w, 0.f);
      __syncthreads();
    }
  }
  if (w < 4 && act) {  // the last step's chunk entries
    gst[(Tp / SC - 1) & 1][SC - 1][row] = pgv;
    if (q == 0) hst[(Tp / SC - 1) & 1][SC - 1][j] = phv;
    else if (q == 1) cst[(Tp / SC - 1) & 1][SC - 1][j] = pcv;
  }
  __syncthreads();
  if (w == 4) flush(Tp / SC - 1);
}

// Backward: compute lane (j, q) holds column j of gate block q (wc[g] = W[q*H + g][j]) and sums
// dG_{s-1}[q*H + g] * wc[g] over g; the quad's four partial sums (DPP xor steps) give dh_rec[j].
// Its ring holds dh, c, c_prev and the four gates of unit j for the next SD steps.
template <int HM, bool FAST, bool TRACE>
__global__ void __launch_bounds__(SNT) lstm_small_bwd(const float* __restrict__ dhout, const float* __restrict__ call,
                                                      const float* __restrict__ gall, const float* __restrict__ whh,
                                                      int T, int H, int dirs, float* __restrict__ dg,
                                                      bf16* __restrict__ dg16, unsigned long long* tr) {
  constexpr int GM = 4 * HM;
  const int b = blockIdx.x, d = blockIdx.y, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int G = 4 * H;
  __shared__ __attribute__((aligned(16))) float dgs[2][GM];  // dG of a step, block q at q*HM
  __shared__ __attribute__((aligned(16))) float ost[2][SC][GM];  // output chunks (block q at q*H)
  const long long ldg = (long long)dirs * G, ldh = (long long)dirs * H;
  // backward walks opposite to the forward recurrence
  const int t0 = d ? 0 : T - 1, dt = d ? 1 : -1;
  const int fwd_prev = d ? 1 : -1;  // offset of the forward's previous time step
  const int Tp = (T + SC - 1) / SC * SC;

  const int j = tid >> 2, q = tid & 3, jc = min(j, H - 1);
  const bool act = w < 4 && j < H;
  f32x2 wc[HM / 2];
  float dc = 0.f;
  struct In {
    float dh, c, cp, i, f, g, o;
  };
  In ring[SD];
  const float* dhb = dhout + (long long)b * T * ldh + d * H + jc;
  const float* cb = call + (long long)b * T * ldh + d * H + jc;
  const float* gb = gall + (long long)b * T * ldg + d * G + jc;
  auto fetch = [&](int sn) {  // unconditional loads; c_prev past the sequence start is zeroed at use
    const int t = t0 + dt * min(sn, T - 1), tp = min(max(t + fwd_prev, 0), T - 1);
    In v;
    v.dh = dhb[(long long)t * ldh];
    v.c = cb[(long long)t * ldh];
    v.cp = cb[(long long)tp * ldh];
    const float* g = gb + (long long)t * ldg;
    v.i = g[0];
    v.f = g[H];
    v.g = g[2 * H];
    v.o = g[3 * H];
    return v;
  };
  const __amdgpu_buffer_rsrc_t dgr = brsrc_opt(dg, (long long)gridDim.x * T * ldg * 4);
  const __amdgpu_buffer_rsrc_t dg16r = brsrc_opt(dg16, (long long)gridDim.x * T * ldg * 2);
  auto flush = [&](int k) {  // fully unrolled, branch-free buffer stores (see the forward)
    const int kb = k & 1;
#pragma unroll
    for (int it = 0; it < SC * GM / 4 / 64; ++it) {
      const int idx = it * 64 + lane, i = idx / (GM / 4), c4 = idx % (GM / 4), st = k * SC + i;
      const bool ok = 4 * c4 < G && st < T;
      const long long o = ((long long)b * T + t0 + dt * st) * ldg + d * G + 4 * c4;
      const f32x4 v = *reinterpret_cast<const f32x4*>(&ost[kb][i][4 * c4]);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), dgr, ok ? (int)(o * 4) : OOB, 0, 0);
      const bf16x4 v16 = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_t, v16), dg16r, ok ? (int)(o * 2) : OOB, 0, 0);
    }
  };
  if (w < 4) {
    const float* W = whh + (long long)d * G * H;
#pragma unroll
    for (int k = 0; k < HM / 2; ++k)
      wc[k] = f32x2{(act && 2 * k < H) ? W[(long long)(q * H + 2 * k) * H + j] : 0.f,
                    (act && 2 * k + 1 < H) ? W[(long long)(q * H + 2 * k + 1) * H + j] : 0.f};
    for (int i = tid; i < 2 * GM; i += 256) dgs[i / GM][i % GM] = 0.f;
  }
#pragma unroll
  for (int r = 0; r < SD; ++r) ring[r] = fetch(r);
  __syncthreads();

  for (int k = 0; k * SC < Tp; ++k) {
    if (w == 4 && k > 0) flush(k - 1);
#pragma unroll
    for (int i = 0; i < SC; ++i) {
      const int s = k * SC + i;
      const In in = ring[i % SD];  // advanced in every wave (see the forward)
      ring[i % SD] = fetch(s + SD);
      if (TRACE && (w == 0 || w == 4)) sstamp(tr, Tp, s, w == 0 ? 0 : 4, 0.f);
      if (w < 4) {
        // recurrent part dh_rec[j] = sum_{q', g} dG_{s-1}[q'*H + g] W[q'*H + g][j]: this lane sums
        // gate block q (entries past H meet zero weights), the quad adds the four blocks
        const float p = dot_lds<HM>(dgs[(s + 1) & 1] + q * HM, wc);
        const float dh = (act ? in.dh : 0.f) + quad_sum(p);
        if (TRACE && w == 0) sstamp(tr, Tp, s, 1, dh);
        if (act) {
          const float cp = s == T - 1 ? 0.f : in.cp;  // the forward's c_{-1} = 0
          const float tc = act_tanh<FAST>(in.c);
          const float dcs = dc + dh * in.o * (1.f - tc * tc);
          const float v = q == 0 ? dcs * in.g * in.i * (1.f - in.i)
                        : q == 1 ? dcs * cp * in.f * (1.f - in.f)
                        : q == 2 ? dcs * in.i * (1.f - in.g * in.g)
                                 : dh * tc * in.o * (1.f - in.o);
          dc = dcs * in.f;
          dgs[s & 1][q * HM + j] = v;  // gate blocks HM apart: 16-B aligned slices, zero tails
          ost[k & 1][i][q * H + j] = v;
        }
        if (TRACE && w == 0) sstamp(tr, Tp, s, 2, dc);
      }
      if (TRACE && (w == 0 || w == 4)) sstamp(tr, Tp, s, w == 0 ? 3 : 5, 0.f);
      __syncthreads();
    }
  }
  if (w == 4) flush(Tp / SC - 1);
}

// =============================================================== small H on MFMA (bf16 compute)
// The encoder BiLSTM (H = 44, AutoVC.py:43,54-55) with its recurrent product on the 4x4x4 bf16
// MFMA (v_mfma_f32_4x4x4_16b_bf16: 16 independent 4x4 blocks per instruction, K = 4 each).  One
// workgroup = 4 utterances (the 4 columns of every block) x one direction; lane l of a wave is
// block l >> 2, column l & 3 (tools/probes/mfma4x4_probe.hip verified the lane map on gfx950:
// A row i / B column j / D column j of block b in lane 4b + i / 4b + j / 4b + j, D row i in
// accumulator register i; 12.7 cycles per dependent MFMA, 8.5 independent).
//
// Forward: block b of compute wave w is hidden unit u = 16w + b and its 4 ROWS are that unit's
// gates i, f, g, o (A = W_hh rows, bf16, in VGPRs for the whole sequence); the B operand is
// h_{s-1} of the block's 4 utterances (bf16, LDS, the same 8 bytes for all 16 blocks).  After
// H/4 MFMAs lane (b, j) holds the four pre-activation gates of cell (u, utterance j) in its four
// accumulator registers: the cell update is lane-local (no DPP, no LDS between the product and
// the cell), one cell per lane, 3 waves for H = 44, and each lane stores its own outputs.
// Backward: dh_rec[u] = sum_r dG[r] W[r][u] over the 4H gate rows r.  Block b = (unit quad ug,
// gate block kq) = (b & 3, b >> 2): its 4 rows are units 16w + 4ug + i, its K runs over gate block
// kq's H rows, so the four blocks kq of a unit quad hold partial sums that two lane exchanges
// (xor 32, xor 16) reduce, each lane keeping the sum of register kq: cell (16w + 4ug + kq, j).
//
// Measured against the packed-FMA kernels above (profiles/r6_bilstm_mfma_ab.txt, B=64, T=128):
// forward 0.585 vs 0.457 us per step, backward 0.727 vs 0.504.  The product is no shorter than the
// FMA dot (0.20 us: LDS read + 11 chained MFMAs), and a lane now activates four gates and tanh(c)
// instead of one gate + tanh(c) (cell 0.22 vs 0.085 us): 64 cells per wave is 4x the
// transcendental work per lane of the one-utterance-per-workgroup form.  Off by default
// (avc_lstm_set_small_mfma / AVC_BILSTM_MFMA=1 select it).
typedef short s16x4 __attribute__((ext_vector_type(4)));
constexpr int MU = 4;   // utterances per workgroup (block columns)
constexpr int MSD = 8;  // input lead, steps (register ring)

__device__ __forceinline__ f32x4 mfma4(s16x4 a, s16x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ s16x4 bf4(float a, float b, float c, float d) {
  return __builtin_bit_cast(s16x4, bf16x4{(bf16)a, (bf16)b, (bf16)c, (bf16)d});
}

// Forward.  KC = H / 4 K-chunks, NW = ceil(H / 16) waves.
template <int KC, int NW, bool TRACE>
__global__ void __launch_bounds__(NW * 64) lstm_mfma_fwd(const float* __restrict__ xproj, const float* __restrict__ whh,
                                                         int B, int T, int dirs, float* __restrict__ hout,
                                                         bf16* __restrict__ hout16, float* __restrict__ cout,
                                                         float* __restrict__ gout, unsigned long long* tr) {
  constexpr int H = 4 * KC, G = 4 * H;
  const int d = blockIdx.y, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int b0 = blockIdx.x * MU;
  __shared__ __attribute__((aligned(16))) bf16 hs[2][MU][H];  // h_{s-1}, the B operand
  const long long ldx = (long long)dirs * G, ldh = (long long)dirs * H;
  const int t0 = d ? T - 1 : 0, dt = d ? -1 : 1;
  const int nu = min(MU, B - b0);  // utterances of this workgroup

  const int j = lane & 3, u = 16 * w + (lane >> 2);
  const bool cell = u < H && j < nu;
  const int bi = b0 + min(j, nu - 1), uc = min(u, H - 1);
  s16x4 wa[KC];
  {  // A: row (lane & 3) = gate of block (lane >> 2) = unit u
    const float* W = whh + (long long)d * G * H + (long long)((lane & 3) * H + uc) * H;
#pragma unroll
    for (int c = 0; c < KC; ++c)
      wa[c] = u < H ? bf4(W[4 * c], W[4 * c + 1], W[4 * c + 2], W[4 * c + 3]) : s16x4{0, 0, 0, 0};
  }
  for (int i = tid; i < 2 * MU * H; i += blockDim.x) (&hs[0][0][0])[i] = (bf16)0.f;
  const float* xl = xproj + (long long)bi * T * ldx + d * G + uc;
  auto xload = [&](int sn) {
    const float* p = xl + (long long)(t0 + dt * min(sn, T - 1)) * ldx;
    return f32x4{p[0], p[H], p[2 * H], p[3 * H]};
  };
  f32x4 ring[MSD];
#pragma unroll
  for (int r = 0; r < MSD; ++r) ring[r] = xload(r);
  float c = 0.f;
  __syncthreads();

  for (int s0 = 0; s0 < T; s0 += MSD) {
#pragma unroll
    for (int r = 0; r < MSD; ++r) {
      const int s = s0 + r;
      if (s >= T) break;
      const f32x4 xv = ring[r];
      ring[r] = xload(s + MSD);
      if (TRACE && w == 0) sstamp(tr, T, s, 0, 0.f);
      const bf16* hr = &hs[s & 1][j][0];
      f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        const s16x4 hb = *reinterpret_cast<const s16x4*>(hr + 4 * k);
        if (k & 1) a1 = mfma4(wa[k], hb, a1);
        else a0 = mfma4(wa[k], hb, a0);
      }
      const f32x4 pre = a0 + a1 + xv;
      if (TRACE && w == 0) sstamp(tr, T, s, 1, pre[0]);
      const float ig = fsig(pre[0]), fg = fsig(pre[1]), gg = ftanh(pre[2]), og = fsig(pre[3]);
      c = fg * c + ig * gg;
      const float h = og * ftanh(c);
      if (cell) {
        hs[(s + 1) & 1][j][u] = (bf16)h;
        const long long t = t0 + dt * s, oh = ((long long)bi * T + t) * ldh + d * H + u;
        float* gp = gout + ((long long)bi * T + t) * ldx + d * G + u;
        gp[0] = ig;
        gp[H] = fg;
        gp[2 * H] = gg;
        gp[3 * H] = og;
        hout[oh] = h;
        cout[oh] = c;
        if (hout16) hout16[oh] = (bf16)h;
      }
      if (TRACE && w == 0) sstamp(tr, T, s, 2, h);
      __syncthreads();
    }
  }
}

// Backward.  Same workgroup shape; see the block comment above for the lane map.
template <int KC, int NW, bool TRACE>
__global__ void __launch_bounds__(NW * 64) lstm_mfma_bwd(const float* __restrict__ dhout, const float* __restrict__ call,
                                                         const float* __restrict__ gall, const float* __restrict__ whh,
                                                         int B, int T, int dirs, float* __restrict__ dg,
                                                         bf16* __restrict__ dg16, unsigned long long* tr) {
  constexpr int H = 4 * KC, G = 4 * H;
  const int d = blockIdx.y, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int b0 = blockIdx.x * MU;
  __shared__ __attribute__((aligned(16))) bf16 gs[2][MU][G];  // dG_{s-1}, the B operand
  const long long ldg = (long long)dirs * G, ldh = (long long)dirs * H;
  const int t0 = d ? 0 : T - 1, dt = d ? 1 : -1;  // opposite to the forward recurrence
  const int fwd_prev = d ? 1 : -1;                // offset of the forward's previous time step
  const int nu = min(MU, B - b0);

  const int j = lane & 3, kq = lane >> 4, u = 16 * w + ((lane >> 2) & 3) * 4 + kq;
  const bool cell = u < H && j < nu;
  const int bi = b0 + min(j, nu - 1), uc = min(u, H - 1);
  s16x4 wa[KC];
  {  // A: block (lane >> 2) = (unit quad, gate block kq), row (lane & 3): unit 16w + (lane & 15)
    const int ua = 16 * w + (lane & 15);
    const float* W = whh + (long long)d * G * H + (long long)(kq * H) * H + min(ua, H - 1);
#pragma unroll
    for (int c = 0; c < KC; ++c)
      wa[c] = ua < H ? bf4(W[(4 * c) * H], W[(4 * c + 1) * H], W[(4 * c + 2) * H], W[(4 * c + 3) * H])
                     : s16x4{0, 0, 0, 0};
  }
  for (int i = tid; i < 2 * MU * G; i += blockDim.x) (&gs[0][0][0])[i] = (bf16)0.f;
  struct In {
    float dh, c, cp, i, f, g, o;
  };
  const float* dhb = dhout + (long long)bi * T * ldh + d * H + uc;
  const float* cb = call + (long long)bi * T * ldh + d * H + uc;
  const float* gb = gall + (long long)bi * T * ldg + d * G + uc;
  auto fetch = [&](int sn) {  // unconditional loads; c_prev past the sequence start is zeroed at use
    const int t = t0 + dt * min(sn, T - 1), tp = min(max(t + fwd_prev, 0), T - 1);
    In v;
    v.dh = dhb[(long long)t * ldh];
    v.c = cb[(long long)t * ldh];
    v.cp = cb[(long long)tp * ldh];
    const float* g = gb + (long long)t * ldg;
    v.i = g[0];
    v.f = g[H];
    v.g = g[2 * H];
    v.o = g[3 * H];
    return v;
  };
  In ring[MSD];
#pragma unroll
  for (int r = 0; r < MSD; ++r) ring[r] = fetch(r);
  float dc = 0.f;
  const bool hi = kq & 2, lo = kq & 1;
  __syncthreads();

  for (int s0 = 0; s0 < T; s0 += MSD) {
#pragma unroll
    for (int r = 0; r < MSD; ++r) {
      const int s = s0 + r;
      if (s >= T) break;
      const In in = ring[r];
      ring[r] = fetch(s + MSD);
      if (TRACE && w == 0) sstamp(tr, T, s, 0, 0.f);
      const bf16* gr = &gs[s & 1][j][kq * H];
      f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        const s16x4 gb4 = *reinterpret_cast<const s16x4*>(gr + 4 * k);
        if (k & 1) a1 = mfma4(wa[k], gb4, a1);
        else a0 = mfma4(wa[k], gb4, a0);
      }
      const f32x4 v = a0 + a1;
      // sum the four gate blocks kq (lanes xor 16, xor 32); this lane keeps register kq
      const float k0 = hi ? v[2] : v[0], k1 = hi ? v[3] : v[1];
      const float r0 = __shfl_xor(hi ? v[0] : v[2], 32, 64), r1 = __shfl_xor(hi ? v[1] : v[3], 32, 64);
      const float e0 = k0 + r0, e1 = k1 + r1;
      const float rec = (lo ? e1 : e0) + __shfl_xor(lo ? e0 : e1, 16, 64);
      if (TRACE && w == 0) sstamp(tr, T, s, 1, rec);
      const float dh = in.dh + rec;
      const float cp = s == T - 1 ? 0.f : in.cp;  // the forward's c_{-1} = 0
      const float tc = ftanh(in.c);
      const float dcs = dc + dh * in.o * (1.f - tc * tc);
      const float di = dcs * in.g * in.i * (1.f - in.i), df = dcs * cp * in.f * (1.f - in.f);
      const float dgg = dcs * in.i * (1.f - in.g * in.g), dob = dh * tc * in.o * (1.f - in.o);
      dc = dcs * in.f;
      if (cell) {
        bf16* gn = &gs[(s + 1) & 1][j][u];
        gn[0] = (bf16)di;
        gn[H] = (bf16)df;
        gn[2 * H] = (bf16)dgg;
        gn[3 * H] = (bf16)dob;
        const long long o = ((long long)bi * T + t0 + dt * s) * ldg + d * G + u;
        dg[o] = di;
        dg[o + H] = df;
        dg[o + 2 * H] = dgg;
        dg[o + 3 * H] = dob;
        if (dg16) {
          dg16[o] = (bf16)di;
          dg16[o + H] = (bf16)df;
          dg16[o + 2 * H] = (bf16)dgg;
          dg16[o + 3 * H] = (bf16)dob;
        }
      }
      if (TRACE && w == 0) sstamp(tr, T, s, 2, dc);
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------- launchers
// (a registered trace buffer selects the TRACE instantiations)
template <int HM>
void launch_small_fwd(dim3 g, hipStream_t s, bool fast, const float* x, const float* w, int T, int H, int dirs,
                      float* h, bf16* h16, float* c, float* gt) {
  unsigned long long* const tr = trace_ptr();
  if (tr) lstm_small_fwd<HM, true, true><<<g, SNT, 0, s>>>(x, w, T, H, dirs, h, h16, c, gt, tr);
  else if (fast) lstm_small_fwd<HM, true, false><<<g, SNT, 0, s>>>(x, w, T, H, dirs, h, h16, c, gt, nullptr);
  else lstm_small_fwd<HM, false, false><<<g, SNT, 0, s>>>(x, w, T, H, dirs, h, h16, c, gt, nullptr);
}
template <int HM>
void launch_small_bwd(dim3 g, hipStream_t s, bool fast, const float* dh, const float* c, const float* gt,
                      const float* w, int T, int H, int dirs, float* dg, bf16* dg16) {
  unsigned long long* const tr = trace_ptr();
  if (tr) lstm_small_bwd<HM, true, true><<<g, SNT, 0, s>>>(dh, c, gt, w, T, H, dirs, dg, dg16, tr);
  else if (fast) lstm_small_bwd<HM, true, false><<<g, SNT, 0, s>>>(dh, c, gt, w, T, H, dirs, dg, dg16, nullptr);
  else lstm_small_bwd<HM, false, false><<<g, SNT, 0, s>>>(dh, c, gt, w, T, H, dirs, dg, dg16, nullptr);
}

// The MFMA form of the encoder BiLSTM (lstm_mfma_fwd / _bwd): bf16 compute, H in {16, 32, 44, 48, 64}.
// Off by default (slower, see the kernels); avc_lstm_set_small_mfma(1) or AVC_BILSTM_MFMA=1 selects it.
std::atomic<int> g_small_mfma{-1};
bool small_mfma(int H, bool fast) {
  int on = g_small_mfma.load(std::memory_order_relaxed);
  if (on < 0) on = getenv("AVC_BILSTM_MFMA") ? atoi(getenv("AVC_BILSTM_MFMA")) != 0 : 0;
  return on && fast && (H == 16 || H == 32 || H == 44 || H == 48 || H == 64);
}
template <int KC>
void launch_mfma_fwd(hipStream_t s, const float* x, const float* w, int B, int T, int dirs, float* h, bf16* h16,
                     float* c, float* gt) {
  constexpr int NW = (4 * KC + 15) / 16;
  const dim3 g(cdiv(B, MU), dirs);
  unsigned long long* const tr = trace_ptr();
  if (tr) lstm_mfma_fwd<KC, NW, true><<<g, NW * 64, 0, s>>>(x, w, B, T, dirs, h, h16, c, gt, tr);
  else lstm_mfma_fwd<KC, NW, false><<<g, NW * 64, 0, s>>>(x, w, B, T, dirs, h, h16, c, gt, nullptr);
}
template <int KC>
void launch_mfma_bwd(hipStream_t s, const float* dh, const float* c, const float* gt, const float* w, int B, int T,
                     int dirs, float* dg, bf16* dg16) {
  constexpr int NW = (4 * KC + 15) / 16;
  const dim3 g(cdiv(B, MU), dirs);
  unsigned long long* const tr = trace_ptr();
  if (tr) lstm_mfma_bwd<KC, NW, true><<<g, NW * 64, 0, s>>>(dh, c, gt, w, B, T, dirs, dg, dg16, tr);
  else lstm_mfma_bwd<KC, NW, false><<<g, NW * 64, 0, s>>>(dh, c, gt, w, B, T, dirs, dg, dg16, nullptr);
}

}  // namespace

int avcl::small_fwd(const float* xproj, const float* w, int B, int T, int H, int dirs, float* h, bf16* h16, float* c,
                    float* gates, bool fast, hipStream_t s) {
  if (small_mfma(H, fast)) {
    switch (H) {
      case 16: launch_mfma_fwd<4>(s, xproj, w, B, T, dirs, h, h16, c, gates); break;
      case 32: launch_mfma_fwd<8>(s, xproj, w, B, T, dirs, h, h16, c, gates); break;
      case 44: launch_mfma_fwd<11>(s, xproj, w, B, T, dirs, h, h16, c, gates); break;
      case 48: launch_mfma_fwd<12>(s, xproj, w, B, T, dirs, h, h16, c, gates); break;
      default: launch_mfma_fwd<16>(s, xproj, w, B, T, dirs, h, h16, c, gates); break;
    }
    return avc_check_launch("avc_lstm_fwd(small, mfma)");
  }
  dim3 g(B, dirs);
  if (H <= 16) launch_small_fwd<16>(g, s, fast, xproj, w, T, H, dirs, h, h16, c, gates);
  else if (H <= 32) launch_small_fwd<32>(g, s, fast, xproj, w, T, H, dirs, h, h16, c, gates);
  else if (H <= 48) launch_small_fwd<48>(g, s, fast, xproj, w, T, H, dirs, h, h16, c, gates);
  else launch_small_fwd<64>(g, s, fast, xproj, w, T, H, dirs, h, h16, c, gates);
  return avc_check_launch("avc_lstm_fwd(small)");
}

int avcl::small_bwd(const float* dh_out, const float* c, const float* gates, const float* w, int B, int T, int H,
                    int dirs, float* dg, bf16* dg16, bool fast, hipStream_t s) {
  if (small_mfma(H, fast)) {
    switch (H) {
      case 16: launch_mfma_bwd<4>(s, dh_out, c, gates, w, B, T, dirs, dg, dg16); break;
      case 32: launch_mfma_bwd<8>(s, dh_out, c, gates, w, B, T, dirs, dg, dg16); break;
      case 44: launch_mfma_bwd<11>(s, dh_out, c, gates, w, B, T, dirs, dg, dg16); break;
      case 48: launch_mfma_bwd<12>(s, dh_out, c, gates, w, B, T, dirs, dg, dg16); break;
      default: launch_mfma_bwd<16>(s, dh_out, c, gates, w, B, T, dirs, dg, dg16); break;
    }
    return avc_check_launch("avc_lstm_bwd(small, mfma)");
  }
  dim3 g(B, dirs);
  if (H <= 16) launch_small_bwd<16>(g, s, fast, dh_out, c, gates, w, T, H, dirs, dg, dg16);
  else if (H <= 32) launch_small_bwd<32>(g, s, fast, dh_out, c, gates, w, T, H, dirs, dg, dg16);
  else if (H <= 48) launch_small_bwd<48>(g, s, fast, dh_out, c, gates, w, T, H, dirs, dg, dg16);
  else launch_small_bwd<64>(g, s, fast, dh_out, c, gates, w, T, H, dirs, dg, dg16);
  return avc_check_launch("avc_lstm_bwd(small)");
}

extern "C" int avc_lstm_small_mfma(int H, int compute) { return small_mfma(H, compute == AVC_BF16) ? 1 : 0; }
extern "C" int avc_lstm_set_small_mfma(int mode) {
  g_small_mfma.store(mode < 0 ? -1 : (mode ? 1 : 0), std::memory_order_relaxed);
  return 0;
}
