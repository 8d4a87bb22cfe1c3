// lstm2.hip — the decoder lstm2 (two stacked LSTM layers, H = 1024) as ONE persistent launch per
// direction of the training step: a layer wavefront forward (lstm2_persist_fwd) and its mirror
// backward (lstm2_persist_bwd), with the avc_lstm2_* entry points.  The hand-off between
// workgroups is the write-through flag form of lstm_internal.h.
#include <cstdlib>

#include "lstm_internal.h"

namespace {
using namespace avcl;

// =============================================================== two stacked layers, one launch
// Decoder lstm2 (nn.LSTM(512 -> 1024, num_layers=2), AutoVC.py:96,110) forward as a layer
// WAVEFRONT: tick k runs layer 0 at step k and layer 1 at step k - 1, so both layers share one
// hand-off per tick -- T + 1 hand-offs instead of 2T -- and layer 1's input projection
// h0_t W_ih1^T happens inside the recurrence (no separate 8192 x 4096 x 1024 GEMM).
// Register budget forces the shape: three H x 4H bf16 matrices (W_hh0, W_ih1, W_hh1) live in
// VGPRs, replicated once per utterance group, so groups are 16 utterances (a full MFMA tile, no
// padding rows: ceil(B/16) groups x H/16 members = 256 workgroups at B = 64, H = 1024) and a
// member owns 16 hidden units of EACH layer: 3 x 64 gate columns x H = 192 VGPRs per thread.
// Per tick every member needs the group's h0_{k-1} and h1_{k-2} (16 x H bf16 each) in LDS;
// wave w = (gate pair w & 1, K quarter w >> 1) multiplies each A fragment it reads against six
// weight fragments (P0 = h0 W_hh0^T, P1 = h0 W_ih1^T + h1 W_hh1^T for its two gates), so every
// A element is read from LDS once per tick; the four K quarters meet in LDS.  Thread tid is
// the cell (layer tid >> 8, utterance (tid >> 4) & 15, unit tid & 15).  Hand-off: the
// write-through flag form above, one flag per member per tick covering both layers' tiles.
struct Persist2Args {
  const float* xproj;  // (B,T,4H) layer-0 input projection incl. b_ih0 + b_hh0
  const bf16* w0;      // W_hh0 [4H][H]
  const bf16* wi1;     // W_ih1 [4H][H]
  const bf16* w1;      // W_hh1 [4H][H]
  const float* bias1;  // b_ih1 + b_hh1 (4H)
  float* hout[2];
  bf16* hout16[2];
  float* call[2];
  float* gall[2];
  unsigned* ctl;
  bf16* pay;  // [layer][2 parities][B][H]
  unsigned long long* trace;
  unsigned* fault;
  unsigned spin;
  int B, T, ng;
};

constexpr int QRG = 16, QJU = 16;  // utterances per group, units per member and layer
constexpr int NLW = 4;             // W_hh1 fragments per wave kept in LDS instead of VGPRs

template <int H>
constexpr size_t persist2_lds() {
  return (size_t)2 * QRG * (H + 8) * 2 + (size_t)4 * 2 * 4 * QRG * QJU * 4 + (size_t)2 * QRG * QJU * 2 +
         (size_t)8 * NLW * 64 * 16 + (size_t)6 * 512 * 4 + 16;
}

// ---- LDS-DMA staging of the backward's hand-off payload: 16-B global_load_lds fills, sc1 like every
// other load of handed-off bytes, retired by counted s_waitcnt vmcnt(n) + s_barrier.
__device__ __attribute__((aligned(16))) unsigned g_zero_l2[256] = {};  // source of zero rows: one 1-KiB fill
typedef __attribute__((address_space(3))) void* l2_lds_ptr;
typedef const __attribute__((address_space(1))) void* l2_gbl_ptr;
// 16-B LDS fragment read as inline asm: the compiler's waitcnt pass would otherwise wait for every
// LDS-DMA in flight (the next chunk's) before it.  OFF is the instruction's immediate byte offset
// (< 64 KiB), so the reads of a chunk tile share one address register: with an address VGPR per read
// the backward spilled weight fragments to scratch.
template <int OFF>
__device__ __forceinline__ bf16x8 l2_ds_read16(unsigned addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds_read offset field is 16 bits");
  u32x4_t v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return __builtin_bit_cast(bf16x8, v);
}
// the block's quit word, read the same way: before a plain LDS read the compiler waits for the previous
// tick's fills with a count that also covers the output stores issued after them
__device__ __forceinline__ int l2_ds_read_word(unsigned addr) {
  int v;
  asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
  return v;
}
__device__ __forceinline__ unsigned l2_lds_addr(const void* p) {
  return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}
// workgroup barrier for LDS traffic alone: __syncthreads() also waits for every global load and store
// of the wave (vmcnt(0)).  (Backward only: its output stores follow the publication.  In the forward,
// whose output stores precede it, the same barriers let them queue in front of wave 0's payload stores:
// measured slower, profiles/r7_recur_fetch_ab.txt.)
__device__ __forceinline__ void l2_lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
// at most N vector-memory operations of this wave still in flight
template <int N>
__device__ __forceinline__ void l2_wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// The same wait for everything, as an instruction the compiler sees.  Its own bookkeeping of what is in
// flight follows every static path (a load under one `if`, its use under another), and where it believes
// a load pending it puts s_waitcnt vmcnt(0) in front of the next write of that register, on every tick.
// Placed where nothing is in flight any more, this costs nothing and clears that bookkeeping.
__device__ __forceinline__ void l2_drain_vm() {
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), expcnt and lgkmcnt left alone
}
// Waves 1..7: the staged outputs of tick kp (all 512 cells) to HBM.  (16-B value-major stores
// of the same bytes measured slower per tick: 5.18 vs 4.99 us.)
template <int H>
__device__ __forceinline__ void lstm2_store_outputs(const Persist2Args& a, const float* outs, int kp, int b0, int j0) {
  constexpr int G = 4 * H;
  for (int cell = threadIdx.x - 64; cell < 2 * QRG * QJU; cell += PNT - 64) {
    const int L = cell >> 8, cb = b0 + ((cell >> 4) & 15), cj = j0 + (cell & 15);
    const int t = L == 0 ? kp : kp - 1;
    if (!(L == 0 ? kp < a.T : kp >= 1) || cb >= a.B) continue;
    const float* o = outs + cell;
    const long long oh = ((long long)cb * a.T + t) * H + cj;
    a.hout[L][oh] = o[0];
    a.hout16[L][oh] = (bf16)o[0];
    a.call[L][oh] = o[PNT];
    float* gpo = a.gall[L] + ((long long)cb * a.T + t) * G + cj;
    gpo[0] = o[2 * PNT];
    gpo[H] = o[3 * PNT];
    gpo[2 * H] = o[4 * PNT];
    gpo[3 * H] = o[5 * PNT];
  }
}

template <int H>
__global__ void __launch_bounds__(PNT, 1) lstm2_persist_fwd(Persist2Args a) {
  // The measured schedule (each alternative was compiled and timed; the other values are gone):
  constexpr int SB = 2;       // scheduling fence every SB k-blocks of the product (without one the compiler
                              // hoists the A fragment reads and spills weight fragments)
  constexpr int LB = 2;       // payload loads in LB batches.  1 batch (all eight loads in flight before one wait;
                              // 253 VGPRs, no scratch, NLW = 4) is no faster: per tick, start -> payload in LDS
                              // 2.48 -> 2.46 us, products 1.47 -> 1.51, -> published 0.82 -> 0.84, period 4.83 ->
                              // 4.88; isolated 656.7 -> 655.6 us (profiles/lstm2_poll_ab.txt)
  constexpr bool OS = false;  // the previous tick's outputs are stored after the products (true: under the
                              // payload loads -- slower)
  constexpr int G = 4 * H, AP = H + 8, NR = H / QJU, NKQ = H / 128;  // k-blocks per K quarter
  constexpr int NCH = 2 * QRG * H / 8 / PNT;                          // 16-B chunks per thread
  static_assert(NCH * PNT * 8 == 2 * QRG * H && NR <= 64, "two-layer tiling");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  bf16* As = reinterpret_cast<bf16*>(smem_raw);                          // [2 layers][16][AP]
  float* red = reinterpret_cast<float*>(smem_raw + 2 * QRG * AP * 2);    // [kq][L][q][16][16]
  bf16* hs16 = reinterpret_cast<bf16*>(red + 4 * 2 * 4 * QRG * QJU);     // [L][16][16] publish tile
  // the tick's outputs (h, c, i, f, g, o per cell), stored to HBM by waves 1..7 during the NEXT
  // tick (after its products), so they never queue in front of wave 0's hand-off
  float* outs = reinterpret_cast<float*>(reinterpret_cast<char*>(hs16 + 2 * QRG * QJU) + (size_t)8 * NLW * 64 * 16);
  int* quit = reinterpret_cast<int*>(outs + 6 * PNT);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, gp = w & 1, kq = w >> 1;
  const int g = blockIdx.x % a.ng, r = blockIdx.x / a.ng;
  const int j0 = r * QJU, b0 = g * QRG;
  const int T = a.T, B = a.B, rows = min(QRG, B - b0);
  const __amdgpu_buffer_rsrc_t pay = brsrc(a.pay, (long long)4 * B * H * 2);
  unsigned* flags = a.ctl + 4 + g * PFL;

  // weight fragments (B operand): gate q = 2gp + i, unit j0 + (lane & 15), k-block kq*NKQ + k.
  // The last NLW W_hh1 fragments of gate 2gp+1 live in LDS (wl, per wave and lane): with all 48
  // in VGPRs the compiler spilled two to scratch and waited on their reload every tick.
  bf16x8 f0[2][NKQ], fi[2][NKQ], f1a[NKQ], f1b[NKQ - NLW];  // W_hh1: gate 2gp (a), 2gp + 1 (b)
  bf16x8* wl = reinterpret_cast<bf16x8*>(hs16 + 2 * QRG * QJU) + (w * NLW) * 64 + lane;  // [w][NLW][64]
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long long ro = (long long)((2 * gp + i) * H + j0 + (lane & 15)) * H + kq * NKQ * 32 + 8 * (lane >> 4);
#pragma unroll
    for (int k = 0; k < NKQ; ++k) {
      f0[i][k] = *reinterpret_cast<const bf16x8*>(a.w0 + ro + 32 * k);
      fi[i][k] = *reinterpret_cast<const bf16x8*>(a.wi1 + ro + 32 * k);
      const bf16x8 v1 = *reinterpret_cast<const bf16x8*>(a.w1 + ro + 32 * k);
      if (i == 0) f1a[k] = v1;
      else if (k < NKQ - NLW) f1b[k < NKQ - NLW ? k : 0] = v1;
      else wl[(k - (NKQ - NLW)) * 64] = v1;
    }
  }
  for (int i = tid; i < 2 * QRG * AP / 2; i += PNT) reinterpret_cast<unsigned*>(As)[i] = 0u;
  if (tid == 0) *quit = 0;
  // cell of this thread
  const int L = tid >> 8, cr = (tid >> 4) & 15, cu = tid & 15, cb = b0 + cr, cj = j0 + cu;
  const bool cv = cb < B;
  float c = 0.f;
  __syncthreads();

  for (int k = 0; k <= T; ++k) {
    const int t = L == 0 ? k : k - 1;  // this thread's step
    const bool act = L == 0 ? k < T : k >= 1;
    if (k < T) stamp(a.trace, T, k, 0);
    // gate inputs besides the recurrent products: layer 0 the x projection of its step (loaded
    // ahead of the exchange), layer 1 its bias (L1-resident re-loads)
    float px[4] = {0.f, 0.f, 0.f, 0.f};
    if (act && cv) {
      const float* xp = L == 0 ? a.xproj + ((long long)cb * T + t) * G + cj : a.bias1 + cj;
#pragma unroll
      for (int q = 0; q < 4; ++q) px[q] = xp[q * H];
    }
    f32x4 p0[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    f32x4 p1[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (k > 0) {
      if (w == 0 && !poll_flags(flags, NR, (unsigned)k, a.ctl, a.fault, a.spin)) *quit = 1;
      __syncthreads();
      if (*quit) return;  // block-uniform exit after a spin timeout
      // h0_{k-1} -> As[0], h1_{k-2} -> As[1] (k >= 2); rows past the batch stay zero
      // (NCH / LB chunks in flight per batch: the weight fragments leave few registers)
      const int slot = (k - 1) & 1;
#pragma unroll
      for (int hf = 0; hf < LB; ++hf) {
        u32x4_t v[NCH / LB];
#pragma unroll
        for (int i = 0; i < NCH / LB; ++i) {
          const int ch = tid + PNT * (hf * NCH / LB + i), l = ch / (QRG * H / 8), rem = ch - l * (QRG * H / 8),
                    row = rem / (H / 8), col = rem - row * (H / 8);
          v[i] = row < rows && (l == 0 || k >= 2)
                     ? __builtin_amdgcn_raw_buffer_load_b128(pay, (((l * 2 + slot) * B + b0 + row) * H + col * 8) * 2,
                                                             0, AUX_SC1)
                     : u32x4_t{0u, 0u, 0u, 0u};
        }
        // OS: the previous tick's outputs leave while this tick's payload loads are in flight
        if (OS && hf == 0 && w > 0) lstm2_store_outputs<H>(a, outs, k - 1, b0, j0);
#pragma unroll
        for (int i = 0; i < NCH / LB; ++i) {
          const int ch = tid + PNT * (hf * NCH / LB + i), l = ch / (QRG * H / 8), rem = ch - l * (QRG * H / 8),
                    row = rem / (H / 8), col = rem - row * (H / 8);
          *reinterpret_cast<u32x4_t*>(As + (l * QRG + row) * AP + col * 8) = v[i];
        }
      }
      __syncthreads();
      if (k < T) stamp(a.trace, T, k, 1);
      const bf16* a0p = As + (lane & 15) * AP + kq * NKQ * 32 + 8 * (lane >> 4);
      const bf16* a1p = a0p + QRG * AP;
#pragma unroll
      for (int kk = 0; kk < NKQ; ++kk) {
        const bf16x8 x0 = *reinterpret_cast<const bf16x8*>(a0p + 32 * kk);
        const bf16x8 x1 = *reinterpret_cast<const bf16x8*>(a1p + 32 * kk);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          p0[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x0, f0[i][kk], p0[i], 0, 0, 0);
          p1[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x0, fi[i][kk], p1[i], 0, 0, 0);
          const bf16x8 wb = i == 0                ? f1a[kk]
                            : kk < NKQ - NLW      ? f1b[kk < NKQ - NLW ? kk : 0]
                                                  : wl[(kk - (NKQ - NLW)) * 64];
          p1[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x1, wb, p1[i], 0, 0, 0);
        }
        // SB > 0: at most SB k-blocks of A fragments in flight (the weights hold 184 VGPRs)
        if (SB > 0 && kk % SB == SB - 1) __builtin_amdgcn_sched_barrier(0);
      }
    }
    // K-quarter partials -> LDS: red[((kq * 2 + L) * 4 + q) * 256 + row * 16 + unit]
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float* d0 = red + ((kq * 2 + 0) * 4 + 2 * gp + i) * (QRG * QJU) + (lane & 15);
      float* d1 = red + ((kq * 2 + 1) * 4 + 2 * gp + i) * (QRG * QJU) + (lane & 15);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        d0[(4 * (lane >> 4) + e) * QJU] = p0[i][e];
        d1[(4 * (lane >> 4) + e) * QJU] = p1[i][e];
      }
    }
    if (!OS && k > 0 && w > 0) lstm2_store_outputs<H>(a, outs, k - 1, b0, j0);
    __syncthreads();
    if (k < T) stamp(a.trace, T, k, 2);
    float pre[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float s = px[q];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) s += red[((kk * 2 + L) * 4 + q) * (QRG * QJU) + cr * QJU + cu];
      pre[q] = s;
    }
    const float ig = fsig(pre[0]), fg = fsig(pre[1]), gg = ftanh(pre[2]), og = fsig(pre[3]);
    float h = 0.f;
    if (act) {
      c = fg * c + ig * gg;
      h = og * ftanh(c);
    }
    hs16[(L * QRG + cr) * QJU + cu] = (bf16)h;
    outs[tid] = h;
    outs[PNT + tid] = c;
    outs[2 * PNT + tid] = ig;
    outs[3 * PNT + tid] = fg;
    outs[4 * PNT + tid] = gg;
    outs[5 * PNT + tid] = og;
    __syncthreads();
    // ---- publish h0_k and h1_{k-1} (wave 0: lanes 0..31 layer 0, 32..63 layer 1; 16 B each),
    // needed by tick k + 1 (none after tick T - 1); the other waves store their outputs meanwhile
    if (w == 0 && k < T) {
      const int l = lane >> 5, row = (lane >> 1) & 15, half = lane & 1;
      if (row < rows) {
        const u32x4_t v = *reinterpret_cast<const u32x4_t*>(hs16 + (l * QRG + row) * QJU + half * 8);
        __builtin_amdgcn_raw_buffer_store_b128(v, pay, (((l * 2 + (k & 1)) * B + b0 + row) * H + j0 + half * 8) * 2, 0,
                                               AUX_SC1);
      }
      raise_flag(flags, r, (unsigned)(k + 1));
    }
    if (k < T) stamp(a.trace, T, k, 3);
  }
  if (w > 0) lstm2_store_outputs<H>(a, outs, T, b0, j0);  // the last tick's (staged above its barrier)
}

// =============================================================== two stacked layers, backward
// Decoder lstm2 backward as a layer WAVEFRONT (the forward's mirror): tick k runs layer 1 at step
// T-1-k and layer 0 at step T-k, so one hand-off per tick serves both layers, and layer 1's input
// gradient dX1 = dG1 W_ih1 -- layer 0's upstream gradient -- is formed inside the recurrence (no
// 8192 x 1024 x 4096 GEMM between two single-layer launches).  Tick k hands over dG1 and dG0 of
// tick k-1 (2 x 16 x 4H bf16 = 256 KB per consumer); member r owns units j0..j0+15 of EACH layer:
//   dh1_t  = dG1_{t+1} W_hh1[:, j] + dL/dh1_t (upstream)
//   dh0_t' = dG0_{t'+1} W_hh0[:, j] + dG1_{t'} W_ih1[:, j]       (t' = t + 1: dG1_{t'} = the same payload)
// so each member keeps three 4H x 16 slices (W_hh1^T, W_ih1^T, W_hh0^T rows j0..) as MFMA B fragments:
// 40 in VGPRs and 8 per wave in LDS.  The payload does not fit the LDS as one A tile: it is staged
// in four 64 KB K-chunks (both layers' 16 rows x 1024 gate rows), the loads of chunk c + 1 in flight
// under chunk c's products; wave w takes k-blocks 4w .. 4w+3 of every chunk, and the eight waves'
// partial 16 x 16 products meet in LDS.  Thread tid is the cell (layer tid >> 8, utterance
// (tid >> 4) & 15, unit tid & 15); dc stays in its register.  Hand-off: the forward's write-through
// flag form, one flag per member per tick for both layers' tiles.
struct Persist2BwdArgs {
  const float* dhout1;  // (B,T,H) dL/dh of the top layer's output
  const float* call[2];  // (B,T,H) cell states of layer 0 / 1
  const float* gall[2];  // (B,T,4H) activated gates
  const bf16* wt0;       // W_hh0^T [H][4H]
  const bf16* wti1;      // W_ih1^T [H][4H]
  const bf16* wt1;       // W_hh1^T [H][4H]
  float* dg[2];          // (B,T,4H) dL/d(pre-activation gates); nullable (bf16 twin only)
  bf16* dg16[2];
  float* dbp;            // [layer][group][4H] per-group bias-gradient partials (sum of dG over the group's
                         // utterances and steps); nullable
  unsigned* ctl;
  bf16* pay;  // [layer][2 parities][B][4H]
  unsigned long long* trace;
  unsigned* fault;
  unsigned spin;
  int B, T, ng;
};

constexpr int BKC = 1024, BNC = 4, BCP = BKC + 8, BNLW = 3;  // K-chunk, chunks, LDS pitch, W_hh0 frags in LDS

// two chunk tiles (LDS-DMA double buffer; the wave partials and the publish tile reuse the first after
// the last chunk), then the LDS-resident weight fragments
template <int H>
constexpr size_t persist2_bwd_lds() {
  return (size_t)2 * 2 * QRG * BCP * 2 + (size_t)8 * BNLW * 64 * 16 + 16;
}

template <int H>
__global__ void __launch_bounds__(PNT, 1) lstm2_persist_bwd(Persist2BwdArgs a) {
  constexpr int G = 4 * H, NR = H / QJU, KPW = BKC / 32 / 8, NF0 = BNC * KPW - BNLW;
  constexpr int CB = 2 * QRG * BCP * 2;  // bytes of one chunk tile
  static_assert(G == BNC * BKC && 2 * QRG * 2 == 8 * 8 && NR <= 64 && NF0 > 0, "wavefront tiling");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* red = reinterpret_cast<float*>(smem_raw);                     // [w][L][16][16] (in tile 0)
  bf16* ds16 = reinterpret_cast<bf16*>(red + 8 * 2 * QRG * QJU);       // [L][16][4 gates x 16] (in tile 0)
  float* st32 = reinterpret_cast<float*>(smem_raw + CB);              // [4 gates][64 cells]: wave 0's dG (in
                                                                       // tile 1, dead after the last chunk)
  bf16x8* wlb = reinterpret_cast<bf16x8*>(smem_raw + 2 * CB);          // [w][BNLW][64]
  int* quit = reinterpret_cast<int*>(wlb + 8 * BNLW * 64);
  static_assert((8 * 2 * QRG * QJU * 4 + 2 * QRG * 4 * QJU * 2) <= CB, "partials fit a chunk tile");
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = blockIdx.x % a.ng, r = blockIdx.x / a.ng;
  const int j0 = r * QJU, b0 = g * QRG;
  const int T = a.T, B = a.B, rows = min(QRG, B - b0);
  const __amdgpu_buffer_rsrc_t pay = brsrc(a.pay, (long long)4 * B * G * 2);
  unsigned* flags = a.ctl + 4 + g * PFL;

  // B fragments: column n = unit j0 + (lane & 15), k = gate row c*BKC + (w*KPW + i)*32 + 8*(lane >> 4)
  bf16x8 f1[BNC][KPW], fi[BNC][KPW], f0[NF0];
  bf16x8* wl = wlb + (w * BNLW) * 64 + lane;
  {
    const long long ro = (long long)(j0 + (lane & 15)) * G + 8 * (lane >> 4);
#pragma unroll
    for (int c = 0; c < BNC; ++c)
#pragma unroll
      for (int i = 0; i < KPW; ++i) {
        const long long o = ro + c * BKC + (w * KPW + i) * 32;
        f1[c][i] = *reinterpret_cast<const bf16x8*>(a.wt1 + o);
        fi[c][i] = *reinterpret_cast<const bf16x8*>(a.wti1 + o);
        const bf16x8 v0 = *reinterpret_cast<const bf16x8*>(a.wt0 + o);
        const int idx = c * KPW + i;
        if (idx < NF0) f0[idx < NF0 ? idx : 0] = v0;
        else wl[(idx - NF0) * 64] = v0;
      }
  }
  // this wave's 8 LDS-DMA fills per chunk: q = 8w + i -> layer q >> 5, row (q >> 1) & 15, half q & 1
  // (1 KiB = 512 gate rows): a wave-uniform base, kept in SGPRs, + the lane's 16-B offset (one register
  // pair for all fills instead of 64-bit vector bases held across the tick); rows past the batch read the
  // zero KiB
  const unsigned lane16 = lane * 16;
  auto issue = [&](int c, int slot) {
    char* tile = smem_raw + (c & 1) * CB;
    // (opaque, or the compiler folds the loop-invariant lane offset into a 64-bit vector base of its own)
    unsigned l16 = lane16;
    asm volatile("" : "+v"(l16));
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int q = 8 * w + i, l = q >> 5, row = (q >> 1) & 15, half = q & 1;
      const bf16* src = row < rows ? a.pay + ((long long)(l * 2 + slot) * B + b0 + row) * G + c * BKC + half * 512
                                   : reinterpret_cast<const bf16*>(g_zero_l2);
      __builtin_amdgcn_global_load_lds((l2_gbl_ptr)(reinterpret_cast<const char*>(src) + l16),
                                       (l2_lds_ptr)(tile + ((l * QRG + row) * BCP + half * 512) * 2), 16, 0, AUX_SC1);
    }
  };
  if (tid == 0) *quit = 0;
  const int L = w >> 2, cr = (tid >> 4) & 15, cu = tid & 15, cb = b0 + cr, cj = j0 + cu;  // (L wave-uniform)
  const bool cv = cb < B;
  const unsigned aoff = (unsigned)(((lane & 15) * BCP + w * KPW * 32 + 8 * (lane >> 4)) * 2);
  float dc = 0.f;
  float sb0 = 0.f, sb1 = 0.f, sb2 = 0.f, sb3 = 0.f;  // this cell's dG summed over its steps (dbp)
  const unsigned quit_addr = l2_lds_addr(quit);
  l2_drain_vm();  // the weight fragments: otherwise waited for at their first use, inside every tick's chunk 0
  __syncthreads();

  for (int k = 0; k <= T; ++k) {
    const int t = L == 1 ? T - 1 - k : T - k;  // this thread's step
    const bool act = (L == 1 ? k < T : k >= 1) && cv;
    if (k < T) stamp(a.trace, T, k, 0);
    f32x4 p1 = {0.f, 0.f, 0.f, 0.f}, p0 = {0.f, 0.f, 0.f, 0.f};
    // per-cell inputs of this step, independent of the exchange.  The layer's pointers come by select
    // on the wave-uniform L: indexed by a per-thread L they were loaded from the argument block through
    // vector memory, each with a wait for everything older, on every tick.  c_{t-1} is loaded at every
    // step (at t = 0 c_t's own address, the value dropped), so a wave with a live cell issues the same
    // number of loads on every tick: wave 0 counts them (below).
    // They are read under `act` alone and deliberately not zeroed here: a write to these registers at the
    // head of the tick waits (vmcnt) for whatever the compiler believes in flight on them, in every wave.
    float dhu, ct, cp, gi, gf, gg, go;
    auto load_inputs = [&]() {
      if (act) {
        const float* callL = L ? a.call[1] : a.call[0];
        const int bt = cb * T + t;  // (32-bit: the row index of a (B,T,.) array; one register less than cb * T in 64)
        const long long oh = (long long)bt * H + cj;
        if (L == 1) dhu = a.dhout1[oh];
        ct = callL[oh];
        cp = callL[t > 0 ? oh - H : oh];
        const float* gp = (L ? a.gall[1] : a.gall[0]) + (long long)bt * G + cj;
        gi = gp[0];
        gf = gp[H];
        gg = gp[2 * H];
        go = gp[3 * H];
      }
    };
    // Waves 1..7 issue them first, ahead of the exchange.  Wave 0 polls the flags, and the poll's wait
    // for a flag word is a wait for every older access of the wave: it issues its inputs behind the
    // first two chunks' fills instead (first used after the products), and its cells' dG are stored by
    // wave 1 (below), so nothing of its own is in flight when it looks at the flags.
    if (w != 0 || k == 0) load_inputs();
    if (k > 0) {
      if (w == 0 && !poll_flags(flags, NR, (unsigned)k, a.ctl, a.fault, a.spin)) *quit = 1;
      __syncthreads();
      // block-uniform exit after a spin timeout, as a scalar branch with a drain: the compiler routes the exit
      // through the loop's latch, a static path from the step's input loads to the loop's head that skips their
      // use, and it then waits for them (vmcnt(0)) at the head of every tick
      if (__builtin_amdgcn_readfirstlane(l2_ds_read_word(quit_addr))) {
        l2_drain_vm();
        return;
      }
      if (k < T) stamp(a.trace, T, k, 1);
      const int slot = (k - 1) & 1;
      issue(0, slot);
      issue(1, slot);
      // wave 0 (layer 0, rows 0..3 of the group: row 0 is always live, so the loads are issued): c_t,
      // c_{t-1} and four gates = W0L loads behind its 16 fills
      constexpr int W0L = 6;
      if (w == 0) load_inputs();
#pragma unroll
      for (int c = 0; c < BNC; ++c) {
        // this wave's fills of chunk c have landed (the next chunk's 8 may be in flight), then
        // every wave's
        // (wave 0: its inputs lie between chunk 1's fills and chunk 2's)
        if (c == BNC - 1) l2_drain_vm();
        else if (w == 0 && c < 2) l2_wait_vm<8 + W0L>();
        else l2_wait_vm<8>();
        asm volatile("s_barrier" ::: "memory");
        const unsigned base = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)(smem_raw + (c & 1) * CB) + aoff;
        // one k-block of A fragments at a time (the weight fragments hold ~180 VGPRs), read at immediate
        // offsets from the tile's one base: layer 0's rows at 64 i, layer 1's at QRG * BCP * 2 + 64 i
#define L2_KBLOCK(I)                                                                                       \
  {                                                                                                        \
    const bf16x8 x0 = l2_ds_read16<64 * (I)>(base), x1 = l2_ds_read16<QRG * BCP * 2 + 64 * (I)>(base);     \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                                     \
    const int idx = c * KPW + (I);                                                                         \
    const bf16x8 wb = idx < NF0 ? f0[idx < NF0 ? idx : 0] : wl[(idx >= NF0 ? idx - NF0 : 0) * 64];         \
    p1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x1, f1[c][I], p1, 0, 0, 0);                               \
    p0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x1, fi[c][I], p0, 0, 0, 0);                               \
    p0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x0, wb, p0, 0, 0, 0);                                     \
    __builtin_amdgcn_sched_barrier(0);                                                                     \
  }
        static_assert(KPW == 4, "four k-blocks per wave and chunk");
        L2_KBLOCK(0)
        L2_KBLOCK(1)
        L2_KBLOCK(2)
        L2_KBLOCK(3)
#undef L2_KBLOCK
        asm volatile("s_barrier" ::: "memory");  // every wave is done reading this tile
        if (c + 2 < BNC) issue(c + 2, slot);
      }
    }
    // wave partials -> LDS: red[((w * 2 + L) * 16 + row) * 16 + unit]
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      red[((w * 2 + 0) * QRG + 4 * (lane >> 4) + e) * QJU + (lane & 15)] = p0[e];
      red[((w * 2 + 1) * QRG + 4 * (lane >> 4) + e) * QJU + (lane & 15)] = p1[e];
    }
    l2_lds_barrier();
    if (k < T) stamp(a.trace, T, k, 2);
    l2_drain_vm();  // the step's inputs, used from here on (the fills were waited for above)
    float dh = act && L == 1 ? dhu : 0.f;
#pragma unroll
    for (int ww = 0; ww < 8; ++ww) dh += red[((ww * 2 + L) * QRG + cr) * QJU + cu];
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
    if (act) {
      // (the compiler otherwise starts tanh(c_t) and the t = 0 select right behind the loads, with a wait
      // for them in front of the exchange)
      asm volatile("" : "+v"(ct), "+v"(cp));
      if (t == 0) cp = 0.f;
      const float tc = ftanh(ct);
      const float dcs = dc + dh * go * (1.f - tc * tc);
      v0 = dcs * gg * gi * (1.f - gi);  // d(pre i)
      v1 = dcs * cp * gf * (1.f - gf);  // d(pre f)
      v2 = dcs * gi * (1.f - gg * gg);  // d(pre g)
      v3 = dh * tc * go * (1.f - go);   // d(pre o)
      dc = dcs * gf;
      sb0 += v0;
      sb1 += v1;
      sb2 += v2;
      sb3 += v3;
    }
    bf16* dsr = ds16 + (L * QRG + cr) * (4 * QJU) + cu;
    dsr[0] = (bf16)v0;
    dsr[QJU] = (bf16)v1;
    dsr[2 * QJU] = (bf16)v2;
    dsr[3 * QJU] = (bf16)v3;
    if (w == 0) {  // its cells' fp32 dG, for wave 1 to store
      st32[lane] = v0;
      st32[64 + lane] = v1;
      st32[2 * 64 + lane] = v2;
      st32[3 * 64 + lane] = v3;
    }
    l2_lds_barrier();
    // ---- publish dG1_{t1} and dG0_{t0} (needed by tick k + 1; none after tick T - 1): wave 0, four
    // 16-B chunks per lane (2 layers x 16 rows x 8 chunks), then the flag
    if (w == 0 && k < T) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ch = lane + 64 * i, l = ch >> 7, row = (ch >> 3) & 15, q8 = ch & 7;
        if (row < rows) {
          const u32x4_t pv = *reinterpret_cast<const u32x4_t*>(ds16 + (l * QRG + row) * (4 * QJU) + q8 * 8);
          __builtin_amdgcn_raw_buffer_store_b128(
              pv, pay, (((l * 2 + (k & 1)) * B + b0 + row) * G + (q8 >> 1) * H + j0 + (q8 & 1) * 8) * 2, 0, AUX_SC1);
        }
      }
      raise_flag(flags, r, (unsigned)(k + 1));
    }
    __syncthreads();  // every wave's stores behind wave 0's flag (the payload doubling as the
                      // output instead measured slower, profiles/r6_lstm2_bwd_payload_out.txt)
    // Waves 1..7 store their cells' dG; wave 1 (rows 4..7 of layer 0) also wave 0's (rows 0..3, the same
    // units and step), read back from st32 before the next tick's barrier lets a fill into that tile.
    auto store_dg = [&](bool on, int row, float x0, float x1, float x2, float x3) {
      if (on) {
        const long long og = (long long)((b0 + row) * T + t) * G + cj;
        float* dgL = L ? a.dg[1] : a.dg[0];
        bf16* dg16L = L ? a.dg16[1] : a.dg16[0];
        if (dgL) {
          float* d = dgL + og;
          d[0] = x0;
          d[H] = x1;
          d[2 * H] = x2;
          d[3 * H] = x3;
        }
        if (dg16L) {
          bf16* d16 = dg16L + og;
          d16[0] = (bf16)x0;
          d16[H] = (bf16)x1;
          d16[2 * H] = (bf16)x2;
          d16[3 * H] = (bf16)x3;
        }
      }
    };
    if (w != 0) store_dg(act, cr, v0, v1, v2, v3);
    if (w == 1) store_dg(k >= 1 && cb - 4 < B, cr - 4, st32[lane], st32[64 + lane], st32[2 * 64 + lane], st32[3 * 64 + lane]);
    if (k < T) stamp(a.trace, T, k, 3);
  }
  if (a.dbp) {
    // the bias gradients' share of this member: dG summed over the group's 16 utterances (LDS, in
    // row order) and T steps (registers, in step order), one plain store per (layer, gate, unit) --
    // deterministic, and the fp32 dG (B x T x 4H per layer) need not be stored for a column sum
    float* sb = red;  // [L][q][16 rows][16 units] = 8 KiB of chunk tile 0
    __syncthreads();  // the last tick's reads of red / ds16 are done
    sb[((L * 4 + 0) * QRG + cr) * QJU + cu] = sb0;
    sb[((L * 4 + 1) * QRG + cr) * QJU + cu] = sb1;
    sb[((L * 4 + 2) * QRG + cr) * QJU + cu] = sb2;
    sb[((L * 4 + 3) * QRG + cr) * QJU + cu] = sb3;
    __syncthreads();
    if (tid < 2 * 4 * QJU) {
      const int l = tid >> 6, q = (tid >> 4) & 3, u = tid & 15;
      float sum = 0.f;
#pragma unroll
      for (int rr = 0; rr < QRG; ++rr) sum += sb[((l * 4 + q) * QRG + rr) * QJU + u];
      a.dbp[((long long)l * a.ng + g) * G + q * H + j0 + u] = sum;
    }
  }
}
}  // namespace

// Two-layer wavefront forward (lstm2_persist_fwd): shape, compute mode and residency.
bool persist2_path(int B, int H, int In1, bool bf) {
  if (!bf || H != 1024 || In1 != H || no_persist_env() || getenv("AVC_LSTM2_OFF")) return false;
  const int ng = (B + QRG - 1) / QRG, grid = ng * (H / QJU);
  if (grid > num_cus()) return false;
  return fits_resident(reinterpret_cast<const void*>(&lstm2_persist_fwd<1024>), PNT, persist2_lds<1024>(), grid);
}

extern "C" int avc_lstm2_persistent(int B, int H, int in1, int compute) {
  return persist2_path(B, H, in1, compute == AVC_BF16) ? 1 : 0;
}

extern "C" size_t avc_lstm2_scratch_bytes(int B, int H) {
  if (B <= 0 || H <= 0) return 0;
  return px_payload_off((B + QRG - 1) / QRG) + (size_t)8 * B * H;
}

extern "C" int avc_lstm2_fwd(const float* xproj0, const void* w_hh0, const void* w_ih1, const void* w_hh1,
                             const float* bias1, int B, int T, int H, float* h0, void* h0_bf16, float* c0,
                             float* gates0, float* h1, void* h1_bf16, float* c1, float* gates1, void* buf,
                             void* stream) {
  AVC_CHECK_ARG(xproj0 && w_hh0 && w_ih1 && w_hh1 && bias1 && h0 && h0_bf16 && c0 && gates0 && h1 && h1_bf16 && c1 &&
                    gates1 && buf && B > 0 && T > 0,
                "avc_lstm2_fwd: bad args");
  AVC_CHECK_ARG(persist2_path(B, H, H, true), "avc_lstm2_fwd: shape B=%d H=%d not supported (see avc_lstm2_persistent)",
                B, H);
  hipStream_t s = as_stream(stream);
  const int ng = (B + QRG - 1) / QRG;
  Persist2Args p;
  p.xproj = xproj0;
  p.w0 = reinterpret_cast<const bf16*>(w_hh0);
  p.wi1 = reinterpret_cast<const bf16*>(w_ih1);
  p.w1 = reinterpret_cast<const bf16*>(w_hh1);
  p.bias1 = bias1;
  p.hout[0] = h0;
  p.hout[1] = h1;
  p.hout16[0] = reinterpret_cast<bf16*>(h0_bf16);
  p.hout16[1] = reinterpret_cast<bf16*>(h1_bf16);
  p.call[0] = c0;
  p.call[1] = c1;
  p.gall[0] = gates0;
  p.gall[1] = gates1;
  p.ctl = reinterpret_cast<unsigned*>(buf);
  p.pay = reinterpret_cast<bf16*>(reinterpret_cast<char*>(buf) + px_payload_off(ng));
  p.trace = trace_ptr();
  p.fault = fault_word();
  p.spin = spin_bound();
  p.B = B;
  p.T = T;
  p.ng = ng;
  if (avc_zero_async(buf, px_ctl_bytes(ng), s)) return -1;
  const dim3 grid(ng * (H / QJU));
  lstm2_persist_fwd<1024><<<grid, PNT, persist2_lds<1024>(), s>>>(p);
  return avc_check_launch("avc_lstm2_fwd");
}

// Two-layer wavefront backward (lstm2_persist_bwd): shape, compute mode and residency.
bool persist2_bwd_path(int B, int H, bool bf) {
  if (!bf || H != 1024 || no_persist_env() || getenv("AVC_LSTM2_OFF")) return false;
  const int ng = (B + QRG - 1) / QRG, grid = ng * (H / QJU);
  if (grid > num_cus()) return false;
  return fits_resident(reinterpret_cast<const void*>(&lstm2_persist_bwd<1024>), PNT, persist2_bwd_lds<1024>(), grid);
}

extern "C" int avc_lstm2_bwd_persistent(int B, int H, int compute) {
  return persist2_bwd_path(B, H, compute == AVC_BF16) ? 1 : 0;
}

extern "C" size_t avc_lstm2_bwd_scratch_bytes(int B, int H) {
  if (B <= 0 || H <= 0) return 0;
  return px_payload_off((B + QRG - 1) / QRG) + (size_t)32 * B * H;  // [2 layers][2 parities][B][4H] bf16
}

extern "C" int avc_lstm2_bwd(const float* dh1, const float* c0, const float* gates0, const float* c1,
                             const float* gates1, const void* w_hh0_t, const void* w_ih1_t, const void* w_hh1_t, int B,
                             int T, int H, float* dg0, void* dg0_bf16, float* dg1, void* dg1_bf16, void* buf,
                             float* db_part, void* stream) {
  AVC_CHECK_ARG(dh1 && c0 && gates0 && c1 && gates1 && w_hh0_t && w_ih1_t && w_hh1_t && (dg0 || dg0_bf16) &&
                    (dg1 || dg1_bf16) && buf && B > 0 && T > 0,
                "avc_lstm2_bwd: bad args");
  AVC_CHECK_ARG(persist2_bwd_path(B, H, true), "avc_lstm2_bwd: shape B=%d H=%d not supported (see avc_lstm2_bwd_persistent)",
                B, H);
  hipStream_t s = as_stream(stream);
  const int ng = (B + QRG - 1) / QRG;
  Persist2BwdArgs p;
  p.dhout1 = dh1;
  p.call[0] = c0;
  p.call[1] = c1;
  p.gall[0] = gates0;
  p.gall[1] = gates1;
  p.wt0 = reinterpret_cast<const bf16*>(w_hh0_t);
  p.wti1 = reinterpret_cast<const bf16*>(w_ih1_t);
  p.wt1 = reinterpret_cast<const bf16*>(w_hh1_t);
  p.dg[0] = dg0;
  p.dg[1] = dg1;
  p.dg16[0] = reinterpret_cast<bf16*>(dg0_bf16);
  p.dg16[1] = reinterpret_cast<bf16*>(dg1_bf16);
  p.dbp = db_part;
  p.ctl = reinterpret_cast<unsigned*>(buf);
  p.pay = reinterpret_cast<bf16*>(reinterpret_cast<char*>(buf) + px_payload_off(ng));
  p.trace = trace_ptr();
  p.fault = fault_word();
  p.spin = spin_bound();
  p.B = B;
  p.T = T;
  p.ng = ng;
  if (avc_zero_async(buf, px_ctl_bytes(ng), s)) return -1;
  lstm2_persist_bwd<1024><<<dim3(ng * (H / QJU)), PNT, persist2_bwd_lds<1024>(), s>>>(p);
  return avc_check_launch("avc_lstm2_bwd");
}
