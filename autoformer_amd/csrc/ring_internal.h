// ring_internal.h — what the eight-wave ring kernels share (gemm_ring.hip: the ring GEMM and the
// dispatcher; conv_ring.hip: the halo conv): the inline-asm fragment reads with their counted
// lgkmcnt wait, and the epilogue of the 2 (M) x 4 (N) wave layout -- bias, conv0-fold row bias, the
// stores staged through LDS (residual, accumulate, GELU forward / backward, column sums, bf16
// twin, transposed blocks), the BatchNorm partial statistics with the finalize by the last-arriving
// row tile, and the BatchNorm-BACKWARD reduction of the halo conv tile (y prefetch, reduction,
// finalize).  All LDS of a kernel is ONE __shared__ array, which the epilogue reuses; the
// last-arriver flags live in it too (gemm_ring.hip's header says why).
#pragma once
#include "gemm_internal.h"

namespace avcg {

constexpr int RROW = 128;  // bytes per LDS row (64 bf16 of K)
constexpr int RBK = 64;    // K per ring slot
constexpr int RNT = 512;   // threads per workgroup

// The halo conv tile (conv_ring.hip): 5 taps, 128 output columns, stages of 32 channels; 128 frames
// per row tile, or 192 for one whole utterance of 128 < T <= 192 frames
constexpr int CV_TM = 128, CU_TM = 192, CV_TN = 128, CV_TAPS = 5, CV_CBK = 32;

// AVC_RING = "BM,BN,NST[,GM]" forces a configuration (benchmarking), "0" disables the kernel;
// AVC_RING_WIN = 0 leaves the conv window operands to gemm_conv.hip, 1 lets forced configurations
// stream them as im2col windows, 2 (default) puts aligned 5-tap convs on the halo conv kernel.
// avc_gemm_set_ring() sets the same at run time (A/B tools in one process).
struct RingCfg {
  int mode = -1;  // -1 auto, 0 off, 1 forced
  int bm = 0, bn = 0, nst = 0, gm = 8, win = 2;
  bool utt = true;  // one-utterance conv tiles for 128 < T <= 192 (win 10 through avc_gemm_set_ring: off)
};

// The halo conv on g (conv_ring.hip; the dispatcher of gemm_ring.hip has checked the shape): the
// one-utterance 192-row tile when utt, else 128-row tiles -- utterance-aligned or straddling, and
// with the BatchNorm-backward epilogue when g.bnb_ws is set.  gm: row tiles per group.
void conv_ring_launch(const GemmArgs& g, bool utt, int gm, hipStream_t s);

// LDS byte address of a pointer into the kernel's dynamic LDS array
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}
// 16-B fragment read issued as inline asm: hipcc's waitcnt pass does not track it, so the caller
// places counted `s_waitcnt lgkmcnt` (+ sched_barrier, cdna_hip_programming.md §5.4 rule 18)
template <int OFF>
__device__ __forceinline__ bf16x8 ds_read16(unsigned addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF) : "memory");
  return __builtin_bit_cast(bf16x8, v);
}
// N reads at BASE, BASE + STRIDE, ... bytes from addr into d[0..N)
template <int N, int STRIDE, int BASE = 0>
__device__ __forceinline__ void ds_read_n(bf16x8* d, unsigned addr) {
  if constexpr (N > 0) {
    d[0] = ds_read16<BASE>(addr);
    ds_read_n<N - 1, STRIDE, BASE + STRIDE>(d + 1, addr);
  }
}
template <int N>
__device__ __forceinline__ void wait_lgkm() {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// "last arrival" on a counter with the flag in the kernel's one LDS array (see header)
__device__ __forceinline__ bool ring_arrive_last(unsigned* cnt, unsigned arrivals, unsigned mine, unsigned* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned old = __hip_atomic_fetch_add(cnt, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = old + mine == arrivals;
    if (last) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *flag = last ? 1u : 0u;
  }
  __syncthreads();
  return *flag != 0;
}

// LDS bytes the staged stores need (ring_store_tile): per wave 64 rows x (TWN + 4) fp32
template <int BM_, int BN_>
constexpr size_t ring_epi_lds() {
  return (size_t)8 * 64 * (BN_ / 4 + 4) * 4;
}

// where a row tile's column sums go: its slot of the self-zeroing workspace, or csum itself
__device__ __forceinline__ float* csum_dst(const GemmArgs& g, int row_tile, int lim) {
  return g.csum_ws ? g.csum_ws + (long long)(row_tile % g.csum_slots) * lim : g.csum;
}

// This wave's rows ch*64 .. +64 of its accumulators `acc` -> its own LDS region `reg` (row pitch RP
// floats; blocks past MI, the partial last chunk of the 192-row tile, are skipped), in the scope of
// ring_store_tile.  The region is the wave's own: the reads that follow only need the wave's LDS
// writes retired, which the caller's barrier also guarantees.
// A macro, not a function: as a __forceinline__ function or a lambda the same loops came out of
// hipcc with other register counts (the plain halo conv 125 -> 129 VGPRs, 4 -> 3 waves per SIMD;
// profiles/ring_refactor_resources.txt), as a macro they are the text the compiler always saw.
#define RING_STAGE_CHUNK(ch)                                                                       \
  _Pragma("unroll") for (int ii = 0; ii < 4; ++ii)                                                 \
  _Pragma("unroll") for (int j = 0; j < NJ; ++j)                                                   \
  _Pragma("unroll") for (int e = 0; e < 4; ++e)                                                    \
    if ((ch) * 4 + ii < MI)                                                                        \
      reg[(ii * 16 + 4 * (lane >> 4) + e) * RP + j * 16 + (lane & 15)] = acc[(ch) * 4 + ii][j][e]

// Stores of the 2 x 4 wave layout's accumulators (wave (wm, wn) owns rows m0 + wm*TWM + i*16 +
// 4*(lane>>4) + e and columns n0 + wn*TWN + j*16 + (lane&15)): each wave stages 64-row chunks of
// its tile in its own LDS region and stores them row-contiguous, 16 B per lane (fp32 C) / 8 B
// (bf16), with the residual, accumulate and GELU epilogues applied per 4-column vector and their
// uniform conditions tested once per vector, not per element (the per-element form carried ~1,800
// uniform branches per 256 x 256 tile: 60 -> 90 us on the 8192 x 4096 x 512 projection).
// Column tails and row strides that are not 16-B multiples take the per-element path.
// Rows >= mlim are not stored (g.M, or the end of a one-utterance conv tile); a wave's rows go in
// 64-row chunks, the last one partial when TWM % 64 != 0 (the 192-row conv tile: 64 + 32).
template <int BM_, int BN_>
__device__ __forceinline__ void ring_store_tile(const GemmArgs& g, f32x4 (&acc)[BM_ / 32][BN_ / 64], int m0, int n0,
                                                int bz, int ks, char* smem_raw, int mlim) {
  constexpr int TWM = BM_ / 2, TWN = BN_ / 4, NJ = TWN / 16, RP = TWN + 4, NIT = TWN / 4;
  constexpr int MI = TWM / 16, NCH = (MI + 3) / 4;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 2, wn = wid & 3;
  float* reg = reinterpret_cast<float*>(smem_raw) + wid * 64 * RP;
  float* C = g.c ? g.c + (long long)bz * g.cbs : nullptr;
  bf16* C16 = g.c16 ? g.c16 + (long long)bz * g.cbs : nullptr;
  const float* res = (g.res && ks == 0) ? g.res + (long long)bz * g.cbs : nullptr;
  // GELU-backward input, fp32 or bf16 (avc_gemm_desc.act_grad_dtype)
  const float* agr = (g.agrad && !g.agrad16) ? static_cast<const float*>(g.agrad) + (long long)bz * g.cbs : nullptr;
  const bf16* agr16 = (g.agrad && g.agrad16) ? static_cast<const bf16*>(g.agrad) + (long long)bz * g.cbs : nullptr;
  bf16* P16 = g.c16pre ? g.c16pre + (long long)bz * g.cbs : nullptr;  // bf16 pre-activation
  const bool vec = (g.ldc & 3) == 0 && (reinterpret_cast<uintptr_t>(C) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(C16) & 7) == 0 && (reinterpret_cast<uintptr_t>(res) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(agr) & 15) == 0 && (reinterpret_cast<uintptr_t>(agr16) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(P16) & 7) == 0;
  const bool acc_c = g.accumulate != 0, gelu16 = g.c16_act != 0;
  float* csum = g.csum;
  if (g.ctr) {
    // transposed blocks (avc_gemm_desc.c_trans_rows): a lane stores 4 consecutive ROWS of one
    // column (contiguous in C, ctr % 4 == 0), consecutive lanes consecutive row quads
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int rlim = min(mlim, m0 + wm * TWM + min(TWM, ch * 64 + 64));
      RING_STAGE_CHUNK(ch);
      __syncthreads();
#pragma unroll 4
      for (int it = 0; it < NIT; ++it) {
        const int q = it * 64 + lane, r4 = q & 15, cl = q >> 4;
        const int row = m0 + wm * TWM + ch * 64 + 4 * r4, col = n0 + wn * TWN + cl;
        if (row >= rlim || col >= g.N) continue;
        f32x4 v = {reg[(4 * r4) * RP + cl], reg[(4 * r4 + 1) * RP + cl], reg[(4 * r4 + 2) * RP + cl],
                   reg[(4 * r4 + 3) * RP + cl]};
        const long long o = out_off(g, row, col);
        if (res) v += *reinterpret_cast<const f32x4*>(res + o);
        if (acc_c) v += *reinterpret_cast<const f32x4*>(C + o);
        *reinterpret_cast<f32x4*>(C + o) = v;
      }
      __syncthreads();
    }
    return;
  }
  if (!C && !res && !acc_c && !agr && (g.ldc & 7) == 0 && (reinterpret_cast<uintptr_t>(C16) & 15) == 0 &&
      (reinterpret_cast<uintptr_t>(P16) & 15) == 0 && (reinterpret_cast<uintptr_t>(agr16) & 15) == 0) {
    // bf16 outputs only (the MLP-Mixer GELU forward / backward, bf16-only C): 8 columns per lane,
    // 16-B stores (8-B bf16 vectors had cost 665 -> 708 us on the 22016 x 7424 x 1856 product)
    constexpr int L8 = TWN / 8, R8 = 64 / L8;
    f32x4 cs0 = {0.f, 0.f, 0.f, 0.f}, cs1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int rlim = min(mlim, m0 + wm * TWM + min(TWM, ch * 64 + 64));
      RING_STAGE_CHUNK(ch);
      __syncthreads();
      // the GELU-backward input is read G4 iterations at a time by UNCONDITIONAL loads (row and
      // column clamped into the tensor: ldc == N, N % 8 == 0 on this path), so the G4 loads are in
      // flight together; a load inside the bounds branch had been waited for at the branch join,
      // one 16-B load per wave in flight at a time (+180-220 us on the 327 MB pre-activations)
      constexpr int G4 = 64 / R8 < 4 ? 64 / R8 : 4;
      for (int it0 = 0; it0 < 64 / R8; it0 += G4) {
        bf16x8 hv[G4];
        if (agr16) {
#pragma unroll
          for (int k = 0; k < G4; ++k) {
            const int r = min(m0 + wm * TWM + ch * 64 + (it0 + k) * R8 + lane / L8, g.M - 1);
            const int cc = min(n0 + wn * TWN + 8 * (lane % L8), g.N - 8);
            hv[k] = *reinterpret_cast<const bf16x8*>(agr16 + (long long)r * g.ldc + cc);
          }
        }
#pragma unroll
        for (int k4 = 0; k4 < G4; ++k4) {
          const int it = it0 + k4;
          const int lr = it * R8 + lane / L8, c8 = lane % L8;
          const int row = m0 + wm * TWM + ch * 64 + lr, col = n0 + wn * TWN + 8 * c8;
          if (row >= rlim || col >= g.N) continue;
          f32x4 v0 = *reinterpret_cast<const f32x4*>(reg + lr * RP + 8 * c8);
          f32x4 v1 = *reinterpret_cast<const f32x4*>(reg + lr * RP + 8 * c8 + 4);
          const long long o = (long long)row * g.ldc + col;
          if (col + 7 < g.N) {
            if (agr16) {
              const bf16x8 h = hv[k4];
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                v0[k] *= gelu_grad_f((float)h[k]);
                v1[k] *= gelu_grad_f((float)h[4 + k]);
              }
            }
            if (csum) {
              cs0 += v0;
              cs1 += v1;
            }
            if (P16)
              *reinterpret_cast<bf16x8*>(P16 + o) = bf16x8{(bf16)v0[0], (bf16)v0[1], (bf16)v0[2], (bf16)v0[3],
                                                           (bf16)v1[0], (bf16)v1[1], (bf16)v1[2], (bf16)v1[3]};
            if (C16) {
              if (gelu16) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                  v0[k] = gelu_f(v0[k]);
                  v1[k] = gelu_f(v1[k]);
                }
              }
              *reinterpret_cast<bf16x8*>(C16 + o) = bf16x8{(bf16)v0[0], (bf16)v0[1], (bf16)v0[2], (bf16)v0[3],
                                                           (bf16)v1[0], (bf16)v1[1], (bf16)v1[2], (bf16)v1[3]};
            }
          } else {
            for (int k = 0; k < 8 && col + k < g.N; ++k) {
              float x = k < 4 ? v0[k] : v1[k - 4];
              if (agr16) x *= gelu_grad_f((float)agr16[o + k]);
              if (P16) P16[o + k] = (bf16)x;
              if (csum) {
                if (k < 4) cs0[k] += x;
                else cs1[k - 4] += x;
              }
              if (C16) C16[o + k] = (bf16)(gelu16 ? gelu_f(x) : x);
            }
          }
        }
      }
      __syncthreads();
    }
    if (csum) {
      // lanes sharing this lane's 8 columns: lane + k * L8
#pragma unroll
      for (int sh = L8; sh < 64; sh *= 2)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          cs0[k] += __shfl_xor(cs0[k], sh, 64);
          cs1[k] += __shfl_xor(cs1[k], sh, 64);
        }
      if (lane < L8) {
        const int col = n0 + wn * TWN + 8 * lane;
        const int lim = g.csum_n > 0 ? g.csum_n : g.N;
        float* dst = csum_dst(g, m0 / BM_ + bz, lim);
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (col + k < lim) atomicAdd(dst + col + k, k < 4 ? cs0[k] : cs1[k - 4]);
      }
    }
    return;
  }
  // column-sum epilogue: lane's 4 columns are the same for every iteration (64 % (TWN/4) == 0)
  f32x4 cs = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int rlim = min(mlim, m0 + wm * TWM + min(TWM, ch * 64 + 64));
    RING_STAGE_CHUNK(ch);
    __syncthreads();
#pragma unroll 4
    for (int it = 0; it < NIT; ++it) {
      const int q = it * 64 + lane, lr = q / (TWN / 4), c4 = q - lr * (TWN / 4);
      const int row = m0 + wm * TWM + ch * 64 + lr, col = n0 + wn * TWN + 4 * c4;
      if (row >= rlim || col >= g.N) continue;
      f32x4 v = *reinterpret_cast<const f32x4*>(reg + lr * RP + 4 * c4);
      const long long o = (long long)row * g.ldc + col;
      if (vec && col + 3 < g.N) {
        if (res) v += *reinterpret_cast<const f32x4*>(res + o);
        if (acc_c) v += *reinterpret_cast<const f32x4*>(C + o);
        if (agr || agr16) {
          f32x4 x;
          if (agr) {
            x = *reinterpret_cast<const f32x4*>(agr + o);
          } else {
            const bf16x4 h = *reinterpret_cast<const bf16x4*>(agr16 + o);
            x = f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
          }
          v = f32x4{v[0] * gelu_grad_f(x[0]), v[1] * gelu_grad_f(x[1]), v[2] * gelu_grad_f(x[2]),
                    v[3] * gelu_grad_f(x[3])};
        }
        if (C) *reinterpret_cast<f32x4*>(C + o) = v;
        if (P16) *reinterpret_cast<bf16x4*>(P16 + o) = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
        if (csum) cs += v;
        if (C16) {
          const f32x4 w = gelu16 ? f32x4{gelu_f(v[0]), gelu_f(v[1]), gelu_f(v[2]), gelu_f(v[3])} : v;
          *reinterpret_cast<bf16x4*>(C16 + o) = bf16x4{(bf16)w[0], (bf16)w[1], (bf16)w[2], (bf16)w[3]};
        }
      } else {
        for (int k = 0; k < 4 && col + k < g.N; ++k) {
          float x = v[k];
          if (res) x += res[o + k];
          if (acc_c) x += C[o + k];
          if (agr) x *= gelu_grad_f(agr[o + k]);
          if (agr16) x *= gelu_grad_f((float)agr16[o + k]);
          if (C) C[o + k] = x;
          if (P16) P16[o + k] = (bf16)x;
          if (csum) cs[k] += x;
          if (C16) C16[o + k] = (bf16)(gelu16 ? gelu_f(x) : x);
        }
      }
    }
    __syncthreads();  // the region is rewritten by the next chunk / reused by the BN epilogue
  }
  if (csum) {
    // lanes sharing this lane's 4 columns: lane + k * (TWN/4)
#pragma unroll
    for (int sh = TWN / 4; sh < 64; sh *= 2)
#pragma unroll
      for (int k = 0; k < 4; ++k) cs[k] += __shfl_xor(cs[k], sh, 64);
    if (lane < TWN / 4) {
      const int col = n0 + wn * TWN + 4 * lane;
      const int lim = g.csum_n > 0 ? g.csum_n : g.N;
      float* dst = csum_dst(g, m0 / BM_ + bz, lim);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (col + k < lim) atomicAdd(dst + col + k, cs[k]);
    }
  }
}
#undef RING_STAGE_CHUNK

// BatchNorm BACKWARD reduction of the layer that produced this data-gradient GEMM's output
// (avc_gemm_bnb on the halo conv ring: C = dL/da of the producing conv + BN + act layer, whose
// stored conv output y, statistics and affine parameters come in g.bnb_*): per column of this
// 128 x 128 tile, over its rows, (sum dz, sum dz*yhat, sum yhat) with yhat = (y - mean)*rstd and
// dz = C * act'(yhat*gamma + beta) -- C rounded to bf16 first when only the bf16 C is stored (the
// value the apply pass reads) -- into the 128-row-tile partials; the last-arriving row tile of the
// column tile reduces them into the apply constants coef[6][N] and the parameter gradients
// (avcbn::bwd_finalize_store).  The separate reduce + finalize launches of the BN backward
// (bn.hip) are gone.  y (bf16, the bf16 step's conv output) is staged through LDS as 16-B rows.
// y prefetch of the tile: 4 x 16 B per thread, issued at kernel start into registers so it lands
// under the K loop (a load-then-store loop in the epilogue had serialised four HBM round trips)
constexpr int BNB_YQ = 128 * 16 / RNT;  // 16-B chunks per thread (128 rows x 16 chunks of 8 bf16)
// LDS offset of the staged y tile (128 rows x 272 B + flag): below the C staging (ring_epi_lds),
// above the partial sums, so the 2-stage conv ring's 98 KiB hold it
constexpr int BNB_YS_LO = 8 * 1024;
__device__ __forceinline__ void ring_bnb_prefetch(const GemmArgs& g, int m0, int n0, u32x4 (&yv)[BNB_YQ]) {
  const bf16* yb = static_cast<const bf16*>(g.bnb_y);
  // unconditional loads at clamped addresses (N % 8 == 0 on this path), zeroed after: a load inside
  // a bounds branch is waited for at the branch join
#pragma unroll
  for (int k = 0; k < BNB_YQ; ++k) {
    const int q = threadIdx.x + k * RNT, r = q >> 4, cc = q & 15;
    const int row = m0 + r, col = n0 + cc * 8;
    yv[k] = *reinterpret_cast<const u32x4*>(yb + (long long)min(row, g.M - 1) * g.ldc + min(col, g.N - 8));
  }
  // (rows / columns outside the tensor are zeroed where the values are written to LDS: a select
  // here would be a use, and hipcc would wait for the loads right away)
}

__device__ __forceinline__ bool ring_bnb_epilogue(const GemmArgs& g, f32x4 (&acc)[4][2], int m0, int n0,
                                                  char* smem_raw, const u32x4* yv) {
  constexpr int BN_ = 128, NJ = 2, FGR = 4;  // 512 threads = 128 columns x 4 row groups (finalize)
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 2, wn = wid & 3;
  const int rbase = m0 + wm * 64 + 4 * (lane >> 4);
  const int cbase = n0 + wn * 32 + (lane & 15);
  const avcbn::BwdFin& f = g.bnb_fin;
  float* red = reinterpret_cast<float*>(smem_raw);  // [3][2 wm][BN_] / the finalize's [3][FGR][BN_]
  constexpr int YP = 2 * BN_ + 16;                  // LDS row pitch of the staged y tile (bytes)
  char* ys = smem_raw + BNB_YS_LO;
  unsigned* flag = reinterpret_cast<unsigned*>(ys + 128 * YP);
  __syncthreads();  // the K loop's fragment reads are done with the LDS
#pragma unroll
  for (int k = 0; k < BNB_YQ; ++k) {
    const int q = tid + k * RNT, r = q >> 4, cc = q & 15;
    const bool in = m0 + r < g.M && n0 + cc * 8 < g.N;
    *reinterpret_cast<u32x4*>(ys + r * YP + cc * 16) = in ? yv[k] : u32x4{0u, 0u, 0u, 0u};
  }
  __syncthreads();
  const bool round16 = g.c == nullptr;
  float s0[NJ], s1[NJ], s2[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = cbase + j * 16;
    const bool cv = col < g.N;
    const float mu = cv ? f.mean[col] : 0.f, rs = cv ? f.rstd[col] : 0.f;
    const float gm = cv && f.gamma ? f.gamma[col] : 1.f, bt = cv && f.beta ? f.beta[col] : 0.f;
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = rbase + i * 16 + e;
        if (!cv || row >= g.M) continue;
        float v = acc[i][j][e];
        if (round16) v = (float)(bf16)v;
        const float yf = __builtin_bit_cast(
            float, (unsigned)*reinterpret_cast<const unsigned short*>(ys + (row - m0) * YP + (col - n0) * 2) << 16);
        const float yh = (yf - mu) * rs;
        const float dz = act_bwd_from_pre(v, yh * gm + bt, g.bnb_act);
        t0 += dz;
        t1 += dz * yh;
        t2 += yh;
      }
    t0 += __shfl_xor(t0, 16, 64);
    t0 += __shfl_xor(t0, 32, 64);
    t1 += __shfl_xor(t1, 16, 64);
    t1 += __shfl_xor(t1, 32, 64);
    t2 += __shfl_xor(t2, 16, 64);
    t2 += __shfl_xor(t2, 32, 64);
    s0[j] = t0;
    s1[j] = t1;
    s2[j] = t2;
  }
  if (lane < 16) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int cl = wn * 32 + j * 16 + lane;
      red[(0 * 2 + wm) * BN_ + cl] = s0[j];
      red[(1 * 2 + wm) * BN_ + cl] = s1[j];
      red[(2 * 2 + wm) * BN_ + cl] = s2[j];
    }
  }
  __syncthreads();
  const int mt = m0 / 128;
  if (tid < BN_) {
    const int col = n0 + tid;
    if (col < g.N) {
      float* p = g.bnb_ws + ((long long)mt * g.N + col) * 3;
#pragma unroll
      for (int q = 0; q < 3; ++q) st_sc1(p + q, red[(q * 2) * BN_ + tid] + red[(q * 2 + 1) * BN_ + tid]);
    }
  }
  const int nrb = (g.M + 127) / 128;
  return ring_arrive_last(g.bnb_cnt + n0 / BN_, (unsigned)nrb, 1u, flag);
}

// the last-arriving row tile of a column tile: the apply constants and parameter gradients of its
// 128 columns from every row tile's partials (after this workgroup's C stores are issued, so their
// drain overlaps these loads)
__device__ __forceinline__ void ring_bnb_finalize(const GemmArgs& g, int n0, char* smem_raw) {
  constexpr int BN_ = 128, FGR = 4;
  const int tid = threadIdx.x;
  const avcbn::BwdFin& f = g.bnb_fin;
  float* red = reinterpret_cast<float*>(smem_raw);
  const int nrb = (g.M + 127) / 128;
  {
    // 128 columns x FGR row groups, the partials handed over within the launch (sc1 loads)
    const int cl = tid & (BN_ - 1), grp = tid >> 7;
    const int c = n0 + cl;
    const bool cv = c < g.N;
    float sv[3] = {0.f, 0.f, 0.f};
    // 16 partial rows per thread in flight (a sequential loop of sc1 loads had cost ~25 us per conv)
    static_assert(FGR == avcbn::FG, "row groups of strided_sums");
    if (cv) avcbn::strided_sums<3, true, 16>(g.bnb_ws, nrb, g.N, c, grp, sv);
    __syncthreads();
    red[(0 * FGR + grp) * BN_ + cl] = sv[0];
    red[(1 * FGR + grp) * BN_ + cl] = sv[1];
    red[(2 * FGR + grp) * BN_ + cl] = sv[2];
    __syncthreads();
    if (grp == 0 && cv) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
      for (int k = 0; k < FGR; ++k) {
        a0 += red[(0 * FGR + k) * BN_ + cl];
        a1 += red[(1 * FGR + k) * BN_ + cl];
        a2 += red[(2 * FGR + k) * BN_ + cl];
      }
      avcbn::bwd_finalize_store(c, a0, a1, a2, g.M, g.N, f);
    }
  }
}

// Epilogue for the 2 x 4 wave layout (see ring_store_tile): bias and conv0-fold row bias in the
// accumulators, the staged stores, then the BatchNorm partial statistics / finalize.
// BNB: compile the BN-backward reduction (128 x 128 only; yv = the y tile prefetched at kernel start)
// mlim < 0: g.M; the one-utterance conv tile passes the end of its utterance.  BM_ == 192 (that tile)
// computes ONE BatchNorm statistics tile of g.bn_rows rows (both wave rows); otherwise 128-row ones.
template <int BM_, int BN_, bool BNB = false>
__device__ __forceinline__ void ring_epilogue(const GemmArgs& g, f32x4 (&acc)[BM_ / 32][BN_ / 64], int m0, int n0,
                                              int bz, int ks, char* smem_raw, const u32x4* yv = nullptr,
                                              int mlim = -1) {
  constexpr int TWM = BM_ / 2, TWN = BN_ / 4, MI = TWM / 16, NJ = TWN / 16;
  if (mlim < 0) mlim = g.M;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 2, wn = wid & 3;
  const int rbase = m0 + wm * TWM + 4 * (lane >> 4);
  const int cbase = n0 + wn * TWN + (lane & 15);
  if (g.bias && ks == 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = cbase + j * 16;
      const float bv = col < g.N ? g.bias[col] : 0.f;
#pragma unroll
      for (int i = 0; i < MI; ++i) acc[i][j] += bv;
    }
  }
  if (g.rbias && ks == 0) {
    const int T = g.rb_t, pad = g.rb_pad, ncls = 2 * pad + 1;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = rbase + i * 16 + e;
        if (row >= mlim) continue;
        const int b = (int)fdiv((uint32_t)row, g.rb_div), t = row - b * T;
        const int cls = t < pad ? t : (t >= T - pad ? 2 * pad - (T - 1 - t) : pad);
        const float* rp = g.rbias + (long long)(b * ncls + cls) * g.N;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int col = cbase + j * 16;
          if (col < g.N) acc[i][j][e] += rp[col];
        }
      }
  }
  bool bnb_last = false;
  if constexpr (BNB && BM_ == 128 && BN_ == 128) {
    // before the C stores, so the last-arrival wait covers the partials only
    if (g.bnb_ws) bnb_last = ring_bnb_epilogue(g, acc, m0, n0, smem_raw, yv);
  }
  ring_store_tile<BM_, BN_>(g, acc, m0, n0, bz, ks, smem_raw, mlim);
  if constexpr (BNB && BM_ == 128 && BN_ == 128) {
    if (bnb_last) {
      __syncthreads();  // the staged stores are done with the LDS
      ring_bnb_finalize(g, n0, smem_raw);
    }
  }
  if (g.bn_partial) {
    // per 128-row statistics tile: column sum and M2 about the tile mean (Chan's form, merged by
    // the finalize).  Waves w with (w's rows)/128 == h contribute to tile h of this workgroup.
    constexpr bool UTT = BM_ == 192;              // one statistics tile of g.bn_rows rows
    constexpr int NH = UTT ? 1 : BM_ / 128;       // statistics tiles per workgroup tile
    constexpr int WPT = UTT ? 2 : 128 / TWM;      // waves (along M) per statistics tile
    const int srows = UTT ? g.bn_rows : 128;
    float* red = reinterpret_cast<float*>(smem_raw);  // [2][BN_] sums, then [2][BN_] M2
    float* red2 = red + 2 * BN_;
    unsigned* flag = reinterpret_cast<unsigned*>(red2 + 2 * BN_);
    const int h = wm / WPT;
    const int cnt = max(1, min(srows, mlim - (m0 + srows * h)));
    float s[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      float t = 0.f;
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) t += (rbase + i * 16 + e < mlim) ? acc[i][j][e] : 0.f;
      t += __shfl_xor(t, 16, 64);
      t += __shfl_xor(t, 32, 64);
      s[j] = t;
    }
    __syncthreads();  // the main loop's last fragment reads of LDS are done
    if (lane < 16) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) red[wm * BN_ + wn * TWN + j * 16 + lane] = s[j];
    }
    __syncthreads();
    float qv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int cl = wn * TWN + j * 16 + (lane & 15);
      float tot = 0.f;
#pragma unroll
      for (int w = 0; w < WPT; ++w) tot += red[(h * WPT + w) * BN_ + cl];
      const float mean = tot / (float)cnt;
      float t = 0.f;
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = acc[i][j][e] - mean;
          t += (rbase + i * 16 + e < mlim) ? d * d : 0.f;
        }
      t += __shfl_xor(t, 16, 64);
      t += __shfl_xor(t, 32, 64);
      qv[j] = t;
    }
    if (lane < 16) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) red2[wm * BN_ + wn * TWN + j * 16 + lane] = qv[j];
    }
    __syncthreads();
    const int mt0 = m0 / srows;
    if (tid < NH * BN_) {
      const int hh = tid / BN_, cl = tid - hh * BN_;
      const int col = n0 + cl;
      if (col < g.N && m0 + srows * hh < g.M) {
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int w = 0; w < WPT; ++w) {
          s0 += red[(hh * WPT + w) * BN_ + cl];
          s1 += red2[(hh * WPT + w) * BN_ + cl];
        }
        float* p = g.bn_partial + ((long long)(mt0 + hh) * g.N + col) * 2;
        if (g.bn_cnt) {
          st_sc1(p, s0);
          st_sc1(p + 1, s1);
        } else {
          p[0] = s0;
          p[1] = s1;
        }
      }
    }
    if (g.bn_cnt) {
      const int ntile = (g.M + srows - 1) / srows;
      const int mine = min(NH, ntile - mt0);
      unsigned* cnt = g.bn_cnt + n0 / BN_;
      if (ring_arrive_last(cnt, (unsigned)ntile, (unsigned)mine, flag)) bn_finalize_cols<BN_>(g, n0, red);
    }
  }
}

}  // namespace avcg
