// gemm_ring.hip — bf16 NT GEMM with a deep LDS-DMA ring, eight waves, one workgroup per CU.
//
// C[M][N] = A[M][K] . B[N][K]^T (fp32 accumulate) for the products whose operands are both
// K-contiguous: the MetaConv MLP-Mixer token / channel mixing (factory/MLPMixer.py:58-92,
// factory/MetaConv.py:23-76), the decoder LSTM input projections and data gradients
// (factory/AutoVC.py:96,103,110), and the Conv1d window stream (factory/Norm.py:21-28: A is the
// frame window of the conv input, K = tap x channel, zero outside the utterance).
//
// Why a new kernel: the 4-wave, two-stage kernels of gemm_nt.hip /
// gemm_conv.hip keep ONE LDS-DMA fill in flight per workgroup and two workgroups per CU; their
// times match the ≈25 GB/s-per-CU fill rate of that regime (MI355X_MICROARCH.md
// "ldsdma-fill"), not the MFMA rate.  Here:
//   * one 512-thread workgroup per CU, 8 waves as 2 (M) x 4 (N), so every SIMD holds two waves
//     that cover each other's LDS-read latency (MI355X_MICROARCH.md "Two waves per SIMD");
//   * a ring of NST K-steps (BK = 64, 128-B LDS rows) with NST-1 K-steps of fills in flight
//     ACROSS the barrier: a counted `s_waitcnt vmcnt` + raw `s_barrier` per K-step, never
//     vmcnt(0) inside the loop (cdna_hip_programming.md §5 "Pipelining across barriers");
//     every wave issues the same number of 16-B LDS-DMA fills (glds16) per K-step (the counts
//     assume it), rows beyond the operand read a 16-B zero granule;
//   * 128 x 128 (4 slots, 3 in flight), 256 x 128 (3 slots) or 256 x 256 tiles (2 slots; half
//     the operand bytes per FLOP of a 128 x 128 tile);
//   * XOR-swizzled 16-B chunks (chunk ^ ((row >> 1) & 7), applied on the SOURCE address, the
//     LDS image stays lane-linear), conflict-free ds_read_b128 fragment reads;
//   * XCD-aware bijective block remap, then grouped tile order (GM row tiles per group) so the
//     workgroups an XCD runs together share A row panels and B column panels in its L2;
//   * all LDS in ONE __shared__ array (a second __shared__ object can make hipcc drain vmcnt
//     before every K-step's first ds_read: cdna_hip_programming.md §5 item 4(a)); the
//     last-arriver flag of the BN finalize lives in that array too.
// The epilogue (ring_internal.h:ring_epilogue, shared with the halo conv of conv_ring.hip): bias,
// conv0-fold row bias, residual, accumulate, fp32 C and / or bf16 twin, the GELU, column-sum and
// transposed-store forms, BatchNorm partial statistics per 128-row tile and the finalize by the
// last-arriving row tile (the semantics of gemm_internal.h:fast_epilogue).
//
// This file: the operand loader, gemm_ring_kernel and its launcher, the tile cost model, the
// dispatcher of both ring families (gemm_ring_launch) and the two extern "C" hooks.
#include <algorithm>
#include <type_traits>

#include "ring_internal.h"

namespace avcg {
namespace {

// R rows x 64 K of one operand per slot: R/64 glds per thread.  Instruction i of wave w covers
// slot rows (8i + w)*8 .. +8; lane L writes row +(L>>3), 16-B slot L&7, which holds global K
// chunk (L&7) ^ ((row>>1)&7) = (L&7) ^ ((4*(w&1) + (L>>4)) & 7) for every i.
template <int R, bool WIN>
struct RingLoader {
  static constexpr int NI = R / 64;
  const bf16* base;
  long long roff[NI];  // element offset of the row (plain) / of the row's frame (window)
  int tt[NI];          // window: frame within the utterance
  bool rok[NI];
  int kc;              // this lane's K offset inside the 64-wide slot
  int ld, pad, t_in, chans;
  const void* zp;      // the 16-B zero granule, held in VGPRs (see init)

  __device__ __forceinline__ void init(const OpDev& o, int row0, int bz) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    base = reinterpret_cast<const bf16*>(o.ptr) + (long long)bz * o.bstride;
    // the zero granule's address pinned in a VGPR pair once: referenced per glds, hipcc had
    // re-materialised it from the GOT (s_getpc + s_load + lgkmcnt(0)) before every fill under
    // SGPR pressure
    zp = (const void*)g_zero16;
    asm volatile("" : "+v"(zp));
    kc = 8 * ((lane & 7) ^ ((4 * (w & 1) + (lane >> 4)) & 7));
    ld = (int)o.ld;
    pad = o.pad;
    t_in = o.t_in;
    chans = o.chans;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int r = row0 + (8 * i + w) * 8 + (lane >> 3);
      rok[i] = r < o.rows;
      const int rr = rok[i] ? r : 0;
      if (WIN) {
        const int b = (int)fdiv((uint32_t)rr, o.tdiv);
        tt[i] = rr - b * o.t_out;
        roff[i] = (long long)(b * o.t_in + tt[i]) * o.ld;
      } else {
        tt[i] = 0;
        roff[i] = (long long)rr * o.ld;
      }
    }
  }

  __device__ __forceinline__ void issue(char* lds, int kbase, int kend, const FastDiv& cdv) {
    const int w = threadIdx.x >> 6;
    const int k = kbase + kc;
    const bool kok = k < kend;
    int tap = 0, cc = k;
    if (WIN) {
      tap = (int)fdiv((uint32_t)k, cdv);
      cc = k - tap * chans;
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      bool ok = kok && rok[i];
      long long off;
      if (WIN) {
        const int t2 = tt[i] + tap - pad;
        ok = ok && t2 >= 0 && t2 < t_in;
        off = roff[i] + (long long)(tap - pad) * ld + cc;
      } else {
        off = roff[i] + k;
      }
      glds16(ok ? (const void*)(base + off) : zp, lds + (8 * i + w) * 8 * RROW);
    }
  }
};

template <int BM_, int BN_, int NST, bool WIN>
__global__ void __launch_bounds__(RNT, 2) gemm_ring_kernel(GemmArgs g, int gm) {
  constexpr int TWM = BM_ / 2, TWN = BN_ / 4, MI = TWM / 16, NJ = TWN / 16;
  constexpr int A_BYTES = BM_ * RROW, STAGE = (BM_ + BN_) * RROW;
  constexpr int LPT = BM_ / 64 + BN_ / 64;  // glds per thread per K-step
  constexpr int P = NST - 1;                // K-steps in flight
  static_assert(NST >= 2 && NST <= 4, "ring depth");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 2, wn = wid & 3;

  // XCD-aware bijective remap (blocks b, b+8, ... share an XCD) ...
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  // ... then grouped order: gm row tiles x all column tiles per group, row tile fastest
  const int nN = (g.N + BN_ - 1) / BN_, nM = (g.M + BM_ - 1) / BM_;
  const int z = lid / (nN * nM);
  const int rem = lid - z * nN * nM;
  const int grp = rem / (gm * nN);
  const int fm = grp * gm;
  const int gsz = min(nM - fm, gm);
  const int wi = rem - grp * gm * nN;
  const int mt = fm + wi % gsz, nt = wi / gsz;
  const int m0 = mt * BM_, n0 = nt * BN_;
  const int bz = z / g.split_k, ks = z - bz * g.split_k;
  const int kbeg = ks * g.klen;
  const int kend = min(g.K, kbeg + g.klen);
  const int nkt = kend > kbeg ? (kend - kbeg + RBK - 1) / RBK : 0;

  RingLoader<BM_, WIN> la;
  RingLoader<BN_, false> lb;
  la.init(g.a, m0, bz);
  lb.init(g.b, n0, bz);
  const FastDiv cdv = g.a.cdv;

  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment reads: row (lane&15) of each 16-row block, logical chunk 4h + (lane>>4) stored at
  // chunk ^ ((row>>1)&7) = chunk ^ ((lane&15)>>1) (block bases are multiples of 16 rows)
  const int frow = lane & 15, sw = frow >> 1;
  const int ch0 = ((lane >> 4) ^ sw) << 4, ch1 = ((4 + (lane >> 4)) ^ sw) << 4;
  const int aoff = (wm * TWM + frow) * RROW, boff = A_BYTES + (wn * TWN + frow) * RROW;

#pragma unroll
  for (int p = 0; p < P; ++p)
    if (p < nkt) {
      char* st = smem_raw + p * STAGE;
      la.issue(st, kbeg + p * RBK, kend, cdv);
      lb.issue(st + A_BYTES, kbeg + p * RBK, kend, cdv);
    }

  for (int kt = 0; kt < nkt; ++kt) {
    ring_wait<P, LPT>(min(P - 1, nkt - 1 - kt));  // K-steps allowed to stay in flight
    raw_barrier();
    if (kt + P < nkt) {
      char* st = smem_raw + ((kt + P) % NST) * STAGE;
      la.issue(st, kbeg + (kt + P) * RBK, kend, cdv);
      lb.issue(st + A_BYTES, kbeg + (kt + P) * RBK, kend, cdv);
    }
    // One K-step = two 32-deep halves h; fragments read by inline asm with counted waits so that
    // the next group's reads are in flight while the current group's MFMAs issue (hipcc's own
    // schedule re-used one register set and drained lgkmcnt(0) before every MFMA group):
    //   read B(h0), A(h0) rows 0..MI/2, A(h0) rows MI/2..MI | MFMA h0 first half
    //   read B(h1), A(h1) first half                       | MFMA h0 second half
    //   read A(h1) second half                             | MFMA h1 first half | MFMA h1 second half
    constexpr int MH = MI / 2;
    const unsigned st = lds_addr(smem_raw + (kt % NST) * STAGE);
    const unsigned a0 = st + aoff + ch0, a1 = st + aoff + ch1, b0 = st + boff + ch0, b1 = st + boff + ch1;
    bf16x8 af0[MI], bf0[NJ], af1[MI], bf1[NJ];
    auto mfma_rows = [&](const bf16x8* af, const bf16x8* bfr, auto i0c) {
      constexpr int I0 = decltype(i0c)::value;
#pragma unroll
      for (int i = 0; i < MH; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[I0 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[I0 + i], bfr[j], acc[I0 + i][j], 0, 0, 0);
    };
    using Z0 = std::integral_constant<int, 0>;
    using ZH = std::integral_constant<int, MH>;
    ds_read_n<NJ, 16 * RROW>(bf0, b0);
    ds_read_n<MH, 16 * RROW>(af0, a0);
    ds_read_n<MH, 16 * RROW, MH * 16 * RROW>(af0 + MH, a0);
    wait_lgkm<MH>();
    mfma_rows(af0, bf0, Z0{});
    __builtin_amdgcn_sched_barrier(0);
    ds_read_n<NJ, 16 * RROW>(bf1, b1);
    ds_read_n<MH, 16 * RROW>(af1, a1);
    wait_lgkm<NJ + MH>();
    mfma_rows(af0, bf0, ZH{});
    __builtin_amdgcn_sched_barrier(0);
    ds_read_n<MH, 16 * RROW, MH * 16 * RROW>(af1 + MH, a1);
    wait_lgkm<MH>();
    mfma_rows(af1, bf1, Z0{});
    wait_lgkm<0>();
    mfma_rows(af1, bf1, ZH{});
  }
  __syncthreads();  // every glds retired (the last wait was vmcnt(0)) and every fragment read done
  ring_epilogue<BM_, BN_>(g, acc, m0, n0, bz, ks, smem_raw);
}

template <int BM_, int BN_, int NST, bool WIN>
void launch(const GemmArgs& g, int gm, hipStream_t s) {
  const size_t lds = std::max((size_t)NST * (BM_ + BN_) * RROW, ring_epi_lds<BM_, BN_>());
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_ring_kernel<BM_, BN_, NST, WIN>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr = true;
  }
  const int nb = ((g.M + BM_ - 1) / BM_) * ((g.N + BN_ - 1) / BN_) * g.batch * g.split_k;
  gemm_ring_kernel<BM_, BN_, NST, WIN><<<nb, RNT, lds, s>>>(g, gm);
}

bool ok16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

bool operand_ok(const OpDev& o, bool allow_win) {
  if (o.dtype != AVC_BF16 || !ok16(o.ptr) || o.ld % 8 || o.bstride % 8) return false;
  if (o.win && (!allow_win || o.chans % 8)) return false;
  return true;
}

// the configuration (ring_internal.h:RingCfg) from AVC_RING / AVC_RING_WIN
RingCfg init_cfg() {
  RingCfg r;
  if (const char* e = getenv("AVC_RING")) {
    int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    const int n = sscanf(e, "%d,%d,%d,%d", &a0, &a1, &a2, &a3);
    if (n >= 1 && a0 <= 0) r.mode = a0 < 0 ? -1 : 0;
    if (n >= 3) {
      r.mode = 1;
      r.bm = a0;
      r.bn = a1;
      r.nst = a2;
    }
    if (n >= 4 && a3 > 0) r.gm = a3;
  }
  if (const char* e = getenv("AVC_RING_WIN")) r.win = atoi(e);
  return r;
}
RingCfg g_ring = init_cfg();

}  // namespace

thread_local int g_ring_last = 0;  // avc_gemm_ring_last

int ring_num_cus() {
  static int n = [] {
    int dev = 0;
    hipDeviceProp_t p;
    return (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) ? p.multiProcessorCount
                                                                                                : 0;
  }();
  return n;
}

bool gemm_ring_launch(const GemmArgs& g, hipStream_t s) {
  g_ring_last = 0;
  const RingCfg& c = g_ring;
  if (c.mode == 0 || (g.a.win && !c.win)) return false;
  if (g.K % 8 || g.klen % RBK || g.atomic || g.cperm) return false;  // (no atomic / cperm stores)
  if (g.ctr && ((reinterpret_cast<uintptr_t>(g.c) & 15) || (reinterpret_cast<uintptr_t>(g.res) & 15) ||
                (g.cbs & 3)))
    return false;  // the transposed stores are 16-B vectors
  if (!operand_ok(g.a, true) || !operand_ok(g.b, false)) return false;
  const long long units = (long long)g.batch * g.split_k;
  const bool win = g.a.win != 0;
  // what the halo conv kernel (conv_ring.hip, win == 2) takes: 5-tap 'same' convs on 32-channel
  // stages, one unsplit product with a plain B
  const OpDev& a = g.a;
  const int T = a.t_out;
  const bool halo_shape = win && c.win == 2 && a.taps == CV_TAPS && a.t_in == T && 2 * a.pad == a.taps - 1 &&
                          g.K == a.taps * a.chans && a.chans % CV_CBK == 0 && g.batch == 1 && g.split_k == 1 &&
                          !g.b.win;
  // its 128-row tiles: utterance-aligned only unless forced (T % 128 != 0 leaves 1.4 tiles per CU at
  // B=64 T=176, where the 128 x 64 tiles of gemm_conv.hip spread better -- profiles/r4_ring_ab.txt)
  const bool halo = halo_shape && (c.mode == 1 || (T % CV_TM == 0 && g.N >= 128));
  // the BatchNorm-backward reduction epilogue (avc_gemm_bnb) exists on the halo conv tile only, for a
  // bf16 y (ring_bnb_epilogue)
  if (g.bnb_ws && !(halo && g.bnb_ydt == AVC_BF16 && g.N % 8 == 0 && g.ldc % 8 == 0 &&
                    (reinterpret_cast<uintptr_t>(g.bnb_y) & 15) == 0 && !g.c16_act && !g.agrad && !g.csum))
    return false;
  // one utterance per row tile (T = 176 of C4 / C5): the 192-row tile, when every epilogue it has is
  // one the 2 x 4 ring epilogue covers (no BN-backward / GELU / column-sum / transposed stores) and
  // the forward BatchNorm statistics are finalized in the kernel (their tiles are T rows, which
  // only bn_finalize_cols is told)
  const bool utt = halo_shape && c.mode != 1 && T > CV_TM && T <= CU_TM && g.M % T == 0 && g.N >= 128 && !g.bnb_ws &&
                   !g.c16_act && !g.agrad && !g.csum && !g.ctr && (!g.bn_partial || g.bn_cnt) && c.utt;
  if (utt || halo) {
    conv_ring_launch(g, utt, c.gm, s);
    g_ring_last = utt ? 3 : 2;
    return true;
  }
  int bm, bn, nst;
  if (c.mode == 1) {
    bm = c.bm;
    bn = c.bn;
    nst = c.nst;
  } else {
    // Tile choice by a wave-quantised cost model: a configuration runs occ workgroups per CU, so
    // a product costs ceil(tiles / (256 occ)) rounds of BM*BN*K work at the configuration's per-flop
    // efficiency (1 : 0.85 : 0.75 for 256x256 / 256x128 / 128x128, fitted to the per-call census
    // of the C2 / C4 steps, tools/gemm_census.py --ring-ab, profiles/r4_gemm_census_*.txt).  Every
    // plain bf16 NN product of those steps ran as fast or faster on the chosen ring tile than on
    // gemm_nt.hip.  Conv windows: the generic window stream only for channel counts the halo form
    // cannot take (344 / 88 / 80 channels) and N <= 512, where it measured faster than
    // gemm_conv.hip; the rest stay on gemm_conv.hip.
    if (win && (g.N > 512 || a.chans % CV_CBK == 0)) return false;
    // 128x128x2 (64 KB of LDS) runs TWO workgroups per CU, one's epilogue under the other's K loop:
    // 512 concurrent tiles at efficiency 0.47, 0.38 under the GELU-backward epilogue (its extra
    // operand stream) -- fitted to the same census with that tile forced (profiles/r4_gemm_census_x2_c*.txt)
    struct Opt {
      int bm, bn, nst, occ;
      double eff;
    };
    const Opt opts[4] = {{256, 256, 2, 1, 1.0}, {256, 128, 3, 1, 0.85}, {128, 128, 4, 1, 0.75},
                         {128, 128, 2, 2, g.agrad ? 0.38 : 0.47}};
    double best = 0;
    bm = 0;
    bn = 0;
    nst = 0;
    for (const Opt& o : opts) {
      const long long tiles = (long long)((g.M + o.bm - 1) / o.bm) * ((g.N + o.bn - 1) / o.bn) * units;
      const long long slots = 256ll * o.occ;
      const double cost = (double)((tiles + slots - 1) / slots) * o.bm * o.bn / o.eff;
      if (!bm || cost < best * 0.999) {
        best = cost;
        bm = o.bm;
        bn = o.bn;
        nst = o.nst;
      }
    }
  }
#define RING_CASE(BMV, BNV, NSV)                       \
  if (bm == BMV && bn == BNV && nst == NSV) {          \
    if (win) launch<BMV, BNV, NSV, true>(g, c.gm, s);  \
    else launch<BMV, BNV, NSV, false>(g, c.gm, s);     \
    g_ring_last = 1;                                   \
    return true;                                       \
  }
  RING_CASE(256, 256, 2) RING_CASE(256, 128, 3) RING_CASE(128, 128, 4) RING_CASE(128, 128, 3)
  RING_CASE(128, 256, 3) RING_CASE(256, 128, 2) RING_CASE(128, 128, 2)  // (128x128x2: 64 KB, two per CU)
#undef RING_CASE
  return false;
}

}  // namespace avcg

extern "C" int avc_gemm_ring_last(void) { return avcg::g_ring_last; }

// Benchmarking hook (tools/ring_ab.py): mode -1 auto, 0 off, 1 forced (bm, bn, nst); gm row
// tiles per group (<= 0 keeps it); win: as AVC_RING_WIN.
extern "C" int avc_gemm_set_ring(int mode, int bm, int bn, int nst, int gm, int win) {
  avcg::g_ring.mode = mode;
  avcg::g_ring.bm = bm;
  avcg::g_ring.bn = bn;
  avcg::g_ring.nst = nst;
  if (gm > 0) avcg::g_ring.gm = gm;
  avcg::g_ring.win = win >= 3 ? 2 : win;
  // 10: the halo convs without the one-utterance tile (T = 176 back on gemm_conv.hip); any other
  // value restores the default
  avcg::g_ring.utt = win != 10;
  return 0;
}
