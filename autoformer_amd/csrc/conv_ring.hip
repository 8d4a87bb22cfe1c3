// conv_ring.hip — the halo Conv1d of the eight-wave ring family: 5 taps, stride 1, 'same' padding,
// bf16, with the input tile staged ONCE for all taps (factory/Norm.py:21-28).
//
// X = activation, W = Wf[co][tap][ci] (forward) or dy and Wd[ci][tap'][co] (data gradient).  One
// 512-thread workgroup per tile, 8 waves as 2 (M) x 4 (N), stages of CV_CBK = 32 channels: the halo
// (TM frames + 4, 64-B rows) and the five 128-column weight slices (640 rows x 64 B).  Tap k reads
// the halo k rows down.  The fill instructions of a stage (16 rows each) are dealt over the 8 waves,
// so the low waves issue one more than the others: the counted waits use each wave's own count.
// One kernel template, conv_ring_kernel<TM, NST, ALIGNED, BNB>, in two tile forms:
//   * TM = 128: 128 frames x 128 columns (the one tile that gives each of the 256 CUs a tile of the
//     AutoVC 8192 x 512 convs), waves of 64 x 32; 9 halo + 40 weight instructions = 49 KiB per
//     stage, TWO stages (98 KiB) rather than three (147 KiB): alone the same time (29.0 vs 28.6 us
//     at 8192 x 512 x 2560), but a side-stream weight-gradient workgroup (48 KiB) now fits on a CU
//     beside it, so a backward conv no longer waits for those to drain from its CUs: C2 5.78-5.80
//     -> 5.74-5.75 ms (profiles/r5_conv_ring_slope.txt).
//     ALIGNED (T % 128 == 0): a tile never spans two utterances, so the loader zero-fills the halo
//     rows of other utterances and the fragments need no per-lane predicate; otherwise a per-lane,
//     per-tap mask zeroes the A fragment rows whose shifted frame leaves the utterance.
//     BNB: the BatchNorm-backward reduction epilogue (avc_gemm_bnb) compiled in, its y tile
//     prefetched at kernel start.
//   * TM = 192: ONE UTTERANCE per row tile (128 < T <= 192, T = 176 for C4 / C5), waves of 96 x 32
//     (6 x 2 MFMA blocks); rows T .. 191 are computed from zero halo rows and never stored, so
//     B = 64 utterances x 4 column tiles = 256 tiles = one round of the CUs (128-row tiles number
//     352 at T = 176: two rounds, no faster than gemm_conv.hip).  13 halo + 40 weight instructions
//     = 53 KiB per stage, THREE stages = 159 KiB (two: 106 KiB, room for a side-stream workgroup
//     beside it -- measured no faster, profiles/r5_conv_ring_slope.txt).  A tile is its utterance,
//     so it needs no mask (ALIGNED); it has no BatchNorm-backward form; the BatchNorm statistics of
//     the forward come as one T-row tile per workgroup (GemmArgs::bn_rows = T, merged by
//     bn_finalize_cols).
// The epilogue is ring_internal.h's.  This file: the kernel, its launcher and conv_ring_launch,
// the entry the dispatcher of gemm_ring.hip calls.
#include <algorithm>
#include <type_traits>

#include "ring_internal.h"

namespace avcg {
namespace {

constexpr int CV_NST = 2, CU_NST = 3;  // LDS stages of the 128-row / 192-row form

// stage layout of a TM-row tile: fill instruction qi writes stage bytes [qi KiB, +1 KiB) = 16 rows of 64 B
template <int TM>
struct ConvTile {
  static constexpr int MI = TM / 32, NJ = 2;                  // 16 x 16 MFMA blocks per wave
  static constexpr int AI = (TM + CV_TAPS - 1 + 15) / 16;     // halo instructions: 9 | 13
  static constexpr int BI = CV_TAPS * CV_TN / 16;             // 40 weight instructions
  static constexpr int TOT = AI + BI;                         // 49 | 53
  static constexpr int LW = (TOT + 7) / 8;                    // 7: instructions of waves < TOT % 8
  static constexpr int ABYTES = AI * 1024, STAGE = TOT * 1024;
};

// one stage of this wave's fills may stay in flight: LW of them, or LW - 1 on the high waves
template <int LW>
__device__ __forceinline__ void wait_conv(bool full) {
  if (full) wait_vm<LW>();
  else wait_vm<LW - 1>();
}

template <int TM, int NST, bool ALIGNED, bool BNB>
__global__ void __launch_bounds__(RNT, 2) conv_ring_kernel(GemmArgs g, int gm) {
  using C = ConvTile<TM>;
  constexpr bool UTT = TM == CU_TM;  // one utterance per row tile
  static_assert(TM == CV_TM || (UTT && ALIGNED && !BNB), "tile form");
  constexpr int MI = C::MI, NJ = C::NJ, P = NST - 1;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 2, wn = wid & 3;
  const bool full = wid < (C::TOT % 8 ? C::TOT % 8 : 8);  // this wave issues C::LW per stage

  // XCD remap, then grouped order: gm row tiles x all column tiles per group, row tile fastest
  const OpDev& A = g.a;
  const OpDev& Bo = g.b;
  const int T = A.t_out;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int nN = (g.N + CV_TN - 1) / CV_TN, nM = UTT ? g.M / T : (g.M + TM - 1) / TM;
  const int grp = lid / (gm * nN), fm = grp * gm, gsz = min(nM - fm, gm);
  const int wi = lid - grp * gm * nN;
  const int mt = fm + wi % gsz, nt = wi / gsz;
  const int m0 = mt * (UTT ? T : TM), n0 = nt * CV_TN;

  const bf16* xa = reinterpret_cast<const bf16*>(A.ptr);
  const bf16* wb = reinterpret_cast<const bf16*>(Bo.ptr);
  const int pad = A.pad, chans = A.chans;
  const int nst = chans / CV_CBK;

  // ---- loader: instruction qi = i*8 + wid (i < C::LW, qi < C::TOT) writes stage bytes
  // [qi KiB, +1 KiB) = rows 16*qi + (lane>>2) of 64 B, 16-B slot lane&3 holding the global chunk
  // (lane&3) ^ ((row>>1)&3)
  const int b0 = (int)fdiv((uint32_t)m0, A.tdiv);  // utterance of the tile's first row
  // a lane whose row is padding reads the 16-B zero granule at every stage (stride 0): no select
  // in the issue loop, and the granule's address pinned in VGPRs (hipcc had re-loaded it from the
  // GOT, s_load + lgkmcnt(0), before every fill: 30 per stage loop)
  const bf16* zp = reinterpret_cast<const bf16*>(g_zero16);
  asm volatile("" : "+v"(zp));
  const bf16* src[C::LW];
  long long sst[C::LW];  // elements per stage
#pragma unroll
  for (int i = 0; i < C::LW; ++i) {
    const int qi = i * 8 + wid;
    const int lrow = lane >> 2, slot = lane & 3;
    src[i] = zp;
    sst[i] = 0;
    if (qi < C::AI) {
      const int hr = 16 * qi + lrow;  // halo row
      int f;                          // its frame
      bool ok;
      if constexpr (UTT) {
        const int t = hr - pad;  // frame within the utterance
        ok = t >= 0 && t < T;
        f = m0 + t;
      } else {
        f = m0 - pad + hr;
        ok = hr < TM + CV_TAPS - 1 && f >= 0 && f < g.M;
        if (ALIGNED && ok) ok = (int)fdiv((uint32_t)f, A.tdiv) == b0;
      }
      if (ok) {
        src[i] = xa + (long long)f * A.ld + 8 * (slot ^ ((hr >> 1) & 3));
        sst[i] = CV_CBK;
      }
    } else if (qi < C::TOT) {
      const int wr = 16 * (qi - C::AI) + lrow;  // weight row = tap * 128 + column
      const int tap = wr / CV_TN, n = n0 + (wr - tap * CV_TN);
      if (n < g.N) {
        src[i] = wb + (long long)n * Bo.ld + (long long)tap * chans + 8 * (slot ^ ((wr >> 1) & 3));
        sst[i] = CV_CBK;
      }
    }
  }
  auto issue = [&](int stg, int cs) {
    char* base = smem_raw + stg * C::STAGE;
#pragma unroll
    for (int i = 0; i < C::LW; ++i) {
      const int qi = i * 8 + wid;
      if (qi < C::TOT) glds16(src[i] + cs * sst[i], base + qi * 1024);
    }
  };

  // ---- fragments: A row (halo) wm*TM/2 + i*16 + frow + k, chunk (lane>>4) ^ ((row>>1)&3); rows
  // 16 apart share the swizzle, so i is an immediate offset of 1 KiB.  B row k*128 + wn*32 + j*16 +
  // frow: its swizzle is ((frow>>1)&3), the (k, j) part an immediate offset.
  const int frow = lane & 15, kq = lane >> 4;
  int aaddr[CV_TAPS];
#pragma unroll
  for (int k = 0; k < CV_TAPS; ++k) {
    const int r = wm * (TM / 2) + frow + k;
    aaddr[k] = r * 64 + 16 * (kq ^ ((r >> 1) & 3));
  }
  const int baddr = C::ABYTES + (wn * 32 + frow) * 64 + 16 * (kq ^ ((frow >> 1) & 3));
  unsigned vmask = 0xFFFFFFFFu;
  if (!ALIGNED) {
    vmask = 0;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int m = min(m0 + wm * (TM / 2) + i * 16 + frow, g.M - 1);
      const int b = (int)fdiv((uint32_t)m, A.tdiv);
      const int t = m - b * T;
#pragma unroll
      for (int k = 0; k < CV_TAPS; ++k) {
        const int t2 = t + k - pad;
        if (t2 >= 0 && t2 < T) vmask |= 1u << (i * 8 + k);
      }
    }
  }

  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 af[2][MI], bfr[2][NJ];
  u32x4 bnb_y[BNB ? BNB_YQ : 1];
  if constexpr (BNB) {
    if (g.bnb_ws) ring_bnb_prefetch(g, m0, n0, bnb_y);
  }

#pragma unroll
  for (int p = 0; p < P; ++p)
    if (p < nst) issue(p, p);

  for (int cs = 0; cs < nst; ++cs) {
    const int ahead = min(P - 1, nst - 1 - cs);
    if (ahead >= 1) wait_conv<C::LW>(full);
    else wait_vm<0>();
    raw_barrier();
    if (cs + P < nst) issue((cs + P) % NST, cs + P);
    const unsigned st = lds_addr(smem_raw + (cs % NST) * C::STAGE);
    auto read_tap = [&](auto kc, int slot) {
      constexpr int k = decltype(kc)::value;
      ds_read_n<MI, 1024>(af[slot], st + aaddr[k]);
      ds_read_n<NJ, 16 * 64, k * CV_TN * 64>(bfr[slot], st + baddr);
    };
    auto mfma_tap = [&](auto kc, int slot) {
      constexpr int k = decltype(kc)::value;
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const bf16x8 av = (ALIGNED || ((vmask >> (i * 8 + k)) & 1u)) ? af[slot][i] : bf16x8{};
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bfr[slot][j], acc[i][j], 0, 0, 0);
      }
    };
    // Software pipeline with inline-asm fragment reads and counted waits: tap k+1's MI + NJ reads
    // are in flight while tap k's MI * NJ MFMAs issue (the wave waits only for tap k's reads).  Left
    // to itself hipcc re-used one register set and waited lgkmcnt(0) twice per tap -- two exposed
    // LDS round trips per tap, 23.5 us of the 128-row conv in its reads + MFMAs alone
    // (profiles/r5_conv_ring_slope.txt).
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
    using I4 = std::integral_constant<int, 4>;
    read_tap(I0{}, 0);
    read_tap(I1{}, 1);
    wait_lgkm<MI + NJ>();
    mfma_tap(I0{}, 0);
    __builtin_amdgcn_sched_barrier(0);
    read_tap(I2{}, 0);
    wait_lgkm<MI + NJ>();
    mfma_tap(I1{}, 1);
    __builtin_amdgcn_sched_barrier(0);
    read_tap(I3{}, 1);
    wait_lgkm<MI + NJ>();
    mfma_tap(I2{}, 0);
    __builtin_amdgcn_sched_barrier(0);
    read_tap(I4{}, 0);
    wait_lgkm<MI + NJ>();
    mfma_tap(I3{}, 1);
    wait_lgkm<0>();
    mfma_tap(I4{}, 0);
  }
  __syncthreads();
  if constexpr (UTT) ring_epilogue<TM, CV_TN>(g, acc, m0, n0, 0, 0, smem_raw, nullptr, m0 + T);
  else ring_epilogue<TM, CV_TN, BNB>(g, acc, m0, n0, 0, 0, smem_raw, bnb_y);
}

template <int TM, int NST, bool ALIGNED, bool BNB>
void launch_conv(const GemmArgs& g0, int gm, hipStream_t s) {
  constexpr bool UTT = TM == CU_TM;
  GemmArgs g = g0;
  if (UTT) g.bn_rows = g.a.t_out;  // one statistics tile per utterance
  const size_t lds = std::max((size_t)NST * ConvTile<TM>::STAGE, ring_epi_lds<TM, CV_TN>());
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_ring_kernel<TM, NST, ALIGNED, BNB>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr = true;
  }
  const int nb = (UTT ? g.M / g.a.t_out : (g.M + TM - 1) / TM) * ((g.N + CV_TN - 1) / CV_TN);
  conv_ring_kernel<TM, NST, ALIGNED, BNB><<<nb, RNT, lds, s>>>(g, gm);
}

}  // namespace

void conv_ring_launch(const GemmArgs& g, bool utt, int gm, hipStream_t s) {
  const bool aligned = g.a.t_out % CV_TM == 0;
  if (utt) launch_conv<CU_TM, CU_NST, true, false>(g, gm, s);
  else if (g.bnb_ws) {  // the BN-backward reduction epilogue
    if (aligned) launch_conv<CV_TM, CV_NST, true, true>(g, gm, s);
    else launch_conv<CV_TM, CV_NST, false, true>(g, gm, s);
  } else if (aligned) launch_conv<CV_TM, CV_NST, true, false>(g, gm, s);
  else launch_conv<CV_TM, CV_NST, false, false>(g, gm, s);
}

}  // namespace avcg
