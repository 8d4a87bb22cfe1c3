// lstm_persist.hip — one LSTM layer as ONE persistent launch for all T steps (bf16 compute, one
// direction, H in {512, 768, 1024}: decoder lstm1, the Adjust variants, single lstm2 layers),
// forward and backward, plus the lstm1 code-fold entry points.  Groups, members and the
// inter-workgroup hand-off (flag form and granule form) are described in lstm_internal.h.
#include "lstm_internal.h"

namespace {
using namespace avcl;

// Hand-off form of the forward (measured): granules where a consumer's
// granule payload is at most 16 KB -- H <= 512 (lstm1: 2.24 -> 1.74 us per step) -- and the flag
// form above that (H = 1024 forward 3.08 vs 3.26 us: the doubled payload fetch costs more than
// the drain and the flag round trip it saves).  The backward always takes the flag form: its
// payload is 4H wide (H = 1024: 4.03 vs 4.43 us; H = 512, 64 KB of granules per consumer:
// C2 5.50 vs 5.53-5.55 ms, profiles/r6_gran_bwd512_ab.txt).
constexpr bool granule_fwd(int H) { return (size_t)PRG * H * 4 <= 16384; }

struct PersistArgs {
  const float* xproj;  // (B, T/seg, 4H): row b*(T/seg) + t/seg is step t's input projection
  const bf16* w;
  float* hout;
  bf16* hout16;  // optional bf16 copy of h
  float* call;
  float* gall;
  unsigned* ctl;              // scratch: ctl[0] timeout flag, flags from word 4
  bf16* pay;                  // payload [2][B][H]
  unsigned long long* trace;  // diagnostics (avc_lstm_trace), null in production
  unsigned* fault;            // process fault word (avc_set_fault_word), bit 0 on a spin timeout; nullable
  unsigned spin;              // spin bound per wait (PSPIN unless avc_lstm_set_spin / AVC_LSTM_SPIN)
  int B, T, ng;
  int seg;                    // frames sharing one xproj row: 1, or T/nc for the lstm1 code fold
};

template <int H>
__global__ void __launch_bounds__(PNT, 1) lstm_persist_fwd(PersistArgs a) {
  constexpr bool GR = granule_fwd(H);
  constexpr int G = 4 * H, NKH = H / 64, AP = H + 8, KH = H / 2;
  constexpr int NCH = (PRG * H / 8 + PNT - 1) / PNT;  // 16-B payload chunks per thread per step
  constexpr int NCG = PRG * H / 4 / PNT;              // granule form: 16-B chunks per thread
  static_assert(!GR || NCG * PNT * 4 == PRG * H, "granule chunks must tile the group payload");
  __shared__ __attribute__((aligned(16))) bf16 As[16 * AP];
  __shared__ __attribute__((aligned(16))) bf16 hs16[PRG * PJU];
  __shared__ float gs[2][PRG][4 * PJU + 1];
  __shared__ float outs[6 * PRG * PJU];  // the step's h, c, i, f, g, o per (utterance, unit) cell
  __shared__ int quit;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, gq = w & 3, kh = w >> 2;
  const int g = blockIdx.x % a.ng, r = blockIdx.x / a.ng;
  const int j0 = r * PJU, b0 = g * PRG;
  const int T = a.T, B = a.B, rows = min(PRG, B - b0);
  const __amdgpu_buffer_rsrc_t pay = brsrc(a.pay, (long long)2 * B * H * (GR ? 4 : 2));
  unsigned* flags = a.ctl + 4 + g * PFL;

  // W_hh rows of gate gq for units j0 + 16n + (lane & 15), K half kh
  bf16x8 wf[2][NKH];
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const bf16* row = a.w + (long long)(gq * H + j0 + n * 16 + (lane & 15)) * H + kh * KH + 8 * (lane >> 4);
#pragma unroll
    for (int k = 0; k < NKH; ++k) wf[n][k] = *reinterpret_cast<const bf16x8*>(row + 32 * k);
  }
  for (int i = tid; i < 16 * AP / 2; i += PNT) reinterpret_cast<unsigned*>(As)[i] = 0u;
  if (tid == 0) quit = 0;
  const int pr = (tid >> 5) & (PRG - 1), pu = tid & 31, pb = b0 + pr, pj = j0 + pu;
  const bool pv = tid < PRG * PJU && pb < B;
  float c = 0.f;
  __syncthreads();

  for (int s = 0; s < T; ++s) {
    const int t = s;
    stamp(a.trace, T, s, 0);
    float px[4] = {0.f, 0.f, 0.f, 0.f};
    if (pv) {
      const float* xp = a.xproj + ((long long)pb * (T / a.seg) + t / a.seg) * G + pj;
#pragma unroll
      for (int q = 0; q < 4; ++q) px[q] = xp[q * H];
    }
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    if (s > 0) {
      // ---- the group's h_{t-1} -> LDS A tile (rows past the batch stay zero)
      if constexpr (GR) {
        if (!sweep_group<H, NCG, PNT>(pay, ((s - 1) & 1) * B + b0, rows, As, AP, (unsigned)s, a.spin, a.ctl, a.fault))
          quit = 1;
        __syncthreads();
        if (quit) return;
      } else {
        if (w == 0 && !poll_flags(flags, H / PJU, (unsigned)s, a.ctl, a.fault, a.spin)) quit = 1;
        __syncthreads();
        if (quit) return;  // block-uniform exit after a spin timeout
        load_group<H, NCH, PNT>(pay, ((s - 1) & 1) * B + b0, rows, As, AP);
        __syncthreads();
      }
      stamp(a.trace, T, s, 1);
      mfma_rows<NKH>(As + (lane & 15) * AP + kh * KH + 8 * (lane >> 4), wf, acc0, acc1);
    }
    if (lane < 32) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        gs[kh][4 * (lane >> 4) + e][gq * PJU + (lane & 15)] = acc0[e];
        gs[kh][4 * (lane >> 4) + e][gq * PJU + 16 + (lane & 15)] = acc1[e];
      }
    }
    __syncthreads();
    stamp(a.trace, T, s, 2);
    float h = 0.f, ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f;
    if (pv) {
      ig = fsig(px[0] + gs[0][pr][pu] + gs[1][pr][pu]);
      fg = fsig(px[1] + gs[0][pr][PJU + pu] + gs[1][pr][PJU + pu]);
      gg = ftanh(px[2] + gs[0][pr][2 * PJU + pu] + gs[1][pr][2 * PJU + pu]);
      og = fsig(px[3] + gs[0][pr][3 * PJU + pu] + gs[1][pr][3 * PJU + pu]);
      c = fg * c + ig * gg;
      h = og * ftanh(c);
    }
    // ---- publish h_t (8 x 32 bf16 tile via LDS; wave 0 stores 4 chunks per row, then the
    // flag) while waves 4..7 write the step's outputs, staged in LDS, to HBM: the publishing
    // wave issues nothing but the hand-off, so its drain waits for the payload alone
    if (tid < PRG * PJU) {
      hs16[pr * PJU + pu] = (bf16)h;
      float* o = outs + tid;
      o[0] = h;
      o[PRG * PJU] = c;
      o[2 * PRG * PJU] = ig;
      o[3 * PRG * PJU] = fg;
      o[4 * PRG * PJU] = gg;
      o[5 * PRG * PJU] = og;
    }
    __syncthreads();
    if (w == 0) {
      if (s + 1 < T) {
        if constexpr (GR) {
          // 8 lanes per row, two granules (4 units) each: the stores are the publication
          const int row = lane >> 3, c4 = lane & 7;
          if (row < rows) {
            const unsigned* hv = reinterpret_cast<const unsigned*>(hs16 + row * PJU + c4 * 4);
            store_granules(pay, ((long long)((s & 1) * B + b0 + row) * H + j0 + c4 * 4) / 2, hv[0], hv[1],
                           (unsigned)(s + 1));
          }
        } else {
          if (lane < 4 * rows) {
            const int row = lane >> 2, c8 = lane & 3;
            const u32x4_t v = *reinterpret_cast<const u32x4_t*>(hs16 + row * PJU + c8 * 8);
            __builtin_amdgcn_raw_buffer_store_b128(v, pay, (((s & 1) * B + b0 + row) * H + j0 + c8 * 8) * 2, 0,
                                                   AUX_SC1);
          }
          raise_flag(flags, r, (unsigned)(s + 1));
        }
      }
    } else if (w >= 4) {
      const int cell = tid - PRG * PJU, ob = b0 + (cell >> 5), oj = j0 + (cell & 31);
      if (ob < B) {
        const float* o = outs + cell;
        const long long oh = ((long long)ob * T + t) * H + oj;
        a.hout[oh] = o[0];
        if (a.hout16) a.hout16[oh] = (bf16)o[0];
        a.call[oh] = o[PRG * PJU];
        float* gp = a.gall + ((long long)ob * T + t) * G + oj;
        gp[0] = o[2 * PRG * PJU];
        gp[H] = o[3 * PRG * PJU];
        gp[2 * H] = o[4 * PRG * PJU];
        gp[3 * H] = o[5 * PRG * PJU];
      }
    }
    stamp(a.trace, T, s, 3);
  }
}

// Backward: same groups and members.  The recurrent product dh_rec[b][j] = sum_q
// dG_{t+1}[b][q] W_hh[q][j] runs over all 4H gate rows q, so each member keeps
// W_hh^T[j0..j0+32][0..4H) in registers (wave w = half (w >> 2) of the K-block of gate
// (w & 3), 2 x H/64 bf16x8 fragments) and loads the group's whole dG_{t+1} (8 x 4H bf16) into
// LDS each step.  The eight waves' partial products are summed through LDS; the cell-gradient
// carry dc stays in a register of the thread that owns (b, j) for the whole sequence.
// Outputs: dG (fp32) and its bf16 twin for the input-gradient / weight-gradient GEMMs.
struct PersistBwdArgs {
  const float* dhout;  // (B,T,H)
  const float* call;   // (B,T,H) cell states
  const float* gall;   // (B,T,4H) activated gates i,f,g,o
  const bf16* wt;      // W_hh^T [H][4H]
  float* dg;           // (B,T,4H)
  bf16* dg16;          // (B,T,4H) or null
  float* sc;           // (B, T/seg, 4H) dG summed over each seg-frame segment, or null
  bf16* sc16;          // its bf16 twin, or null
  unsigned* ctl;       // scratch: ctl[0] timeout flag, flags from word 4
  bf16* pay;           // payload [2][B][4H]
  unsigned long long* trace;  // diagnostics (avc_lstm_trace), null in production
  unsigned* fault;            // as PersistArgs
  unsigned spin;
  int B, T, ng;
  int seg;  // frames per sc row (the lstm1 code fold: T/nc)
};

template <int H>
__global__ void __launch_bounds__(PNT, 1) lstm_persist_bwd(PersistBwdArgs a) {
  constexpr int G = 4 * H, NKH = H / 64, AP = G + 8, KH = H / 2, NW = PNT / 64;
  constexpr int NCH = (PRG * G / 8 + PNT - 1) / PNT;  // 16-B payload chunks per thread per step
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  bf16* As = reinterpret_cast<bf16*>(smem_raw);                          // [PRG + 1][AP], row PRG = zeros
  float* red = reinterpret_cast<float*>(smem_raw + (PRG + 1) * AP * 2);  // [NW][PRG][PJU + 1]
  bf16* ds16 = reinterpret_cast<bf16*>(red + NW * PRG * (PJU + 1));      // [PRG][4 * PJU] publish tile
  float* outs = reinterpret_cast<float*>(ds16 + PRG * 4 * PJU);         // [4][PRG * PJU] dG of the step
  int* quit = reinterpret_cast<int*>(outs + 4 * PRG * PJU);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, gq = w & 3, kh = w >> 2;
  const int g = blockIdx.x % a.ng, r = blockIdx.x / a.ng;
  const int j0 = r * PJU, b0 = g * PRG;
  const int T = a.T, B = a.B, rows = min(PRG, B - b0);
  const __amdgpu_buffer_rsrc_t pay = brsrc(a.pay, (long long)2 * B * G * 2);
  unsigned* flags = a.ctl + 4 + g * PFL;

  // W_hh^T fragments: B operand of the product, n = unit j0 + 16n + (lane&15), k = gate row
  bf16x8 wf[2][NKH];
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const bf16* row = a.wt + (long long)(j0 + n * 16 + (lane & 15)) * G + gq * H + kh * KH + 8 * (lane >> 4);
#pragma unroll
    for (int k = 0; k < NKH; ++k) wf[n][k] = *reinterpret_cast<const bf16x8*>(row + 32 * k);
  }
  for (int i = tid; i < (PRG + 1) * AP / 2; i += PNT) reinterpret_cast<unsigned*>(As)[i] = 0u;
  if (tid == 0) *quit = 0;
  const int pr = (tid >> 5) & (PRG - 1), pu = tid & 31, pb = b0 + pr, pj = j0 + pu;
  const bool pv = tid < PRG * PJU && pb < B;
  // MFMA A rows: 0..7 loaded utterances, 8..15 read the zero row
  const int arow = (lane & 15) < PRG ? (lane & 15) : PRG;
  float dc = 0.f;
  float ssum[4] = {0.f, 0.f, 0.f, 0.f};  // waves 4..7: the cell's dG over the current segment
  __syncthreads();

  for (int s = 0; s < T; ++s) {
    const int t = T - 1 - s;
    stamp(a.trace, T, s, 0);
    // per-element inputs of this step (independent of the exchange: issued first)
    float dh = 0.f, ct = 0.f, cp = 0.f, gi = 0.f, gf = 0.f, gg = 0.f, go = 0.f;
    if (pv) {
      const long long oh = ((long long)pb * T + t) * H + pj;
      dh = a.dhout[oh];
      ct = a.call[oh];
      cp = t > 0 ? a.call[oh - H] : 0.f;
      const float* gp = a.gall + ((long long)pb * T + t) * G + pj;
      gi = gp[0];
      gf = gp[H];
      gg = gp[2 * H];
      go = gp[3 * H];
    }
    if (s > 0) {
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      if (w == 0 && !poll_flags(flags, H / PJU, (unsigned)s, a.ctl, a.fault, a.spin)) *quit = 1;
      __syncthreads();
      if (*quit) return;  // block-uniform exit after a spin timeout
      load_group<G, NCH, PNT>(pay, ((s - 1) & 1) * B + b0, rows, As, AP);
      __syncthreads();
      stamp(a.trace, T, s, 1);
      mfma_rows<NKH>(As + arow * AP + gq * H + kh * KH + 8 * (lane >> 4), wf, acc0, acc1);
      // rows 4*(lane>>4)+e < 8 only for lanes 0..31
      if (lane < 32) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          red[(w * PRG + 4 * (lane >> 4) + e) * (PJU + 1) + (lane & 15)] = acc0[e];
          red[(w * PRG + 4 * (lane >> 4) + e) * (PJU + 1) + 16 + (lane & 15)] = acc1[e];
        }
      }
      __syncthreads();
      stamp(a.trace, T, s, 2);
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) dh += red[(ww * PRG + pr) * (PJU + 1) + pu];
    }
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
    if (pv) {
      const float tc = ftanh(ct);
      const float dcs = dc + dh * go * (1.f - tc * tc);
      v0 = dcs * gg * gi * (1.f - gi);        // d(pre i)
      v1 = dcs * cp * gf * (1.f - gf);        // d(pre f)
      v2 = dcs * gi * (1.f - gg * gg);        // d(pre g)
      v3 = dh * tc * go * (1.f - go);         // d(pre o)
      dc = dcs * gf;
    }
    // ---- publish dG_t (8 x (4 gates x 32 units) bf16 tile via LDS; wave 0 stores 16 chunks
    // per row, 2 per lane, then the flag) while waves 4..7 write dG to HBM from LDS
    if (tid < PRG * PJU) {
      bf16* dsr = ds16 + pr * (4 * PJU) + pu;
      dsr[0] = (bf16)v0;
      dsr[PJU] = (bf16)v1;
      dsr[2 * PJU] = (bf16)v2;
      dsr[3 * PJU] = (bf16)v3;
      float* o = outs + tid;
      o[0] = v0;
      o[PRG * PJU] = v1;
      o[2 * PRG * PJU] = v2;
      o[3 * PRG * PJU] = v3;
    }
    __syncthreads();
    if (w == 0) {
      if (s + 1 < T) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int ch = lane + 64 * i, row = ch >> 4, q = (ch >> 2) & 3, c8 = ch & 3;
          if (row < rows) {
            const u32x4_t v = *reinterpret_cast<const u32x4_t*>(ds16 + row * (4 * PJU) + q * PJU + c8 * 8);
            __builtin_amdgcn_raw_buffer_store_b128(v, pay, (((s & 1) * B + b0 + row) * G + q * H + j0 + c8 * 8) * 2, 0,
                                                   AUX_SC1);
          }
        }
        raise_flag(flags, r, (unsigned)(s + 1));
      }
    } else if (w >= 4) {
      const int cell = tid - PRG * PJU, ob = b0 + (cell >> 5), oj = j0 + (cell & 31);
      if (ob < B) {
        const float* o = outs + cell;
        const long long og = ((long long)ob * T + t) * G + oj;
        if (a.dg) {
#pragma unroll
          for (int q = 0; q < 4; ++q) a.dg[og + q * H] = o[q * PRG * PJU];
        }
        if (a.dg16) {
#pragma unroll
          for (int q = 0; q < 4; ++q) a.dg16[og + q * H] = (bf16)o[q * PRG * PJU];
        }
        if (a.sc) {  // segment sums (frames t .. t + seg - 1, taken in reverse) for the code fold
#pragma unroll
          for (int q = 0; q < 4; ++q) ssum[q] += o[q * PRG * PJU];
          if (t % a.seg == 0) {
            const long long os = ((long long)ob * (T / a.seg) + t / a.seg) * G + oj;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              a.sc[os + q * H] = ssum[q];
              if (a.sc16) a.sc16[os + q * H] = (bf16)ssum[q];
              ssum[q] = 0.f;
            }
          }
        }
      }
    }
    stamp(a.trace, T, s, 3);
  }
}

template <int H>
constexpr size_t persist_bwd_lds() {
  return (size_t)(PRG + 1) * (4 * H + 8) * 2 + (size_t)(PNT / 64) * PRG * (PJU + 1) * 4 + (size_t)PRG * 4 * PJU * 2 +
         (size_t)4 * PRG * PJU * 4 + 16;
}

template <int H>
bool resident(bool bwd, int grid) {
  return bwd ? fits_resident(reinterpret_cast<const void*>(&lstm_persist_bwd<H>), PNT, persist_bwd_lds<H>(), grid)
             : fits_resident(reinterpret_cast<const void*>(&lstm_persist_fwd<H>), PNT, 0, grid);
}

}  // namespace

bool avcl::persistent_path(int B, int H, int dirs, bool bf, bool bwd) {
  if (!bf || dirs != 1 || !(H == 1024 || H == 768 || H == 512) || no_persist_env()) return false;
  const int ng = (B + PRG - 1) / PRG, grid = ng * (H / PJU);
  if (grid > num_cus()) return false;
  return H == 1024 ? resident<1024>(bwd, grid) : H == 768 ? resident<768>(bwd, grid) : resident<512>(bwd, grid);
}

int avcl::persist_fwd(const float* xproj, int seg, const void* w_hh, int B, int T, int H, float* h, void* h_bf16, float* c,
                float* gates, void* hbuf, hipStream_t s, const char* what) {
  const int ng = (B + PRG - 1) / PRG;
  PersistArgs p;
  p.xproj = xproj;
  p.w = reinterpret_cast<const bf16*>(w_hh);
  p.hout = h;
  p.hout16 = reinterpret_cast<bf16*>(h_bf16);
  p.call = c;
  p.gall = gates;
  p.ctl = reinterpret_cast<unsigned*>(hbuf);
  p.pay = reinterpret_cast<bf16*>(reinterpret_cast<char*>(hbuf) + px_payload_off(ng));
  p.trace = trace_ptr();
  p.fault = fault_word();
  p.spin = spin_bound();
  p.B = B;
  p.T = T;
  p.ng = ng;
  p.seg = seg;
  // flag form: only ctl + flags are polled; granule form: every tag of the payload too
  if (avc_zero_async(hbuf, granule_fwd(H) ? px_payload_off(ng) + (size_t)8 * B * H : px_ctl_bytes(ng), s)) return -1;
  const dim3 grid(ng * (H / PJU));
  if (H == 1024) lstm_persist_fwd<1024><<<grid, PNT, 0, s>>>(p);
  else if (H == 768) lstm_persist_fwd<768><<<grid, PNT, 0, s>>>(p);  // Adjust.py:30
  else lstm_persist_fwd<512><<<grid, PNT, 0, s>>>(p);
  return avc_check_launch(what);
}

int avcl::persist_bwd(const float* dh_out, const float* c, const float* gates, const void* w_hh_t, int B, int T, int H,
                float* dg, void* dg16, float* sc, void* sc16, int seg, void* gbuf, hipStream_t s, const char* what) {
  const int ng = (B + PRG - 1) / PRG;
  PersistBwdArgs p;
  p.dhout = dh_out;
  p.call = c;
  p.gall = gates;
  p.wt = reinterpret_cast<const bf16*>(w_hh_t);
  p.dg = dg;
  p.dg16 = reinterpret_cast<bf16*>(dg16);
  p.sc = sc;
  p.sc16 = reinterpret_cast<bf16*>(sc16);
  p.ctl = reinterpret_cast<unsigned*>(gbuf);
  p.pay = reinterpret_cast<bf16*>(reinterpret_cast<char*>(gbuf) + px_payload_off(ng));
  p.trace = trace_ptr();
  p.fault = fault_word();
  p.spin = spin_bound();
  p.B = B;
  p.T = T;
  p.ng = ng;
  p.seg = seg;
  if (avc_zero_async(gbuf, px_ctl_bytes(ng), s)) return -1;
  // (persistent_path set the dynamic-LDS attributes)
  const dim3 grid(ng * (H / PJU));
  if (H == 1024) lstm_persist_bwd<1024><<<grid, PNT, persist_bwd_lds<1024>(), s>>>(p);
  else if (H == 768) lstm_persist_bwd<768><<<grid, PNT, persist_bwd_lds<768>(), s>>>(p);
  else lstm_persist_bwd<512><<<grid, PNT, persist_bwd_lds<512>(), s>>>(p);
  return avc_check_launch(what);
}

extern "C" int avc_lstm_persistent(int B, int H, int dirs, int compute, int backward) {
  return persistent_path(B, H, dirs, compute == AVC_BF16, backward != 0) ? 1 : 0;
}

extern "C" int avc_lstm_fwd_fold(const float* pcode, int nc, const void* w_hh, int B, int T, int H, float* h,
                                 void* h_bf16, float* c, float* gates, void* hbuf, void* stream) {
  AVC_CHECK_ARG(pcode && w_hh && h && h_bf16 && c && gates && hbuf && B > 0 && T > 0 && nc > 0 && T % nc == 0,
                "avc_lstm_fwd_fold: bad args");
  AVC_CHECK_ARG(persistent_path(B, H, 1, true, false), "avc_lstm_fwd_fold: B=%d H=%d is not on the persistent path",
                B, H);
  return persist_fwd(pcode, T / nc, w_hh, B, T, H, h, h_bf16, c, gates, hbuf, as_stream(stream),
                     "avc_lstm_fwd_fold");
}

extern "C" int avc_lstm_bwd_fold(const float* dh_out, const float* c, const float* gates, const void* w_hh_t, int B,
                                 int T, int H, int nc, float* dgates, void* dgates_bf16, float* s_code,
                                 void* s_code_bf16, void* gbuf, void* stream) {
  AVC_CHECK_ARG(dh_out && c && gates && w_hh_t && dgates_bf16 && s_code && gbuf && B > 0 && T > 0 && nc > 0 &&
                    T % nc == 0,
                "avc_lstm_bwd_fold: bad args");
  AVC_CHECK_ARG(persistent_path(B, H, 1, true, true), "avc_lstm_bwd_fold: B=%d H=%d is not on the persistent path",
                B, H);
  return persist_bwd(dh_out, c, gates, w_hh_t, B, T, H, dgates, dgates_bf16, s_code, s_code_bf16, T / nc, gbuf,
                     as_stream(stream), "avc_lstm_bwd_fold");
}
