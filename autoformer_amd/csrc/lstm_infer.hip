// lstm_infer.hip — the persistent recurrence of lstm_persist.hip in a forward-only form for embedding
// extraction (the LstmDV speaker embedder, factory/LstmDV.py: nn.LSTM(80, 768, 3) -> last step):
// same groups, members, per-step arithmetic and flag-form hand-off (lstm_internal.h), but nothing is
// kept for a backward.  Per frame it writes at most the bf16 h (the next layer's GEMM operand); the
// fp32 h of ONE step per utterance -- step lens[b] - 1, the utterance's own last frame inside a
// padded batch -- goes to h_last.  No cell states, no gates, no fp32 h per frame.
//
// Rows per group RG is a template parameter: 8 (lstm_persist.hip's choice, made for its backward's
// 4H-wide payload) or 16, where every row of the 16-row MFMA tile is an utterance, all 512 threads
// own one (utterance, unit) cell and a launch holds twice as many utterances on the same CUs.
#include "lstm_internal.h"

namespace {
using namespace avcl;

constexpr int IMAXB = 512;  // utterances per launch (capture steps travel in the kernel arguments)

struct InferArgs {
  const float* xproj;  // (B, T, 4H)
  const bf16* w;       // W_hh (4H, H)
  bf16* hout16;        // (B, T, H) or null
  float* hlast;        // (B, H) or null
  unsigned* ctl;       // scratch: ctl[0] timeout flag, flags from word 4
  bf16* pay;           // payload [2][B][H]
  unsigned long long* trace;
  unsigned* fault;
  unsigned spin;
  int B, T, ng;
  unsigned short cap[IMAXB];  // cap[b] = lens[b] - 1: the step whose h is utterance b's h_last
};

template <int H, int RG>
__global__ void __launch_bounds__(PNT, 1) lstm_infer_kernel(InferArgs a) {
  constexpr int G = 4 * H, NKH = H / 64, AP = H + 8, KH = H / 2;
  constexpr int NCH = (RG * H / 8 + PNT - 1) / PNT;  // 16-B payload chunks per thread per step
  constexpr int CELLS = RG * PJU;                    // (utterance, unit) cells: threads 0..CELLS-1
  static_assert(RG == 8 || RG == 16, "a group fills half or all of the 16-row MFMA tile");
  static_assert(CELLS <= PNT && 4 * RG <= 64, "one cell per thread, one publishing wave");
  __shared__ __attribute__((aligned(16))) bf16 As[16 * AP];
  __shared__ __attribute__((aligned(16))) bf16 hs16[CELLS];
  __shared__ float gs[2][RG][4 * PJU + 1];
  __shared__ int quit;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, gq = w & 3, kh = w >> 2;
  const int g = blockIdx.x % a.ng, r = blockIdx.x / a.ng;
  const int j0 = r * PJU, b0 = g * RG;
  const int T = a.T, B = a.B, rows = min(RG, B - b0);
  const __amdgpu_buffer_rsrc_t pay = brsrc(a.pay, (long long)2 * B * H * 2);
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
  const int pr = (tid >> 5) & (RG - 1), pu = tid & 31, pb = b0 + pr, pj = j0 + pu;
  const bool pv = tid < CELLS && pb < B;
  const int cap = pv ? (int)a.cap[pb] : -1;
  float c = 0.f, hl = 0.f;
  __syncthreads();

  for (int s = 0; s < T; ++s) {
    stamp(a.trace, T, s, 0);
    float px[4] = {0.f, 0.f, 0.f, 0.f};
    if (pv) {
      const float* xp = a.xproj + ((long long)pb * T + s) * G + pj;
#pragma unroll
      for (int q = 0; q < 4; ++q) px[q] = xp[q * H];
    }
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    if (s > 0) {
      // ---- the group's h_{t-1} -> LDS A tile (rows past the batch stay zero)
      if (w == 0 && !poll_flags(flags, H / PJU, (unsigned)s, a.ctl, a.fault, a.spin)) quit = 1;
      __syncthreads();
      if (quit) return;  // block-uniform exit after a spin timeout
      load_group<H, NCH, PNT, RG>(pay, ((s - 1) & 1) * B + b0, rows, As, AP);
      __syncthreads();
      stamp(a.trace, T, s, 1);
      mfma_rows<NKH>(As + (lane & 15) * AP + kh * KH + 8 * (lane >> 4), wf, acc0, acc1);
    }
    // accumulator rows 4*(lane>>4) + e: lanes 0..31 hold rows 0..7, all lanes rows 0..15
    if (4 * (lane >> 4) < RG) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        gs[kh][4 * (lane >> 4) + e][gq * PJU + (lane & 15)] = acc0[e];
        gs[kh][4 * (lane >> 4) + e][gq * PJU + 16 + (lane & 15)] = acc1[e];
      }
    }
    __syncthreads();
    stamp(a.trace, T, s, 2);
    if (tid < CELLS) {
      float h = 0.f;
      if (pv) {
        const float ig = fsig(px[0] + gs[0][pr][pu] + gs[1][pr][pu]);
        const float fg = fsig(px[1] + gs[0][pr][PJU + pu] + gs[1][pr][PJU + pu]);
        const float gg = ftanh(px[2] + gs[0][pr][2 * PJU + pu] + gs[1][pr][2 * PJU + pu]);
        const float og = fsig(px[3] + gs[0][pr][3 * PJU + pu] + gs[1][pr][3 * PJU + pu]);
        c = fg * c + ig * gg;
        h = og * ftanh(c);
        if (s == cap) hl = h;
      }
      hs16[pr * PJU + pu] = (bf16)h;
    }
    __syncthreads();
    // ---- the RG x 32 bf16 tile of h_t leaves LDS as 16-B chunks, four per row: wave 0 publishes it
    // (sc1 stores, drain, flag) and issues nothing else; wave 1 stores the same chunks to h_bf16
    if (w < 2 && lane < 4 * rows) {
      const int row = lane >> 2, c8 = lane & 3;
      const u32x4_t v = *reinterpret_cast<const u32x4_t*>(hs16 + row * PJU + c8 * 8);
      if (w == 0) {
        if (s + 1 < T)
          __builtin_amdgcn_raw_buffer_store_b128(v, pay, (((s & 1) * B + b0 + row) * H + j0 + c8 * 8) * 2, 0, AUX_SC1);
      } else if (a.hout16) {
        *reinterpret_cast<u32x4_t*>(a.hout16 + ((long long)(b0 + row) * T + s) * H + j0 + c8 * 8) = v;
      }
    }
    if (w == 0 && s + 1 < T) raise_flag(flags, r, (unsigned)(s + 1));
    stamp(a.trace, T, s, 3);
  }
  if (pv && a.hlast) a.hlast[(long long)pb * H + pj] = hl;
}

template <int H, int RG>
bool infer_resident(int grid) {
  return fits_resident(reinterpret_cast<const void*>(&lstm_infer_kernel<H, RG>), PNT, 0, grid);
}

// rows = 0: the measured default (profiles/dvec_infer_ab.txt) -- 8-row groups while their grid fits
// the device, 16-row groups for the larger batches that only they admit
int pick_rows(int B, int H, int rows) {
  if (rows) return rows;
  return cdiv(B, 8) * (H / PJU) <= num_cus() ? 8 : 16;
}

bool infer_path(int B, int H, int rows) {
  if (H != 768 || B <= 0 || B > IMAXB || !(rows == 8 || rows == 16) || no_persist_env()) return false;
  const int grid = cdiv(B, rows) * (H / PJU);
  if (grid > num_cus()) return false;
  return rows == 8 ? infer_resident<768, 8>(grid) : infer_resident<768, 16>(grid);
}

}  // namespace

extern "C" int avc_lstm_infer_persistent(int B, int H, int rows) {
  if (B <= 0 || H <= 0 || rows < 0) return 0;
  return infer_path(B, H, pick_rows(B, H, rows)) ? 1 : 0;
}

extern "C" size_t avc_lstm_infer_scratch_bytes(int B, int H, int rows) {
  if (B <= 0 || H <= 0) return 0;
  (void)rows;  // sized for 8-row groups (the larger flag block), so one buffer serves either form
  return px_payload_off(cdiv(B, 8)) + (size_t)4 * B * H;
}

extern "C" int avc_lstm_infer(const float* xproj, const void* w_hh, const int* lens, int B, int T, int H, int rows,
                              void* h_bf16, float* h_last, void* hbuf, void* stream) {
  AVC_CHECK_ARG(xproj && w_hh && hbuf && (h_bf16 || h_last) && B > 0 && T > 0 && T <= 65535 && H > 0 && rows >= 0,
                "avc_lstm_infer: bad args (B=%d T=%d H=%d rows=%d; one of h_bf16 / h_last is required)", B, T, H, rows);
  AVC_CHECK_ARG((((uintptr_t)h_bf16 | (uintptr_t)w_hh | (uintptr_t)hbuf) & 15) == 0,
                "avc_lstm_infer: w_hh, h_bf16 and hbuf must be 16-byte aligned");
  rows = pick_rows(B, H, rows);
  AVC_CHECK_ARG(infer_path(B, H, rows), "avc_lstm_infer: B=%d H=%d rows=%d is not on the persistent path", B, H, rows);
  const int ng = cdiv(B, rows);
  InferArgs p = {};
  for (int b = 0; b < B; ++b) {
    const int len = lens ? lens[b] : T;
    AVC_CHECK_ARG(len >= 1 && len <= T, "avc_lstm_infer: lens[%d] = %d outside 1..T = %d", b, len, T);
    p.cap[b] = (unsigned short)(len - 1);
  }
  p.xproj = xproj;
  p.w = reinterpret_cast<const bf16*>(w_hh);
  p.hout16 = reinterpret_cast<bf16*>(h_bf16);
  p.hlast = h_last;
  p.ctl = reinterpret_cast<unsigned*>(hbuf);
  p.pay = reinterpret_cast<bf16*>(reinterpret_cast<char*>(hbuf) + px_payload_off(ng));
  p.trace = trace_ptr();
  p.fault = fault_word();
  p.spin = spin_bound();
  p.B = B;
  p.T = T;
  p.ng = ng;
  hipStream_t s = as_stream(stream);
  if (avc_zero_async(hbuf, px_ctl_bytes(ng), s)) return -1;
  const dim3 grid(ng * (H / PJU));
  if (rows == 8) lstm_infer_kernel<768, 8><<<grid, PNT, 0, s>>>(p);
  else lstm_infer_kernel<768, 16><<<grid, PNT, 0, s>>>(p);
  return avc_check_launch("avc_lstm_infer");
}
