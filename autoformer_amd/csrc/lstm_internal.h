// lstm_internal.h — what lstm.hip, lstm_small.hip, lstm_persist.hip, lstm_infer.hip and lstm2.hip share (internal
// to libautovc_hip.so): the device helpers of the recurrences, the inter-workgroup hand-off
// protocol of the persistent kernels, and the host state / entry points that cross files.
#pragma once
#include "common.h"

namespace avcl {

// ---------------------------------------------------------------- host state (lstm.hip)
// Process-wide and set up under std::call_once / a mutex: forward calls come from the Python
// thread, backward calls from PyTorch's autograd device thread.
constexpr int MAXDEV = 64;
int num_cus();                    // CUs of the current device (0 on error)
unsigned* fault_word();           // the current device's fault word (avc_set_fault_word), nullable
unsigned spin_bound();            // per wait: PSPIN, avc_lstm_set_spin / AVC_LSTM_SPIN; 0 = injected timeout
bool no_persist_env();            // AVC_LSTM_NO_PERSIST set
unsigned long long* trace_ptr();  // the avc_lstm_trace buffer (null in production)
// Co-residency of a persistent grid: every workgroup must be resident at once (the members
// wait on each other), so the launch is taken only when the occupancy API admits `grid`
// workgroups over the device's CUs.  Cached per (kernel, device); the first query also sets the
// kernel's dynamic-LDS attribute to `lds`, so it precedes every launch.
bool fits_resident(const void* fn, int threads, size_t lds, int grid);

// ---------------------------------------------------------------- entry points across files
// H <= 64 (lstm_small.hip); fast = bf16 compute mode (fp32 weights and state either way)
int small_fwd(const float* xproj, const float* w_hh, int B, int T, int H, int dirs, float* h, bf16* h16, float* c,
              float* gates, bool fast, hipStream_t s);
int small_bwd(const float* dh_out, const float* c, const float* gates, const float* w_hh, int B, int T, int H,
              int dirs, float* dg, bf16* dg16, bool fast, hipStream_t s);
// One layer in one launch (lstm_persist.hip).  persistent_path: whether it applies (the launches'
// own test).  persist_fwd: hbuf = control words + flags + the [2][B][H] payload (layout below); xproj
// row b*(T/seg) + t/seg feeds step t.  persist_bwd: gbuf likewise, [2][B][4H]; dg (fp32), dg16
// nullable; sc / sc16 (nullable): dG summed over each seg-frame segment.
bool persistent_path(int B, int H, int dirs, bool bf, bool bwd);
int persist_fwd(const float* xproj, int seg, const void* w_hh, int B, int T, int H, float* h, void* h_bf16, float* c,
                float* gates, void* hbuf, hipStream_t s, const char* what);
int persist_bwd(const float* dh_out, const float* c, const float* gates, const void* w_hh_t, int B, int T, int H,
                float* dg, void* dg16, float* sc, void* sc16, int seg, void* gbuf, hipStream_t s, const char* what);

// ---------------------------------------------------------------- activations
__device__ __forceinline__ float fsig(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float ftanh(float x) { return 2.f * fsig(2.f * x) - 1.f; }
// FAST (bf16 compute mode): v_exp_f32 / v_rcp_f32 forms; otherwise the IEEE library forms, so
// the fp32 parity mode keeps the reference's activation arithmetic
template <bool FAST>
__device__ __forceinline__ float act_sig(float x) { return FAST ? fsig(x) : sigmoidf_(x); }
template <bool FAST>
__device__ __forceinline__ float act_tanh(float x) { return FAST ? ftanh(x) : tanhf(x); }

// ---------------------------------------------------------------- small-H step (lstm_small.hip, ragged.hip)
// broadcast lane N of each lane quad (DPP quad_perm, no LDS traffic)
template <int N>
__device__ __forceinline__ float quad_bcast(float v) {
  constexpr int ctl = N | (N << 2) | (N << 4) | (N << 6);
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), ctl, 0xf, 0xf, false));
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// sum_k w[k] * h[k] with the HM/4 float4 slices of h already in registers, as packed fp32 FMAs
// (v_pk_fma_f32): four independent accumulation chains, so no FMA waits on its predecessor's result
template <int HM>
__device__ __forceinline__ float dot_regs(const f32x4 (&hv)[HM / 4], const f32x2 (&w)[HM / 2]) {
  f32x2 a[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
  for (int k = 0; k < HM / 4; ++k) {
    a[(2 * k) & 3] = __builtin_elementwise_fma(f32x2{hv[k][0], hv[k][1]}, w[2 * k], a[(2 * k) & 3]);
    a[(2 * k + 1) & 3] = __builtin_elementwise_fma(f32x2{hv[k][2], hv[k][3]}, w[2 * k + 1], a[(2 * k + 1) & 3]);
  }
  const f32x2 t = (a[0] + a[1]) + (a[2] + a[3]);
  return t[0] + t[1];
}

// ---------------------------------------------------------------- buffer resources
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) unsigned gu32;
constexpr int AUX_SC1 = 16;  // buffer-instruction cache-policy bits: sc1

// Raw buffer resource over `bytes` bytes: accesses at offsets past it are dropped.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t brsrc(const void* p, long long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
// The same for an optional output (0 bytes for a null pointer: every store dropped).  The small
// kernels' flush wave predicates its stores this way and with out-of-range offsets, so its unrolled
// flush has no branches and every store keeps its own registers: no store waits for an earlier one.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t brsrc_opt(const void* p, long long bytes) {
  return brsrc(p, p ? bytes : 0);
}

// ---------------------------------------------------------------- diagnostic timeline
// avc_lstm_trace(buf) makes the kernels record the 100 MHz REALTIME clock into buf; the stamps go
// to that buffer only, nothing reads them inside a kernel.  Two layouts, one per workgroup shape:
//  * sstamp (small kernels, TRACE instantiations only; workgroups on a 2-D grid): lane 0 of the
//    calling wave writes tr[(block*Tp + s)*8 + j] once the value `dep` exists (the asm's input
//    operand orders the stamp after the code that produces it);
//  * stamp (persistent kernels, tr null in production): thread 0 of the workgroup writes
//    tr[(wg*T + step)*4 + j] at four points of every step: j = 0 step start, 1 exchange complete,
//    2 recurrent product reduced, 3 step published.
__device__ __forceinline__ void sstamp(unsigned long long* tr, int Tp, int s, int j, float dep) {
  unsigned long long t;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : "v"(dep));
  if ((threadIdx.x & 63) == 0)
    tr[((long long)(blockIdx.y * gridDim.x + blockIdx.x) * Tp + s) * 8 + j] = t;
}
__device__ __forceinline__ void stamp(unsigned long long* tr, int T, int s, int j) {
  if (tr && threadIdx.x == 0) tr[((long long)blockIdx.x * T + s) * 4 + j] = __builtin_amdgcn_s_memrealtime();
}

// =============================================================== large H: persistent recurrences
// One launch for all T steps of a dirs == 1 layer (decoder lstm1 H=512, lstm2 H=1024).
// Workgroups form NG groups of H/32 members; group g owns utterance rows [8g, 8g+8), member r
// owns hidden units [32r, 32r+32) and keeps the matching W_hh slice in VGPRs for the whole
// sequence.  Every step each member needs the whole group's previous output (forward h_{t-1}:
// 8 x H bf16; backward dG_{t+1}: 8 x 4H bf16), handed over inside the launch by the
// write-through form of MI355X_MICROARCH.md "Valid forms" (table row 1):
//   producer: its tile is staged in LDS, wave 0 stores it with 16-B sc1 (write-through)
//             buffer stores, waits s_waitcnt vmcnt(0), then lane 0 stores the member's flag
//             = step + 1 (agent-scope relaxed atomic store = an sc1 store);
//   consumer: wave 0 polls the group's flags with sc1 loads until every member reached the
//             step, the workgroup barrier releases the other waves, and every thread loads its
//             16-B chunks with sc1 buffer loads (L1 bypassed; every handed-off byte is stored
//             and loaded sc1, so no acquire fence).
// Compared with 8-byte {tag, 2 x bf16} granules this moves half the bytes per consumer with
// 16-B accesses, and a waiting consumer re-reads only the flag words.  The payload is
// double-buffered by step parity: a member publishes step s+1 only after consuming step s-1
// from every member, so no slot is overwritten while it is read.  Flags are monotone step
// tags zeroed before every launch; every spin is bounded (timeout -> ctl[0] raised, exit).
// Groups are blockIdx % NG: with round-robin dispatch a group shares one XCD -- a speed
// assumption only, correctness holds for any placement.
//
// Scratch (hbuf forward / gbuf backward):
//   u32 ctl[4] (ctl[0] = timeout flag) | u32 flags[NG][64] | pad to 256 B | bf16 payload [2][B][W]
// with W = H (forward) or 4H (backward); only ctl + flags are zeroed per launch.
constexpr int PRG = 8, PJU = 32, PFL = 64;
constexpr unsigned PSPIN = 1u << 22;

constexpr size_t px_ctl_bytes(int ng) { return 16 + (size_t)ng * PFL * 4; }
constexpr size_t px_payload_off(int ng) { return (px_ctl_bytes(ng) + 255) & ~(size_t)255; }

// Wave 0: poll the NR flag words of the group (one lane each, sc1 loads, s_sleep between
// passes) until every member has published step `tag`.  false = spin timeout: the launch's
// ctl[0] and the process fault word (when registered) get bit 0, so the host sees the
// failure at its next fault check instead of training on the unfinished outputs.
__device__ __forceinline__ bool poll_flags(unsigned* flags, int NR, unsigned tag, unsigned* ctl, unsigned* fault,
                                           unsigned spin) {
  const int lane = threadIdx.x & 63;
  gu32* f = (gu32*)flags;
  unsigned spins = 0;
  if (spin == 0) {  // injected timeout (avc_lstm_set_spin(~0u)): fail without polling
    if (lane == 0) {
      atomicOr(ctl, 1u);
      if (fault) atomicOr(fault, 1u);
    }
    return false;
  }
  while (true) {
    bool ok = true;
    if (lane < NR) ok = __hip_atomic_load(f + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= tag;
    if (__all(ok)) return true;
    if (++spins > spin) {
      if (lane == 0) {
        atomicOr(ctl, 1u);
        if (fault) atomicOr(fault, 1u);
      }
      return false;
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

// Wave 0, after its write-through payload stores: drain them, then raise the member's flag.
__device__ __forceinline__ void raise_flag(unsigned* flags, int r, unsigned tag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if ((threadIdx.x & 63) == 0)
    __hip_atomic_store((gu32*)flags + r, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Every thread of the NT-thread workgroup: copy the group's `rows` payload rows of W bf16
// (parity slot row0) into the LDS tile (row stride ap), 16-B sc1 loads, NCH chunks per
// thread, all in flight together.  RG = rows of the LDS tile that a group may fill (PRG; the
// forward-only recurrence of lstm_infer.hip also runs 16-row groups).
template <int W, int NCH, int NT, int RG = PRG>
__device__ __forceinline__ void load_group(__amdgpu_buffer_rsrc_t pay, int row0, int rows, bf16* lds, int ap) {
  constexpr int CPR = W / 8;
  const int tid = threadIdx.x;
  u32x4_t v[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int ch = tid + NT * i, row = ch / CPR, col = ch - row * CPR;
    v[i] = row < rows ? __builtin_amdgcn_raw_buffer_load_b128(pay, ((row0 + row) * W + col * 8) * 2, 0, AUX_SC1)
                      : u32x4_t{0u, 0u, 0u, 0u};
  }
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int ch = tid + NT * i, row = ch / CPR, col = ch - row * CPR;
    // NCH is rounded up when NT does not divide the tile (H = 768): skip the overhang
    if (NCH * NT == RG * CPR || row < RG) *reinterpret_cast<u32x4_t*>(lds + row * ap + col * 8) = v[i];
  }
}

// Granule form (MI355X_MICROARCH.md "Valid forms", R2; cdna_hip_programming.md G16 recipe):
// the payload IS the flag.  Each 8-byte granule {u32 data = 2 bf16, u32 tag = step + 1} is
// written by one sc1 store (two granules per 16-B store, whose 8-B halves land untorn), so
// the producer needs no drain and no flag, and a consumer needs no flag poll before loading:
// every thread re-reads its own 16-B chunks (sc1, L1 bypassed) until both tags match, then
// stages the data in LDS.  Twice the bytes of the bf16 payload, one fabric round trip fewer
// on both sides.  NCH chunks per thread (chunk = 2 granules = 4 values; a row of W values has
// W/4 chunks), re-read back to back (s_sleep between failed sweeps measured no better).
// false = spin timeout (ctl[0] / fault word raised).
template <int W, int NCH, int NT>
__device__ __forceinline__ bool sweep_group(__amdgpu_buffer_rsrc_t pay, int row0, int rows, bf16* lds, int ap,
                                            unsigned tag, unsigned spin, unsigned* ctl, unsigned* fault) {
  constexpr int CPR = W / 4;
  const int tid = threadIdx.x;
  u32x4_t v[NCH];
  bool ok[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) ok[i] = (tid + NT * i) / CPR >= rows;
  if (spin == 0) {  // injected timeout (avc_lstm_set_spin(~0u)): fail without reading
    if ((threadIdx.x & 63) == 0) {
      atomicOr(ctl, 1u);
      if (fault) atomicOr(fault, 1u);
    }
    return false;
  }
  for (unsigned spins = 0;; ++spins) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int ch = tid + NT * i, row = ch / CPR, col = ch - row * CPR;
      if (!ok[i]) v[i] = __builtin_amdgcn_raw_buffer_load_b128(pay, ((row0 + row) * (W / 2) + col * 2) * 8, 0, AUX_SC1);
    }
    bool all = true;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      ok[i] = ok[i] || (v[i][1] == tag && v[i][3] == tag);
      all = all && ok[i];
    }
    if (__all(all)) break;
    if (spins >= spin) {
      if ((threadIdx.x & 63) == 0) {
        atomicOr(ctl, 1u);
        if (fault) atomicOr(fault, 1u);
      }
      return false;
    }
    asm volatile("" ::: "memory");  // the re-reads are real loads, never hoisted
  }
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int ch = tid + NT * i, row = ch / CPR, col = ch - row * CPR;
    if (row < rows) *reinterpret_cast<u32x2_t*>(lds + row * ap + col * 4) = u32x2_t{v[i][0], v[i][2]};
  }
  return true;
}

// One 16-B sc1 store of two granules: values (d0, d1) = 4 bf16 at granule index gi (even).
__device__ __forceinline__ void store_granules(__amdgpu_buffer_rsrc_t pay, long long gi, unsigned d0, unsigned d1,
                                               unsigned tag) {
  __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{d0, tag, d1, tag}, pay, (int)(gi * 8), 0, AUX_SC1);
}

// acc_n += A . W_n over NK K-blocks of 32: A rows (16 per lane group) are read from LDS at
// `a` + 32k, W fragments live in registers; A fragments are read up to eight K-blocks ahead.
template <int NK>
__device__ __forceinline__ void mfma_rows(const bf16* a, const bf16x8 (&wf)[2][NK], f32x4& acc0, f32x4& acc1) {
  // K-blocks per fragment batch: the largest divisor of NK up to 8 (NK = 12 at H = 768)
  constexpr int KG = NK % 8 == 0 ? 8 : NK % 6 == 0 ? 6 : NK % 4 == 0 ? 4 : NK < 8 ? NK : 1;
#pragma unroll
  for (int k0 = 0; k0 < NK; k0 += KG) {
    bf16x8 af[KG];
#pragma unroll
    for (int i = 0; i < KG; ++i) af[i] = *reinterpret_cast<const bf16x8*>(a + 32 * (k0 + i));
#pragma unroll
    for (int i = 0; i < KG; ++i) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], wf[0][k0 + i], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], wf[1][k0 + i], acc1, 0, 0, 0);
    }
  }
}

// Workgroups of PNT = 512 threads: eight waves, two per SIMD.  Wave w takes gate (w & 3) and
// half (w >> 2) of the K range, so it holds 128 registers of W fragments instead of 256 and
// the SIMD's two waves hide each other's LDS fragment reads under MFMAs (with four waves of
// 256 W registers the compiler had one A-fragment register left and waited on every read).
// Threads 0..255 own the (utterance, unit) cells of the element-wise stages.
constexpr int PNT = 512;

}  // namespace avcl
