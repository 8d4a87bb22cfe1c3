// resample.hip — band-limited sample-rate conversion in one launch (declared in
// include/autovc_hip_resample.h): the notebook's librosa.resample(x, fs, 22050), resampy's
// Kaiser-windowed sinc interpolator, applied as the exact polyphase FIR it is.  For fs_out / fs_in =
// L / M the weights of output t depend only on r = t mod L; the host tabulates them (fp64, rounded
// once to fp32) tap-major, W[k][r], and this kernel is the FIR.
//
// A workgroup of 256 threads produces RS_J * PJ whole periods of one utterance: outputs
// [j0 L, (j0 + RS_J PJ) L), which read the inputs [j0 M + lo, j0 M + lo + span).
//   1. That span is loaded once into LDS, zeros outside [0, N): an utterance's ends and the padding of
//      a shorter row are never read.
//   2. Work item q < L * PJ is (r, jg) = (q mod L, q div L).  It owns residue r in the RS_J periods
//      j0 + jg + i PJ: each weight W[k][r] is loaded once (consecutive lanes, consecutive words; the
//      table stays in L2) and used for RS_J outputs, whose inputs sit PJ * M words apart in the span.
//      Taps ascending, one fp32 FMA each: the order of every sum is fixed.
//   3. Output t is stored as the sum for t < floor(N L / M) and as 0.0 from there to out_stride, so
//      every element of out is written.
//
// LDS: the span only, span = (RS_J PJ - 1) M + (hi - lo) floats <= RS_SPAN_MAX (48 KiB, three
// workgroups per CU).  Lanes of one residue run read words M apart (periods interleaved, not
// consecutive: RS_J M apart would put L = 1 pairs such as 44100 -> 22050 on every eighth bank);
// lanes of consecutive residues read words about M / L apart, a 2- to 3-way conflict of a
// ds_read_b32 when downsampling and a broadcast when upsampling.  The host picks PJ per rate pair:
// the largest share of busy lanes in the last pass over the L * PJ items, then the larger tile.
#include "common.h"

#include "../../include/autovc_hip_resample.h"

namespace {

constexpr int RS_THREADS = 256, RS_J = 4;
constexpr int RS_SPAN_MAX = 12288;  // floats of LDS

__global__ void __launch_bounds__(RS_THREADS) resample_kernel(
    const float* __restrict__ x, long long stride, const int* __restrict__ lens, const float* __restrict__ W,
    const int* __restrict__ tab, int L, int M, int PJ, int lo, int span, float* __restrict__ out,
    long long out_stride) {
  extern __shared__ __attribute__((aligned(16))) float rs_sm[];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int N = (int)min((long long)lens[b], stride);  // lens_dev is the caller's copy: never read past the row
  const long long nvalid = (long long)N * L / M;
  const long long j0 = (long long)blockIdx.x * PJ * RS_J;
  const long long t0 = j0 * L;
  const int tile = PJ * RS_J * L;
  float* o = out + (long long)b * out_stride;
  if (t0 >= nvalid) {  // uniform over the workgroup: the pad sample and the row padding
    for (int i = tid; i < tile; i += RS_THREADS)
      if (t0 + i < out_stride) o[t0 + i] = 0.f;
    return;
  }
  const float* xb = x + (long long)b * stride;
  const long long g0 = j0 * M + lo;
  for (int i = tid; i < span; i += RS_THREADS) {
    const long long g = g0 + i;
    rs_sm[i] = (g >= 0 && g < N) ? xb[g] : 0.f;
  }
  __syncthreads();
  const int items = L * PJ, pm = PJ * M;
  for (int q = tid; q < items; q += RS_THREADS) {
    const int jg = q / L, r = q - jg * L;
    const int first = tab[3 * r + 1], cnt = tab[3 * r + 2];
    const float* xs = rs_sm + (jg * M + tab[3 * r] + first - lo);
    const float* w = W + ((long long)first * L + r);
    float acc[RS_J];
#pragma unroll
    for (int i = 0; i < RS_J; ++i) acc[i] = 0.f;
    for (int k = 0; k < cnt; ++k) {
      const float wv = w[(long long)k * L];
#pragma unroll
      for (int i = 0; i < RS_J; ++i) acc[i] = fmaf(wv, xs[i * pm + k], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < RS_J; ++i) {
      const long long t = t0 + (long long)(jg + i * PJ) * L + r;
      if (t < out_stride) o[t] = t < nvalid ? acc[i] : 0.f;
    }
  }
}

// Periods-per-lane-run PJ of a tile: RS_J * PJ periods, span bound RS_J PJ M + taps floats.
int rs_pick(int L, int M, int taps) {
  int best = 0;
  double best_u = 0.0;
  for (int pj = 1; (long long)pj * RS_J * M + taps <= RS_SPAN_MAX && (long long)pj * RS_J * L < (1 << 24); ++pj) {
    const long long items = (long long)L * pj;
    const double u = (double)items / (double)(((items + RS_THREADS - 1) / RS_THREADS) * RS_THREADS);
    if (u >= best_u) best_u = u, best = pj;
  }
  return best;
}

int rs_check_pair(const char* who, int L, int M, int taps) {
  AVC_CHECK_ARG(L >= 1 && M >= 1, "%s: L = %d, M = %d: both must be at least 1", who, L, M);
  AVC_CHECK_ARG(taps >= 1, "%s: taps = %d", who, taps);
  AVC_CHECK_ARG((long long)taps * L <= AVC_RESAMPLE_MAX_WEIGHTS,
                "%s: the polyphase table of L = %d residues x %d taps has %lld weights; at most "
                "AVC_RESAMPLE_MAX_WEIGHTS = %d are taken (a rate pair with a large reduced L, or a steep "
                "downsampling, is not supported)",
                who, L, taps, (long long)taps * L, AVC_RESAMPLE_MAX_WEIGHTS);
  AVC_CHECK_ARG(rs_pick(L, M, taps) >= 1,
                "%s: M = %d, taps = %d: one tile of %d periods needs more than the %d floats of the LDS budget", who,
                M, taps, RS_J, RS_SPAN_MAX);
  return 0;
}

}  // namespace

extern "C" int avc_resample_tile(int L, int M, int taps) {
  if (rs_check_pair("avc_resample_tile", L, M, taps)) return -1;
  return rs_pick(L, M, taps) * RS_J * L;
}

extern "C" int avc_resample(const float* x, long long stride, const int* lens, const int* lens_dev, int B,
                            const float* weights, int n_weights, const int* tab, const int* tab_dev, int L, int M,
                            int taps, float* out, long long out_stride, void* stream) {
  AVC_CHECK_ARG(x && lens && lens_dev && weights && tab && tab_dev && out, "avc_resample: null pointer");
  if (rs_check_pair("avc_resample", L, M, taps)) return -1;
  AVC_CHECK_ARG((long long)n_weights == (long long)taps * L, "avc_resample: n_weights = %d, expected taps * L = %lld",
                n_weights, (long long)taps * L);
  AVC_CHECK_ARG(B >= 1 && B <= 65535 && stride >= 1 && out_stride >= 1 && out_stride < (1ll << 31),
                "avc_resample: bad shape B=%d stride=%lld out_stride=%lld", B, stride, out_stride);
  for (int b = 0; b < B; ++b) {
    const int N = lens[b];
    AVC_CHECK_ARG(N >= 1, "avc_resample: lens[%d] = %d: an utterance has at least one sample", b, N);
    AVC_CHECK_ARG(N <= stride, "avc_resample: lens[%d] = %d exceeds the row stride %lld", b, N, stride);
    AVC_CHECK_ARG(N <= (1 << 30), "avc_resample: lens[%d] = %d: more than 2^30 samples", b, N);
    const long long need = ((long long)N * L + M - 1) / M;
    AVC_CHECK_ARG(need <= out_stride, "avc_resample: utterance %d gives %lld samples, out_stride = %lld", b, need,
                  out_stride);
  }
  long long lo = 0, hi = 0;  // inputs one period reaches, relative to j M: [lo, hi)
  for (int r = 0; r < L; ++r) {
    const int off = tab[3 * r], first = tab[3 * r + 1], cnt = tab[3 * r + 2];
    AVC_CHECK_ARG(first >= 0 && cnt >= 0 && first + cnt <= taps,
                  "avc_resample: residue %d (offset %d, first tap %d, count %d) outside the %d taps", r, off, first, cnt,
                  taps);
    const long long a = (long long)off + first, e = a + cnt;
    if (r == 0 || a < lo) lo = a;
    if (r == 0 || e > hi) hi = e;
  }
  AVC_CHECK_ARG(hi - lo <= (long long)M + taps && lo > -(1 << 30) && hi < (1 << 30),
                "avc_resample: the residues' inputs span [%lld, %lld) of a period, more than M + taps = %lld", lo, hi,
                (long long)M + taps);
  const int pj = rs_pick(L, M, taps);
  const long long span = (long long)(RS_J * pj - 1) * M + (hi - lo);
  AVC_CHECK_ARG(span >= 1 && span <= RS_SPAN_MAX, "avc_resample: input span %lld outside 1..%d", span, RS_SPAN_MAX);
  const int tile = pj * RS_J * L;
  const dim3 grid(cdiv(out_stride, tile), B);
  resample_kernel<<<grid, RS_THREADS, (size_t)span * sizeof(float), as_stream(stream)>>>(
      x, stride, lens_dev, weights, tab_dev, L, M, pj, (int)lo, (int)span, out, out_stride);
  return avc_check_launch("avc_resample");
}
