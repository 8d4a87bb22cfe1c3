// Device helpers shared by the MelGAN glue kernels: melgan.hip (rectangular batches) and
// melgan_ragged.hip (a length per utterance).  One definition of the element maths -- LeakyReLU as one
// fp32 multiply, 4-channel accesses, ReflectionPad1d's index -- is what makes the ragged forms
// bit-identical to the rectangular ones at full lengths.
#pragma once
#include "common.h"

namespace avmg {

__device__ __forceinline__ float lrelu(float v, float s) { return v >= 0.f ? v : v * s; }

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 ld4(const bf16* p) {
  const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
  return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void st4(bf16* p, f32x4 v) {
  *reinterpret_cast<bf16x4*>(p) = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
}

// reflect (ReflectionPad1d: -1 -> 1, L -> L-2) or -1 = zero
__device__ __forceinline__ int src_frame(int s, int L, int reflect) {
  if (s >= 0 && s < L) return s;
  if (!reflect) return -1;
  return s < 0 ? -s : 2 * (L - 1) - s;
}

}  // namespace avmg
