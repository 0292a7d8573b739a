// Device helpers of the kernels that gather whole table rows against a vector (list_loss.hip, diversity.hip): a lane takes
// the elements [4 l, 4 l + 4) + 256 j of a row in ascending j as one fma chain, a butterfly adds the 64 lanes.  The scalar
// form of load4 gives a lane the SAME elements in the same order as the 16-byte form, so both produce the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace xnrs {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// the four floats [i, i + 4) of a row of E floats; beyond E: 0.  VEC: one 16-byte load (E % 4 == 0, aligned base)
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* __restrict__ p, int i, int E) {
  if constexpr (VEC) {
    return *reinterpret_cast<const float4*>(p + i);
  } else {
    float4 v;
    v.x = i < E ? p[i] : 0.f;
    v.y = i + 1 < E ? p[i + 1] : 0.f;
    v.z = i + 2 < E ? p[i + 2] : 0.f;
    v.w = i + 3 < E ? p[i + 3] : 0.f;
    return v;
  }
}
__device__ __forceinline__ float dot4(float4 a, float4 b, float acc) {
  acc = fmaf(a.x, b.x, acc);
  acc = fmaf(a.y, b.y, acc);
  acc = fmaf(a.z, b.z, acc);
  return fmaf(a.w, b.w, acc);
}

}  // namespace xnrs
