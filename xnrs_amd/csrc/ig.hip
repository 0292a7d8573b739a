// Integrated gradients with ONE Q|K|V projection: the two streaming kernels around the per-step work.
//
// Along the interpolation path the scaled tokens are ga_i = a_i x, and a TextEncoder with an attention stage reads its tokens
// through q_linear | k_linear | v_linear alone (layers.py:128-130), so
//   forward :  QKV_i = ga_i W^T + b = a_i P + b,  P = x W^T          -> xnrs_ig_expand: n images from ONE product
//   backward:  sum_i d s_i / d ga_i = (sum_i dQKV_i) W               -> xnrs_ig_reduce: ONE image for ONE product
// Both kernels stream: (n + 1) rows x W floats each way, no reuse, HBM-bound.  A lane owns one 16-byte group of P / of the sum
// (W % 4 == 0 and 16-byte aligned bases; one float otherwise -- the same arithmetic per element, hence the same bits) and
// walks the n steps; consecutive lanes own consecutive groups, so every wave-instruction moves 1 KiB of one image.  The grid
// is sized to the chip and strides over the groups; every offset is int64 (n * rows * W passes 2^31 at sizes users run).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

#include "host.h"

namespace xnrs {

namespace {

constexpr int IG_THREADS = 256;
constexpr int IG_BLOCKS_PER_CU = 8;
constexpr int IG_ALPHAS = 1024;  // steps staged in LDS per sweep of a block over its groups
constexpr int IG_UNROLL = 8;     // loads of the reduce in flight per lane

struct Vec1 {
  float v[1];
};
struct alignas(16) Vec4 {
  float v[4];
};

// out[i * E + e] = fmaf(alphas[i], p[e], bias[e % W]),  e < E = rows * W, i < n.  groups = E / V.
template <class Vec, int V>
__global__ __launch_bounds__(IG_THREADS) void ig_expand_kernel(const float* __restrict__ p, const float* __restrict__ bias,
                                                                const float* __restrict__ alphas, int64_t n, int64_t groups,
                                                                int64_t W, float* __restrict__ out) {
  __shared__ float al[IG_ALPHAS];
  const int64_t E = groups * V;
  const int64_t stride = (int64_t)gridDim.x * IG_THREADS;
  for (int64_t i0 = 0; i0 < n; i0 += IG_ALPHAS) {
    const int nc = (int)(n - i0 < IG_ALPHAS ? n - i0 : IG_ALPHAS);
    __syncthreads();  // (the sweep before has finished reading al)
    for (int i = threadIdx.x; i < nc; i += IG_THREADS) al[i] = alphas[i0 + i];  // the alphas once per row block
    __syncthreads();
    for (int64_t g = (int64_t)blockIdx.x * IG_THREADS + threadIdx.x; g < groups; g += stride) {
      const int64_t e = g * V;
      const Vec pv = *reinterpret_cast<const Vec*>(p + e);
      Vec bv;
      const int64_t col = e % W;  // (V == 4: W % 4 == 0, a group never straddles a row)
#pragma unroll
      for (int j = 0; j < V; ++j) bv.v[j] = bias ? bias[col + j] : 0.f;
      float* dst = out + i0 * E + e;
      for (int i = 0; i < nc; ++i, dst += E) {
        const float a = al[i];
        Vec ov;
#pragma unroll
        for (int j = 0; j < V; ++j) ov.v[j] = fmaf(a, pv.v[j], bv.v[j]);
        *reinterpret_cast<Vec*>(dst) = ov;
      }
    }
  }
}

// s = g[0 * E + e] + g[1 * E + e] + ... (one fp32 chain, ascending i); out[e] = scale * s (+ out[e]): product and sums rounded
// one by one.  The chain of an element lives in one lane, so no launch geometry changes a bit.
template <class Vec, int V>
__global__ __launch_bounds__(IG_THREADS) void ig_reduce_kernel(const float* __restrict__ gsrc, int64_t n, int64_t groups, float scale,
                                                                float* __restrict__ out, int accumulate) {
// plain * and + below: the __f*_rn helpers are inlined C and the compiler may still contract them into one fma
#pragma clang fp contract(off)
  const int64_t E = groups * V;
  const int64_t stride = (int64_t)gridDim.x * IG_THREADS;
  for (int64_t g = (int64_t)blockIdx.x * IG_THREADS + threadIdx.x; g < groups; g += stride) {
    const int64_t e = g * V;
    const float* src = gsrc + e;
    Vec s = *reinterpret_cast<const Vec*>(src);
    int64_t i = 1;
    for (; i + IG_UNROLL <= n; i += IG_UNROLL) {
      Vec t[IG_UNROLL];
#pragma unroll
      for (int u = 0; u < IG_UNROLL; ++u) t[u] = *reinterpret_cast<const Vec*>(src + (i + u) * E);
#pragma unroll
      for (int u = 0; u < IG_UNROLL; ++u)
#pragma unroll
        for (int j = 0; j < V; ++j) s.v[j] = s.v[j] + t[u].v[j];
    }
    for (; i < n; ++i) {
      const Vec t = *reinterpret_cast<const Vec*>(src + i * E);
#pragma unroll
      for (int j = 0; j < V; ++j) s.v[j] = s.v[j] + t.v[j];
    }
    Vec o;
    if (accumulate) o = *reinterpret_cast<const Vec*>(out + e);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float prod = scale * s.v[j];
      o.v[j] = accumulate ? o.v[j] + prod : prod;
    }
    *reinterpret_cast<Vec*>(out + e) = o;
  }
}

int ig_cu_count() {  // per device, cached (as cu_count in additive_fused.hip)
  static std::mutex mu;
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  std::lock_guard<std::mutex> lk(mu);
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
  }
  return cus[dev];
}

// blocks for `groups` lanes of work: every group once, at most IG_BLOCKS_PER_CU blocks per CU (the rest by the grid stride)
int ig_grid(int64_t groups) {
  const int cus = ig_cu_count();
  const int64_t want = (groups + IG_THREADS - 1) / IG_THREADS;
  const int64_t cap = (int64_t)cus * IG_BLOCKS_PER_CU;
  return (int)(want < cap ? want : cap);
}

}  // namespace

}  // namespace xnrs

using namespace xnrs;

extern "C" {

int32_t xnrs_ig_expand(const float* p, const float* bias, const float* alphas, int64_t n, int64_t rows, int32_t W, float* out,
                       void* stream) {
  if (n < 0 || rows < 0 || W <= 0) return XNRS_EINVAL;
  if (n == 0 || rows == 0) return XNRS_OK;
  if (!p || !alphas || !out) return XNRS_EINVAL;
  const int64_t E = rows * (int64_t)W;
  hipStream_t st = (hipStream_t)stream;
  if (W % 4 == 0 && aligned16(p) && aligned16(out)) {  // (bias is read one float at a time on both routes)
    const int64_t groups = E / 4;
    hipLaunchKernelGGL((ig_expand_kernel<Vec4, 4>), dim3(ig_grid(groups)), dim3(IG_THREADS), 0, st, p, bias, alphas, n, groups,
                       (int64_t)W, out);
  } else {
    hipLaunchKernelGGL((ig_expand_kernel<Vec1, 1>), dim3(ig_grid(E)), dim3(IG_THREADS), 0, st, p, bias, alphas, n, E, (int64_t)W, out);
  }
  return hip_rc(hipGetLastError());
}

int32_t xnrs_ig_reduce(const float* g, int64_t n, int64_t rows, int32_t W, float scale, float* out, int32_t accumulate,
                       void* stream) {
  if (n < 0 || rows < 0 || W <= 0 || accumulate < 0 || accumulate > 1) return XNRS_EINVAL;
  if (n == 0 || rows == 0) return XNRS_OK;
  if (!g || !out) return XNRS_EINVAL;
  const int64_t E = rows * (int64_t)W;
  hipStream_t st = (hipStream_t)stream;
  if (W % 4 == 0 && aligned16(g) && aligned16(out)) {
    const int64_t groups = E / 4;
    hipLaunchKernelGGL((ig_reduce_kernel<Vec4, 4>), dim3(ig_grid(groups)), dim3(IG_THREADS), 0, st, g, n, groups, scale, out, accumulate);
  } else {
    hipLaunchKernelGGL((ig_reduce_kernel<Vec1, 1>), dim3(ig_grid(E)), dim3(IG_THREADS), 0, st, g, n, E, scale, out, accumulate);
  }
  return hip_rc(hipGetLastError());
}

}  // extern "C"
