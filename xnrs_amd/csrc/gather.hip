// Row gathers: whole news blocks copied out of the device-resident news table (fp32 or bf16), with or without the towers'
// input dropout in the same launch.  HBM-bound block copies, no MFMA.
//
//   gather_rows    : the dict look-ups + torch.cat of NewsRecDataset.__getitem__ (dataset.py:63-85,97-109) as a
//                    device copy: out[i] = table[ids[i]] for whole news blocks (S*D floats, 150 KB at the shipped
//                    shape) -- the materialised batch for consumers that need dense token tensors (input gradients
//                    of the explainer, explain.py:160-166); the encoders themselves gather inside their first load.
//   dropout_rows   : the towers' input dropout (news_encoding.py:51, user_encoding.py:69) on dense rows, or fused with
//                    gather_rows for the id path: the dropped batch is materialised in the launch that gathers it.
#include "host.h"

namespace xnrs {

// ---------------------------------------------------------------- gather_rows (HBM-bound block copy)
// one workgroup per (output row, 16-KB piece): 4 independent 16-byte loads per thread, streaming (nontemporal) on both
// sides -- every byte is touched once.  Each load sits behind its own bounds branch, and the compiler waits for it inside
// that branch, so a wave has ONE of the four in flight at a time and the other waves of the CU cover the latency: a
// branch-free path for full pieces (all four in flight) was measured on dropout_rows_kernel below, which has this loop
// shape, and moved nothing
template <bool VEC>
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ table, const int32_t* __restrict__ ids,
                                                           float* __restrict__ out, int64_t row_floats, int pieces) {
  const int64_t row = blockIdx.x / pieces;
  const int piece = (int)(blockIdx.x - row * pieces);
  const int64_t src = (int64_t)ids[row] * row_floats, dst = row * row_floats;
  if (VEC) {
    const int64_t n4 = row_floats >> 2;
    const f32x4* s4 = reinterpret_cast<const f32x4*>(table + src);
    f32x4* d4 = reinterpret_cast<f32x4*>(out + dst);
    const int64_t base = (int64_t)piece * 1024 + threadIdx.x;
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (base + 256 * u < n4) v[u] = __builtin_nontemporal_load(s4 + base + 256 * u);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (base + 256 * u < n4) __builtin_nontemporal_store(v[u], d4 + base + 256 * u);
  } else {
    const int64_t base = (int64_t)piece * 4096 + threadIdx.x;
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (base + 256 * u < row_floats) out[dst + base + 256 * u] = table[src + base + 256 * u];
  }
}

hipError_t launch_gather_rows(const float* table, const int32_t* ids, float* out, int64_t n, int64_t row_floats,
                              hipStream_t stream) {
  if (n <= 0 || row_floats <= 0) return hipSuccess;
  const bool vec = row_floats % 4 == 0 && ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int64_t pieces = (row_floats + 4095) / 4096;  // 16 KB per workgroup
  if (n * pieces > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(n * pieces));
  if (vec) hipLaunchKernelGGL((gather_rows_kernel<true>), grid, dim3(256), 0, stream, table, ids, out, row_floats, (int)pieces);
  else hipLaunchKernelGGL((gather_rows_kernel<false>), grid, dim3(256), 0, stream, table, ids, out, row_floats, (int)pieces);
  return hipGetLastError();
}

// ---------------------------------------------------------------- dropout_rows (gather_rows + the towers' input dropout)
// The shape of gather_rows_kernel: one workgroup per (output row, 16-KB piece), 16-byte streaming accesses.  Element j of
// output row i draws drop_uniform(row i of the CALL, j): the 64-bit part of the draw depends on (seed, i) alone -- uniform
// over the workgroup, computed once -- and each element pays the 32-bit finaliser.  x and out are not __restrict__: a dense
// call may run in place (every thread loads its elements before it stores them, and no other thread touches them).
__device__ __forceinline__ float drop_element(const DropRowsArgs& a, int64_t row, uint32_t j, float v, float keep, float scale) {
  return drop_uniform(a, row, j) < keep ? v * scale : 0.f;
}
template <bool VEC>
__global__ __launch_bounds__(256) void dropout_rows_kernel(const float* x, const int32_t* __restrict__ ids, float* out,
                                                            int64_t row_floats, int pieces, float p, DropRowsArgs a0) {
  // the device word is read ONCE, before any store (out is not __restrict__: a later read would have to be repeated)
  const DropRowsArgs a{drop_seed(a0), nullptr, 1};
  const int64_t row = blockIdx.x / pieces;
  const int piece = (int)(blockIdx.x - row * pieces);
  const int64_t src = (ids ? (int64_t)ids[row] : row) * row_floats, dst = row * row_floats;
  const float keep = 1.f - p, scale = 1.f / (1.f - p);
  if (VEC) {
    const int64_t n4 = row_floats >> 2;
    const f32x4* s4 = reinterpret_cast<const f32x4*>(x + src);
    f32x4* d4 = reinterpret_cast<f32x4*>(out + dst);
    const int64_t base = (int64_t)piece * 1024 + threadIdx.x;
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (base + 256 * u < n4) v[u] = __builtin_nontemporal_load(s4 + base + 256 * u);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (base + 256 * u < n4) {
        const uint32_t j = (uint32_t)(base + 256 * u) * 4u;  // < row_floats < 2^32
#pragma unroll
        for (int c = 0; c < 4; ++c) v[u][c] = drop_element(a, row, j + c, v[u][c], keep, scale);
        __builtin_nontemporal_store(v[u], d4 + base + 256 * u);
      }
  } else {
    const int64_t base = (int64_t)piece * 4096 + threadIdx.x;
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (base + 256 * u < row_floats)
        out[dst + base + 256 * u] = drop_element(a, row, (uint32_t)(base + 256 * u), x[src + base + 256 * u], keep, scale);
  }
}

// 0 < p < 1
hipError_t launch_dropout_rows(const float* x, const int32_t* ids, float* out, int64_t n, int64_t row_floats, float p,
                               uint64_t seed, const uint64_t* seed_dev, hipStream_t stream) {
  if (n <= 0 || row_floats <= 0) return hipSuccess;
  const bool vec = row_floats % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int64_t pieces = (row_floats + 4095) / 4096;  // 16 KB per workgroup
  if (n * pieces > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(n * pieces));
  const DropRowsArgs a{seed, seed_dev, 1};
  if (vec) hipLaunchKernelGGL((dropout_rows_kernel<true>), grid, dim3(256), 0, stream, x, ids, out, row_floats, (int)pieces, p, a);
  else hipLaunchKernelGGL((dropout_rows_kernel<false>), grid, dim3(256), 0, stream, x, ids, out, row_floats, (int)pieces, p, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------- gather_rows / dropout_rows from a table stored in bf16
// The streaming shape of the two kernels above with the widening on the way (a bf16 value is the high half of its fp32 value:
// bits << 16, exact): one workgroup per (output row, 16 KB of output), a thread's 8 consecutive elements are ONE 16-byte
// load and two 16-byte stores.  Logical row i is table row ids[i / S] * S + i % S (ids nullable: row i).  DROP: the input
// dropout of dropout_rows_kernel on the widened value -- the same drop_element with the same (seed, row of the call, column).
typedef unsigned u32x4b __attribute__((ext_vector_type(4)));
template <bool VEC, bool DROP>
__global__ __launch_bounds__(256) void gather_rows_bf16_kernel(const unsigned short* __restrict__ table, const int32_t* __restrict__ ids,
                                                                int S, int64_t row0, float* __restrict__ out, int64_t row_elems,
                                                                int pieces, float p, DropRowsArgs a0) {
  const DropRowsArgs a{DROP ? drop_seed(a0) : 0ull, nullptr, 1};
  const int64_t row = blockIdx.x / pieces;
  const int piece = (int)(blockIdx.x - row * pieces);
  int64_t srow = row0 + row;  // (row0: the launch writes logical rows row0 .. row0 + n of a longer list to out rows 0 .. n)
  if (ids) {
    const int64_t n = srow / S;
    srow = (int64_t)ids[n] * S + (srow - n * S);
  }
  const int64_t src = srow * row_elems, dst = row * row_elems;
  const float keep = 1.f - p, scale = 1.f / (1.f - p);
  if (VEC) {
    const int64_t n8 = row_elems >> 3;
    const u32x4b* s8 = reinterpret_cast<const u32x4b*>(table + src);
    f32x4* d4 = reinterpret_cast<f32x4*>(out + dst);
    const int64_t base = (int64_t)piece * 512 + threadIdx.x;
    u32x4b v[2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (base + 256 * u < n8) v[u] = __builtin_nontemporal_load(s8 + base + 256 * u);
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (base + 256 * u < n8) {
        const int64_t c = base + 256 * u;
        f32x4 lo, hi;  // elements 0..3 and 4..7 of the chunk: the low half of a word is the earlier element
#pragma unroll
        for (int w = 0; w < 2; ++w) {
          lo[2 * w] = __uint_as_float(v[u][w] << 16);
          lo[2 * w + 1] = __uint_as_float(v[u][w] & 0xffff0000u);
          hi[2 * w] = __uint_as_float(v[u][2 + w] << 16);
          hi[2 * w + 1] = __uint_as_float(v[u][2 + w] & 0xffff0000u);
        }
        if (DROP) {
          const uint32_t j = (uint32_t)c * 8u;  // < row_elems < 2^32
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            lo[e] = drop_element(a, row, j + e, lo[e], keep, scale);
            hi[e] = drop_element(a, row, j + 4 + e, hi[e], keep, scale);
          }
        }
        __builtin_nontemporal_store(lo, d4 + 2 * c);
        __builtin_nontemporal_store(hi, d4 + 2 * c + 1);
      }
  } else {
    const int64_t base = (int64_t)piece * 4096 + threadIdx.x;
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (base + 256 * u < row_elems) {
        const float x = __uint_as_float((unsigned)table[src + base + 256 * u] << 16);
        out[dst + base + 256 * u] = DROP ? drop_element(a, row, (uint32_t)(base + 256 * u), x, keep, scale) : x;
      }
  }
}

template <bool DROP>
static hipError_t launch_rows_bf16(const unsigned short* table, const int32_t* ids, int S, int64_t row0, float* out, int64_t n,
                                   int64_t row_elems, float p, uint64_t seed, const uint64_t* seed_dev, hipStream_t stream) {
  if (n <= 0 || row_elems <= 0) return hipSuccess;
  if (ids && S <= 0) return hipErrorInvalidValue;
  const bool vec = row_elems % 8 == 0 && ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int64_t pieces = (row_elems + 4095) / 4096;  // 16 KB of output per workgroup
  if (n * pieces > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(n * pieces));
  const DropRowsArgs a{seed, seed_dev, 1};
  if (vec)
    hipLaunchKernelGGL((gather_rows_bf16_kernel<true, DROP>), grid, dim3(256), 0, stream, table, ids, S, row0, out, row_elems, (int)pieces, p, a);
  else
    hipLaunchKernelGGL((gather_rows_bf16_kernel<false, DROP>), grid, dim3(256), 0, stream, table, ids, S, row0, out, row_elems, (int)pieces, p, a);
  return hipGetLastError();
}

hipError_t launch_gather_rows_bf16(const unsigned short* table, const int32_t* ids, int S, float* out, int64_t n, int64_t row_elems,
                                   hipStream_t stream, int64_t row0) {
  return launch_rows_bf16<false>(table, ids, S, row0, out, n, row_elems, 0.f, 0, nullptr, stream);
}

// 0 < p < 1
hipError_t launch_dropout_rows_bf16(const unsigned short* table, const int32_t* ids, float* out, int64_t n, int64_t row_elems, float p,
                                    uint64_t seed, const uint64_t* seed_dev, hipStream_t stream) {
  return launch_rows_bf16<true>(table, ids, 1, 0, out, n, row_elems, p, seed, seed_dev, stream);
}

}  // namespace xnrs

// ---------------------------------------------------------------- C entry points (include/xnrs_hip.h)
using namespace xnrs;

extern "C" {

int32_t xnrs_gather_rows(const float* table, const int32_t* ids, float* out, int64_t n, int64_t row_floats, void* stream) {
  if (n == 0) return XNRS_OK;
  if (!table || !ids || !out || n < 0 || row_floats <= 0) return XNRS_EINVAL;
  return hip_rc(launch_gather_rows(table, ids, out, n, row_floats, (hipStream_t)stream));
}

int32_t xnrs_dropout_rows(const float* x, const int32_t* ids, float* out, int64_t n, int64_t row_floats, float p, uint64_t seed,
                          const uint64_t* seed_dev, void* stream) {
  if (!(p >= 0.f && p <= 1.f)) return XNRS_EINVAL;  // (NaN fails both comparisons)
  if (n == 0) return XNRS_OK;
  if (!x || !out || n < 0 || row_floats <= 0 || row_floats >= (1LL << 32)) return XNRS_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const size_t bytes = (size_t)n * (size_t)row_floats * F32;
  if (p >= 1.f) return hip_rc(hipMemsetAsync(out, 0, bytes, st));
  if (p <= 0.f) {  // no draw: the plain gather, or a copy (nothing at all in place)
    if (ids) return hip_rc(launch_gather_rows(x, ids, out, n, row_floats, st));
    return out == x ? XNRS_OK : hip_rc(hipMemcpyAsync(out, x, bytes, hipMemcpyDeviceToDevice, st));
  }
  return hip_rc(launch_dropout_rows(x, ids, out, n, row_floats, p, seed, seed_dev, st));
}

int32_t xnrs_gather_rows_bf16(const uint16_t* table, const int32_t* ids, float* out, int64_t n, int64_t row_elems, void* stream) {
  if (n == 0) return XNRS_OK;
  if (!table || !ids || !out || n < 0 || row_elems <= 0) return XNRS_EINVAL;
  return hip_rc(launch_gather_rows_bf16(table, ids, 1, out, n, row_elems, (hipStream_t)stream));
}

int32_t xnrs_dropout_rows_bf16(const uint16_t* table, const int32_t* ids, float* out, int64_t n, int64_t row_elems, float p,
                               uint64_t seed, const uint64_t* seed_dev, void* stream) {
  if (!(p >= 0.f && p <= 1.f)) return XNRS_EINVAL;  // (NaN fails both comparisons)
  if (n == 0) return XNRS_OK;
  if (!table || !ids || !out || n < 0 || row_elems <= 0 || row_elems >= (1LL << 32)) return XNRS_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (p >= 1.f) return hip_rc(hipMemsetAsync(out, 0, (size_t)n * (size_t)row_elems * F32, st));
  if (p <= 0.f) return hip_rc(launch_gather_rows_bf16(table, ids, 1, out, n, row_elems, st));  // no draw: the widening gather
  return hip_rc(launch_dropout_rows_bf16(table, ids, out, n, row_elems, p, seed, seed_dev, st));
}

}  // extern "C"
