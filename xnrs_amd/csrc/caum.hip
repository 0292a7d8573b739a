// CAUM's candidate-aware user tower (xnrs/models/full_models/caum.py:31-111), forward and backward, fp32:
//
//   attn_long   unmasked scaled-dot-product attention over a packed Q|K|V image at ANY sequence length (CAUM attends
//               along the batch x candidate axis: L = B * n_c, hundreds to thousands), online softmax over 32-key tiles so
//               the L x L scores never reach memory; the training forward keeps the per-row log-sum-exp, the backward
//               recomputes the probabilities from it.  v_mfma_f32_32x32x2_f32 for every product.
//   pair        the circular three-slot window + candidate broadcast behind linear1 / linear2, from the two small
//               projections Hp = h' [Wl; Wm; Wr; W2h]^T and Cp = c' [Wc; W2c]^T + [b1; b2] (the reference's (B, C, H, 4E)
//               and (B, C, H, 2E) concatenations never exist), and its reduction backward
//   bias_tanh   t = tanh(pre + cb[pair]): the candidate half of dense_att.linear added per (candidate, slot) row
//   pool        score dot, softmax over the H slots of a (user, candidate) pair (no mask), weighted sum; backward
//   act_bwd     dpre = dy f'(y) for the activations the GEMM epilogue fuses
//
// Attention tiling.  A score tile is computed TRANSPOSED, S^T = K . Q^T (32 keys x 32 queries): in the accumulator a lane
// then holds 16 keys of ONE query (its column), the other 16 sit in lane ^ 32 -- the row maximum and sum are 16 in-lane
// steps and one exchange, and the probabilities are already the B operand of O^T += V^T . P^T: the contraction runs over
// the keys in the order the accumulator holds them (register i of half h is key 8 (i / 4) + 4 h + i % 4), V^T is read
// from LDS by that rule, and no probability ever moves between lanes or through LDS.  A workgroup is up to four waves of
// 32 queries each around one shared K / V tile; the backward is two kernels of the same shape (dQ: a wave owns 32 queries
// and walks the keys; dK | dV: a wave owns 32 keys and walks the queries), each output element written by exactly one
// lane in a fixed order -- no atomics, the same bits every run.  Head rows are zero-padded in LDS to a multiple of 32
// columns (+ 1: an odd row pitch keeps the 32 rows a wave reads on 32 banks).
// LDS per workgroup: (2 + W) tiles forward, (2 + 2 W) backward, a tile = 32 x (32 NBLK + 1) floats: 25 KB / 37 KB at
// d_k <= 32 with W = 4, 99 KB at d_k = 128 (W = 4 forward, W = 2 backward).
#include <atomic>
#include <cmath>

#include "host.h"

using namespace xnrs;

namespace {

struct AttnLongArgs {
  const float* qkv;  // element (l, nb, col) at qkv[l * ss + nb * bs + col]; q | k | v at columns 0 | E | 2E
  int64_t ss, bs;
  float* o;          // forward output, head h at columns [h d_k, (h + 1) d_k); element (l, nb, col) at o[l * oss + nb * obs + col]
  const float* d_o;  // backward: gradient of o, same addressing
  int64_t oss, obs;
  float* lse;        // [L, Nb, heads] log-sum-exp of every score row (nullable in the inference forward)
  float* delta;      // backward scratch [L, Nb, heads]: rowsum(dO * O) per head
  float* dqkv;       // backward output, addressed like qkv
  int32_t L, Nb, heads, dk, E;
  float scale;
};

__device__ __forceinline__ int reg_row(int i, int half) { return 8 * (i >> 2) + 4 * half + (i & 3); }

// a 32-row tile of head rows into LDS: row r of the tile is sequence position r0 + r (zeros past L and past d_k)
template <int NBLK>
__device__ __forceinline__ void load_tile(float* dst, const float* __restrict__ src, int64_t row_stride, int r0, int L, int dk,
                                          float scale, int tid, int nthreads) {
  constexpr int WPAD = NBLK * 32, LD = WPAD + 1;
  for (int idx = tid; idx < 32 * WPAD; idx += nthreads) {
    const int r = idx / WPAD, d = idx - r * WPAD;
    const int pos = r0 + r;
    dst[r * LD + d] = (pos < L && d < dk) ? src[(int64_t)pos * row_stride + d] * scale : 0.f;
  }
}

// acc (32 x 32) += A . B^T over the padded head width: A, B tiles in LDS, row l31 of each is this lane's row / column
template <int NBLK>
__device__ __forceinline__ void tile_scores(const float* A, const float* B, int dk, int l31, int half, f32x16& acc) {
  constexpr int LD = NBLK * 32 + 1;
  const int nk2 = (dk + 1) >> 1;  // (an odd d_k reads the zero column d_k)
  const float* ap = A + l31 * LD + half;
  const float* bp = B + l31 * LD + half;
  for (int t = 0; t < nk2; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * t], bp[2 * t], acc, 0, 0, 0);
}

// the accumulator blocks (element (column block b, register i) = head column 32 b + reg_row(i), sequence row l31) through a
// wave-private LDS tile to global rows: row r of the tile goes to dst + (r0 + r) * row_stride
template <int NBLK>
__device__ __forceinline__ void store_tile(const f32x16 (&acc)[NBLK], float f, float* tile, float* __restrict__ dst,
                                           int64_t row_stride, int r0, int L, int dk, int lane) {
  constexpr int LD = NBLK * 32 + 1;
  const int half = lane >> 5, l31 = lane & 31;
#pragma unroll
  for (int b = 0; b < NBLK; ++b)
#pragma unroll
    for (int i = 0; i < 16; ++i) tile[l31 * LD + b * 32 + reg_row(i, half)] = acc[b][i] * f;
  __syncthreads();
  for (int idx = lane; idx < 32 * dk; idx += 64) {
    const int r = idx / dk, d = idx - r * dk;
    if (r0 + r < L) dst[(int64_t)(r0 + r) * row_stride + d] = tile[r * LD + d];
  }
}

// workgroup -> (tile group, batch column, head): heads of one batch column next to each other (they share cache lines)
__device__ __forceinline__ void decode_block(const AttnLongArgs& a, int W, int* grp, int* nb, int* h) {
  const int ngrp = (a.L + 32 * W - 1) / (32 * W);
  int64_t x = blockIdx.x;
  *h = (int)(x % a.heads);
  x /= a.heads;
  *grp = (int)(x % ngrp);
  *nb = (int)(x / ngrp);
}

template <int NBLK>
__global__ __launch_bounds__(256) void attn_long_fwd_kernel(AttnLongArgs a) {
  extern __shared__ float lds[];
  constexpr int LD = NBLK * 32 + 1, TILE = 32 * LD;
  const int W = blockDim.x >> 6;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
  float *Ks = lds, *Vs = lds + TILE, *Qs = lds + (2 + wave) * TILE;
  int grp, nb, h;
  decode_block(a, W, &grp, &nb, &h);
  const int L = a.L, dk = a.dk;
  const int q0 = (grp * W + wave) * 32;
  const float* base = a.qkv + (int64_t)nb * a.bs + (int64_t)h * dk;
  load_tile<NBLK>(Qs, base, a.ss, q0, L, dk, a.scale, lane, 64);
  f32x16 oacc[NBLK];
#pragma unroll
  for (int b = 0; b < NBLK; ++b)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[b][i] = 0.f;
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < L; k0 += 32) {
    __syncthreads();  // every wave is done with the previous K / V tile (first round: the Q tiles are written)
    load_tile<NBLK>(Ks, base + a.E, a.ss, k0, L, dk, 1.f, threadIdx.x, blockDim.x);
    load_tile<NBLK>(Vs, base + 2 * a.E, a.ss, k0, L, dk, 1.f, threadIdx.x, blockDim.x);
    __syncthreads();
    if (q0 >= L) continue;  // (a wave without queries only helps loading)
    f32x16 s;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0.f;
    tile_scores<NBLK>(Ks, Qs, dk, l31, half, s);  // s[i] = score of (key k0 + reg_row(i), query q0 + l31)
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (k0 + reg_row(i, half) >= L) s[i] = -INFINITY;
      mx = fmaxf(mx, s[i]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));  // finite: key k0 exists
    const float mn = fmaxf(m, mx);
    const float alpha = __expf(m - mn);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      s[i] = __expf(s[i] - mn);
      sum += s[i];
    }
    sum += __shfl_xor(sum, 32);
    l = fmaf(l, alpha, sum);
    m = mn;
#pragma unroll
    for (int b = 0; b < NBLK; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) oacc[b][i] *= alpha;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float* vp = Vs + reg_row(i, half) * LD + l31;
#pragma unroll
      for (int b = 0; b < NBLK; ++b) oacc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[b * 32], s[i], oacc[b], 0, 0, 0);
    }
  }
  __syncthreads();
  const bool live = q0 + l31 < L;
  store_tile<NBLK>(oacc, live ? 1.f / l : 0.f, Qs, a.o + (int64_t)nb * a.obs + (int64_t)h * dk, a.oss, q0, L, dk, lane);
  if (a.lse && live && half == 0) a.lse[((int64_t)(q0 + l31) * a.Nb + nb) * a.heads + h] = m + logf(l);
}

// delta[l, nb, h] = sum_d dO O over the head's columns
__global__ __launch_bounds__(256) void attn_long_delta_kernel(AttnLongArgs a) {
  const int64_t n = (int64_t)a.L * a.Nb * a.heads;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const int h = (int)(idx % a.heads);
  const int64_t r = idx / a.heads;
  const int64_t off = (r / a.Nb) * a.oss + (r % a.Nb) * a.obs + (int64_t)h * a.dk;
  float s = 0.f;
  for (int d = 0; d < a.dk; ++d) s = fmaf(a.d_o[off + d], a.o[off + d], s);
  a.delta[idx] = s;
}

// dQ: a wave owns 32 queries and walks the key tiles
template <int NBLK>
__global__ __launch_bounds__(256) void attn_long_dq_kernel(AttnLongArgs a) {
  extern __shared__ float lds[];
  constexpr int LD = NBLK * 32 + 1, TILE = 32 * LD;
  const int W = blockDim.x >> 6;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
  float *Ks = lds, *Vs = lds + TILE, *Qs = lds + (2 + 2 * wave) * TILE, *Gs = Qs + TILE;
  int grp, nb, h;
  decode_block(a, W, &grp, &nb, &h);
  const int L = a.L, dk = a.dk;
  const int q0 = (grp * W + wave) * 32;
  const float* base = a.qkv + (int64_t)nb * a.bs + (int64_t)h * dk;
  load_tile<NBLK>(Qs, base, a.ss, q0, L, dk, a.scale, lane, 64);
  load_tile<NBLK>(Gs, a.d_o + (int64_t)nb * a.obs + (int64_t)h * dk, a.oss, q0, L, dk, 1.f, lane, 64);
  const bool live = q0 + l31 < L;
  const int64_t row = ((int64_t)(q0 + l31) * a.Nb + nb) * a.heads + h;
  const float lse = live ? a.lse[row] : 0.f, delta = live ? a.delta[row] : 0.f;
  f32x16 dq[NBLK];
#pragma unroll
  for (int b = 0; b < NBLK; ++b)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[b][i] = 0.f;
  for (int k0 = 0; k0 < L; k0 += 32) {
    __syncthreads();
    load_tile<NBLK>(Ks, base + a.E, a.ss, k0, L, dk, 1.f, threadIdx.x, blockDim.x);
    load_tile<NBLK>(Vs, base + 2 * a.E, a.ss, k0, L, dk, 1.f, threadIdx.x, blockDim.x);
    __syncthreads();
    if (q0 >= L) continue;
    f32x16 s, dp;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = dp[i] = 0.f;
    tile_scores<NBLK>(Ks, Qs, dk, l31, half, s);
    tile_scores<NBLK>(Vs, Gs, dk, l31, half, dp);  // dP[query, key] = dO[query] . V[key]
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float p = k0 + reg_row(i, half) < L ? __expf(s[i] - lse) : 0.f;
      s[i] = p * (dp[i] - delta);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float* kp = Ks + reg_row(i, half) * LD + l31;
#pragma unroll
      for (int b = 0; b < NBLK; ++b) dq[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(kp[b * 32], s[i], dq[b], 0, 0, 0);
    }
  }
  __syncthreads();
  store_tile<NBLK>(dq, a.scale, Qs, a.dqkv + (int64_t)nb * a.bs + (int64_t)h * dk, a.ss, q0, L, dk, lane);
}

// dK | dV: a wave owns 32 keys and walks the query tiles
template <int NBLK>
__global__ __launch_bounds__(256) void attn_long_dkv_kernel(AttnLongArgs a) {
  extern __shared__ float lds[];
  constexpr int LD = NBLK * 32 + 1, TILE = 32 * LD;
  const int W = blockDim.x >> 6;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
  float *Qs = lds, *Gs = lds + TILE, *Ks = lds + (2 + 2 * wave) * TILE, *Vs = Ks + TILE;
  float* stat = lds + (2 + 2 * W) * TILE;  // lse[32] | delta[32] of the query tile
  int grp, nb, h;
  decode_block(a, W, &grp, &nb, &h);
  const int L = a.L, dk = a.dk;
  const int kw = (grp * W + wave) * 32;
  const float* base = a.qkv + (int64_t)nb * a.bs + (int64_t)h * dk;
  const float* gbase = a.d_o + (int64_t)nb * a.obs + (int64_t)h * dk;
  load_tile<NBLK>(Ks, base + a.E, a.ss, kw, L, dk, 1.f, lane, 64);
  load_tile<NBLK>(Vs, base + 2 * a.E, a.ss, kw, L, dk, 1.f, lane, 64);
  const bool live = kw + l31 < L;
  f32x16 dkacc[NBLK], dvacc[NBLK];
#pragma unroll
  for (int b = 0; b < NBLK; ++b)
#pragma unroll
    for (int i = 0; i < 16; ++i) dkacc[b][i] = dvacc[b][i] = 0.f;
  for (int q0 = 0; q0 < L; q0 += 32) {
    __syncthreads();
    load_tile<NBLK>(Qs, base, a.ss, q0, L, dk, a.scale, threadIdx.x, blockDim.x);
    load_tile<NBLK>(Gs, gbase, a.oss, q0, L, dk, 1.f, threadIdx.x, blockDim.x);
    if (threadIdx.x < 64) {
      const int q = q0 + (threadIdx.x & 31);
      const int64_t row = ((int64_t)q * a.Nb + nb) * a.heads + h;
      // a query row past L: Q = dO = 0, and with lse = delta = 0 its probability is exp(0) = 1 against zero operands
      stat[threadIdx.x] = q < L ? (threadIdx.x < 32 ? a.lse[row] : a.delta[row]) : 0.f;
    }
    __syncthreads();
    if (kw >= L) continue;
    f32x16 s, dp;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = dp[i] = 0.f;
    tile_scores<NBLK>(Qs, Ks, dk, l31, half, s);   // s[i] = score of (query q0 + reg_row(i), key kw + l31)
    tile_scores<NBLK>(Gs, Vs, dk, l31, half, dp);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = reg_row(i, half);
      const float p = live ? __expf(s[i] - stat[r]) : 0.f;
      s[i] = p;
      dp[i] = p * (dp[i] - stat[32 + r]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = reg_row(i, half);
      const float* gp = Gs + r * LD + l31;
      const float* qp = Qs + r * LD + l31;
#pragma unroll
      for (int b = 0; b < NBLK; ++b) {
        dvacc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(gp[b * 32], s[i], dvacc[b], 0, 0, 0);
        dkacc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(qp[b * 32], dp[i], dkacc[b], 0, 0, 0);  // (Q is stored scaled)
      }
    }
  }
  __syncthreads();
  float* dbase = a.dqkv + (int64_t)nb * a.bs + (int64_t)h * dk;
  store_tile<NBLK>(dkacc, 1.f, Ks, dbase + a.E, a.ss, kw, L, dk, lane);
  store_tile<NBLK>(dvacc, 1.f, Vs, dbase + 2 * a.E, a.ss, kw, L, dk, lane);
}

// ---- launch: one instantiation per padded head width; dynamic LDS above the default limit is granted once per device
constexpr int KIND_FWD = 0, KIND_DQ = 1, KIND_DKV = 2;
std::atomic<uint64_t> g_lds_granted[3][4];

template <int NBLK>
hipError_t launch_attn_kernel(int kind, const AttnLongArgs& a, hipStream_t stream) {
  constexpr size_t TILE = (size_t)32 * (NBLK * 32 + 1) * F32;
  const int W = (kind == KIND_FWD || NBLK <= 2) ? 4 : 2;
  const size_t lds = kind == KIND_FWD ? (2 + W) * TILE : (2 + 2 * W) * TILE + (kind == KIND_DKV ? 64 * F32 : 0);
  const void* fn = kind == KIND_FWD  ? reinterpret_cast<const void*>(&attn_long_fwd_kernel<NBLK>)
                   : kind == KIND_DQ ? reinterpret_cast<const void*>(&attn_long_dq_kernel<NBLK>)
                                     : reinterpret_cast<const void*>(&attn_long_dkv_kernel<NBLK>);
  if (lds > 48 * 1024) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (!(g_lds_granted[kind][NBLK - 1].load(std::memory_order_acquire) & bit)) {
      e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      g_lds_granted[kind][NBLK - 1].fetch_or(bit, std::memory_order_release);
    }
  }
  const int64_t ngrp = (a.L + 32 * W - 1) / (32 * W);
  const dim3 grid((unsigned)(ngrp * a.Nb * a.heads)), block(64 * W);
  if (kind == KIND_FWD) hipLaunchKernelGGL(attn_long_fwd_kernel<NBLK>, grid, block, lds, stream, a);
  else if (kind == KIND_DQ) hipLaunchKernelGGL(attn_long_dq_kernel<NBLK>, grid, block, lds, stream, a);
  else hipLaunchKernelGGL(attn_long_dkv_kernel<NBLK>, grid, block, lds, stream, a);
  return hipGetLastError();
}

hipError_t launch_attn(int kind, const AttnLongArgs& a, hipStream_t stream) {
  switch ((a.dk + 31) / 32) {
    case 1: return launch_attn_kernel<1>(kind, a, stream);
    case 2: return launch_attn_kernel<2>(kind, a, stream);
    case 3: return launch_attn_kernel<3>(kind, a, stream);
    default: return launch_attn_kernel<4>(kind, a, stream);
  }
}

// ---------------------------------------------------------------- pair broadcast / combine
// row (b, i, j):  h_cnn = Hp[b, j-1, 0:E] + Hp[b, j, E:2E] + Hp[b, j+1, 2E:3E] + Cp[b, i, 0:E]   (slots modulo H)
//                 z     = Hp[b, j, 3E:4E] + Cp[b, i, E:2E]
__global__ __launch_bounds__(256) void caum_pair_fwd_kernel(const float* __restrict__ hp, const float* __restrict__ cp, int64_t ldc,
                                                            float* __restrict__ hcnn, float* __restrict__ z, int64_t rows, int C,
                                                            int H, int E) {
  const int64_t n = rows * E;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = idx / E;
    const int e = (int)(idx - r * E);
    const int j = (int)(r % H);
    const int64_t p = r / H, b = p / C;
    const int jl = j == 0 ? H - 1 : j - 1, jr = j == H - 1 ? 0 : j + 1;
    const float* hb = hp + b * H * 4 * (int64_t)E;
    const float* cr = cp + p * ldc;
    hcnn[idx] = hb[(int64_t)jl * 4 * E + e] + hb[(int64_t)j * 4 * E + E + e] + hb[(int64_t)jr * 4 * E + 2 * E + e] + cr[e];
    z[idx] = hb[(int64_t)j * 4 * E + 3 * E + e] + cr[E + e];
  }
}

// dHp: thread (b, j, e) sums over the candidates in order and writes the three shifted destinations (each written once);
// dCp: thread (p, e) sums over the slots in order
__global__ __launch_bounds__(256) void caum_pair_bwd_h_kernel(const float* __restrict__ dh, const float* __restrict__ dz,
                                                              float* __restrict__ dhp, int64_t B, int C, int H, int E) {
  const int64_t n = B * H * E;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
    const int e = (int)(idx % E);
    const int64_t bj = idx / E;
    const int j = (int)(bj % H);
    const int64_t b = bj / H;
    float sh = 0.f, sz = 0.f;
    for (int i = 0; i < C; ++i) {
      const int64_t r = ((b * C + i) * H + j) * E + e;
      sh += dh[r];
      sz += dz[r];
    }
    const int jl = j == 0 ? H - 1 : j - 1, jr = j == H - 1 ? 0 : j + 1;
    float* out = dhp + b * H * 4 * (int64_t)E;
    out[(int64_t)jl * 4 * E + e] = sh;          // slot j read its left neighbour through Wl
    out[(int64_t)j * 4 * E + E + e] = sh;
    out[(int64_t)jr * 4 * E + 2 * E + e] = sh;  // ... and its right neighbour through Wr
    out[(int64_t)j * 4 * E + 3 * E + e] = sz;
  }
}

__global__ __launch_bounds__(256) void caum_pair_bwd_c_kernel(const float* __restrict__ dh, const float* __restrict__ dz,
                                                              float* __restrict__ dcp, int64_t ldc, int64_t P, int H, int E) {
  const int64_t n = P * E;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = idx / E;
    const int e = (int)(idx - p * E);
    float sh = 0.f, sz = 0.f;
    for (int j = 0; j < H; ++j) {
      const int64_t r = (p * H + j) * E + e;
      sh += dh[r];
      sz += dz[r];
    }
    dcp[p * ldc + e] = sh;
    dcp[p * ldc + E + e] = sz;
  }
}

// ---------------------------------------------------------------- t = tanh(pre + cb[pair]) and activation backward
__global__ __launch_bounds__(256) void caum_bias_tanh_fwd_kernel(const float* __restrict__ pre, const float* __restrict__ cb,
                                                                 int64_t ldc, float* __restrict__ t, int64_t rows, int H, int E,
                                                                 int fast) {
  const int64_t n = rows * E;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = idx / E;
    const float v = pre[idx] + cb[(r / H) * ldc + (idx - r * E)];
    t[idx] = fast ? fast_tanh(v) : tanhf(v);
  }
}

__global__ __launch_bounds__(256) void caum_bias_tanh_bwd_kernel(const float* __restrict__ t, const float* __restrict__ dt,
                                                                 float* __restrict__ dpre, float* __restrict__ dcb, int64_t P, int H,
                                                                 int E) {
  const int64_t n = P * E;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = idx / E;
    const int e = (int)(idx - p * E);
    float s = 0.f;
    for (int j = 0; j < H; ++j) {
      const int64_t r = (p * H + j) * E + e;
      const float tv = t[r], g = dt[r] * (1.f - tv * tv);
      dpre[r] = g;
      s += g;
    }
    if (dcb) dcb[idx] = s;
  }
}

__global__ __launch_bounds__(256) void act_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy,
                                                      float* __restrict__ dpre, int64_t n, int act) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
    const float v = y[idx], g = dy[idx];
    dpre[idx] = act == XNRS_ACT_TANH ? g * (1.f - v * v) : act == XNRS_ACT_RELU ? (v > 0.f ? g : 0.f) : g;
  }
}

// ---------------------------------------------------------------- candidate pooling
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// one workgroup per (user, candidate) pair: s_j = w3 . t2[p, j] + b3, a = softmax_j(s), u[p] = sum_j a_j h_all[p, j]
__global__ __launch_bounds__(256) void caum_pool_fwd_kernel(const float* __restrict__ t2, const float* __restrict__ w3,
                                                            const float* __restrict__ b3, const float* __restrict__ hall,
                                                            float* __restrict__ u, float* __restrict__ a_out, int H, int A, int E) {
  extern __shared__ float sc[];  // [H]
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float bias = b3 ? b3[0] : 0.f;
  for (int j = wave; j < H; j += 4) {
    const float* tr = t2 + (p * H + j) * A;
    float s = 0.f;
    for (int k = lane; k < A; k += 64) s = fmaf(tr[k], w3[k], s);
    s = wave_sum(s);
    if (lane == 0) sc[j] = s + bias;
  }
  __syncthreads();
  if (wave == 0) {
    float mx = -INFINITY;
    for (int j = lane; j < H; j += 64) mx = fmaxf(mx, sc[j]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < H; j += 64) {
      const float ev = expf(sc[j] - mx);
      sc[j] = ev;
      sum += ev;
    }
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    for (int j = lane; j < H; j += 64) {
      const float av = sc[j] * inv;
      sc[j] = av;
      if (a_out) a_out[p * H + j] = av;
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < E; e += blockDim.x) {
    float s = 0.f;
    for (int j = 0; j < H; ++j) s = fmaf(sc[j], hall[(p * H + j) * E + e], s);
    u[p * E + e] = s;
  }
}

// da_j = du . h_all[p, j]; ds_j = a_j (da_j - c), c = sum_j a_j da_j / sum_j a_j; dh_all = a_j du; dt2 = ds_j w3; ds kept for dw3.
// c is the a-weighted MEAN of da, taken in double: sum_j ds_j -- the pair's share of db3, a bias in front of a softmax, 0 in
// exact arithmetic -- then cancels down to the rounding of c itself, although the fp32 weights do not sum to exactly 1.  That
// share is evaluated here, in double over the unrounded terms (dbias_out[p]): summed from the rounded fp32 ds_j it carried
// their rounding, ~2^-24 |ds|_2 per pair, several times what is left this way (tests/test_hip_length_limits.py).
__global__ __launch_bounds__(256) void caum_pool_bwd_kernel(const float* __restrict__ t2, const float* __restrict__ w3,
                                                            const float* __restrict__ hall, const float* __restrict__ a,
                                                            const float* __restrict__ du, float* __restrict__ dt2,
                                                            float* __restrict__ dhall, float* __restrict__ ds_out,
                                                            float* __restrict__ dbias_out, int H, int A, int E) {
  extern __shared__ float sc[];  // da / ds [H] | a [H]
  float* av = sc + H;
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* dur = du + p * E;
  for (int j = wave; j < H; j += 4) {
    const float* hr = hall + (p * H + j) * E;
    float s = 0.f;
    for (int e = lane; e < E; e += 64) s = fmaf(dur[e], hr[e], s);
    s = wave_sum(s);
    if (lane == 0) {
      sc[j] = s;
      av[j] = a[p * H + j];
    }
  }
  __syncthreads();
  if (wave == 0) {
    double dot = 0., suma = 0.;
    for (int j = lane; j < H; j += 64) {
      dot += (double)av[j] * (double)sc[j];
      suma += (double)av[j];
    }
    dot = wave_sum(dot);
    suma = wave_sum(suma);
    const float c = (float)(dot / suma);  // (suma = 1 up to rounding: softmax weights)
    double res = 0.;
    for (int j = lane; j < H; j += 64) {
      res += (double)av[j] * ((double)sc[j] - (double)c);
      const float ds = av[j] * (sc[j] - c);
      sc[j] = ds;
      ds_out[p * H + j] = ds;
    }
    res = wave_sum(res);
    if (lane == 0) dbias_out[p] = (float)res;
  }
  __syncthreads();
  if (dhall)
    for (int idx = threadIdx.x; idx < H * E; idx += blockDim.x) dhall[p * H * E + idx] = av[idx / E] * dur[idx % E];
  if (dt2)
    for (int idx = threadIdx.x; idx < H * A; idx += blockDim.x) dt2[p * H * A + idx] = sc[idx / A] * w3[idx % A];
}

// partial[c][k] = sum over the rows of chunk c of ds[r] t2[r, k] (k < A), rows in order; k == A: the sum of the pairs' bias
// shares dbias[p] over chunk c of the PAIRS (pairs_per each)
__global__ __launch_bounds__(256) void caum_pool_dw_kernel(const float* __restrict__ ds, const float* __restrict__ t2,
                                                           const float* __restrict__ dbias, float* __restrict__ partial, int64_t R,
                                                           int A, int64_t rows_per, int64_t P, int64_t pairs_per) {
  const int64_t r0 = blockIdx.x * rows_per, r1 = r0 + rows_per < R ? r0 + rows_per : R;
  const int64_t p0 = blockIdx.x * pairs_per, p1 = p0 + pairs_per < P ? p0 + pairs_per : P;
  for (int k = threadIdx.x; k <= A; k += blockDim.x) {
    float s = 0.f;
    if (k < A) {
      for (int64_t r = r0; r < r1; ++r) s = fmaf(ds[r], t2[r * A + k], s);
    } else {
      double sb = 0.;
      for (int64_t p = p0; p < p1; ++p) sb += (double)dbias[p];
      s = (float)sb;
    }
    partial[(int64_t)blockIdx.x * (A + 1) + k] = s;
  }
}

__global__ __launch_bounds__(256) void caum_pool_dw_final_kernel(const float* __restrict__ partial, int nchunk, int A,
                                                                 float* __restrict__ dw3, float* __restrict__ db3) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > A) return;
  float s = 0.f;
  for (int c = 0; c < nchunk; ++c) s += partial[(int64_t)c * (A + 1) + k];
  if (k < A) {
    if (dw3) dw3[k] = s;
  } else if (db3) {
    db3[0] = s;  // a bias in front of a softmax: sum_j ds_j cancels analytically, what is left is the rounding of each pair's c
  }
}

constexpr int POOL_CHUNKS = 64;
constexpr int POOL_MAX_H = 8192;  // two [H] float arrays of dynamic LDS

unsigned ew_grid(int64_t n) {
  const int64_t g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

bool attn_shape_ok(int64_t L, int64_t Nb, int32_t E, int32_t heads) {
  return L >= 0 && Nb >= 0 && E > 0 && heads > 0 && L < (1LL << 30) && Nb < (1LL << 30) &&
         ((L + 63) / 64) * Nb * heads < (1LL << 31) && L * Nb * 3 * (int64_t)E < (1LL << 40);
}

int32_t attn_check(int64_t L, int64_t Nb, int32_t E, int32_t heads) {
  if (!attn_shape_ok(L, Nb, E, heads)) return XNRS_EINVAL;
  if (E % heads != 0) return XNRS_EHEADS;
  if (E / heads > 128) return XNRS_EUNSUPPORTED;
  return XNRS_OK;
}

size_t attn_rows_bytes(int64_t L, int64_t Nb, int32_t heads) { return align_up((size_t)L * Nb * heads * F32); }

int32_t attn_forward(const float* qkv, int64_t ss, int64_t bs, float* o, int64_t oss, int64_t obs, int64_t L, int64_t Nb, int32_t E,
                     int32_t heads, void* saved, size_t saved_bytes, bool train, hipStream_t stream) {
  XNRS_TRY_RC(attn_check(L, Nb, E, heads));
  if (L == 0 || Nb == 0) return XNRS_OK;
  if (!qkv || !o) return XNRS_EINVAL;
  if (train && (!saved || saved_bytes < attn_rows_bytes(L, Nb, heads))) return XNRS_EWORKSPACE;
  AttnLongArgs a{};
  a.qkv = qkv;
  a.ss = ss;
  a.bs = bs;
  a.o = o;
  a.oss = oss;
  a.obs = obs;
  a.lse = train ? at(saved, 0) : nullptr;
  a.L = (int32_t)L;
  a.Nb = (int32_t)Nb;
  a.heads = heads;
  a.dk = E / heads;
  a.E = E;
  a.scale = 1.f / sqrtf((float)a.dk);
  ProfScope ps(1, 4.0 * (double)L * (double)L * (double)E * (double)Nb, stream);
  XNRS_TRY(launch_attn(KIND_FWD, a, stream));
  return XNRS_OK;
}

}  // namespace

extern "C" {

size_t xnrs_attn_long_saved_bytes(int64_t L, int64_t Nb, int32_t E, int32_t n_heads) {
  return attn_check(L, Nb, E, n_heads) == XNRS_OK ? attn_rows_bytes(L, Nb, n_heads) : 0;
}

size_t xnrs_attn_long_workspace_bytes(int64_t L, int64_t Nb, int32_t E, int32_t n_heads) {
  return attn_check(L, Nb, E, n_heads) == XNRS_OK ? attn_rows_bytes(L, Nb, n_heads) : 0;
}

int32_t xnrs_attn_long_fwd(const float* qkv, int64_t seq_stride, int64_t batch_stride, float* o, int64_t o_seq_stride,
                           int64_t o_batch_stride, int64_t L, int64_t Nb, int32_t E, int32_t n_heads, void* stream) {
  return attn_forward(qkv, seq_stride, batch_stride, o, o_seq_stride, o_batch_stride, L, Nb, E, n_heads, nullptr, 0, false,
                      (hipStream_t)stream);
}

int32_t xnrs_attn_long_fwd_train(const float* qkv, int64_t seq_stride, int64_t batch_stride, float* o, int64_t o_seq_stride,
                                 int64_t o_batch_stride, int64_t L, int64_t Nb, int32_t E, int32_t n_heads, void* saved,
                                 size_t saved_bytes, void* stream) {
  return attn_forward(qkv, seq_stride, batch_stride, o, o_seq_stride, o_batch_stride, L, Nb, E, n_heads, saved, saved_bytes, true,
                      (hipStream_t)stream);
}

int32_t xnrs_attn_long_bwd(const float* qkv, int64_t seq_stride, int64_t batch_stride, const float* o, const float* d_o,
                           int64_t o_seq_stride, int64_t o_batch_stride, const void* saved, size_t saved_bytes, float* dqkv,
                           int64_t L, int64_t Nb, int32_t E, int32_t n_heads, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  XNRS_TRY_RC(attn_check(L, Nb, E, n_heads));
  if (L == 0 || Nb == 0) return XNRS_OK;
  if (!qkv || !o || !d_o || !dqkv || !saved) return XNRS_EINVAL;
  const size_t rows = attn_rows_bytes(L, Nb, n_heads);
  if (saved_bytes < rows) return XNRS_EINVAL;
  if (!ws || ws_bytes < rows) return XNRS_EWORKSPACE;
  AttnLongArgs a{};
  a.qkv = qkv;
  a.ss = seq_stride;
  a.bs = batch_stride;
  a.o = const_cast<float*>(o);
  a.d_o = d_o;
  a.oss = o_seq_stride;
  a.obs = o_batch_stride;
  a.lse = const_cast<float*>(at(saved, 0));
  a.delta = at(ws, 0);
  a.dqkv = dqkv;
  a.L = (int32_t)L;
  a.Nb = (int32_t)Nb;
  a.heads = n_heads;
  a.dk = E / n_heads;
  a.E = E;
  a.scale = 1.f / sqrtf((float)a.dk);
  ProfScope ps(9, 14.0 * (double)L * (double)L * (double)E * (double)Nb, stream);
  const int64_t n = L * Nb * n_heads;
  hipLaunchKernelGGL(attn_long_delta_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  XNRS_TRY(hipGetLastError());
  XNRS_TRY(launch_attn(KIND_DQ, a, stream));
  XNRS_TRY(launch_attn(KIND_DKV, a, stream));
  return XNRS_OK;
}

static bool pair_shape_ok(int64_t B, int32_t C, int32_t H, int32_t E) {
  return B >= 0 && C > 0 && H > 0 && E > 0 && B * C * H * (int64_t)E < (1LL << 40) && B * C * (int64_t)H < (1LL << 31);
}

int32_t xnrs_caum_pair_fwd(const float* hp, const float* cp, int64_t ld_cp, float* h_cnn, float* z, int64_t B, int32_t C,
                           int32_t H, int32_t E, void* stream) {
  if (!pair_shape_ok(B, C, H, E) || ld_cp < 2 * (int64_t)E) return XNRS_EINVAL;
  if (B == 0) return XNRS_OK;
  if (!hp || !cp || !h_cnn || !z) return XNRS_EINVAL;
  const int64_t rows = B * C * H;
  hipLaunchKernelGGL(caum_pair_fwd_kernel, dim3(ew_grid(rows * E)), dim3(256), 0, (hipStream_t)stream, hp, cp, ld_cp, h_cnn, z, rows,
                     C, H, E);
  return hip_rc(hipGetLastError());
}

int32_t xnrs_caum_pair_bwd(const float* d_hcnn, const float* d_z, float* d_hp, float* d_cp, int64_t ld_dcp, int64_t B, int32_t C,
                           int32_t H, int32_t E, void* stream) {
  if (!pair_shape_ok(B, C, H, E) || (d_cp && ld_dcp < 2 * (int64_t)E)) return XNRS_EINVAL;
  if (B == 0) return XNRS_OK;
  if (!d_hcnn || !d_z) return XNRS_EINVAL;
  if (d_hp) {
    hipLaunchKernelGGL(caum_pair_bwd_h_kernel, dim3(ew_grid(B * H * E)), dim3(256), 0, (hipStream_t)stream, d_hcnn, d_z, d_hp, B, C, H,
                       E);
    XNRS_TRY(hipGetLastError());
  }
  if (d_cp) {
    hipLaunchKernelGGL(caum_pair_bwd_c_kernel, dim3(ew_grid(B * C * E)), dim3(256), 0, (hipStream_t)stream, d_hcnn, d_z, d_cp, ld_dcp,
                       B * C, H, E);
    XNRS_TRY(hipGetLastError());
  }
  return XNRS_OK;
}

int32_t xnrs_caum_bias_tanh_fwd(const float* pre, const float* cb, int64_t ld_cb, float* t, int64_t P, int32_t H, int32_t E,
                                void* stream) {
  if (!pair_shape_ok(P, 1, H, E) || ld_cb < E) return XNRS_EINVAL;
  if (P == 0) return XNRS_OK;
  if (!pre || !cb || !t) return XNRS_EINVAL;
  hipLaunchKernelGGL(caum_bias_tanh_fwd_kernel, dim3(ew_grid(P * H * E)), dim3(256), 0, (hipStream_t)stream, pre, cb, ld_cb, t, P * H,
                     H, E, knobs().fast_tanh ? 1 : 0);
  return hip_rc(hipGetLastError());
}

int32_t xnrs_caum_bias_tanh_bwd(const float* t, const float* dt, float* dpre, float* dcb, int64_t P, int32_t H, int32_t E,
                                void* stream) {
  if (!pair_shape_ok(P, 1, H, E)) return XNRS_EINVAL;
  if (P == 0) return XNRS_OK;
  if (!t || !dt || !dpre) return XNRS_EINVAL;
  hipLaunchKernelGGL(caum_bias_tanh_bwd_kernel, dim3(ew_grid(P * E)), dim3(256), 0, (hipStream_t)stream, t, dt, dpre, dcb, P, H, E);
  return hip_rc(hipGetLastError());
}

int32_t xnrs_act_bwd(const float* y, const float* dy, float* dpre, int64_t n, int32_t act, void* stream) {
  if (n < 0 || act < XNRS_ACT_NONE || act > XNRS_ACT_TANH) return XNRS_EINVAL;
  if (n == 0) return XNRS_OK;
  if (!y || !dy || !dpre) return XNRS_EINVAL;
  hipLaunchKernelGGL(act_bwd_kernel, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, y, dy, dpre, n, act);
  return hip_rc(hipGetLastError());
}

static int32_t pool_check(int64_t P, int32_t H, int32_t A, int32_t E) {
  if (P < 0 || H <= 0 || A <= 0 || E <= 0 || P >= (1LL << 31) || P * H * (int64_t)(A > E ? A : E) >= (1LL << 40)) return XNRS_EINVAL;
  return H > POOL_MAX_H ? XNRS_EUNSUPPORTED : XNRS_OK;
}

int32_t xnrs_caum_pool_fwd(const float* t2, const float* w3, const float* b3, const float* h_all, float* u, float* a_out,
                           int64_t P, int32_t H, int32_t A, int32_t E, void* stream) {
  XNRS_TRY_RC(pool_check(P, H, A, E));
  if (P == 0) return XNRS_OK;
  if (!t2 || !w3 || !h_all || !u) return XNRS_EINVAL;
  ProfScope ps(4, 2.0 * (double)P * H * ((double)A + E), (hipStream_t)stream);
  hipLaunchKernelGGL(caum_pool_fwd_kernel, dim3((unsigned)P), dim3(256), (size_t)H * F32, (hipStream_t)stream, t2, w3, b3, h_all, u,
                     a_out, H, A, E);
  return hip_rc(hipGetLastError());
}

size_t xnrs_caum_pool_bwd_workspace_bytes(int64_t P, int32_t H, int32_t A) {
  if (P < 0 || H <= 0 || A <= 0) return 0;
  return carve_total({(size_t)P * H * F32, (size_t)POOL_CHUNKS * (A + 1) * F32, (size_t)P * F32});
}

int32_t xnrs_caum_pool_bwd(const float* t2, const float* w3, const float* h_all, const float* a, const float* du, float* d_t2,
                           float* d_w3, float* d_b3, float* d_hall, int64_t P, int32_t H, int32_t A, int32_t E, void* ws,
                           size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  XNRS_TRY_RC(pool_check(P, H, A, E));
  if (P == 0) {
    if (d_w3) XNRS_TRY(hipMemsetAsync(d_w3, 0, (size_t)A * F32, stream));
    if (d_b3) XNRS_TRY(hipMemsetAsync(d_b3, 0, F32, stream));
    return XNRS_OK;
  }
  if (!t2 || !w3 || !h_all || !a || !du) return XNRS_EINVAL;
  if (!ws || ws_bytes < xnrs_caum_pool_bwd_workspace_bytes(P, H, A)) return XNRS_EWORKSPACE;
  Carver c;
  float* ds = at(ws, c.take((size_t)P * H * F32));
  float* partial = at(ws, c.take((size_t)POOL_CHUNKS * (A + 1) * F32));
  float* dbias = at(ws, c.take((size_t)P * F32));
  hipLaunchKernelGGL(caum_pool_bwd_kernel, dim3((unsigned)P), dim3(256), (size_t)2 * H * F32, stream, t2, w3, h_all, a, du, d_t2,
                     d_hall, ds, dbias, H, A, E);
  XNRS_TRY(hipGetLastError());
  if (d_w3 || d_b3) {
    const int64_t R = P * H;
    const int64_t rows_per = (R + POOL_CHUNKS - 1) / POOL_CHUNKS;
    const int nchunk = (int)((R + rows_per - 1) / rows_per);
    const int64_t pairs_per = (P + nchunk - 1) / nchunk;
    hipLaunchKernelGGL(caum_pool_dw_kernel, dim3((unsigned)nchunk), dim3(256), 0, stream, ds, t2, dbias, partial, R, A, rows_per, P,
                       pairs_per);
    XNRS_TRY(hipGetLastError());
    hipLaunchKernelGGL(caum_pool_dw_final_kernel, dim3((unsigned)((A + 256) / 256)), dim3(256), 0, stream, partial, nchunk, A, d_w3,
                       d_b3);
    XNRS_TRY(hipGetLastError());
  }
  return XNRS_OK;
}

}  // extern "C"
