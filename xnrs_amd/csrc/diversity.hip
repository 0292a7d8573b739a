// Beyond-accuracy kernels over an encoded news table (include/xnrs_hip.h: xnrs_row_inv_norms, xnrs_mmr_rerank,
// xnrs_list_diversity): the reciprocal row norms, greedy MMR (maximal marginal relevance) re-ranking of a deep candidate list
// and the intra-list distance of a recommended list, all on the cosine of two table rows
//   inv[r] = 1 / sqrt(sum_e x[r][e]^2) (0 for a zero row)      cos(a, b) = (sum_e x[a][e] x[b][e]) * inv[a] * inv[b].
//
// The similarity is defined once (wave_cos): a wave holds one row `b` in LDS and gathers up to DV_UNROLL rows `a` from the
// table; lane l takes the elements [4 l, 4 l + 4) + 256 j of a row in ascending j as one fma chain from 0 and a butterfly
// adds the 64 chains.  The order is a function of E alone.  The scalar-load form (E % 4 != 0 or a table off the 16-byte
// boundary) gives a lane the SAME elements in the same order as the 16-byte form: both produce the same bits.  The norms
// are the same sum with a == b (the lane's chain and the butterfly: row_dot.h, shared with list_loss.hip).  This is a row
// gather with no reuse across sessions, so it is VALU work, not MFMA.
//   mmr  : the greedy loop of greedy.h under the penalty m_i, the largest cosine of place i to a selected place.  LDS holds
//          m, the reciprocal norm and the row of each of the P places and the row selected last; a pick is one update of m_i
//          over the alive places, DV_UNROLL rows in flight per wave, against the selected row in LDS.  The pool is streamed
//          again every step (k P E 4 bytes per session, from L2 / Infinity Cache for the pools this is built for); nothing
//          is staged.
//   ild  : one workgroup per session; place i < k - 1 in turn is the row in LDS and the waves take the places j > i in
//          groups.  Lane 0 of a wave adds its terms 1 - cos in the order (i, group, j); the four wave sums are added in
//          wave order: the order is a function of (k, E).  Category counts go through an LDS histogram with integer atomics.
// No workspace, no float atomics, no host synchronisation; a session's bits depend on nothing but its own operands.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "greedy.h"
#include "host.h"
#include "row_dot.h"

namespace xnrs {

namespace {

constexpr int DV_THREADS = GREEDY_THREADS;  // 4 waves per workgroup
constexpr int DV_WAVES = DV_THREADS / 64;
constexpr int DV_UNROLL = 8;     // table rows a wave has in flight against the row in LDS

// the row in LDS of a workgroup: s_row[0, pad4(E)) = table[row][0, E), zeros behind (every thread of the workgroup calls it)
__device__ __forceinline__ void stage_row(float* s_row, const float* __restrict__ table, int64_t row, int E) {
  const float* __restrict__ x = table + row * E;
  for (int e = threadIdx.x; e < pad4(E); e += DV_THREADS) s_row[e] = e < E ? x[e] : 0.f;
}

// THE similarity: cos[q] of table row r[q] (inverse norm inv_r[q]; skipped and 0 where !ok[q]) and the row in LDS (inverse
// norm inv_s), for every lane of the wave.  All lanes of a wave call it with the same arguments.
template <bool VEC>
__device__ __forceinline__ void wave_cos(const float* __restrict__ table, int E, const int (&r)[DV_UNROLL], const bool (&ok)[DV_UNROLL],
                                         const float (&inv_r)[DV_UNROLL], const float* s_row, float inv_s, int lane,
                                         float (&cos)[DV_UNROLL]) {
  float acc[DV_UNROLL];
#pragma unroll
  for (int q = 0; q < DV_UNROLL; ++q) acc[q] = 0.f;
  for (int i = lane * 4; i < E; i += 256) {
    const float4 u = *reinterpret_cast<const float4*>(s_row + i);
    float4 x[DV_UNROLL];
#pragma unroll
    for (int q = 0; q < DV_UNROLL; ++q)
      x[q] = ok[q] ? load4<VEC>(table + (int64_t)r[q] * E, i, E) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int q = 0; q < DV_UNROLL; ++q) acc[q] = dot4(x[q], u, acc[q]);
  }
#pragma unroll
  for (int q = 0; q < DV_UNROLL; ++q) cos[q] = ok[q] ? wave_sum(acc[q]) * inv_r[q] * inv_s : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------ norms
template <bool VEC>
__global__ __launch_bounds__(DV_THREADS) void inv_norms_kernel(const float* __restrict__ table, int64_t n_rows, int E,
                                                               float* __restrict__ inv) {
  const int64_t r = (int64_t)blockIdx.x * DV_WAVES + (threadIdx.x >> 6);
  if (r >= n_rows) return;
  const int lane = threadIdx.x & 63;
  const float* __restrict__ x = table + r * E;
  float acc = 0.f;
  for (int i = lane * 4; i < E; i += 256) {
    const float4 v = load4<VEC>(x, i, E);
    acc = dot4(v, v, acc);
  }
  const float ss = wave_sum(acc);
  if (lane == 0) inv[r] = ss > 0.f ? 1.f / sqrtf(ss) : 0.f;
}

// -------------------------------------------------------------------------------------------------------------------- mmr
struct MmrArgs {
  GreedyArgs g;
  const float* table;
  const float* inv;
  int E;
};

// dynamic LDS of a session, in floats: the scratch words of the loop, the selected row, then lam * r, m, inv, row (int32) per
// place, then the alive bytes (every LDS word of the kernel lies in the dynamic region, every region on 16 bytes)
__host__ __device__ __forceinline__ size_t mmr_lds_bytes(int P, int E) {
  return (size_t)(GREEDY_SCRATCH + pad4(E)) * 4 + (size_t)pad4(P) * 16 + (size_t)pad4(P);
}

// the penalty of MMR (greedy.h): m_i, the largest cosine of place i to a selected place
template <bool VEC>
struct MmrPolicy {
  const float* table;
  const float* inv;
  int E, P;
  float* s_sel;  // the row selected last
  float* s_m;
  float* s_inv;
  int* s_row;
  const unsigned char* s_alive;

  __device__ __forceinline__ void stage(int i, int r, bool ok) {
    s_row[i] = ok ? r : -1;
    s_m[i] = 0.f;
    s_inv[i] = ok ? inv[r] : 0.f;
  }
  __device__ __forceinline__ void prepare(int) {}
  __device__ __forceinline__ float penalty(int i) const { return s_m[i]; }
  // m_i of the alive places against the selected row: wave w takes the groups of DV_UNROLL places w, w + DV_WAVES, ...
  __device__ __forceinline__ void take(int bi, int t, bool last) {
    if (last) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float sel_inv = s_inv[bi];
    stage_row(s_sel, table, s_row[bi], E);  // (every use of the row before lies behind the barrier of the argmax)
    __syncthreads();
    for (int j0 = wave * DV_UNROLL; j0 < P; j0 += DV_WAVES * DV_UNROLL) {
      int r[DV_UNROLL];
      bool ok[DV_UNROLL];
      float ir[DV_UNROLL], c[DV_UNROLL];
      bool any = false;
#pragma unroll
      for (int q = 0; q < DV_UNROLL; ++q) {
        const int j = j0 + q;
        ok[q] = j < P && s_alive[j] != 0;
        r[q] = ok[q] ? s_row[j] : 0;
        ir[q] = ok[q] ? s_inv[j] : 0.f;
        any |= ok[q];
      }
      if (!any) continue;
      wave_cos<VEC>(table, E, r, ok, ir, s_sel, sel_inv, lane, c);
      if (lane == 0) {
        float* m = s_m + j0;  // (one address for the group: written as s_m[j0 + q] it is computed again at every use)
#pragma unroll
        for (int q = 0; q < DV_UNROLL; ++q)
          if (ok[q]) m[q] = t == 0 ? c[q] : fmaxf(m[q], c[q]);
      }
    }
    __syncthreads();
  }
};

template <bool VEC>
__global__ __launch_bounds__(DV_THREADS) void mmr_kernel(MmrArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  const int P = a.g.P, E = a.E;
  float* s_scratch = reinterpret_cast<float*>(s_raw);
  float* s_sel = s_scratch + GREEDY_SCRATCH;
  float* s_lr = s_sel + pad4(E);
  float* s_m = s_lr + pad4(P);
  float* s_inv = s_m + pad4(P);
  int* s_row = reinterpret_cast<int*>(s_inv + pad4(P));
  unsigned char* s_alive = reinterpret_cast<unsigned char*>(s_row + pad4(P));
  MmrPolicy<VEC> pol{a.table, a.inv, E, P, s_sel, s_m, s_inv, s_row, s_alive};
  greedy_stage(a.g, blockIdx.x, s_scratch, s_lr, s_alive, pol);
  __syncthreads();
  greedy_loop(a.g, blockIdx.x, s_scratch, s_lr, s_alive, pol);
}

// -------------------------------------------------------------------------------------------------------------------- ild
struct DivArgs {
  const float* table;
  const float* inv;
  int64_t n_rows;
  int E;
  const int32_t* rows;
  int k;
  const int32_t* row_cat;
  int n_cat;
  float* out_ild;
  int32_t* out_n;
  int32_t* out_ncat;
  int32_t* out_diffcat;
};

// dynamic LDS of a session: the wave sums and the four counts, the row in turn, then inv and row per place, then the
// category histogram
constexpr int DIV_SCRATCH = 8;
__host__ __device__ __forceinline__ size_t div_lds_bytes(int k, int E, int n_cat) {
  return (size_t)(DIV_SCRATCH + pad4(E)) * 4 + (size_t)pad4(k) * 8 + (size_t)n_cat * 4;
}

template <bool VEC>
__global__ __launch_bounds__(DV_THREADS) void div_kernel(DivArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  const int k = a.k, E = a.E;
  float* s_acc = reinterpret_cast<float*>(s_raw);
  int* s_cnt = reinterpret_cast<int*>(s_acc + DV_WAVES);  // valid places, places with a category, distinct categories, pairs of one category
  float* s_sel = s_acc + DIV_SCRATCH;
  float* s_inv = s_sel + pad4(E);
  int* s_row = reinterpret_cast<int*>(s_inv + pad4(k));
  int* s_hist = s_row + pad4(k);
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_cat = a.row_cat ? a.n_cat : 0;
  if (tid < 4) s_cnt[tid] = 0;
  for (int c = tid; c < n_cat; c += DV_THREADS) s_hist[c] = 0;
  __syncthreads();
  for (int i = tid; i < k; i += DV_THREADS) {
    const int r = a.rows[b * k + i];
    const bool ok = r >= 0 && r < a.n_rows;
    s_row[i] = ok ? r : -1;
    s_inv[i] = ok ? a.inv[r] : 0.f;
    if (ok) {
      atomicAdd(&s_cnt[0], 1);
      if (a.row_cat) {
        const int c = a.row_cat[r];
        if (c >= 0 && c < n_cat) {
          const int before = atomicAdd(&s_hist[c], 1);  // (the place pairs with every earlier place of its category)
          atomicAdd(&s_cnt[1], 1);
          if (before == 0) atomicAdd(&s_cnt[2], 1);
          atomicAdd(&s_cnt[3], before);
        }
      }
    }
  }
  __syncthreads();

  float acc = 0.f;  // (lane 0 of every wave)
  for (int i = 0; i + 1 < k; ++i) {
    const int ri = s_row[i];
    if (ri < 0) continue;  // (the same for every thread)
    __syncthreads();       // (the waves are done with the row before)
    stage_row(s_sel, a.table, ri, E);
    __syncthreads();
    const float inv_i = s_inv[i];
    for (int j0 = i + 1 + wave * DV_UNROLL; j0 < k; j0 += DV_WAVES * DV_UNROLL) {
      int r[DV_UNROLL];
      bool ok[DV_UNROLL];
      float ir[DV_UNROLL], c[DV_UNROLL];
      bool any = false;
#pragma unroll
      for (int q = 0; q < DV_UNROLL; ++q) {
        const int j = j0 + q;
        ok[q] = j < k && s_row[j] >= 0;
        r[q] = ok[q] ? s_row[j] : 0;
        ir[q] = ok[q] ? s_inv[j] : 0.f;
        any |= ok[q];
      }
      if (!any) continue;
      wave_cos<VEC>(a.table, E, r, ok, ir, s_sel, inv_i, lane, c);
#pragma unroll
      for (int q = 0; q < DV_UNROLL; ++q)
        if (ok[q]) acc += 1.f - c[q];
    }
  }
  if (lane == 0) s_acc[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    const int n = s_cnt[0];
    const float sum = (s_acc[0] + s_acc[1]) + (s_acc[2] + s_acc[3]);
    a.out_n[b] = n;
    a.out_ild[b] = n >= 2 ? sum / (float)(n * (n - 1) / 2) : 0.f;
    if (a.row_cat) {
      const int nc = s_cnt[1];
      a.out_ncat[b] = s_cnt[2];
      a.out_diffcat[b] = nc * (nc - 1) / 2 - s_cnt[3];
    }
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- launchers
hipError_t launch_row_inv_norms(const float* table, int64_t n_rows, int E, float* inv, hipStream_t stream) {
  if (n_rows <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n_rows + DV_WAVES - 1) / DV_WAVES));
  if (E % 4 == 0 && aligned16(table))
    inv_norms_kernel<true><<<grid, DV_THREADS, 0, stream>>>(table, n_rows, E, inv);
  else
    inv_norms_kernel<false><<<grid, DV_THREADS, 0, stream>>>(table, n_rows, E, inv);
  return hipGetLastError();
}

hipError_t launch_mmr_rerank(const float* table, const float* inv, int64_t n_rows, int E, const int32_t* pool_rows,
                             const float* pool_scores, int64_t B, int P, int k, float lam, int rel_mode, int32_t* out_rows,
                             float* out_scores, int32_t* out_pos, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const MmrArgs a{{pool_rows, pool_scores, P, k, n_rows, lam, rel_mode, out_rows, out_scores, out_pos}, table, inv, E};
  const size_t lds = mmr_lds_bytes(P, E);
  if (E % 4 == 0 && aligned16(table))
    mmr_kernel<true><<<dim3((unsigned)B), DV_THREADS, lds, stream>>>(a);
  else
    mmr_kernel<false><<<dim3((unsigned)B), DV_THREADS, lds, stream>>>(a);
  return hipGetLastError();
}

hipError_t launch_list_diversity(const float* table, const float* inv, int64_t n_rows, int E, const int32_t* rows, int64_t B, int k,
                                 const int32_t* row_cat, int n_cat, float* out_ild, int32_t* out_n, int32_t* out_ncat,
                                 int32_t* out_diffcat, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const DivArgs a{table, inv, n_rows, E, rows, k, row_cat, n_cat, out_ild, out_n, out_ncat, out_diffcat};
  const size_t lds = div_lds_bytes(k, E, row_cat ? n_cat : 0);
  if (E % 4 == 0 && aligned16(table))
    div_kernel<true><<<dim3((unsigned)B), DV_THREADS, lds, stream>>>(a);
  else
    div_kernel<false><<<dim3((unsigned)B), DV_THREADS, lds, stream>>>(a);
  return hipGetLastError();
}

}  // namespace xnrs

using namespace xnrs;

extern "C" {

int32_t xnrs_row_inv_norms(const float* table, int64_t n_rows, int32_t E, float* inv_out, void* stream) {
  if (n_rows < 0 || n_rows > INT32_MAX || E < 1) return XNRS_EINVAL;
  if (n_rows == 0) return XNRS_OK;
  if (!table || !inv_out) return XNRS_EINVAL;
  return hip_rc(launch_row_inv_norms(table, n_rows, E, inv_out, (hipStream_t)stream));
}

int32_t xnrs_mmr_rerank(const float* table, const float* inv, int64_t n_rows, int32_t E, const int32_t* pool_rows,
                        const float* pool_scores, int64_t B, int32_t P, int32_t k, float lam, int32_t rel_mode, int32_t* out_rows,
                        float* out_scores, int32_t* out_pos, void* stream) {
  if (B < 0 || B > INT32_MAX || n_rows < 0 || n_rows > INT32_MAX || E < 1 || E > XNRS_DIVERSITY_MAX_E) return XNRS_EINVAL;
  if (k < 1 || k > P || P > XNRS_TOPK_DEEP_MAX_K) return XNRS_EINVAL;
  if (!(lam >= 0.f && lam <= 1.f)) return XNRS_EINVAL;  // (NaN too)
  if (rel_mode != XNRS_MMR_REL_RAW && rel_mode != XNRS_MMR_REL_MINMAX) return XNRS_EINVAL;
  if (B == 0) return XNRS_OK;
  if (!pool_rows || !pool_scores || !out_rows || !out_scores || !out_pos || (n_rows > 0 && (!table || !inv))) return XNRS_EINVAL;
  return hip_rc(launch_mmr_rerank(table, inv, n_rows, E, pool_rows, pool_scores, B, P, k, lam, rel_mode, out_rows, out_scores,
                                  out_pos, (hipStream_t)stream));
}

int32_t xnrs_list_diversity(const float* table, const float* inv, int64_t n_rows, int32_t E, const int32_t* rows, int64_t B,
                            int32_t k, const int32_t* row_cat, int32_t n_cat, float* out_ild, int32_t* out_n, int32_t* out_ncat,
                            int32_t* out_diffcat, void* stream) {
  if (B < 0 || B > INT32_MAX || n_rows < 0 || n_rows > INT32_MAX || E < 1 || E > XNRS_DIVERSITY_MAX_E) return XNRS_EINVAL;
  if (k < 1 || k > XNRS_TOPK_MAX_K) return XNRS_EINVAL;
  if (n_cat < 0 || n_cat > XNRS_DIVERSITY_MAX_CATEGORIES) return XNRS_EINVAL;
  if (B == 0) return XNRS_OK;
  if (!rows || !out_ild || !out_n || (n_rows > 0 && (!table || !inv)) || (row_cat && (!out_ncat || !out_diffcat))) return XNRS_EINVAL;
  return hip_rc(launch_list_diversity(table, inv, n_rows, E, rows, B, k, row_cat, n_cat, out_ild, out_n, out_ncat, out_diffcat,
                                      (hipStream_t)stream));
}

}  // extern "C"
