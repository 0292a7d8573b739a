// Calibrated lists (include/xnrs_hip.h: xnrs_csr_category_counts, xnrs_calibrated_rerank, xnrs_list_calibration): the
// category histogram of CSR lists, the greedy re-ranking of a deep candidate list towards a target category mix (Steck,
// "Calibrated Recommendations", RecSys 2018) and the miscalibration of a list.  Only categories are read, never a news vector.
//
// Everything rests on three device functions, each called by every thread of a workgroup of 4 waves:
//   block_sum2   two fp32 sums at once: thread t adds its terms c = t, t + 256, ... in ascending c as a chain from 0, a
//                butterfly adds the 64 chains of a wave, the four wave sums are added as (w0 + w1) + (w2 + w3).  The order is a
//                function of n_cat alone.
//   stage_target p_c = w_c / W into LDS (w_c counts when finite and > 0, W their block_sum2); false when W == 0
//   block_kl     sum over c with p_c > 0 of kl_term(p_c, n_c, N) = p_c logf(p_c / ((1 - alpha) n_c / N + alpha p_c)) (n_c / N
//                is 0 at N == 0), again a block_sum2 -- beside it the same sum at N + 1, which the greedy needs
// kl_term rounds every operation on its own (no contraction) and calls logf (OCML).  xnrs_list_calibration's out_kl and the
// out_kl of xnrs_calibrated_rerank are both block_kl over LDS counts: the same bits for the same counts.
//   rerank : the greedy loop of greedy.h under the penalty KL(p || mix of the picks with the place added); LDS holds the
//            category of each of the P places, and p, the counts and the penalty of each of the n_cat categories.  Before a
//            step's argmax (1) every category's term at N + 1 goes to LDS while block_kl adds them to S1 and the terms at N to
//            S0; (2) pen[c] = (S1 - term_c(n_c)) + term_c(n_c + 1), a place without a category takes S0; thread 0 counts the
//            pick.  A session without a target skips (1) and (2): its penalty is 0.
//   counts : one workgroup per list, an LDS histogram with integer atomics, every output word written.
// Every load is of one element (4 bytes; the CSR offsets 8): an operand may sit at any address of its element type, and no
// second code path exists.  No workspace, no float atomics, no host synchronisation; a session's bits depend on its own
// operands alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "greedy.h"
#include "host.h"

namespace xnrs {

namespace {

constexpr int CB_THREADS = GREEDY_THREADS;  // 4 waves per workgroup
constexpr int CB_WAVES = GREEDY_WAVES;
constexpr int CB_SCRATCH = GREEDY_SCRATCH;  // words in front of the dynamic LDS: two sums or an argmax per wave, the integer counters

// (a, b) summed over the workgroup in the order of the header; red: 2 * CB_WAVES floats nobody else writes.  The barrier in
// front keeps a second call from overwriting sums a slower wave has yet to read.
__device__ __forceinline__ void block_sum2(float& a, float& b, float* red) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    a += __shfl_xor(a, m);
    b += __shfl_xor(b, m);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = a;
    red[CB_WAVES + (threadIdx.x >> 6)] = b;
  }
  __syncthreads();
  a = (red[0] + red[1]) + (red[2] + red[3]);
  b = (red[CB_WAVES] + red[CB_WAVES + 1]) + (red[CB_WAVES + 2] + red[CB_WAVES + 3]);
}

__device__ __forceinline__ bool counts_weight(float w) { return w > 0.f && w < INFINITY; }  // (NaN compares false)

// s_p[c] = p_c; true when the session has a target.  (Ends in a barrier: s_p is readable.)
__device__ __forceinline__ bool stage_target(const float* __restrict__ target, int n_cat, float* s_p, float* red) {
  float W = 0.f, none = 0.f;
  for (int c = threadIdx.x; c < n_cat; c += CB_THREADS) {
    const float w = target[c];
    if (counts_weight(w)) W += w;
  }
  block_sum2(W, none, red);
  for (int c = threadIdx.x; c < n_cat; c += CB_THREADS) {
    const float w = target[c];
    s_p[c] = (W > 0.f && counts_weight(w)) ? w / W : 0.f;
  }
  __syncthreads();
  return W > 0.f;
}

// one category's share of the penalty with n of N categorised picks in it; every operation rounded on its own
__device__ __forceinline__ float kl_term(float p, int n, int N, float oma, float alpha) {
#pragma clang fp contract(off)
  if (!(p > 0.f)) return 0.f;
  const float frac = N > 0 ? (float)n / (float)N : 0.f;
  const float mix = oma * frac;
  const float floor_ = alpha * p;
  const float q = mix + floor_;
  return p * logf(p / q);
}

// THE miscalibration: sum_c kl_term(p_c, n_c, N), for every thread.  next (nullable): beside it the sum at N + 1 (returned
// through s1), whose terms are left in next[c].
__device__ __forceinline__ float block_kl(const float* s_p, const int* s_cnt, int n_cat, int N, float oma, float alpha, float* red,
                                          float* next, float* s1) {
  float a = 0.f, b = 0.f;
  for (int c = threadIdx.x; c < n_cat; c += CB_THREADS) {
    const float p = s_p[c];
    const int n = s_cnt[c];
    a += kl_term(p, n, N, oma, alpha);
    if (next) {
      const float t = kl_term(p, n, N + 1, oma, alpha);
      next[c] = t;
      b += t;
    }
  }
  block_sum2(a, b, red);
  if (s1) *s1 = b;
  return a;
}

// ------------------------------------------------------------------------------------------------------------ CSR counts
__global__ __launch_bounds__(CB_THREADS) void csr_counts_kernel(const int64_t* __restrict__ off, const int32_t* __restrict__ rows,
                                                                const int32_t* __restrict__ row_cat, int64_t n_rows, int n_cat,
                                                                int pad_row, int32_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  int* s_cnt = reinterpret_cast<int*>(s_raw);
  const int64_t b = blockIdx.x;
  for (int c = threadIdx.x; c < n_cat; c += CB_THREADS) s_cnt[c] = 0;
  __syncthreads();
  const int64_t end = off[b + 1];
  for (int64_t j = off[b] + threadIdx.x; j < end; j += CB_THREADS) {
    const int r = rows[j];
    if (r < 0 || r >= n_rows || r == pad_row) continue;
    const int c = row_cat[r];
    if (c >= 0 && c < n_cat) atomicAdd(&s_cnt[c], 1);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < n_cat; c += CB_THREADS) out[b * n_cat + c] = s_cnt[c];
}

// --------------------------------------------------------------------------------------------------------------- rerank
struct CalArgs {
  GreedyArgs g;
  const int32_t* row_cat;
  int n_cat;
  const float* target;
  float alpha;
  float* out_kl;
};

// (S1 - term_c(n_c)) + term_c(n_c + 1), each rounded
__device__ __forceinline__ float cal_penalty(float s1, float now, float then) {
#pragma clang fp contract(off)
  const float rest = s1 - now;
  return rest + then;
}

// dynamic LDS of a session: the scratch words, then lam * r and the category (int32) per place, then p, the counts and the
// penalty per category, then the alive bytes
__host__ __device__ __forceinline__ size_t cal_lds_bytes(int P, int n_cat) {
  return (size_t)CB_SCRATCH * 4 + (size_t)pad4(P) * 8 + (size_t)pad4(n_cat) * 12 + (size_t)pad4(P);
}

// the penalty of calibration (greedy.h): the miscalibration of the picks so far with place i added
struct CalPolicy {
  const int32_t* row_cat;
  int C;
  float alpha, oma;
  float* s_red;
  int* s_cat;
  const float* s_p;
  int* s_cnt;
  float* s_pen;
  bool has_target = false;
  int N = 0;         // categorised picks so far (the same in every thread)
  float pen0 = 0.f;  // the penalty of a place without a category

  // the category is read for a valid place only
  __device__ __forceinline__ void stage(int i, int r, bool ok) {
    int c = -1;
    if (ok) {
      c = row_cat[r];
      if (c < 0 || c >= C) c = -1;
    }
    s_cat[i] = c;
  }
  __device__ __forceinline__ void prepare(int) {
    if (has_target) {
      float s1;
      pen0 = block_kl(s_p, s_cnt, C, N, oma, alpha, s_red, s_pen, &s1);  // s_pen[c] = term_c(n_c) at N + 1 for now
      for (int c = threadIdx.x; c < C; c += CB_THREADS)                  // (a thread rewrites the categories it wrote)
        s_pen[c] = cal_penalty(s1, s_pen[c], kl_term(s_p[c], s_cnt[c] + 1, N + 1, oma, alpha));
    }
    __syncthreads();
  }
  __device__ __forceinline__ float penalty(int i) const {
    const int c = s_cat[i];
    return !has_target ? 0.f : (c >= 0 ? s_pen[c] : pen0);
  }
  // the last pick is counted too: out_kl is over all of them
  __device__ __forceinline__ void take(int bi, int, bool) {
    const int c = s_cat[bi];
    if (c >= 0) {
      if (threadIdx.x == 0) s_cnt[c] += 1;
      ++N;
    }
    __syncthreads();  // (the pick is counted before the next step's sums; the argmax words are read before block_sum2 writes over them)
  }
};

__global__ __launch_bounds__(CB_THREADS) void cal_kernel(CalArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  const int P = a.g.P, C = a.n_cat;
  float* s_red = reinterpret_cast<float*>(s_raw);  // the scratch words of the loop; [0, 2 * CB_WAVES) are block_sum2's too
  float* s_lr = s_red + CB_SCRATCH;
  int* s_cat = reinterpret_cast<int*>(s_lr + pad4(P));
  float* s_p = reinterpret_cast<float*>(s_cat + pad4(P));
  int* s_cnt = reinterpret_cast<int*>(s_p + pad4(C));
  float* s_pen = reinterpret_cast<float*>(s_cnt + pad4(C));
  unsigned char* s_alive = reinterpret_cast<unsigned char*>(s_pen + pad4(C));
  const int64_t b = blockIdx.x;
  CalPolicy pol{a.row_cat, C, a.alpha, 1.f - a.alpha, s_red, s_cat, s_p, s_cnt, s_pen};
  for (int c = threadIdx.x; c < C; c += CB_THREADS) s_cnt[c] = 0;
  greedy_stage(a.g, b, s_red, s_lr, s_alive, pol);
  pol.has_target = stage_target(a.target + b * (int64_t)C, C, s_p, s_red);  // (its barriers cover the loops above)
  greedy_loop(a.g, b, s_red, s_lr, s_alive, pol);
  float kl = 0.f;
  if (pol.has_target) kl = block_kl(s_p, s_cnt, C, pol.N, pol.oma, pol.alpha, s_red, nullptr, nullptr);
  if (threadIdx.x == 0) a.out_kl[b] = kl;
}

// ------------------------------------------------------------------------------------------------------ list calibration
struct ListCalArgs {
  const int32_t* rows;
  int k;
  const int32_t* row_cat;
  int64_t n_rows;
  int n_cat;
  const float* target;
  float alpha;
  float* out_kl;
  int32_t* out_n;
  int32_t* out_counts;
};

// dynamic LDS of a list: the scratch words, then p and the counts per category
__host__ __device__ __forceinline__ size_t listcal_lds_bytes(int n_cat) { return (size_t)CB_SCRATCH * 4 + (size_t)pad4(n_cat) * 8; }

__global__ __launch_bounds__(CB_THREADS) void listcal_kernel(ListCalArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  const int C = a.n_cat, k = a.k;
  float* s_red = reinterpret_cast<float*>(s_raw);
  int* s_n = reinterpret_cast<int*>(s_red + 2 * CB_WAVES);
  float* s_p = s_red + CB_SCRATCH;
  int* s_cnt = reinterpret_cast<int*>(s_p + pad4(C));
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid == 0) *s_n = 0;
  for (int c = tid; c < C; c += CB_THREADS) s_cnt[c] = 0;
  __syncthreads();
  for (int i = tid; i < k; i += CB_THREADS) {
    const int r = a.rows[b * k + i];
    if (r < 0 || r >= a.n_rows) continue;
    const int c = a.row_cat[r];
    if (c >= 0 && c < C) {
      atomicAdd(&s_cnt[c], 1);
      atomicAdd(s_n, 1);
    }
  }
  const bool has_target = stage_target(a.target + b * (int64_t)C, C, s_p, s_red);  // (its barriers cover the histogram)
  const int N = *s_n;
  const float alpha = a.alpha, oma = 1.f - a.alpha;
  float kl = 0.f;
  if (has_target) kl = block_kl(s_p, s_cnt, C, N, oma, alpha, s_red, nullptr, nullptr);
  if (tid == 0) {
    a.out_kl[b] = kl;
    a.out_n[b] = N;
  }
  if (a.out_counts)
    for (int c = tid; c < C; c += CB_THREADS) a.out_counts[b * C + c] = s_cnt[c];
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- launchers
hipError_t launch_csr_category_counts(const int64_t* off, const int32_t* rows, int64_t B, const int32_t* row_cat, int64_t n_rows,
                                      int n_cat, int pad_row, int32_t* counts_out, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  csr_counts_kernel<<<dim3((unsigned)B), CB_THREADS, (size_t)n_cat * 4, stream>>>(off, rows, row_cat, n_rows, n_cat, pad_row,
                                                                                  counts_out);
  return hipGetLastError();
}

hipError_t launch_calibrated_rerank(const int32_t* pool_rows, const float* pool_scores, int64_t B, int P, int k,
                                    const int32_t* row_cat, int64_t n_rows, int n_cat, const float* target, float lam, float alpha,
                                    int rel_mode, int32_t* out_rows, float* out_scores, int32_t* out_pos, float* out_kl,
                                    hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const CalArgs a{{pool_rows, pool_scores, P, k, n_rows, lam, rel_mode, out_rows, out_scores, out_pos}, row_cat, n_cat, target, alpha,
                  out_kl};
  cal_kernel<<<dim3((unsigned)B), CB_THREADS, cal_lds_bytes(P, n_cat), stream>>>(a);
  return hipGetLastError();
}

hipError_t launch_list_calibration(const int32_t* rows, int64_t B, int k, const int32_t* row_cat, int64_t n_rows, int n_cat,
                                   const float* target, float alpha, float* out_kl, int32_t* out_n, int32_t* out_counts,
                                   hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const ListCalArgs a{rows, k, row_cat, n_rows, n_cat, target, alpha, out_kl, out_n, out_counts};
  listcal_kernel<<<dim3((unsigned)B), CB_THREADS, listcal_lds_bytes(n_cat), stream>>>(a);
  return hipGetLastError();
}

}  // namespace xnrs

using namespace xnrs;

extern "C" {

int32_t xnrs_csr_category_counts(const int64_t* off, const int32_t* rows, int64_t B, const int32_t* row_cat, int64_t n_rows,
                                 int32_t n_cat, int32_t pad_row, int32_t* counts_out, void* stream) {
  if (B < 0 || B > INT32_MAX || n_rows < 0 || n_rows > INT32_MAX) return XNRS_EINVAL;
  if (n_cat < 1 || n_cat > XNRS_DIVERSITY_MAX_CATEGORIES) return XNRS_EINVAL;
  if (B == 0) return XNRS_OK;
  if (!off || !counts_out || (n_rows > 0 && !row_cat)) return XNRS_EINVAL;  // (rows may be NULL: every list may be empty)
  return hip_rc(launch_csr_category_counts(off, rows, B, row_cat, n_rows, n_cat, pad_row, counts_out, (hipStream_t)stream));
}

int32_t xnrs_calibrated_rerank(const int32_t* pool_rows, const float* pool_scores, int64_t B, int32_t P, int32_t k,
                               const int32_t* row_cat, int64_t n_rows, int32_t n_cat, const float* target, float lam, float alpha,
                               int32_t rel_mode, int32_t* out_rows, float* out_scores, int32_t* out_pos, float* out_kl,
                               void* stream) {
  if (B < 0 || B > INT32_MAX || n_rows < 0 || n_rows > INT32_MAX) return XNRS_EINVAL;
  if (k < 1 || k > P || P > XNRS_TOPK_DEEP_MAX_K) return XNRS_EINVAL;
  if (n_cat < 1 || n_cat > XNRS_DIVERSITY_MAX_CATEGORIES) return XNRS_EINVAL;
  if (!(lam >= 0.f && lam <= 1.f) || !(alpha > 0.f && alpha < 1.f)) return XNRS_EINVAL;  // (NaN too)
  if (rel_mode != XNRS_MMR_REL_RAW && rel_mode != XNRS_MMR_REL_MINMAX) return XNRS_EINVAL;
  if (B == 0) return XNRS_OK;
  if (!pool_rows || !pool_scores || !target || !out_rows || !out_scores || !out_pos || !out_kl || (n_rows > 0 && !row_cat))
    return XNRS_EINVAL;
  return hip_rc(launch_calibrated_rerank(pool_rows, pool_scores, B, P, k, row_cat, n_rows, n_cat, target, lam, alpha, rel_mode,
                                         out_rows, out_scores, out_pos, out_kl, (hipStream_t)stream));
}

int32_t xnrs_list_calibration(const int32_t* rows, int64_t B, int32_t k, const int32_t* row_cat, int64_t n_rows, int32_t n_cat,
                              const float* target, float alpha, float* out_kl, int32_t* out_n, int32_t* out_counts, void* stream) {
  if (B < 0 || B > INT32_MAX || n_rows < 0 || n_rows > INT32_MAX) return XNRS_EINVAL;
  if (k < 1 || k > XNRS_TOPK_DEEP_MAX_K) return XNRS_EINVAL;
  if (n_cat < 1 || n_cat > XNRS_DIVERSITY_MAX_CATEGORIES) return XNRS_EINVAL;
  if (!(alpha > 0.f && alpha < 1.f)) return XNRS_EINVAL;  // (NaN too)
  if (B == 0) return XNRS_OK;
  if (!rows || !target || !out_kl || !out_n || (n_rows > 0 && !row_cat)) return XNRS_EINVAL;
  return hip_rc(launch_list_calibration(rows, B, k, row_cat, n_rows, n_cat, target, alpha, out_kl, out_n, out_counts,
                                        (hipStream_t)stream));
}

}  // extern "C"
