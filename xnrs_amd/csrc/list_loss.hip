// The softmax ranking loss over per-user row LISTS (xnrs_list_loss_fwd / _bwd, include/xnrs_hip.h): the reference's
// ranking_loss(p, n) with the m negatives a caller lists per user (mined by xnrs_topk_deep, sampled, stale) instead of the
// whole table, forward and backward, without a (B, L, E) copy of the listed rows.
//
// The work is a row gather with no reuse across users (every user lists other rows), so it is VALU work, not MFMA:
//   forward : one workgroup of 4 waves per user.  A wave takes 4 slots at a time, gathers the 4 table rows (16-byte loads
//             per lane where the operands allow it) against the user vector in LDS and reduces each dot product with a
//             butterfly; the scores go to neg_scores, then the workgroup folds max and sum exp over the L slots and the
//             waves score the user's queries.
//   d_up    : the same walk; a wave adds ds * table[row] for its slots in ascending slot order, the four wave partials
//             are added in wave order through LDS.
//   d_table : `order` lists the entries (slots, then queries) grouped by row.  The sorted positions are cut into G equal
//             spans, one wave per span (G <= LL_SPANS, the cut is computed on the device from the position count).  A wave
//             takes its span in pieces of 64 positions and decodes a piece with one lane per position (entry -> row, user, ds), then
//             walks it: it adds ds * up[user] in order and stores the sum whenever the row changes.  A run of equal rows
//             that lies inside a span is stored straight into d_table; the first and the last run of a span may continue
//             in the neighbours, so they go to the workspace (one head and one tail row per span), and a second launch
//             adds the pieces of every such run in ascending span order.  However long a run is -- a popular news listed
//             by every user of the batch -- it is cut at the span bounds and summed by as many waves as it touches.
// Every sum has one fixed order (slot position, wave index, sorted position, span index): no float atomics, the same
// bits on every run; scores, lse, loss and d_up of a user depend on nothing but that user's operands.
// The scalar-load forms (E % 4 != 0 or a base off the 16-byte boundary) give a lane the SAME elements in the same order
// as the 16-byte forms, so both produce the same bits.
//
// The soft-target loss over the same lists (xnrs_list_xent_fwd / _bwd) lives here too: a weight per slot and no queries,
// loss[b] = sum w (lse - s), d s = g (W p - w).  It runs the SAME slot scoring, slot sums, walk and join -- the forward and
// d_up kernels differ in what follows the slot scores, the walk in the decode of a sorted position (RankDecode / XentDecode).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "host.h"
#include "row_dot.h"

namespace xnrs {

namespace {

constexpr int LL_THREADS = 256;     // 4 waves per workgroup
constexpr int LL_WAVES = LL_THREADS / 64;
constexpr int LL_UNROLL = 4;        // slots / positions a wave has in flight
constexpr int LL_UP_LDS = 4096;     // floats of a user vector kept in LDS (longer ones are read from global memory)
constexpr int LL_PIECE = 64;        // sorted positions a wave decodes at once, one per lane
constexpr int LL_SPANS = 8192;      // most spans (waves) of the d_table walk
constexpr int LL_NO_RUN = -2;       // tail_row of a span that is one run (or empty); -1 is the "row" of entries without a gradient

struct ListArgs {
  const float* table;
  const float* up;
  const float* bias;
  int64_t n_rows;
  int E;
  int64_t B;
  const int64_t* tgt_off;
  const int32_t* tgt_rows;
  const int32_t* neg_rows;
  int L;
  int pad_row;
  float* scores;      // (T)
  float* lse;         // (B)
  float* neg_scores;  // (B, L)
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}

template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ p, int i, int E, float4 v) {
  if constexpr (VEC) {
    *reinterpret_cast<float4*>(p + i) = v;
  } else {
    if (i < E) p[i] = v.x;
    if (i + 1 < E) p[i + 1] = v.y;
    if (i + 2 < E) p[i + 2] = v.z;
    if (i + 3 < E) p[i + 3] = v.w;
  }
}
__device__ __forceinline__ void axpy4(float4& acc, float s, float4 x) {
  acc.x = fmaf(s, x.x, acc.x);
  acc.y = fmaf(s, x.y, acc.y);
  acc.z = fmaf(s, x.z, acc.z);
  acc.w = fmaf(s, x.w, acc.w);
}

// is row r one of the n rows at t?  (all lanes of the wave call it with the same arguments)
__device__ __forceinline__ bool wave_listed(const int32_t* __restrict__ t, int64_t n, int r, int lane) {
  bool hit = false;
  for (int64_t k = lane; k < n; k += 64) hit |= t[k] == r;
  return __any(hit);
}

// logaddexp(s, l) - s for finite s and finite l
__device__ __forceinline__ float loss_of(float s, float l) {
  const float d = l - s;
  return d <= 0.f ? log1pf(expf(d)) : d + log1pf(expf(-d));
}
// 1 - p = sigmoid(l - s), p = exp(s - logaddexp(s, l))
__device__ __forceinline__ float one_minus_p(float s, float l) {
  const float d = s - l;
  if (d >= 0.f) {
    const float t = expf(-d);
    return t / (1.f + t);
  }
  return 1.f / (1.f + expf(d));
}
// c_b = sum_{e of b} g_e (1 - p_e) in query order; 0 for a user without negatives
__device__ __forceinline__ float user_coef(const ListArgs& a, const float* __restrict__ g, int64_t b) {
  const float l = a.lse[b];
  if (!(l > -INFINITY)) return 0.f;
  float c = 0.f;
  for (int64_t e = a.tgt_off[b]; e < a.tgt_off[b + 1]; ++e) {
    const float s = a.scores[e];
    if (s == s) c += g[e] * one_minus_p(s, l);
  }
  return c;
}

// the user vector of the workgroup: in LDS up to LL_UP_LDS floats, else where it lies
template <bool VEC>
__device__ __forceinline__ float4 up4(const float* __restrict__ s_up, const float* __restrict__ g_up, int i, int E) {
  if (E <= LL_UP_LDS) return load4<VEC>(s_up, i, E);
  return load4<VEC>(g_up, i, E);
}

// ------------------------------------------------------------------------------------------ the slots of one user (forward)
// What both losses do with the L slots of the workgroup's user; they differ in which slots count and in the loss behind.
struct UserSlots {
  const float* table;
  int64_t n_rows;
  int E, L, pad_row;
  const int32_t* rows;  // the L rows of the user
  const float* gu;      // the user vector in global memory
  float bias;
};

// the user vector of the workgroup into LDS (up to LL_UP_LDS floats)
__device__ __forceinline__ void stage_up(float* __restrict__ s_up, const float* __restrict__ gu, int E, int tid) {
  if (E <= LL_UP_LDS)
    for (int i = tid; i < E; i += LL_THREADS) s_up[i] = gu[i];
  __syncthreads();
}

// ns[j] = the score of slot j, NaN for an empty one: wave w takes the groups of LL_UNROLL slots w, w + LL_WAVES, ...
// empty(row): beyond "outside the table or the pad row", is this row's slot empty?  (wave-uniform)
template <bool VEC, class Empty>
__device__ __forceinline__ void score_slots(const UserSlots& u, const float* __restrict__ s_up, float* ns, int tid, Empty empty) {
  const int lane = tid & 63, wave = tid >> 6;
  const int E = u.E, L = u.L;
  for (int j0 = wave * LL_UNROLL; j0 < L; j0 += LL_WAVES * LL_UNROLL) {
    int r[LL_UNROLL];
    bool ok[LL_UNROLL];
    float acc[LL_UNROLL];
#pragma unroll
    for (int q = 0; q < LL_UNROLL; ++q) {
      const int j = j0 + q;
      r[q] = j < L ? u.rows[j] : -1;
      ok[q] = r[q] >= 0 && r[q] < u.n_rows && r[q] != u.pad_row;
      if (ok[q]) ok[q] = !empty(r[q]);
      acc[q] = 0.f;
    }
    for (int i = lane * 4; i < E; i += 256) {
      const float4 v = up4<VEC>(s_up, u.gu, i, E);
      float4 x[LL_UNROLL];
#pragma unroll
      for (int q = 0; q < LL_UNROLL; ++q)
        x[q] = ok[q] ? load4<VEC>(u.table + (int64_t)r[q] * E, i, E) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int q = 0; q < LL_UNROLL; ++q) acc[q] = dot4(x[q], v, acc[q]);
    }
#pragma unroll
    for (int q = 0; q < LL_UNROLL; ++q) {
      const float s = wave_sum(acc[q]) + u.bias;
      if (lane == 0 && j0 + q < L) ns[j0 + q] = ok[q] ? s : NAN;
    }
  }
  __syncthreads();  // (the slot scores of the workgroup are visible to all its threads)
}

// a sum over the L slots of the workgroup's user, the same value in every thread: thread t folds the slots t, t + 256, ...
// in ascending order (acc = fold(j, acc)), a butterfly adds the lanes, the four waves are added as (0 + 1) + (2 + 3).
// (s_red may still be read by a slower wave when this is called twice in a row: the barrier in front)
template <class Fold>
__device__ __forceinline__ float slot_sum(int L, float* s_red, int tid, Fold fold) {
  float sum = 0.f;
  for (int j = tid; j < L; j += LL_THREADS) sum = fold(j, sum);
  sum = wave_sum(sum);
  __syncthreads();
  if ((tid & 63) == 0) s_red[tid >> 6] = sum;
  __syncthreads();
  return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// lse = m + log_sum over the filled slots (ns not NaN): m their maximum, log_sum = log sum exp(s - m); -inf without one
__device__ __forceinline__ float slot_lse(const float* ns, int L, float* s_red, int tid, float& m, float& log_sum) {
  m = -INFINITY;
  for (int j = tid; j < L; j += LL_THREADS) {
    const float s = ns[j];
    if (s == s) m = fmaxf(m, s);
  }
  m = wave_max(m);
  if ((tid & 63) == 0) s_red[tid >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
  const float mx = m;
  const float sum = slot_sum(mx > -INFINITY ? L : 0, s_red, tid, [&](int j, float acc) {
    const float s = ns[j];
    return s == s ? acc + expf(s - mx) : acc;
  });
  log_sum = logf(sum);
  return m > -INFINITY ? m + log_sum : -INFINITY;
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <bool VEC>
__global__ __launch_bounds__(LL_THREADS) void ll_fwd_kernel(ListArgs a, float* __restrict__ loss) {
  __shared__ __attribute__((aligned(16))) float s_up[LL_UP_LDS];
  __shared__ float s_red[LL_WAVES];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int E = a.E, L = a.L;
  const float* __restrict__ gu = a.up + b * E;
  stage_up(s_up, gu, E, tid);
  const float bias = a.bias ? a.bias[0] : 0.f;
  const int64_t t0 = a.tgt_off[b], t1 = a.tgt_off[b + 1];
  float* ns = a.neg_scores + b * (int64_t)L;  // (written here and read back behind the barrier)
  // a user's own click is never their negative
  score_slots<VEC>(UserSlots{a.table, a.n_rows, E, L, a.pad_row, a.neg_rows + b * (int64_t)L, gu, bias}, s_up, ns, tid,
                   [&](int r) { return wave_listed(a.tgt_rows + t0, t1 - t0, r, lane); });
  float m, log_sum;
  const float lse = slot_lse(ns, L, s_red, tid, m, log_sum);
  if (tid == 0) a.lse[b] = lse;

  // the queries of the user: one wave per query
  for (int64_t e = t0 + wave; e < t1; e += LL_WAVES) {
    const int t = a.tgt_rows[e];
    const bool ok = t >= 0 && t < a.n_rows && t != a.pad_row;
    float acc = 0.f;
    if (ok)
      for (int i = lane * 4; i < E; i += 256) acc = dot4(load4<VEC>(a.table + (int64_t)t * E, i, E), up4<VEC>(s_up, gu, i, E), acc);
    const float s = wave_sum(acc) + bias;
    if (lane == 0) {
      a.scores[e] = ok ? s : NAN;
      loss[e] = ok && lse > -INFINITY ? loss_of(s, lse) : 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ d_up
// the end of a 256-feature pass: the four wave partials are added in wave order through LDS and wave 0 stores the sum
template <bool VEC>
__device__ __forceinline__ void store_wave_sum(float (*s_part)[256], float4 acc, float* __restrict__ dst, int i, int E, int lane,
                                               int wave) {
  *reinterpret_cast<float4*>(&s_part[wave][lane * 4]) = acc;
  __syncthreads();
  if (wave == 0 && i < E) {
    float4 r = *reinterpret_cast<const float4*>(&s_part[0][lane * 4]);
#pragma unroll
    for (int w = 1; w < LL_WAVES; ++w) {
      const float4 p = *reinterpret_cast<const float4*>(&s_part[w][lane * 4]);
      r.x += p.x;
      r.y += p.y;
      r.z += p.z;
      r.w += p.w;
    }
    store4<VEC>(dst, i, E, r);
  }
  __syncthreads();
}

template <bool VEC>
__global__ __launch_bounds__(LL_THREADS) void ll_dup_kernel(ListArgs a, const float* __restrict__ g, float* __restrict__ d_up) {
  __shared__ __attribute__((aligned(16))) float s_part[LL_WAVES][256];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int E = a.E, L = a.L;
  const float lse = a.lse[b];
  const float c = user_coef(a, g, b);  // (every thread the same sum in the same order)
  const int64_t t0 = a.tgt_off[b], t1 = a.tgt_off[b + 1];
  const int32_t* __restrict__ rows = a.neg_rows + b * (int64_t)L;
  const float* __restrict__ ns = a.neg_scores + b * (int64_t)L;
  for (int i0 = 0; i0 < E; i0 += 256) {  // 256 features per pass, four per lane
    const int i = i0 + lane * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c != 0.f)
      for (int j0 = wave * LL_UNROLL; j0 < L; j0 += LL_WAVES * LL_UNROLL) {
        float ds[LL_UNROLL];
        float4 x[LL_UNROLL];
#pragma unroll
        for (int q = 0; q < LL_UNROLL; ++q) {
          const int j = j0 + q;
          const float s = j < L ? ns[j] : NAN;
          const int r = j < L ? rows[j] : -1;
          const bool ok = s == s && r >= 0 && r < a.n_rows;
          ds[q] = ok ? c * expf(s - lse) : 0.f;
          x[q] = ok && i < E ? load4<VEC>(a.table + (int64_t)r * E, i, E) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int q = 0; q < LL_UNROLL; ++q) axpy4(acc, ds[q], x[q]);
      }
    if (lse > -INFINITY)
      for (int64_t e = t0 + wave; e < t1; e += LL_WAVES) {
        const float s = a.scores[e];
        const int t = a.tgt_rows[e];
        if (s == s && t >= 0 && t < a.n_rows && i < E)
          axpy4(acc, -g[e] * one_minus_p(s, lse), load4<VEC>(a.table + (int64_t)t * E, i, E));
      }
    store_wave_sum<VEC>(s_part, acc, d_up + b * E, i, E, lane, wave);
  }
}

// ------------------------------------------------------------------------------------------- the soft-target loss (xent)
// xnrs_list_xent_*: the same slots with a weight each and no queries; loss[b] = sum_filled w (lse - s), d s = g (W p - w).
struct XentArgs {
  const float* table;
  const float* up;
  const float* bias;
  int64_t n_rows;
  int E;
  int64_t B;
  const int32_t* rows;     // (B, L)
  const float* weights;    // (B, L)
  int L;
  int pad_row;
  float* lse;              // (B)
  float* slot_scores;      // (B, L)
};

// W_b = the sum of the weights of b's filled slots, in the tree of slot_sum (the same bits wherever it is computed)
__device__ __forceinline__ float weight_sum(const XentArgs& a, int64_t b, float* s_red, int tid) {
  const float* __restrict__ ns = a.slot_scores + b * (int64_t)a.L;
  const float* __restrict__ w = a.weights + b * (int64_t)a.L;
  return slot_sum(a.L, s_red, tid, [&](int j, float acc) { return ns[j] == ns[j] ? acc + w[j] : acc; });
}
// d s of a filled slot: g (W p - w), p = exp(s - lse)
__device__ __forceinline__ float xent_ds(float g, float W, float s, float lse, float w) { return g * fmaf(W, expf(s - lse), -w); }

template <bool VEC>
__global__ __launch_bounds__(LL_THREADS) void lx_fwd_kernel(XentArgs a, float* __restrict__ loss) {
  __shared__ __attribute__((aligned(16))) float s_up[LL_UP_LDS];
  __shared__ float s_red[LL_WAVES];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int E = a.E, L = a.L;
  const float* __restrict__ gu = a.up + b * E;
  stage_up(s_up, gu, E, tid);
  float* ns = a.slot_scores + b * (int64_t)L;  // (written here and read back behind the barrier)
  score_slots<VEC>(UserSlots{a.table, a.n_rows, E, L, a.pad_row, a.rows + b * (int64_t)L, gu, a.bias ? a.bias[0] : 0.f}, s_up,
                   ns, tid, [](int) { return false; });
  float m, log_sum;
  const float lse = slot_lse(ns, L, s_red, tid, m, log_sum);
  // term by term, never W lse - sum w s: that difference cancels at large scores.  lse - s is taken as (m - s) + log sum
  // exp(s - m): lse itself is rounded to the ulp of m, which at max|s| ~ 300 is more than the whole loss of a user whose
  // weight sits on its best slot.  For the same user sum exp(s - m) is 1 + a little, and logf of it is that little rounded
  // to the ulp of 1: the sum is split at the maximum -- c slots AT it, r summed over the others -- and its log taken as
  // log(c) + log1p(r / c), which keeps the relative precision of r
  const int n = lse > -INFINITY ? L : 0;
  const float c = slot_sum(n, s_red, tid, [&](int j, float acc) { return ns[j] == m ? acc + 1.f : acc; });
  const float r = slot_sum(n, s_red, tid, [&](int j, float acc) {
    const float s = ns[j];
    return s < m ? acc + expf(s - m) : acc;
  });
  const float log_rest = n ? logf(c) + log1pf(r / c) : 0.f;
  const float* __restrict__ w = a.weights + b * (int64_t)L;
  const float l = slot_sum(n, s_red, tid, [&](int j, float acc) {
    const float s = ns[j];
    return s == s ? fmaf(w[j], (m - s) + log_rest, acc) : acc;
  });
  if (tid == 0) {
    a.lse[b] = lse;
    loss[b] = l;
  }
}

template <bool VEC>
__global__ __launch_bounds__(LL_THREADS) void lx_dup_kernel(XentArgs a, const float* __restrict__ g, float* __restrict__ d_up) {
  __shared__ __attribute__((aligned(16))) float s_part[LL_WAVES][256];
  __shared__ float s_red[LL_WAVES];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int E = a.E, L = a.L;
  const float lse = a.lse[b], gb = g[b];
  const float W = weight_sum(a, b, s_red, tid);
  const int32_t* __restrict__ rows = a.rows + b * (int64_t)L;
  const float* __restrict__ ns = a.slot_scores + b * (int64_t)L;
  const float* __restrict__ wt = a.weights + b * (int64_t)L;
  for (int i0 = 0; i0 < E; i0 += 256) {  // 256 features per pass, four per lane
    const int i = i0 + lane * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j0 = wave * LL_UNROLL; j0 < L; j0 += LL_WAVES * LL_UNROLL) {
      float ds[LL_UNROLL];
      float4 x[LL_UNROLL];
#pragma unroll
      for (int q = 0; q < LL_UNROLL; ++q) {
        const int j = j0 + q;
        const float s = j < L ? ns[j] : NAN;
        const int r = j < L ? rows[j] : -1;
        const bool ok = s == s && r >= 0 && r < a.n_rows;
        ds[q] = ok ? xent_ds(gb, W, s, lse, wt[j]) : 0.f;
        x[q] = ok && i < E ? load4<VEC>(a.table + (int64_t)r * E, i, E) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int q = 0; q < LL_UNROLL; ++q) axpy4(acc, ds[q], x[q]);
    }
    store_wave_sum<VEC>(s_part, acc, d_up + b * E, i, E, lane, wave);
  }
}

// W_b of every user for the d_table walk: one workgroup per user, the tree of the d_up launch
__global__ __launch_bounds__(LL_THREADS) void lx_wsum_kernel(XentArgs a, float* __restrict__ wsum) {
  __shared__ float s_red[LL_WAVES];
  const float W = weight_sum(a, blockIdx.x, s_red, threadIdx.x);
  if (threadIdx.x == 0) wsum[blockIdx.x] = W;
}

// --------------------------------------------------------------------------------------------------------------- d_table
__global__ __launch_bounds__(LL_THREADS) void ll_coef_kernel(ListArgs a, const float* __restrict__ g, float* __restrict__ coef) {
  const int64_t b = (int64_t)blockIdx.x * LL_THREADS + threadIdx.x;
  if (b < a.B) coef[b] = user_coef(a, g, b);
}

template <bool VEC>
__global__ __launch_bounds__(LL_THREADS) void ll_zero_kernel(float* __restrict__ p, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * LL_THREADS;
  if constexpr (VEC) {
    float4* __restrict__ p4 = reinterpret_cast<float4*>(p);
    for (int64_t i = (int64_t)blockIdx.x * LL_THREADS + threadIdx.x; i < n / 4; i += stride) p4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    for (int64_t i = (int64_t)blockIdx.x * LL_THREADS + threadIdx.x; i < n; i += stride) p[i] = 0.f;
  }
}

// what the walk and the join share, whatever the loss: the sorted entries, the user vectors, the outputs
struct WalkOut {
  const float* up;
  int E;
  int64_t n_rows;
  const int32_t* order;
  float* d_table;
  float* head;        // (G, E): the sum of the first run of every span
  float* tail;        // (G, E): the sum of its last run, when that is another one
  int32_t* head_row;  // (G): the row of the first run; -1: none
  int32_t* tail_row;  // (G): the row of the last run; LL_NO_RUN: the span is one run (or empty)
  int G;
};

// An entry of `order` decoded: decode(v, row, user, ds) gives the row (>= 0) the entry adds ds * up[user] to and leaves
// row = -1 for an entry without a gradient; positions() = how many sorted positions can carry one.
// The ranking loss: slot (b, j) is entry b L + j, query e is entry B L + e.
struct RankDecode {
  ListArgs a;
  const float* g;
  const float* coef;  // (B)
  // every slot and the queries up to tgt_off[B]
  __device__ __forceinline__ int64_t positions() const { return a.B * (int64_t)a.L + a.tgt_off[a.B]; }
  __device__ __forceinline__ void decode(int64_t v, int& row, int& user, float& ds) const {
    const int64_t slots = a.B * (int64_t)a.L;
    const int64_t q0 = a.tgt_off[0], q1 = a.tgt_off[a.B];
    if (v >= 0 && v < slots) {
      const float s = a.neg_scores[v];
      const int r = a.neg_rows[v];
      if (s == s && r >= 0 && r < a.n_rows) {
        user = (int)(v / a.L);
        row = r;
        ds = coef[user] * expf(s - a.lse[user]);
      }
    } else if (v >= slots + q0 && v < slots + q1) {
      const int64_t e = v - slots;
      const float s = a.scores[e];
      const int r = a.tgt_rows[e];
      if (s == s && r >= 0 && r < a.n_rows) {
        int64_t l = 0, h = a.B;  // the user of query e: the last b with tgt_off[b] <= e
        while (h - l > 1) {
          const int64_t mid = (l + h) >> 1;
          if (a.tgt_off[mid] <= e) l = mid; else h = mid;
        }
        // (a user without negatives passes no gradient, but its query is sorted by its row like any other and lies
        // INSIDE the run of that row: it stays an entry of the run with ds = 0, or it would cut the run in two)
        const float lse = a.lse[l];
        user = (int)l;
        row = r;
        ds = lse > -INFINITY ? -g[e] * one_minus_p(s, lse) : 0.f;
      }
    }
  }
};
// The soft-target loss: the B L slots and nothing else.
struct XentDecode {
  XentArgs a;
  const float* g;
  const float* wsum;  // (B): W_b
  __device__ __forceinline__ int64_t positions() const { return a.B * (int64_t)a.L; }
  __device__ __forceinline__ void decode(int64_t v, int& row, int& user, float& ds) const {
    if (v < 0 || v >= a.B * (int64_t)a.L) return;
    const float s = a.slot_scores[v];
    const int r = a.rows[v];
    if (s == s && r >= 0 && r < a.n_rows) {
      user = (int)(v / a.L);
      row = r;
      ds = xent_ds(g[user], wsum[user], s, a.lse[user], a.weights[v]);
    }
  }
};

template <class Decode>
struct WalkArgs {
  Decode d;
  WalkOut o;
};

// positions per span: an even share, the same for every span (a span is walked in pieces of LL_PIECE positions from its
// first one; it need not be a whole number of them, so no span stays empty while another holds two pieces)
__device__ __forceinline__ int64_t walk_span(int64_t M, int G) { return (M + G - 1) / G; }

template <bool VEC, class Decode>
__global__ __launch_bounds__(LL_THREADS) void ll_walk_kernel(WalkArgs<Decode> wa) {
  const WalkOut& w = wa.o;
  const int lane = threadIdx.x & 63;
  const int span_id = blockIdx.x * LL_WAVES + (threadIdx.x >> 6);
  if (span_id >= w.G) return;
  const int E = w.E;
  const int64_t M = wa.d.positions(), span = walk_span(M, w.G);
  const int64_t lo = span_id * span, hi = lo + span < M ? lo + span : M;
  float* __restrict__ head = w.head + (int64_t)span_id * E;
  float* __restrict__ tail = w.tail + (int64_t)span_id * E;

  int first_row = -1, last_row = LL_NO_RUN;
  for (int i0 = 0; i0 < E; i0 += 256) {  // 256 features per pass, four per lane
    const int i = i0 + lane * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int cur = -1;          // the row of the running sum; -1: entries without a gradient
    bool started = false;  // cur is the row of a position of the span
    bool first = true;     // the running sum is the first run of the span
    first_row = -1;
    last_row = LL_NO_RUN;
    for (int64_t p0 = lo; p0 < hi; p0 += LL_PIECE) {
      // decode: lane k holds position p0 + k
      int row = -1, user = 0;
      float ds = 0.f;
      const int64_t p = p0 + lane;
      if (p < hi) wa.d.decode(w.order[p], row, user, ds);
      const int n = (int)(hi - p0 < LL_PIECE ? hi - p0 : LL_PIECE);
      for (int k0 = 0; k0 < n; k0 += LL_UNROLL) {
        int rk[LL_UNROLL];
        float dk[LL_UNROLL];
        float4 x[LL_UNROLL];
#pragma unroll
        for (int q = 0; q < LL_UNROLL; ++q) {  // (lanes past n decoded to row -1, ds 0, user 0)
          const int k = (k0 + q) & 63;
          rk[q] = __shfl(row, k);
          dk[q] = __shfl(ds, k);
          const int uk = __shfl(user, k);
          x[q] = rk[q] >= 0 && i < E ? load4<VEC>(w.up + (int64_t)uk * E, i, E) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int q = 0; q < LL_UNROLL; ++q) {
          if (k0 + q >= n) break;
          if (!started) {
            cur = rk[q];
            started = true;
          } else if (rk[q] != cur) {  // the run ends: store its sum
            if (first) {
              if (i < E) store4<VEC>(head, i, E, acc);
              first_row = cur;
              first = false;
            } else if (cur >= 0 && i < E) {
              store4<VEC>(w.d_table + (int64_t)cur * E, i, E, acc);
            }
            acc = make_float4(0.f, 0.f, 0.f, 0.f);
            cur = rk[q];
          }
          axpy4(acc, dk[q], x[q]);
        }
      }
    }
    if (first) {
      if (i < E) store4<VEC>(head, i, E, acc);
      first_row = cur;
    } else {
      if (i < E) store4<VEC>(tail, i, E, acc);
      last_row = cur;
    }
  }
  if (lane == 0) {
    w.head_row[span_id] = first_row;
    w.tail_row[span_id] = last_row;
  }
}

// One wave per span: the first and the last run of the span, when they BEGIN in it, are summed over the spans they continue
// in, in ascending span order, and stored.  (A first run that continues the span before belongs to the wave of the span it
// began in.)
template <bool VEC>
__global__ __launch_bounds__(LL_THREADS) void ll_join_kernel(WalkOut w) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * LL_WAVES + (threadIdx.x >> 6);
  if (s >= w.G) return;
  const int E = w.E;
  const int hr = w.head_row[s], tr = w.tail_row[s];
  // the last row of the span before: the head run continues it when the rows are equal
  int prev = -1;
  if (s > 0) prev = w.tail_row[s - 1] != LL_NO_RUN ? w.tail_row[s - 1] : w.head_row[s - 1];
  // candidates: the head run when it begins here, the tail run (it always begins here)
  for (int which = 0; which < 2; ++which) {
    const int row = which == 0 ? hr : tr;
    if (row < 0 || row >= w.n_rows) continue;
    if (which == 0 && s > 0 && prev == row) continue;      // begun in an earlier span: that span's wave sums it
    const bool reaches_end = which == 1 || tr == LL_NO_RUN;  // a head run with a tail behind it ends inside the span
    const float* __restrict__ src = (which == 0 ? w.head : w.tail) + (int64_t)s * E;
    for (int i = lane * 4; i < E; i += 256) {
      float4 acc = load4<VEC>(src, i, E);
      if (reaches_end)
        for (int q = s + 1; q < w.G && w.head_row[q] == row; ++q) {
          const float4 p = load4<VEC>(w.head + (int64_t)q * E, i, E);
          acc.x += p.x;
          acc.y += p.y;
          acc.z += p.z;
          acc.w += p.w;
          if (w.tail_row[q] != LL_NO_RUN) break;  // the run ended inside span q
        }
      store4<VEC>(w.d_table + (int64_t)row * E, i, E, acc);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ host
// spans of the walk over at most `entries` sorted positions (the ranking loss: B (L + 1), a query per user; xent: B L)
int ll_spans(int64_t entries) {
  const int64_t pieces = (entries + LL_PIECE - 1) / LL_PIECE;
  return (int)(pieces < 1 ? 1 : pieces > LL_SPANS ? LL_SPANS : pieces);
}
int ll_spans(int64_t B, int L) { return ll_spans(B * ((int64_t)L + 1)); }

struct WalkRegions {
  size_t coef, head, tail, head_row, tail_row, total;
};
// coef: one float per user (c_b of the ranking loss, W_b of xent), then the head and tail rows of G spans
WalkRegions ll_carve(int64_t B, int G, int E, bool want_d_table) {
  Carver c;
  WalkRegions r{};
  r.coef = c.take_if(want_d_table, (size_t)B * F32);
  r.head = c.take_if(want_d_table, (size_t)G * E * F32);
  r.tail = c.take_if(want_d_table, (size_t)G * E * F32);
  r.head_row = c.take_if(want_d_table, (size_t)G * sizeof(int32_t));
  r.tail_row = c.take_if(want_d_table, (size_t)G * sizeof(int32_t));
  r.total = c.total();
  return r;
}

bool ll_shape_ok(int64_t B, int L, int64_t n_rows, int E) {
  return B >= 0 && L >= 0 && n_rows >= 0 && n_rows <= INT32_MAX && E >= 1 && B <= INT32_MAX &&
         B * ((int64_t)L + 1) <= (int64_t)INT32_MAX;
}

bool lx_shape_ok(int64_t B, int L, int64_t n_rows, int E) {
  return B >= 0 && L >= 0 && n_rows >= 0 && n_rows <= INT32_MAX && E >= 1 && B <= INT32_MAX && B * (int64_t)L <= (int64_t)INT32_MAX;
}

// the three launches of d_table behind the per-user coefficients: the zero fill, the walk of the sorted entries with the
// loss's decode, the join of the runs that cross span bounds
template <class Decode>
hipError_t launch_d_table(const Decode& d, const float* up, int64_t n_rows, int E, const int32_t* order, float* d_table, void* ws,
                          const WalkRegions& r, int G, hipStream_t st) {
  const WalkArgs<Decode> w{d, WalkOut{up, E, n_rows, order, d_table, at<float>(ws, r.head), at<float>(ws, r.tail),
                                      at<int32_t>(ws, r.head_row), at<int32_t>(ws, r.tail_row), G}};
  const int64_t n = n_rows * (int64_t)E;
  const bool zvec = n % 4 == 0 && aligned16(d_table);
  const int64_t zitems = zvec ? n / 4 : n;
  const unsigned zgrid = (unsigned)std::min<int64_t>((zitems + LL_THREADS - 1) / LL_THREADS, 8192);
  if (zvec)
    ll_zero_kernel<true><<<dim3(zgrid ? zgrid : 1), LL_THREADS, 0, st>>>(d_table, n);
  else
    ll_zero_kernel<false><<<dim3(zgrid ? zgrid : 1), LL_THREADS, 0, st>>>(d_table, n);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  // (head / tail rows of the workspace are 256-byte aligned and E % 4 == 0 keeps every row of them on 16 bytes)
  const bool vec = E % 4 == 0 && aligned16(up) && aligned16(d_table) && aligned16(ws);
  const unsigned grid = (unsigned)((G + LL_WAVES - 1) / LL_WAVES);
  if (vec) {
    ll_walk_kernel<true><<<dim3(grid), LL_THREADS, 0, st>>>(w);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    ll_join_kernel<true><<<dim3(grid), LL_THREADS, 0, st>>>(w.o);
  } else {
    ll_walk_kernel<false><<<dim3(grid), LL_THREADS, 0, st>>>(w);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    ll_join_kernel<false><<<dim3(grid), LL_THREADS, 0, st>>>(w.o);
  }
  return hipGetLastError();
}

}  // namespace

}  // namespace xnrs

using namespace xnrs;

extern "C" {

size_t xnrs_list_loss_workspace_bytes(int64_t B, int32_t L, int64_t T, int32_t E, int32_t want_d_table) {
  (void)T;  // (the spans of the d_table walk are cut on the device; their number follows B and L alone)
  if (B < 0 || L < 0 || E < 1) return 0;
  return ll_carve(B, ll_spans(B, L), E, want_d_table != 0).total;
}

size_t xnrs_list_xent_workspace_bytes(int64_t B, int32_t L, int32_t E, int32_t want_d_table) {
  if (B < 0 || L < 0 || E < 1) return 0;
  return ll_carve(B, ll_spans(B * (int64_t)L), E, want_d_table != 0).total;
}

int32_t xnrs_list_xent_fwd(const float* table, int64_t n_rows, int32_t E, const float* up, const float* bias, int64_t B,
                           const int32_t* rows, const float* weights, int32_t L, int32_t pad_row, float* loss, float* lse,
                           float* slot_scores, void* ws, size_t ws_bytes, void* stream) {
  (void)ws;
  (void)ws_bytes;  // (the forward needs no workspace)
  if (!lx_shape_ok(B, L, n_rows, E)) return XNRS_EINVAL;
  if (B == 0) return XNRS_OK;
  if (!up || !loss || !lse || (n_rows > 0 && !table) || (L > 0 && (!rows || !weights || !slot_scores))) return XNRS_EINVAL;
  const XentArgs a{table, up, bias, n_rows, E, B, rows, weights, L, pad_row, lse, slot_scores};
  const bool vec = E % 4 == 0 && aligned16(table) && aligned16(up);
  if (vec)
    lx_fwd_kernel<true><<<dim3((unsigned)B), LL_THREADS, 0, (hipStream_t)stream>>>(a, loss);
  else
    lx_fwd_kernel<false><<<dim3((unsigned)B), LL_THREADS, 0, (hipStream_t)stream>>>(a, loss);
  return hip_rc(hipGetLastError());
}

int32_t xnrs_list_xent_bwd(const float* table, int64_t n_rows, int32_t E, const float* up, const float* bias, int64_t B,
                           const int32_t* rows, const float* weights, int32_t L, int32_t pad_row, const float* lse,
                           const float* slot_scores, const float* g, const int32_t* order, float* d_up, float* d_table, void* ws,
                           size_t ws_bytes, void* stream) {
  if (!lx_shape_ok(B, L, n_rows, E)) return XNRS_EINVAL;
  if ((order == nullptr) != (d_table == nullptr)) return XNRS_EINVAL;
  if (B == 0) return XNRS_OK;
  if (!up || !lse || !g || (n_rows > 0 && !table) || (L > 0 && (!rows || !weights || !slot_scores))) return XNRS_EINVAL;
  const int G = ll_spans(B * (int64_t)L);
  const WalkRegions r = ll_carve(B, G, E, d_table != nullptr);
  if (r.total > 0 && (!ws || ws_bytes < r.total)) return XNRS_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const XentArgs a{table, up, bias, n_rows, E, B, rows, weights, L, pad_row, const_cast<float*>(lse), const_cast<float*>(slot_scores)};
  if (d_up) {
    const bool vec = E % 4 == 0 && aligned16(table) && aligned16(d_up);
    if (vec)
      lx_dup_kernel<true><<<dim3((unsigned)B), LL_THREADS, 0, st>>>(a, g, d_up);
    else
      lx_dup_kernel<false><<<dim3((unsigned)B), LL_THREADS, 0, st>>>(a, g, d_up);
    XNRS_TRY(hipGetLastError());
  }
  if (d_table && n_rows > 0) {
    lx_wsum_kernel<<<dim3((unsigned)B), LL_THREADS, 0, st>>>(a, at<float>(ws, r.coef));
    XNRS_TRY(hipGetLastError());
    XNRS_TRY(launch_d_table(XentDecode{a, g, at<float>(ws, r.coef)}, up, n_rows, E, order, d_table, ws, r, G, st));
  }
  return XNRS_OK;
}

int32_t xnrs_list_loss_fwd(const float* table, int64_t n_rows, int32_t E, const float* up, const float* bias, int64_t B,
                           const int64_t* tgt_off, const int32_t* tgt_rows, const int32_t* neg_rows, int32_t L, int32_t pad_row,
                           float* scores, float* loss, float* lse, float* neg_scores, void* ws, size_t ws_bytes, void* stream) {
  (void)ws;
  (void)ws_bytes;  // (the forward needs no workspace)
  if (!ll_shape_ok(B, L, n_rows, E)) return XNRS_EINVAL;
  if (B == 0) return XNRS_OK;
  if (!up || !tgt_off || !tgt_rows || !scores || !loss || !lse || (n_rows > 0 && !table) || (L > 0 && (!neg_rows || !neg_scores)))
    return XNRS_EINVAL;
  const ListArgs a{table, up, bias, n_rows, E, B, tgt_off, tgt_rows, neg_rows, L, pad_row, scores, lse, neg_scores};
  const bool vec = E % 4 == 0 && aligned16(table) && aligned16(up);
  if (vec)
    ll_fwd_kernel<true><<<dim3((unsigned)B), LL_THREADS, 0, (hipStream_t)stream>>>(a, loss);
  else
    ll_fwd_kernel<false><<<dim3((unsigned)B), LL_THREADS, 0, (hipStream_t)stream>>>(a, loss);
  return hip_rc(hipGetLastError());
}

int32_t xnrs_list_loss_bwd(const float* table, int64_t n_rows, int32_t E, const float* up, const float* bias, int64_t B,
                           const int64_t* tgt_off, const int32_t* tgt_rows, const int32_t* neg_rows, int32_t L, int32_t pad_row,
                           const float* scores, const float* lse, const float* neg_scores, const float* g, const int32_t* order,
                           float* d_up, float* d_table, void* ws, size_t ws_bytes, void* stream) {
  if (!ll_shape_ok(B, L, n_rows, E)) return XNRS_EINVAL;
  if ((order == nullptr) != (d_table == nullptr)) return XNRS_EINVAL;
  if (B == 0) return XNRS_OK;
  if (!up || !tgt_off || !tgt_rows || !scores || !lse || !g || (n_rows > 0 && !table) || (L > 0 && (!neg_rows || !neg_scores)))
    return XNRS_EINVAL;
  const int G = ll_spans(B, L);
  const WalkRegions r = ll_carve(B, G, E, d_table != nullptr);
  if (r.total > 0 && (!ws || ws_bytes < r.total)) return XNRS_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const ListArgs a{table, up, bias, n_rows, E, B, tgt_off, tgt_rows, neg_rows, L, pad_row, const_cast<float*>(scores),
                   const_cast<float*>(lse), const_cast<float*>(neg_scores)};
  if (d_up) {
    const bool vec = E % 4 == 0 && aligned16(table) && aligned16(d_up);
    if (vec)
      ll_dup_kernel<true><<<dim3((unsigned)B), LL_THREADS, 0, st>>>(a, g, d_up);
    else
      ll_dup_kernel<false><<<dim3((unsigned)B), LL_THREADS, 0, st>>>(a, g, d_up);
    XNRS_TRY(hipGetLastError());
  }
  if (d_table && n_rows > 0) {
    ll_coef_kernel<<<dim3((unsigned)((B + LL_THREADS - 1) / LL_THREADS)), LL_THREADS, 0, st>>>(a, g, at<float>(ws, r.coef));
    XNRS_TRY(hipGetLastError());
    XNRS_TRY(launch_d_table(RankDecode{a, g, at<float>(ws, r.coef)}, up, n_rows, E, order, d_table, ws, r, G, st));
  }
  return XNRS_OK;
}

}  // extern "C"
