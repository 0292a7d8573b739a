// The greedy re-ranking of a deep candidate list, written once (diversity.hip: mmr_kernel; calibration.hip: cal_kernel).  One
// workgroup of 4 waves per session picks k of the P places of its pool, one per step: the alive place with the largest
//   lam * r_i - (1 - lam) * penalty_i
// where r is the pool's score (raw, or min-max rescaled over the valid places) and the penalty is the policy's.  A place is
// valid when its row lies in the table and its score is finite; a session that runs out of valid places ends in fillers
// (-1, -inf, -1).  Equal objectives go to the lower place; a pick carries the pool's own score bits.
//
// A policy is a struct of the kernel with
//   void  stage(int i, int r, bool ok)      its state of place i (called by the thread that owns the place, before any barrier)
//   void  prepare(int t)                    whatever penalty() reads in step t; leaves it readable (its own barriers)
//   float penalty(int i)                    the penalty of the alive place i
//   void  take(int bi, int t, bool last)    the pick of step t is place bi; ends in a barrier unless it is the last pick and
//                                           nothing reads the policy's state afterwards
// The barrier that closes take is part of the loop's correctness, not only of the policy's: it stands between this step's
// reads of the argmax words [0, 4) and [8, 12) -- and of the alive byte thread 0 has just cleared -- and the next step's
// scan and lane-0 writes of those words (and whatever the policy's prepare writes over [0, 8)).  A policy without it races.
// prepare and take are called by every thread of the workgroup with the same arguments.  The loop itself has one barrier per
// step (the argmax through LDS); the alive byte of the pick is cleared behind it, so a policy's take may scan the alive
// places once it has passed a barrier of its own.
//
// LDS: GREEDY_SCRATCH words in front of the dynamic region ([0, 4) the waves' argmax values or maxima, [4, 8) their minima,
// [8, 12) their argmax places; a policy may use [0, 8) between the loop's barriers: calibration.hip's block_sum2 does), then
// lam * r per place and one alive byte per place, carved by the kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "host.h"

namespace xnrs {

constexpr int GREEDY_THREADS = 256;  // 4 waves per workgroup
constexpr int GREEDY_WAVES = GREEDY_THREADS / 64;
constexpr int GREEDY_SCRATCH = 16;   // words in front of the dynamic LDS

__host__ __device__ __forceinline__ int pad4(int n) { return (n + 3) & ~3; }

// what the two re-rankers share of their arguments
struct GreedyArgs {
  const int32_t* pool_rows;
  const float* pool_scores;
  int P, k;
  int64_t n_rows;
  float lam;
  int rel_mode;
  int32_t* out_rows;
  float* out_scores;
  int32_t* out_pos;
};

// lam r - (1 - lam) pen, two products and one difference, each rounded (no contraction: at lam = 1 it is r exactly)
__device__ __forceinline__ float greedy_objective(float lam_r, float oml, float pen) {
#pragma clang fp contract(off)
  const float cost = oml * pen;
  return lam_r - cost;
}
// does the candidate (v, i) come before (bv, bi)?  higher objective, then the lower place; (-inf, INT_MAX) is "none"
__device__ __forceinline__ bool greedy_before(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// the places of session b: s_alive[i] = valid, s_lr[i] = lam * r_i, the policy's state.  No barrier behind it: the kernel
// puts one before greedy_loop.
template <class Policy>
__device__ __forceinline__ void greedy_stage(const GreedyArgs& a, int64_t b, float* s_scratch, float* s_lr, unsigned char* s_alive,
                                             Policy& pol) {
  const int P = a.P, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t* __restrict__ rows = a.pool_rows + b * (int64_t)P;
  const float* __restrict__ scores = a.pool_scores + b * (int64_t)P;
  float* s_hi = s_scratch;
  float* s_lo = s_scratch + GREEDY_WAVES;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = tid; i < P; i += GREEDY_THREADS) {
    const int r = rows[i];
    const float s = scores[i];
    const bool ok = r >= 0 && r < a.n_rows && fabsf(s) < INFINITY;  // (NaN compares false)
    pol.stage(i, r, ok);
    s_alive[i] = ok ? 1 : 0;
    s_lr[i] = ok ? s : 0.f;  // (the score for now)
    if (ok) {
      lo = fminf(lo, s);
      hi = fmaxf(hi, s);
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, m));
    hi = fmaxf(hi, __shfl_xor(hi, m));
  }
  if (lane == 0) {
    s_lo[wave] = lo;
    s_hi[wave] = hi;
  }
  __syncthreads();
  lo = fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3]));
  hi = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3]));
  const float span = hi - lo;
  for (int i = tid; i < P; i += GREEDY_THREADS) {  // (a thread rewrites the places it wrote)
    float r = s_lr[i];
    if (a.rel_mode == XNRS_MMR_REL_MINMAX) r = span > 0.f ? (r - lo) / span : 0.f;
    s_lr[i] = a.lam * r;
  }
}

// the k steps of session b and the fillers behind its picks
template <class Policy>
__device__ __forceinline__ void greedy_loop(const GreedyArgs& a, int64_t b, float* s_scratch, const float* s_lr,
                                            unsigned char* s_alive, Policy& pol) {
  const int P = a.P, k = a.k, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t* __restrict__ rows = a.pool_rows + b * (int64_t)P;
  const float* __restrict__ scores = a.pool_scores + b * (int64_t)P;
  float* s_wv = s_scratch;
  int* s_wi = reinterpret_cast<int*>(s_scratch + 2 * GREEDY_WAVES);
  const float oml = 1.f - a.lam;
  int t = 0;
  for (; t < k; ++t) {
    pol.prepare(t);
    // argmax of the objective over the alive places: ascending places per thread, so `>` keeps the lower of two equals
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int i = tid; i < P; i += GREEDY_THREADS)
      if (s_alive[i]) {
        const float v = greedy_objective(s_lr[i], oml, pol.penalty(i));
        if (greedy_before(v, i, bv, bi)) {
          bv = v;
          bi = i;
        }
      }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const float ov = __shfl_xor(bv, m);
      const int oi = __shfl_xor(bi, m);
      if (greedy_before(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) {
      s_wv[wave] = bv;
      s_wi[wave] = bi;
    }
    __syncthreads();
    bv = s_wv[0];
    bi = s_wi[0];
#pragma unroll
    for (int w = 1; w < GREEDY_WAVES; ++w)
      if (greedy_before(s_wv[w], s_wi[w], bv, bi)) {
        bv = s_wv[w];
        bi = s_wi[w];
      }
    if (bi == INT_MAX) break;  // no valid place is left (the same for every thread)
    if (tid == 0) {            // (every scan of this step lies behind the barrier above)
      a.out_rows[b * k + t] = rows[bi];
      a.out_scores[b * k + t] = scores[bi];  // the pool's own bits
      a.out_pos[b * k + t] = bi;
      s_alive[bi] = 0;
    }
    pol.take(bi, t, t + 1 == k);
  }
  for (int u = t + tid; u < k; u += GREEDY_THREADS) {  // fillers behind the picks
    a.out_rows[b * k + u] = -1;
    a.out_scores[b * k + u] = -INFINITY;
    a.out_pos[b * k + u] = -1;
  }
}

}  // namespace xnrs
