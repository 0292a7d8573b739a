// Top-k news per user over a whole pre-encoded table: the scores of a (users x table rows) product are ranked while they are
// formed, so the (B, n_rows) score matrix never exists.  Two launches per call (plus the user-side projection GEMM of the
// bilinear / MLP scorer); results cross from one launch to the next at the kernel boundary only: no flags, no float atomics.
//
//   partial : grid = user tiles x table slices.  A workgroup takes TK_TILE users and one contiguous slice of table rows, walks
//             the slice in chunks of TK_TILE rows, forms the chunk's score tile and keeps each user's k best of the slice so
//             far as a sorted list of 64-bit keys in the workspace (the list of slice s of user b: part[(s * B + b) * k ..]).
//             Only a score that beats the user's current k-th best (kept in LDS) is appended to the user's LDS candidate buffer
//             (an integer LDS atomic hands out the slot); a full buffer, and the end of the slice, drop the candidates on the
//             user's exclusion list (half a wave per user, one candidate per lane, the list read once for all of them), merge
//             the rest into the list and raise the threshold.  Arrival order in the buffer
//             varies from run to run; the merged list does not (the keys are totally ordered and a dropped candidate was
//             already below k others).
//   merge   : one wave per user merges the `slices` sorted lists into the final k and decodes rows and scores.
// xnrs_topk_deep* (k up to 1024) runs the same two kernels instantiated for longer lists (KCAP), for the inner-product forms
// behind a first sweep that finds each user a threshold to start from (tk_launch, topk_floor_kernel).
//
// Order: key = (order-preserving score bits << 32) | ~row, so "higher score first, equal scores (-0 == +0) lower row first" is
// one unsigned compare.  A NaN score is never selected; -inf is a legal score.  Missing entries (fewer than k eligible rows)
// are fillers -- row -1, score -inf -- whose key lies below every real key.  The ranking is by the RAW score: no ReLU (the
// evaluation's relu would tie every negative score).
//
// The score tile and the row windows of xnrs_topk_deep*_win: sweep.h.
#include <cmath>

#include "sweep.h"

namespace xnrs {

namespace {

constexpr uint64_t TK_FILLER = 0x007FFFFFull << 32;  // score -inf, row -1: below the key of row 2^31 - 2 at score -inf

__device__ __forceinline__ uint64_t tk_key(float s, uint32_t row) {
  const uint32_t b = __float_as_uint(s == 0.f ? 0.f : s);  // -0 ties with +0
  return ((uint64_t)((b & 0x80000000u) ? ~b : (b | 0x80000000u)) << 32) | (uint32_t)~row;
}
__device__ __forceinline__ float tk_score(uint64_t key) {
  const uint32_t o = (uint32_t)(key >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

// what one wave wrote to LDS / the workspace is read by its other lanes
__device__ __forceinline__ void tk_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}
// the same for LDS alone: a wave's LDS accesses are performed in program order, so the compiler must keep that order and no
// wait is needed -- loads from global memory stay in flight across it
__device__ __forceinline__ void tk_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// how many of the descending keys a[0, n), n <= MAXN (a power of two), are greater than key: a binary search of a fixed
// number of branch-free steps, so that several searches side by side overlap their LDS latencies
template <int MAXN>
__device__ __forceinline__ int tk_count_greater(const uint64_t* a, int n, uint64_t key) {
  int c = 0;
#pragma unroll
  for (int step = MAXN; step > 0; step >>= 1) {
    const int t = c + step;
    const uint64_t at = a[t <= n ? t - 1 : 0];
    if (t <= n && at > key) c = t;
  }
  return c;
}

struct TopkArgs : TkOperands {
  int k;
  uint64_t* part;
  const uint64_t* floor;  // xnrs_topk_deep*, k > XNRS_TOPK_MAX_K: per user a key below which nothing is wanted (topk_floor_kernel), or NULL
};
// xnrs_topk_sample*: the keys are score * inv_tau + g, g the standard Gumbel draw of the pair (seed, user key) at the table row
// (kernels.h: drop_pair, drop_word, drop_gumbel); user_keys NULL: the user's index in the call
struct TopkSampleArgs : TopkArgs {
  float inv_tau;
  uint64_t seed;
  const int64_t* user_keys;
};
template <bool SAMPLE>
struct TkArgsOf {
  using type = TopkArgs;
};
template <>
struct TkArgsOf<true> {
  using type = TopkSampleArgs;
};

// One wave merges the candidate buffers of up to two users at once, one user per half-wave (32 lanes = TK_CB candidates, one
// per lane): list[0, k) (sorted, in the workspace) <- the k greatest of list and the candidates buf[0, n) (unsorted, distinct
// real keys) that are not on the user's exclusion list.  The exclusion list goes through LDS 64 ids at a time and every
// candidate is compared with each (ids are compared, never dereferenced); an excluded candidate becomes key 0, below every
// filler.  Every key's place is its count of greater keys: a list entry's index (fillers are told apart by it) plus the
// surviving candidates above it, a candidate's rank among the candidates plus the list entries above it.
template <int KCAP>
struct TkListLen {};  // (empty: the lists of xnrs_topk* are filled with fillers and always k long)
template <>
struct TkListLen<XNRS_TOPK_DEEP_MAX_K> {
  int32_t nreal[32];  // of the first half of a wave: how many keys the list of the wave's user wave + 4 j holds so far
};
template <int KCAP>
struct TkHalfT : TkListLen<KCAP> {  // the LDS of one half-wave; KCAP: the longest list it stages
  uint64_t stage[KCAP], sorted[TK_CB];
  int32_t excl[64];
};
using TkHalf = TkHalfT<XNRS_TOPK_MAX_K>;
// what a merge reads from global memory, fetched while the merge before it computes
struct TkFetch {
  uint64_t key[XNRS_TOPK_MAX_K / 32];  // list[hl + 32 t]
  int32_t id0, id1;                    // excl_rows[lo + hl], [lo + hl + 32]; -1 past the end
  int64_t lo, hi;
  int uc;      // the half's user in the tile (an idle half addresses user 0 and writes nothing)
  int active;  // (an int: no padding bytes to carry around)
};
__device__ __forceinline__ int32_t tk_excl_id(const TopkArgs& a, int64_t e, int64_t hi) { return e < hi ? a.excl_rows[e] : -1; }
__device__ __forceinline__ TkFetch tk_fetch(const TopkArgs& a, int64_t u0, const uint64_t* lists, int k, int ul, int hl) {
  TkFetch f;
  const bool active = ul >= 0;  // (tk_pop_pair: a negative user is none)
  f.active = active;
  f.uc = active ? ul : 0;
  const uint64_t* list = lists + (int64_t)f.uc * k;
#pragma unroll
  for (int t = 0; t < XNRS_TOPK_MAX_K / 32; ++t) f.key[t] = active && hl + 32 * t < k ? list[hl + 32 * t] : 0;
  f.lo = f.hi = 0;
  if (a.excl_off && active) {
    f.lo = a.excl_off[u0 + f.uc];
    f.hi = a.excl_off[u0 + f.uc + 1];
  }
  f.id0 = tk_excl_id(a, f.lo + hl, f.hi);
  f.id1 = tk_excl_id(a, f.lo + hl + 32, f.hi);
  return f;
}
__device__ __forceinline__ void tk_merge_pair(const TopkArgs& a, const TkFetch& f, uint64_t* lists, int k, TkHalf& w, uint64_t* bufs,
                                              uint64_t* thr, int* cnt, int hl, int h) {
  uint64_t* list = lists + (int64_t)f.uc * k;
  uint64_t* buf = bufs + f.uc * TK_CB;
  const int n = !f.active ? 0 : cnt[f.uc] < TK_CB ? cnt[f.uc] : TK_CB;
#pragma unroll
  for (int t = 0; t < XNRS_TOPK_MAX_K / 32; ++t)
    if (hl + 32 * t < k) w.stage[hl + 32 * t] = f.key[t];
  uint64_t cand = hl < n ? buf[hl] : 0;
  if (a.excl_off) {
    const int32_t row = (int32_t)~(uint32_t)cand;  // (-1 without a candidate)
    int32_t id0 = f.id0, id1 = f.id1;
    bool hit = false;
    for (int64_t base = f.lo; __any(base < f.hi); base += 64) {
      if (base != f.lo) {
        id0 = tk_excl_id(a, base + hl, f.hi);
        id1 = tk_excl_id(a, base + hl + 32, f.hi);
      }
      tk_lds_sync();
      w.excl[hl] = id0;
      w.excl[hl + 32] = id1;
      tk_lds_sync();
#pragma unroll
      for (int e = 0; e < 64; ++e) hit |= w.excl[e] == row;
    }
    if (hit && row >= 0) cand = 0;
  }
  if (f.active) buf[hl] = cand;
  tk_lds_sync();
  int rank = 0;
  if (cand) {
#pragma unroll 8
    for (int j = 0; j < TK_CB; ++j) rank += buf[j] > cand;
    w.sorted[rank] = cand;
  }
  const int alive = __popc((uint32_t)(__ballot(cand != 0) >> (32 * h)));
  tk_lds_sync();
  uint64_t key[XNRS_TOPK_MAX_K / 32];
  int place[XNRS_TOPK_MAX_K / 32];
#pragma unroll
  for (int t = 0; t < XNRS_TOPK_MAX_K / 32; ++t) {  // (four searches side by side)
    const int i = hl + 32 * t;
    key[t] = f.active && i < k ? w.stage[i] : 0;
    place[t] = i + tk_count_greater<TK_CB>(w.sorted, alive, key[t]);
  }
  const int cand_place = rank + tk_count_greater<XNRS_TOPK_MAX_K>(w.stage, k, cand);
#pragma unroll
  for (int t = 0; t < XNRS_TOPK_MAX_K / 32; ++t)
    if (key[t] && place[t] < k) {
      if (place[t] != hl + 32 * t) list[place[t]] = key[t];
      if (place[t] == k - 1) thr[f.uc] = key[t];
    }
  if (cand && cand_place < k) {
    list[cand_place] = cand;
    if (cand_place == k - 1) thr[f.uc] = cand;
  }
  if (f.active && hl == 0) cnt[f.uc] = 0;
  // (stage / sorted / excl may be written again; the list's stores complete by the workgroup barrier that ends the phase,
  // before any later merge of the same user fetches it)
  tk_lds_sync();
}

// The same merge for a list of up to KCAP > XNRS_TOPK_MAX_K keys (xnrs_topk_deep*).  Such a list does not fit the registers
// of a fetch ahead, so it goes from the workspace straight into LDS and its entries are placed 256 at a time (eight searches
// side by side).  Every entry is read from LDS, which holds the whole list before the first store to the workspace.
// A list in the workspace is not filled with fillers first: nreal[] says how many keys it holds, only those are read, moved
// and written, and the kernel ends every list that is not full with one filler (the merge kernel reads up to it).  So a
// merge costs what the list holds, not k -- after the floor of the first sweep that is a few dozen keys.
template <int KCAP>
__device__ __forceinline__ void tk_merge_pair_deep(const TopkArgs& a, int64_t u0, uint64_t* lists, int k, int ul, TkHalfT<KCAP>& w,
                                                   int32_t* nreal, uint64_t* bufs, uint64_t* thr, int* cnt, int hl, int h) {
  const bool active = ul >= 0;  // (tk_pop_pair: a negative user is none; an idle half addresses user 0 and writes nothing)
  const int uc = active ? ul : 0;
  uint64_t* list = lists + (int64_t)uc * k;
  uint64_t* buf = bufs + uc * TK_CB;
  const int n = !active ? 0 : cnt[uc] < TK_CB ? cnt[uc] : TK_CB;
  const int nl = active ? nreal[uc >> 2] : 0;                  // the keys of the list
  const int nl2 = max(__shfl(nl, 0), __shfl(nl, 32));          // ... of the longer list of the two halves: uniform loop bounds
  int64_t lo = 0, hi = 0;
  if (a.excl_off && active) {
    lo = a.excl_off[u0 + uc];
    hi = a.excl_off[u0 + uc + 1];
  }
  int32_t id0 = tk_excl_id(a, lo + hl, hi), id1 = tk_excl_id(a, lo + hl + 32, hi);  // (on their way with the list)
  for (int i0 = hl; i0 < nl2; i0 += 256) {  // eight loads in flight per lane
    uint64_t t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = i0 + 32 * j < nl ? list[i0 + 32 * j] : 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (i0 + 32 * j < nl) w.stage[i0 + 32 * j] = t[j];
  }
  uint64_t cand = hl < n ? buf[hl] : 0;
  if (a.excl_off) {
    const int32_t row = (int32_t)~(uint32_t)cand;  // (-1 without a candidate)
    bool hit = false;
    for (int64_t base = lo; __any(base < hi); base += 64) {
      if (base != lo) {
        id0 = tk_excl_id(a, base + hl, hi);
        id1 = tk_excl_id(a, base + hl + 32, hi);
      }
      tk_lds_sync();
      w.excl[hl] = id0;
      w.excl[hl + 32] = id1;
      tk_lds_sync();
#pragma unroll
      for (int e = 0; e < 64; ++e) hit |= w.excl[e] == row;
    }
    if (hit && row >= 0) cand = 0;
  }
  if (active) buf[hl] = cand;
  tk_lds_sync();
  int rank = 0;
  if (cand) {
#pragma unroll 8
    for (int j = 0; j < TK_CB; ++j) rank += buf[j] > cand;
    w.sorted[rank] = cand;
  }
  const int alive = __popc((uint32_t)(__ballot(cand != 0) >> (32 * h)));
  tk_lds_sync();
  const int cand_place = rank + tk_count_greater<KCAP>(w.stage, nl, cand);
  for (int i0 = 0; i0 < nl2; i0 += 256) {
    uint64_t key[8];
    int place[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int i = i0 + hl + 32 * t;
      key[t] = i < nl ? w.stage[i] : 0;
      place[t] = i + tk_count_greater<TK_CB>(w.sorted, alive, key[t]);
    }
#pragma unroll
    for (int t = 0; t < 8; ++t)
      if (key[t] && place[t] < k) {
        if (place[t] != i0 + hl + 32 * t) list[place[t]] = key[t];
        if (place[t] == k - 1) thr[uc] = key[t];
      }
  }
  if (cand && cand_place < k) {
    list[cand_place] = cand;
    if (cand_place == k - 1) thr[uc] = cand;
  }
  if (active && hl == 0) {
    cnt[uc] = 0;
    nreal[uc >> 2] = nl + alive < k ? nl + alive : k;
  }
  tk_lds_sync();  // (as tk_merge_pair: the LDS of the half may be written again)
}

// the two lowest set bits of `todo`, taken out of it: the lower for half 0, the other (or -1: none) for half 1
__device__ __forceinline__ int tk_pop_pair(uint32_t& todo, int h) {
  const int j0 = __ffs(todo) - 1;
  todo &= todo - 1;
  const int j1 = todo ? __ffs(todo) - 1 : -1;
  todo &= todo - 1;  // (0 stays 0)
  return h ? j1 : j0;
}

// the merges of one wave: its users (wave, wave + 4, ...) whose buffer is full -- at the end of the slice: not empty -- two at a
// time, the next two users' lists on their way while these two merge (KCAP > XNRS_TOPK_MAX_K: without the fetch ahead)
template <int KCAP>
__device__ __forceinline__ void tk_merge_phase(const TopkArgs& a, int64_t u0, uint64_t* lists, int k, int nu, bool final, TkHalfT<KCAP>* w,
                                               uint64_t* bufs, uint64_t* thr, int* cnt, int wave, int lane) {
  const int hl = lane & 31, h = lane >> 5;
  const int mine = wave + 4 * hl;
  const int c = h == 0 && mine < nu ? cnt[mine] : 0;
  uint32_t todo = (uint32_t)__ballot(final ? c > 0 : c >= TK_CB);
  if (!todo) return;
  if constexpr (KCAP > XNRS_TOPK_MAX_K) {
    while (todo) tk_merge_pair_deep<KCAP>(a, u0, lists, k, wave + 4 * tk_pop_pair(todo, h), w[h], w[0].nreal, bufs, thr, cnt, hl, h);
  } else {
    TkFetch cur = tk_fetch(a, u0, lists, k, wave + 4 * tk_pop_pair(todo, h), hl);
    for (;;) {
      const bool more = todo != 0;
      TkFetch nxt = cur;
      if (more) nxt = tk_fetch(a, u0, lists, k, wave + 4 * tk_pop_pair(todo, h), hl);
      tk_merge_pair(a, cur, lists, k, w[h], bufs, thr, cnt, hl, h);
      if (!more) break;
      cur = nxt;
    }
  }
}

// (two workgroups per CU for the MFMA form; the MLP form's 64 tanhf per feature want more than 256 registers.  KCAP: the
// longest list of the call -- XNRS_TOPK_MAX_K for xnrs_topk*; the 1024 of xnrs_topk_deep* stages 8 KB per half-wave, 135 KB of
// LDS in all, and is alone on its CU.
// SAMPLE (xnrs_topk_sample*): the score becomes the perturbed key s * inv_tau + g before it meets the threshold, and nothing
// behind that line knows: the lists, the merges, the floor and the merge kernel order perturbed keys as they order scores.
// A lane holds the splitmix64 word of each of its two users in registers; a draw is one fmix32 and two logarithms.  The fp32
// add is monotone, so a score p = s * inv_tau whose fl(p + b) lies below the user's threshold for an upper bound b of its
// draw cannot become a candidate and needs no draw.  DROP_GUMBEL_MAX is the bound that costs nothing, and it only bites at a
// cold temperature: a draw near 22.9 is one in 2^33, and in the unrolled loop over the lane's 64 scores a wave takes the
// logarithms of an element whenever ONE of its 64 lanes needs them.  Measured (profiles/topk_sample_resource_usage.md), the
// k <= 128 form is fastest with the draw where the score is formed, a flat cost per score; the long-list form, whose
// thresholds start at the floor of the first sweep, tests the bound of the pair's own word instead (drop_gumbel_bound: the
// fmix32 and the exponent of the uniform), puts what passes into `pend` as a score at the threshold, and takes the logarithms
// in the candidate loop, where each lane walks its own few set bits (DRAW_LATE).  The keys are the same bits either way.  The
// product and the sum are rounded separately (__fmul_rn, __fadd_rn: no contraction), so tests and key share the product's bits.)
template <bool MLP, int KCAP = XNRS_TOPK_MAX_K, bool SAMPLE = false>
__global__ __launch_bounds__(256, MLP || KCAP > XNRS_TOPK_MAX_K ? 1 : 2) void topk_partial_kernel(typename TkArgsOf<SAMPLE>::type a) {
  __shared__ float At[TK_KT * TK_PITCH], Bt[TK_KT * TK_PITCH];  // table rows / users of one stage, feature-major
  __shared__ float w2s[TK_KT];
  __shared__ uint64_t buf[TK_TILE * TK_CB], thr[TK_TILE];
  __shared__ TkHalfT<KCAP> halves[4][2];
  __shared__ int cnt[TK_TILE];
  __shared__ int rng[4];
  constexpr bool DRAW_LATE = SAMPLE && KCAP > XNRS_TOPK_MAX_K;  // the logarithms of a draw: in the candidate loop
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, half = lane >> 5;
  const int rw = (wave >> 1) * 64, uw = (wave & 1) * 64;  // (TkThread's coordinates, spelled out: profiles/sweep_split_resource_usage.md)
  const int64_t u0 = (int64_t)blockIdx.x * TK_TILE;
  const int nu = a.B - u0 < TK_TILE ? (int)(a.B - u0) : TK_TILE;
  const int k = a.k;
  TkWin win;
  int64_t c_lo, c_hi;
  tk_tile_range(a, u0, nu, rng, win, c_lo, c_hi);
  uint64_t* lists = a.part + ((int64_t)blockIdx.y * a.B + u0) * k;
  if constexpr (KCAP > XNRS_TOPK_MAX_K) {
    if (tid < TK_TILE) halves[tid & 3][0].nreal[tid >> 2] = 0;  // (the lists start empty, and are not filled)
  } else {
    for (int i = tid; i < nu * k; i += 256) lists[i] = TK_FILLER;
  }
  for (int i = tid; i < TK_TILE; i += 256) {
    uint64_t t0 = TK_FILLER;
    if constexpr (KCAP > XNRS_TOPK_MAX_K)
      if (a.floor && i < nu) t0 = a.floor[u0 + i];  // the threshold starts where the first sweep proved k rows to be
    thr[i] = t0;
    cnt[i] = 0;
  }
  __syncthreads();
  const float bias = a.bias ? a.bias[0] : 0.f;
  uint32_t z_lo[2] = {0u, 0u}, z_hi[2] = {0u, 0u};  // SAMPLE: the 64-bit part of the draws of the lane's two users
  if constexpr (SAMPLE) {
#pragma unroll
    for (int ub = 0; ub < 2; ++ub) {
      const int ul = uw + ub * 32 + l32;
      const int64_t key = ul >= nu ? 0 : a.user_keys ? a.user_keys[u0 + ul] : u0 + ul;
      const uint64_t z = drop_pair(a.seed, key);
      z_lo[ub] = (uint32_t)z;
      z_hi[ub] = (uint32_t)(z >> 32);
    }
  }
  for (int64_t c = c_lo; c < c_hi; ++c) {
    const int64_t r0 = c * TK_TILE;
    if (win.gaps && !tk_chunk_live(win, r0)) continue;
    f32x16 acc[2][2];
    tk_score_tile<MLP, false>(a, r0, nullptr, u0, At, Bt, w2s, acc);
    // ---- selection: append what beats the threshold, merge full buffers, go round again while a buffer overflowed
    uint64_t pend = 0;  // bit ub * 32 + rb * 16 + j: a score at or above the threshold as the chunk begins
#pragma unroll
    for (int ub = 0; ub < 2; ++ub) {
      const int ul = uw + ub * 32 + l32;
      const float tS = ul < nu ? tk_score(thr[ul]) : __builtin_inff();
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          float s = acc[rb][ub][j] + bias;
          if constexpr (DRAW_LATE) {
            const float p = __fmul_rn(s, a.inv_tau);
            acc[rb][ub][j] = p;  // (the key is p + g: formed in the candidate loop, for what may reach the threshold)
            bool may = ul < nu && __fadd_rn(p, DROP_GUMBEL_MAX) >= tS;  // (false for a NaN)
            if (may) {
              const uint32_t row = (uint32_t)(r0 + rw + rb * 32 + (j >> 2) * 8 + half * 4 + (j & 3));
              may = __fadd_rn(p, drop_gumbel_bound(drop_word(z_lo[ub], z_hi[ub], row))) >= tS;
            }
            if (may) pend |= 1ull << (ub * 32 + rb * 16 + j);
          } else {
            if constexpr (SAMPLE) {
              const float p = __fmul_rn(s, a.inv_tau);
              s = p;  // (without a draw: p <= fl(p + DROP_GUMBEL_MAX) < tS, or a NaN -- not a candidate either way)
              if (ul < nu && __fadd_rn(p, DROP_GUMBEL_MAX) >= tS) {  // (false for a NaN)
                const uint32_t row = (uint32_t)(r0 + rw + rb * 32 + (j >> 2) * 8 + half * 4 + (j & 3));
                s = __fadd_rn(p, drop_gumbel(drop_word(z_lo[ub], z_hi[ub], row)));
              }
            }
            acc[rb][ub][j] = s;
            if (ul < nu && s >= tS) pend |= 1ull << (ub * 32 + rb * 16 + j);  // (false for a NaN)
          }
        }
    }
    // only what lies inside the user's window -- and so inside the table -- is a candidate: a user whose window is elsewhere
    // keeps its threshold at the filler, and would otherwise walk all 64 scores of the lane through the loop below
    const int64_t first = r0 + rw + half * 4;
    pend &= (uint64_t)win.inside(0, first) | ((uint64_t)win.inside(1, first) << 32);
    for (;;) {
      int overflow = 0;
      for (uint64_t todo = pend; todo; todo &= todo - 1) {
        const int b = __ffsll((unsigned long long)todo) - 1;
        // element b of the lane's 64 scores
        float s = (b & 32) ? ((b & 16) ? tk_pick16(acc[1][1], b) : tk_pick16(acc[0][1], b))
                           : ((b & 16) ? tk_pick16(acc[1][0], b) : tk_pick16(acc[0][0], b));
        const int ul = uw + (b >> 5) * 32 + l32;
        const int64_t row = r0 + rw + ((b >> 4) & 1) * 32 + ((b & 15) >> 2) * 8 + half * 4 + (b & 3);
        if constexpr (DRAW_LATE) s = __fadd_rn(s, drop_gumbel(drop_word((b & 32) ? z_lo[1] : z_lo[0], (b & 32) ? z_hi[1] : z_hi[0], (uint32_t)row)));
        const uint64_t key = tk_key(s, (uint32_t)row);
        bool keep = false;
        if (row != a.pad_row && key > thr[ul]) {  // (`pend` holds rows inside the table and the user's window only)
          const int slot = atomicAdd(&cnt[ul], 1);
          if (slot < TK_CB) buf[ul * TK_CB + slot] = key;
          else keep = true;
        }
        if (keep) overflow = 1;
        else pend &= ~(1ull << b);
      }
      const int again = __syncthreads_or(overflow);
      tk_merge_phase<KCAP>(a, u0, lists, k, nu, false, halves[wave], buf, thr, cnt, wave, lane);
      __syncthreads();
      if (!again) break;
    }
  }
  tk_merge_phase<KCAP>(a, u0, lists, k, nu, true, halves[wave], buf, thr, cnt, wave, lane);  // the slice is done: what is still buffered
  if constexpr (KCAP > XNRS_TOPK_MAX_K) {
    __syncthreads();
    if (tid < nu) {  // a filler ends a list that is not full
      const int n = halves[tid & 3][0].nreal[tid >> 2];
      if (n < k) lists[(int64_t)tid * k + n] = TK_FILLER;
    }
  }
}

// dst[0, n) <- the keys of a deep list up to its filler (or all k), 256 at a time -> n; all 64 lanes of a wave
__device__ __forceinline__ int tk_load_list(const uint64_t* list, int k, uint64_t* dst, int lane) {
  for (int i0 = 0; i0 < k; i0 += 256) {
    uint64_t t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = i0 + 64 * j + lane < k ? list[i0 + 64 * j + lane] : TK_FILLER;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint64_t end = __ballot(t[j] == TK_FILLER);
      const int n = end ? __ffsll((unsigned long long)end) - 1 : 64;  // (the keys of these 64 before the first filler)
      if (lane < n) dst[i0 + 64 * j + lane] = t[j];
      if (end) return i0 + 64 * j + n;
    }
  }
  return k;
}

// rows[b, :], scores[b, :] <- the k greatest keys of the `slices` sorted lists of user b; one wave per user (KCAP = 1024: 96 KB)
template <int KCAP>
__global__ __launch_bounds__(256) void topk_merge_kernel(const uint64_t* part, int slices, int64_t B, int k, int32_t* rows,
                                                         float* scores) {
  __shared__ uint64_t lds[4][3][KCAP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * 4 + wave;
  if (b >= B) return;  // (no workgroup barrier below)
  uint64_t *cur = lds[wave][0], *in = lds[wave][1], *nxt = lds[wave][2];
  if constexpr (KCAP > XNRS_TOPK_MAX_K) {
    // long lists that the floor of the first sweep leaves mostly empty, each ended by a filler when it is not full (what lies
    // behind that filler was never written): only the real keys are loaded, searched and placed.  cur[0, nc) and in[0, ni)
    // are the real keys; what lies past them is never read
    int nc = tk_load_list(part + b * k, k, cur, lane);
    for (int s = 1; s < slices; ++s) {
      tk_wave_sync();  // (the searches of the round before have read `in`)
      const int ni = tk_load_list(part + ((int64_t)s * B + b) * k, k, in, lane);
      tk_wave_sync();
      for (int i = lane; i < nc; i += 64) {
        const int rc = i + tk_count_greater<KCAP>(in, ni, cur[i]);
        if (rc < k) nxt[rc] = cur[i];
      }
      for (int i = lane; i < ni; i += 64) {
        const int ri = i + tk_count_greater<KCAP>(cur, nc, in[i]);
        if (ri < k) nxt[ri] = in[i];
      }
      nc = nc + ni < k ? nc + ni : k;
      tk_wave_sync();
      uint64_t* t = cur;
      cur = nxt;
      nxt = t;
    }
    tk_wave_sync();
    for (int i = lane; i < k; i += 64) {
      const uint64_t key = i < nc ? cur[i] : TK_FILLER;
      rows[b * k + i] = (int32_t)~(uint32_t)key;
      scores[b * k + i] = tk_score(key);
    }
  } else {
    for (int i = lane; i < k; i += 64) cur[i] = part[b * k + i];
    for (int s = 1; s < slices; ++s) {
      const uint64_t* list = part + ((int64_t)s * B + b) * k;
      for (int i = lane; i < k; i += 64) in[i] = list[i];
      tk_wave_sync();
      // two sorted lists: a key's place is its index plus the other list's count of greater keys.  Real keys are distinct;
      // two fillers may land on one place, with the same value
      for (int i = lane; i < k; i += 64) {
        const int rc = i + tk_count_greater<KCAP>(in, k, cur[i]);
        if (rc < k) nxt[rc] = cur[i];
        const int ri = i + tk_count_greater<KCAP>(cur, k, in[i]);
        if (ri < k) nxt[ri] = in[i];
      }
      tk_wave_sync();
      uint64_t* t = cur;
      cur = nxt;
      nxt = t;
    }
    tk_wave_sync();
    for (int i = lane; i < k; i += 64) {
      rows[b * k + i] = (int32_t)~(uint32_t)cur[i];
      scores[b * k + i] = tk_score(cur[i]);
    }
  }
}

// floor[b] <- a key that at least k eligible rows of user b are known to reach, less one -- so that "key > floor" admits them
// all -- from the first sweep's lists of kl keys per slice: the lowest kl-th key among the slices whose list is full, when those
// lists hold k keys between them; the filler (no floor) when they do not.  One thread per user.
__global__ __launch_bounds__(256) void topk_floor_kernel(const uint64_t* part, int slices, int64_t B, int kl, int k, uint64_t* floor) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  uint64_t lowest = ~0ull;
  int64_t full = 0;
  for (int s = 0; s < slices; ++s) {
    const uint64_t last = part[((int64_t)s * B + b) * kl + kl - 1];
    if (last > TK_FILLER) {  // (a real key: the slice has kl eligible rows)
      ++full;
      lowest = last < lowest ? last : lowest;
    }
  }
  floor[b] = full * kl >= k ? lowest - 1 : TK_FILLER;
}

struct TopkCall : SweepCall {
  int32_t k;
  int32_t* rows;
  float* scores;
  bool deep;  // xnrs_topk_deep*: k up to XNRS_TOPK_DEEP_MAX_K
  // xnrs_topk_sample*: the keys are score / temperature + Gumbel noise of (seed, user key, row); `scores` receives the keys
  bool sample;
  float temperature;
  uint64_t seed;
  const int64_t* user_keys;
};

// the projected user side [B, proj_width] | k > XNRS_TOPK_MAX_K: the floor keys [B] | the partial lists [slices, B, k] of 64-bit keys
size_t tk_workspace_bytes(int64_t B, int64_t n_rows, int32_t proj_width, int32_t k, int32_t max_k) {
  if (B <= 0 || n_rows < 0 || proj_width < 0 || k < 1 || k > max_k) return 0;
  return carve_total({(size_t)B * proj_width * F32, k > XNRS_TOPK_MAX_K ? (size_t)B * sizeof(uint64_t) : 0,
                      (size_t)xnrs_topk_slices(B, n_rows) * B * k * sizeof(uint64_t)});
}

int32_t tk_check(const TopkCall& c, const float* u, bool* run) {
  const int32_t max_k = c.deep ? XNRS_TOPK_DEEP_MAX_K : XNRS_TOPK_MAX_K;
  if (c.k < 1 || c.k > max_k) return XNRS_EINVAL;
  // (!(x > 0) refuses a NaN; a temperature so small that its reciprocal overflows would turn a zero score into a NaN key)
  if (c.sample && (!(c.temperature > 0.f) || !std::isfinite(c.temperature) || !std::isfinite(1.f / c.temperature))) return XNRS_EINVAL;
  XNRS_TRY_RC(sweep_check(c, u, run));
  if (*run && (!c.rows || !c.scores)) return XNRS_EINVAL;
  if (*run && (!c.ws || c.ws_bytes < tk_workspace_bytes(c.B, c.n_rows, c.proj_width, c.k, max_k))) return XNRS_EWORKSPACE;
  return XNRS_OK;
}

// the launches; up, w2, bias as sweep_operands takes them.  k <= XNRS_TOPK_MAX_K runs
// the two kernels of xnrs_topk* whichever entry point was called.  A longer list runs their XNRS_TOPK_DEEP_MAX_K instantiations,
// which move a list of k keys through LDS on every merge: the inner-product forms therefore sweep the table twice.  The first
// sweep, with the kernels of xnrs_topk*, keeps kl = ceil(k / (slices - 1)) keys per slice -- one slice may be short -- and
// topk_floor_kernel turns them into a key that k rows of the user are known to reach; the second sweep starts its thresholds
// there, so that about k rows of the whole table pass instead of about k (1 + ln(slice rows / k)) per slice.  The floor only
// removes rows that cannot be among the k, so the result does not depend on it.  The MLP form sweeps once: its tanhf cost more
// than its merges.  The first sweep's lists lie where the second sweep's will (they are dead by then).
// SAMPLE (xnrs_topk_sample*): the same launches with the sampled instantiations of the partial kernel; both sweeps of a deep
// call draw the same noise, so the floor is a floor of the perturbed keys.
template <bool SAMPLE>
hipError_t tk_launch_as(const TopkCall& c, const float* up, const float* w2, const float* bias, hipStream_t stream) {
  const int32_t slices = xnrs_topk_slices(c.B, c.n_rows);
  typename TkArgsOf<SAMPLE>::type a{};
  sweep_operands(c, up, w2, bias, a);
  a.k = c.k;
  if constexpr (SAMPLE) {
    a.inv_tau = 1.f / c.temperature;
    a.seed = c.seed;
    a.user_keys = c.user_keys;
  }
  const bool deep = c.k > XNRS_TOPK_MAX_K;
  Carver carve;
  carve.take((size_t)c.B * c.proj_width * F32);
  uint64_t* floor = at<uint64_t>(c.ws, carve.take_if(deep, (size_t)c.B * sizeof(uint64_t)));
  a.part = at<uint64_t>(c.ws, carve.take(0));
  const int64_t tiles = (c.B + TK_TILE - 1) / TK_TILE;
  if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)tiles, (unsigned)slices);
  const int kl = slices > 1 ? (c.k + slices - 2) / (slices - 1) : 0;
  if (deep && !w2 && kl >= 1 && kl <= XNRS_TOPK_MAX_K) {
    a.k = kl;
    hipLaunchKernelGGL((topk_partial_kernel<false, XNRS_TOPK_MAX_K, SAMPLE>), grid, dim3(256), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(topk_floor_kernel, dim3((unsigned)((c.B + 255) / 256)), dim3(256), 0, stream, a.part, slices, c.B, kl, c.k, floor);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    a.k = c.k;
    a.floor = floor;
  }
  if (deep && w2) hipLaunchKernelGGL((topk_partial_kernel<true, XNRS_TOPK_DEEP_MAX_K, SAMPLE>), grid, dim3(256), 0, stream, a);
  else if (deep) hipLaunchKernelGGL((topk_partial_kernel<false, XNRS_TOPK_DEEP_MAX_K, SAMPLE>), grid, dim3(256), 0, stream, a);
  else if (w2) hipLaunchKernelGGL((topk_partial_kernel<true, XNRS_TOPK_MAX_K, SAMPLE>), grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((topk_partial_kernel<false, XNRS_TOPK_MAX_K, SAMPLE>), grid, dim3(256), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 mgrid((unsigned)((c.B + 3) / 4));
  if (deep) hipLaunchKernelGGL(topk_merge_kernel<XNRS_TOPK_DEEP_MAX_K>, mgrid, dim3(256), 0, stream, a.part, slices, c.B, c.k, c.rows, c.scores);
  else hipLaunchKernelGGL(topk_merge_kernel<XNRS_TOPK_MAX_K>, mgrid, dim3(256), 0, stream, a.part, slices, c.B, c.k, c.rows, c.scores);
  return hipGetLastError();
}
hipError_t tk_launch(const TopkCall& c, const float* up, const float* w2, const float* bias, hipStream_t stream) {
  return c.sample ? tk_launch_as<true>(c, up, w2, bias, stream) : tk_launch_as<false>(c, up, w2, bias, stream);
}

// what xnrs_topk_sample* adds to a deep call
struct TkNoise {
  float temperature;
  uint64_t seed;
  const int64_t* user_keys;
};

// the one body of the twelve entry points: W the table's width (E, or H of the MLP form); win_lo, win_hi NULL without windows;
// noise NULL but for xnrs_topk_sample*
int32_t tk_run(bool deep, const Scorer& s, const float* table, int64_t n_rows, int32_t W, const float* u, int64_t B,
               const int64_t* excl_off, const int32_t* excl_rows, const int32_t* win_lo, const int32_t* win_hi, int32_t pad_row,
               int32_t k, int32_t* rows, float* scores, void* ws, size_t ws_bytes, void* stream, const TkNoise* noise = nullptr) {
  const SweepCall sc(table, n_rows, W, B, excl_off, excl_rows, win_lo, win_hi, pad_row, ws, ws_bytes, s.form == Scorer::DOT ? 0 : W);
  TopkCall c{sc, k, rows, scores, deep};
  if (noise) c.sample = true, c.temperature = noise->temperature, c.seed = noise->seed, c.user_keys = noise->user_keys;
  return sweep_scored<TopkCall>(c, s, u, tk_check, tk_launch, (hipStream_t)stream);
}

}  // namespace

}  // namespace xnrs

using namespace xnrs;

extern "C" {

int32_t xnrs_topk_slices(int64_t B, int64_t n_rows) {
  const int64_t chunks = (n_rows + TK_TILE - 1) / TK_TILE;
  if (B <= 0 || chunks <= 0) return 1;
  const int64_t cps = tk_chunks_per_slice(B, n_rows);
  return (int32_t)((chunks + cps - 1) / cps);
}

size_t xnrs_topk_workspace_bytes(int64_t B, int64_t n_rows, int32_t proj_width, int32_t k) {
  return tk_workspace_bytes(B, n_rows, proj_width, k, XNRS_TOPK_MAX_K);
}

int32_t xnrs_topk(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const int64_t* excl_off,
                  const int32_t* excl_rows, int32_t pad_row, int32_t k, int32_t* rows, float* scores, void* ws, size_t ws_bytes,
                  void* stream) {
  return tk_run(false, {}, table, n_rows, E, u, B, excl_off, excl_rows, nullptr, nullptr, pad_row, k, rows, scores, ws, ws_bytes, stream);
}

int32_t xnrs_topk_bilinear(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const float* w,
                           const float* bias, const int64_t* excl_off, const int32_t* excl_rows, int32_t pad_row, int32_t k,
                           int32_t* rows, float* scores, void* ws, size_t ws_bytes, void* stream) {
  return tk_run(false, sc_bilinear(w, bias), table, n_rows, E, u, B, excl_off, excl_rows, nullptr, nullptr, pad_row, k, rows, scores, ws,
                ws_bytes, stream);
}

int32_t xnrs_topk_mlp(const float* P, int64_t n_rows, int32_t E, int32_t H, const float* u, int64_t B, const float* w1,
                      const float* b1, const float* w2, const float* b2, const int64_t* excl_off, const int32_t* excl_rows,
                      int32_t pad_row, int32_t k, int32_t* rows, float* scores, void* ws, size_t ws_bytes, void* stream) {
  return tk_run(false, sc_mlp(E, w1, b1, w2, b2), P, n_rows, H, u, B, excl_off, excl_rows, nullptr, nullptr, pad_row, k, rows, scores, ws,
                ws_bytes, stream);
}

size_t xnrs_topk_deep_workspace_bytes(int64_t B, int64_t n_rows, int32_t proj_width, int32_t k) {
  return tk_workspace_bytes(B, n_rows, proj_width, k, XNRS_TOPK_DEEP_MAX_K);
}

// ---- the row-window entry points: the argument lists of their parents with win_lo, win_hi behind excl_rows
int32_t xnrs_topk_deep_win(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const int64_t* excl_off,
                           const int32_t* excl_rows, const int32_t* win_lo, const int32_t* win_hi, int32_t pad_row, int32_t k,
                           int32_t* rows, float* scores, void* ws, size_t ws_bytes, void* stream) {
  return tk_run(true, {}, table, n_rows, E, u, B, excl_off, excl_rows, win_lo, win_hi, pad_row, k, rows, scores, ws, ws_bytes, stream);
}

int32_t xnrs_topk_deep_bilinear_win(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const float* w,
                                    const float* bias, const int64_t* excl_off, const int32_t* excl_rows, const int32_t* win_lo,
                                    const int32_t* win_hi, int32_t pad_row, int32_t k, int32_t* rows, float* scores, void* ws,
                                    size_t ws_bytes, void* stream) {
  return tk_run(true, sc_bilinear(w, bias), table, n_rows, E, u, B, excl_off, excl_rows, win_lo, win_hi, pad_row, k, rows, scores, ws,
                ws_bytes, stream);
}

int32_t xnrs_topk_deep_mlp_win(const float* P, int64_t n_rows, int32_t E, int32_t H, const float* u, int64_t B, const float* w1,
                               const float* b1, const float* w2, const float* b2, const int64_t* excl_off,
                               const int32_t* excl_rows, const int32_t* win_lo, const int32_t* win_hi, int32_t pad_row, int32_t k,
                               int32_t* rows, float* scores, void* ws, size_t ws_bytes, void* stream) {
  return tk_run(true, sc_mlp(E, w1, b1, w2, b2), P, n_rows, H, u, B, excl_off, excl_rows, win_lo, win_hi, pad_row, k, rows, scores, ws,
                ws_bytes, stream);
}

// ---- xnrs_topk_sample*_win: the deep twins with the noise behind k
int32_t xnrs_topk_sample_win(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const int64_t* excl_off,
                             const int32_t* excl_rows, const int32_t* win_lo, const int32_t* win_hi, int32_t pad_row, int32_t k,
                             float temperature, uint64_t seed, const int64_t* user_keys, int32_t* rows, float* scores, void* ws,
                             size_t ws_bytes, void* stream) {
  const TkNoise noise{temperature, seed, user_keys};
  return tk_run(true, {}, table, n_rows, E, u, B, excl_off, excl_rows, win_lo, win_hi, pad_row, k, rows, scores, ws, ws_bytes, stream,
                &noise);
}

int32_t xnrs_topk_sample_bilinear_win(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const float* w,
                                      const float* bias, const int64_t* excl_off, const int32_t* excl_rows, const int32_t* win_lo,
                                      const int32_t* win_hi, int32_t pad_row, int32_t k, float temperature, uint64_t seed,
                                      const int64_t* user_keys, int32_t* rows, float* scores, void* ws, size_t ws_bytes,
                                      void* stream) {
  const TkNoise noise{temperature, seed, user_keys};
  return tk_run(true, sc_bilinear(w, bias), table, n_rows, E, u, B, excl_off, excl_rows, win_lo, win_hi, pad_row, k, rows, scores, ws,
                ws_bytes, stream, &noise);
}

int32_t xnrs_topk_sample_mlp_win(const float* P, int64_t n_rows, int32_t E, int32_t H, const float* u, int64_t B, const float* w1,
                                 const float* b1, const float* w2, const float* b2, const int64_t* excl_off,
                                 const int32_t* excl_rows, const int32_t* win_lo, const int32_t* win_hi, int32_t pad_row, int32_t k,
                                 float temperature, uint64_t seed, const int64_t* user_keys, int32_t* rows, float* scores,
                                 void* ws, size_t ws_bytes, void* stream) {
  const TkNoise noise{temperature, seed, user_keys};
  return tk_run(true, sc_mlp(E, w1, b1, w2, b2), P, n_rows, H, u, B, excl_off, excl_rows, win_lo, win_hi, pad_row, k, rows, scores, ws,
                ws_bytes, stream, &noise);
}

// ---- xnrs_topk_deep*: their _win twins without windows
int32_t xnrs_topk_deep(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const int64_t* excl_off,
                       const int32_t* excl_rows, int32_t pad_row, int32_t k, int32_t* rows, float* scores, void* ws,
                       size_t ws_bytes, void* stream) {
  return xnrs_topk_deep_win(table, n_rows, E, u, B, excl_off, excl_rows, nullptr, nullptr, pad_row, k, rows, scores, ws, ws_bytes, stream);
}

int32_t xnrs_topk_deep_bilinear(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const float* w,
                                const float* bias, const int64_t* excl_off, const int32_t* excl_rows, int32_t pad_row, int32_t k,
                                int32_t* rows, float* scores, void* ws, size_t ws_bytes, void* stream) {
  return xnrs_topk_deep_bilinear_win(table, n_rows, E, u, B, w, bias, excl_off, excl_rows, nullptr, nullptr, pad_row, k, rows, scores, ws,
                                     ws_bytes, stream);
}

int32_t xnrs_topk_deep_mlp(const float* P, int64_t n_rows, int32_t E, int32_t H, const float* u, int64_t B, const float* w1,
                           const float* b1, const float* w2, const float* b2, const int64_t* excl_off, const int32_t* excl_rows,
                           int32_t pad_row, int32_t k, int32_t* rows, float* scores, void* ws, size_t ws_bytes, void* stream) {
  return xnrs_topk_deep_mlp_win(P, n_rows, E, H, u, B, w1, b1, w2, b2, excl_off, excl_rows, nullptr, nullptr, pad_row, k, rows, scores,
                                ws, ws_bytes, stream);
}

}  // extern "C"
