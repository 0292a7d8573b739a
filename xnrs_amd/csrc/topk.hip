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
// Score tile
//   inner product (dot, bilinear): the fp32 MFMA v_mfma_f32_32x32x2_f32 over ascending feature index, no split-K: bit for bit
//             one fp32 fma chain from 0 per (user, row); the bias is added last.
//   MLP     : w2 . tanh(q_b + P_n) + b2 on the VALU, h ascending, the tanhf of score_csr_mlp_kernel.
// Either way the score of a (user, row) pair depends on nothing but that pair, so a user's result does not depend on B, on the
// user's position in the batch or on the slicing, and is the same bits on every run.
//
// Row windows (xnrs_topk_deep*_win, xnrs_rank*_win): user b sees the rows [win_lo[b], win_hi[b]) only -- the result of the call
// with every other row on b's exclusion list.  Both sweeps take their windows and their chunk range from tk_tile_range: a
// workgroup walks the union of its users' windows, split evenly over the slices, instead of a fixed share of the table.
//
// Order: key = (order-preserving score bits << 32) | ~row, so "higher score first, equal scores (-0 == +0) lower row first" is
// one unsigned compare.  A NaN score is never selected; -inf is a legal score.  Missing entries (fewer than k eligible rows)
// are fillers -- row -1, score -inf -- whose key lies below every real key.  The ranking is by the RAW score: no ReLU (the
// evaluation's relu would tie every negative score).
#include "host.h"

namespace xnrs {

namespace {

constexpr int TK_TILE = 128;             // users per workgroup = table rows per chunk
constexpr int TK_KT = 32;                // features per LDS stage
constexpr int TK_PITCH = TK_TILE + 1;    // feature-major LDS tiles: conflict-free transposing writes (4 * pitch = 4 mod 32)
constexpr int TK_CB = 32;                // candidate buffer entries per user
constexpr int TK_WGS = 512;              // workgroups that fill the chip: 256 CUs x 2 resident (79 872 B of LDS each, 160 KB per CU)
// the most slices of a call (a single user tile is the only case that wants more): the merge kernel folds a user's slice lists
// one after the other, which with 512 lists takes longer than the partial kernel; 256 still gives every CU a workgroup
constexpr int TK_MAX_SLICES = 256;
constexpr uint64_t TK_FILLER = 0x007FFFFFull << 32;  // score -inf, row -1: below the key of row 2^31 - 2 at score -inf

using f32x16 = __attribute__((ext_vector_type(16))) float;

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

// rows [r0, r0 + 128) x features [k0, k0 + 32) of a row-major [n][W] matrix, four float4 per thread: eight consecutive
// threads read 128 contiguous bytes of one row.  Rows past n and features past W read as 0.
// With GATHER the 128 rows are gather[0, 128) (LDS; a negative id reads as 0) instead of r0 + [0, 128).
struct TkTile {
  float4 v[4];
};
template <bool GATHER = false>
__device__ __forceinline__ void tk_load(TkTile& t, const float* x, int64_t n, int64_t r0, int W, int k0, int vec,
                                        const int32_t* gather = nullptr) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int idx = threadIdx.x + 256 * p;
    const int64_t r = GATHER ? (int64_t)gather[idx >> 3] : r0 + (idx >> 3);
    const int k = k0 + (idx & 7) * 4;
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if ((!GATHER || r >= 0) && r < n && k < W) {
      const float* s = x + r * W + k;
      if (vec) v = *reinterpret_cast<const float4*>(s);  // (W % 4 == 0 and a 16-B base: the four are inside the row)
      else {
        v.x = s[0];
        if (k + 1 < W) v.y = s[1];
        if (k + 2 < W) v.z = s[2];
        if (k + 3 < W) v.w = s[3];
      }
    }
    t.v[p] = v;
  }
}
__device__ __forceinline__ void tk_store(const TkTile& t, float* lds) {  // lds[feature][row]
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int idx = threadIdx.x + 256 * p;
    float* d = lds + (idx & 7) * 4 * TK_PITCH + (idx >> 3);
    d[0] = t.v[p].x;
    d[TK_PITCH] = t.v[p].y;
    d[2 * TK_PITCH] = t.v[p].z;
    d[3 * TK_PITCH] = t.v[p].w;
  }
}

// x[b & 15]: a tree of selects on the bits of b (no register is indexed at run time)
__device__ __forceinline__ float tk_pick16(const f32x16 x, int b) {
  const bool b0 = b & 1, b1 = b & 2, b2 = b & 4, b3 = b & 8;
  const float a0 = b0 ? x[1] : x[0], a1 = b0 ? x[3] : x[2], a2 = b0 ? x[5] : x[4], a3 = b0 ? x[7] : x[6];
  const float a4 = b0 ? x[9] : x[8], a5 = b0 ? x[11] : x[10], a6 = b0 ? x[13] : x[12], a7 = b0 ? x[15] : x[14];
  const float c0 = b1 ? a1 : a0, c1 = b1 ? a3 : a2, c2 = b1 ? a5 : a4, c3 = b1 ? a7 : a6;
  const float d0 = b2 ? c1 : c0, d1 = b2 ? c3 : c2;
  return b3 ? d1 : d0;
}

// what a score tile reads, and what every kernel over score tiles is told about the call
struct TkOperands {
  const float *table, *u, *w2, *bias;  // table:(n_rows, W), u:(B, W); w2:(W) in the MLP form
  const int64_t* excl_off;
  const int32_t* excl_rows;
  const int32_t *win_lo, *win_hi;  // xnrs_*_win: per user the row window [win_lo[b], win_hi[b]); both NULL: the whole table
  int64_t n_rows, B, chunks_per_slice;
  int W, pad_row, vec_t, vec_u;
};

// Row windows (xnrs_*_win).  A lane keeps the windows of its two users -- uw + l32 and uw + 32 + l32, the users of its score
// elements -- in registers, clamped to [0, n_rows], an empty one (lo >= hi, or no such user) as [0, 0); a bound is compared,
// never dereferenced.  Without windows every lane holds [0, n_rows): the window is the test for the table's end as well.
struct TkWin {
  int32_t lo[2], hi[2];
  int gaps;  // the tile's windows have no row in common: chunks between them may hold no window at all (tk_chunk_live)
  // Which of the lane's 32 score elements of user block ub lie inside the user's window: bit rb * 16 + j for element (rb, j),
  // the bit order of `pend`.  The element lies o = 32 rb + 8 (j / 4) + j % 4 rows behind the lane's first row of the chunk,
  // `first`; o grows with the bit index, so the elements with o < x are the lowest 4 (x / 8) + min(x % 8, 4) bits.
  __device__ __forceinline__ static uint32_t below(int64_t x) {
    const int c = x <= 0 ? 0 : x >= 64 ? 32 : 4 * ((int)x >> 3) + (((int)x & 7) < 4 ? ((int)x & 7) : 4);
    return c >= 32 ? ~0u : (1u << c) - 1u;
  }
  __device__ __forceinline__ uint32_t inside(int ub, int64_t first) const { return below(hi[ub] - first) & ~below(lo[ub] - first); }
};

// The chunks [c_lo, c_hi) of the sweep that workgroup (tile blockIdx.x, slice blockIdx.y) walks, and the lane's windows.
// Without windows: the fixed share chunks_per_slice of the whole table.  With windows: the tile's users reduce their windows
// to the chunk range of their union (integer min / max in LDS, rng[4]: found on the device, no host synchronisation), and
// the gridDim.y slices split THAT range evenly -- slice s takes [n s / S, n (s + 1) / S) of its n chunks, so that no slice is
// idle while another holds two chunks more; with n < S some slices are empty (they write fillers / an empty list).  All
// 256 threads call it (two workgroup barriers).  A user's result does not depend on the split: the slices are disjoint and
// cover every chunk that holds a row of a window of the tile.
__device__ __forceinline__ void tk_tile_range(const TkOperands& a, int64_t u0, int nu, int* rng, TkWin& w, int64_t& c_lo, int64_t& c_hi) {
  const int tid = threadIdx.x, wave = tid >> 6, l32 = tid & 31, uw = (wave & 1) * 64;
  if (!a.win_lo) {
    w.lo[0] = w.lo[1] = 0;
    w.hi[0] = w.hi[1] = (int32_t)a.n_rows;
    w.gaps = 0;
    const int64_t chunks = (a.n_rows + TK_TILE - 1) / TK_TILE;
    c_lo = (int64_t)blockIdx.y * a.chunks_per_slice;
    c_hi = c_lo + a.chunks_per_slice < chunks ? c_lo + a.chunks_per_slice : chunks;
    return;
  }
  if (tid == 0) {
    rng[0] = rng[3] = 0x7fffffff;  // the least lo / TK_TILE, the least hi
    rng[1] = rng[2] = 0;           // the greatest ceil(hi / TK_TILE), the greatest lo
  }
  __syncthreads();
#pragma unroll
  for (int ub = 0; ub < 2; ++ub) {
    const int ul = uw + ub * 32 + l32;
    int32_t lo = 0, hi = 0;
    if (ul < nu) {
      lo = a.win_lo[u0 + ul];
      hi = a.win_hi[u0 + ul];
      lo = lo < 0 ? 0 : lo;
      hi = hi > a.n_rows ? (int32_t)a.n_rows : hi;
      if (lo >= hi) lo = hi = 0;
    }
    w.lo[ub] = lo;
    w.hi[ub] = hi;
    if (wave < 2 && hi > lo) {  // (waves 0 and 1 hold every user of the tile once)
      atomicMin(&rng[0], lo / TK_TILE);
      atomicMax(&rng[1], (int)(((int64_t)hi + TK_TILE - 1) / TK_TILE));
      atomicMax(&rng[2], lo);
      atomicMin(&rng[3], hi);
    }
  }
  __syncthreads();
  const int64_t t_lo = rng[0], n = rng[1] > rng[0] ? rng[1] - t_lo : 0, S = gridDim.y;  // n == 0: every window of the tile is empty
  c_lo = t_lo + n * blockIdx.y / S;
  c_hi = t_lo + n * (blockIdx.y + 1) / S;
  w.gaps = rng[2] >= rng[3];  // (a row common to all windows: their union is one range, every chunk of it holds a window)
}

// whether chunk [r0, r0 + 128) holds a row of a window of the tile: the tile's windows may be disjoint, and the chunks of
// their union that lie between them are not scored.  Uniform over the workgroup (one barrier); called when w.gaps only.
__device__ __forceinline__ bool tk_chunk_live(const TkWin& w, int64_t r0) {
  const int64_t r1 = r0 + TK_TILE;
  return __syncthreads_or((w.lo[0] < r1 && w.hi[0] > r0) || (w.lo[1] < r1 && w.hi[1] > r0)) != 0;
}
struct TopkArgs : TkOperands {
  int k;
  uint64_t* part;
  const uint64_t* floor;  // xnrs_topk_deep*, k > XNRS_TOPK_MAX_K: per user a key below which nothing is wanted (topk_floor_kernel), or NULL
};

// The score tile, the ONE definition of every kernel that ranks: acc <- the scores, before the bias, of table rows
// r0 + [0, 128) (GATHER: rows gather[0, 128)) x users u0 + [0, 128).  acc[row block][user block]: element j of a lane is row
// 8 (j / 4) + 4 half + j % 4 of the wave's row block, user l32 of its user block.  A (row, user) score depends on nothing but
// that pair: not on the other rows and users of the tile, nor on where in the tile the pair sits.  All 256 threads call it;
// it begins and ends between workgroup barriers of its own, and on return At / Bt / w2s may still be read by other waves.
template <bool MLP, bool GATHER>
__device__ __forceinline__ void tk_score_tile(const TkOperands& a, int64_t r0, const int32_t* gather, int64_t u0, float* At, float* Bt,
                                              float* w2s, f32x16 (&acc)[2][2]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, half = lane >> 5;
  const int rw = (wave >> 1) * 64, uw = (wave & 1) * 64;  // the wave's 64 x 64 part of the score tile
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[i >> 1][i & 1][j] = 0.f;
  TkTile ta, tb;
  // the MFMA form loads the next stage while it computes this one; the MLP form is bound by its tanhf and keeps the registers
  if (!MLP) {
    tk_load<GATHER>(ta, a.table, a.n_rows, r0, a.W, 0, a.vec_t, gather);
    tk_load(tb, a.u, a.B, u0, a.W, 0, a.vec_u);
  }
  for (int k0 = 0; k0 < a.W; k0 += TK_KT) {
    if (MLP) {
      tk_load<GATHER>(ta, a.table, a.n_rows, r0, a.W, k0, a.vec_t, gather);
      tk_load(tb, a.u, a.B, u0, a.W, k0, a.vec_u);
    }
    __syncthreads();  // (the previous stage has been read)
    tk_store(ta, At);
    tk_store(tb, Bt);
    if (MLP && tid < TK_KT) w2s[tid] = k0 + tid < a.W ? a.w2[k0 + tid] : 0.f;
    __syncthreads();
    if (!MLP && k0 + TK_KT < a.W) {
      tk_load<GATHER>(ta, a.table, a.n_rows, r0, a.W, k0 + TK_KT, a.vec_t, gather);
      tk_load(tb, a.u, a.B, u0, a.W, k0 + TK_KT, a.vec_u);
    }
    const int kn = a.W - k0 < TK_KT ? a.W - k0 : TK_KT;
    if (!MLP) {
      for (int kk = 0; kk < kn; kk += 2) {  // (an odd width ends on a zero feature: the tile is zero-filled)
        const float* ap = At + (kk + half) * TK_PITCH + rw + l32;
        const float* bp = Bt + (kk + half) * TK_PITCH + uw + l32;
        const float a0 = ap[0], a1 = ap[32], b0 = bp[0], b1 = bp[32];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
    } else {
      for (int kk = 0; kk < kn; ++kk) {
        const float q0 = Bt[kk * TK_PITCH + uw + l32], q1 = Bt[kk * TK_PITCH + uw + 32 + l32], w = w2s[kk];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const float p = At[kk * TK_PITCH + rw + rb * 32 + (j >> 2) * 8 + half * 4 + (j & 3)];
            acc[rb][0][j] = fmaf(w, tanhf(q0 + p), acc[rb][0][j]);
            acc[rb][1][j] = fmaf(w, tanhf(q1 + p), acc[rb][1][j]);
          }
      }
    }
  }
}

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
// LDS in all, and is alone on its CU)
template <bool MLP, int KCAP = XNRS_TOPK_MAX_K>
__global__ __launch_bounds__(256, MLP || KCAP > XNRS_TOPK_MAX_K ? 1 : 2) void topk_partial_kernel(TopkArgs a) {
  __shared__ float At[TK_KT * TK_PITCH], Bt[TK_KT * TK_PITCH];  // table rows / users of one stage, feature-major
  __shared__ float w2s[TK_KT];
  __shared__ uint64_t buf[TK_TILE * TK_CB], thr[TK_TILE];
  __shared__ TkHalfT<KCAP> halves[4][2];
  __shared__ int cnt[TK_TILE];
  __shared__ int rng[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, half = lane >> 5;
  const int rw = (wave >> 1) * 64, uw = (wave & 1) * 64;  // the wave's 64 x 64 part of the score tile
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
          const float s = acc[rb][ub][j] + bias;
          acc[rb][ub][j] = s;
          if (ul < nu && s >= tS) pend |= 1ull << (ub * 32 + rb * 16 + j);  // (false for a NaN)
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
        const float s = (b & 32) ? ((b & 16) ? tk_pick16(acc[1][1], b) : tk_pick16(acc[0][1], b))
                                 : ((b & 16) ? tk_pick16(acc[1][0], b) : tk_pick16(acc[0][0], b));
        const int ul = uw + (b >> 5) * 32 + l32;
        const int64_t row = r0 + rw + ((b >> 4) & 1) * 32 + ((b & 15) >> 2) * 8 + half * 4 + (b & 3);
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

// ---------------------------------------------------------------------------------------------------------------- rank
// Where a user's target rows rank within the whole table: the sweep of topk_partial_kernel that COUNTS instead of selects.
//
//   target : grid = user tiles.  Round j gathers target j of each of the tile's users into one 128-row tile, forms that tile's
//            scores with tk_score_tile -- the function and the instruction of the sweep -- and keeps the diagonal: the score of
//            (user i, its own target).  It writes scores[] and starts ranks[] at 0, or at -1 for a query without an answer.
//            The round count (the most targets of a user of the tile) is found in the kernel.
//   sweep  : the grid, the slices and the score tiles of topk_partial_kernel.  Ineligible scores of a tile become NaN in the
//            registers (a NaN is greater than nothing and equal to nothing); then every lane counts, for each target of its
//            users, those of its 32 rows that come before the target in the order of tk_key -- s > s_t, or s == s_t in a
//            lower row.  The target's own row holds the very bits of s_t, so it never counts itself.  Counts are integers:
//            the first RK_SLOTS targets of a user add up in LDS across the chunks of the slice and reach ranks[] in one
//            global integer atomic per slice, the others take one per chunk.
//   Exclusions: a bitmap of the chunk, users x rows, in LDS, filled by walking each user's list (half a wave per user); ids
//            are compared, duplicates set a set bit again.
constexpr int RK_SLOTS = 4;

struct RankArgs : TkOperands {
  const int64_t* tgt_off;
  const int32_t* tgt_rows;
  int32_t* ranks;
  float* scores;
};

template <bool MLP>
__global__ __launch_bounds__(256, MLP ? 1 : 2) void rank_target_kernel(RankArgs a) {
  __shared__ float At[TK_KT * TK_PITCH], Bt[TK_KT * TK_PITCH];
  __shared__ float w2s[TK_KT];
  __shared__ int64_t t_lo[TK_TILE], t_n[TK_TILE];
  __shared__ int32_t gather[TK_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, half = lane >> 5;
  const int rw = (wave >> 1) * 64, uw = (wave & 1) * 64;
  const int64_t u0 = (int64_t)blockIdx.x * TK_TILE;
  const int nu = a.B - u0 < TK_TILE ? (int)(a.B - u0) : TK_TILE;
  if (tid < TK_TILE) {
    const int64_t lo = tid < nu ? a.tgt_off[u0 + tid] : 0, hi = tid < nu ? a.tgt_off[u0 + tid + 1] : 0;
    t_lo[tid] = lo;
    t_n[tid] = hi > lo ? hi - lo : 0;
  }
  __syncthreads();
  int64_t rounds = 0;
#pragma unroll 8
  for (int i = 0; i < TK_TILE; ++i) rounds = t_n[i] > rounds ? t_n[i] : rounds;  // (uniform: every thread reads the same LDS)
  const float bias = a.bias ? a.bias[0] : 0.f;
  const float nan = __builtin_nanf("");
  for (int64_t j = 0; j < rounds; ++j) {
    if (tid < TK_TILE) {
      int32_t g = -1;  // no target in this round, or one that is never dereferenced: outside the table, the pad row
      if (j < t_n[tid]) {
        const int32_t t = a.tgt_rows[t_lo[tid] + j];
        if (t >= 0 && t < a.n_rows && t != a.pad_row) g = t;
      }
      gather[tid] = g;
    }
    __syncthreads();
    f32x16 acc[2][2];
    tk_score_tile<MLP, true>(a, 0, gather, u0, At, Bt, w2s, acc);
    // the diagonal: row i of the tile is the target of user i.  It lies in the waves whose row half is their user half, in
    // block [b][b], in the lanes whose half holds row l32 of the block: 8 (j / 4) + 4 half + j % 4 == l32
    if (rw == uw && ((l32 >> 2) & 1) == half) {
      const int el = (l32 >> 3) * 4 + (l32 & 3);
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int ul = uw + b * 32 + l32;
        const float s = tk_pick16(acc[b][b], el) + bias;
        if (j < t_n[ul]) {
          const bool ok = gather[ul] >= 0 && s == s;
          a.scores[t_lo[ul] + j] = ok ? s : nan;
          if (a.ranks) a.ranks[t_lo[ul] + j] = ok ? 0 : -1;  // (NULL: xnrs_table_loss_fwd wants the scores alone)
        }
      }
    }
    __syncthreads();  // (gather is written again)
  }
}

template <bool MLP>
__global__ __launch_bounds__(256, MLP ? 1 : 2) void rank_sweep_kernel(RankArgs a) {
  __shared__ float At[TK_KT * TK_PITCH], Bt[TK_KT * TK_PITCH];
  __shared__ float w2s[TK_KT];
  __shared__ uint32_t excl[4 * TK_TILE];      // bit r % 32 of excl[(r / 32) * 128 + user]: row r of the chunk is excluded
  __shared__ int32_t slot[RK_SLOTS * TK_TILE];  // slot[i * 128 + user]: the slice's count for target i of the user
  __shared__ int rng[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, half = lane >> 5;
  const int rw = (wave >> 1) * 64, uw = (wave & 1) * 64;
  const int64_t u0 = (int64_t)blockIdx.x * TK_TILE;
  const int nu = a.B - u0 < TK_TILE ? (int)(a.B - u0) : TK_TILE;
  for (int i = tid; i < RK_SLOTS * TK_TILE; i += 256) slot[i] = 0;
  int64_t e_lo[2], e_hi[2];  // the targets of the lane's two users
#pragma unroll
  for (int ub = 0; ub < 2; ++ub) {
    const int ul = uw + ub * 32 + l32;
    e_lo[ub] = ul < nu ? a.tgt_off[u0 + ul] : 0;
    e_hi[ub] = ul < nu ? a.tgt_off[u0 + ul + 1] : 0;
  }
  const float bias = a.bias ? a.bias[0] : 0.f;
  const float nan = __builtin_nanf("");
  TkWin win;
  int64_t c_lo, c_hi;
  tk_tile_range(a, u0, nu, rng, win, c_lo, c_hi);
  for (int64_t c = c_lo; c < c_hi; ++c) {
    const int64_t r0 = c * TK_TILE;
    if (win.gaps && !tk_chunk_live(win, r0)) continue;  // (a target outside its window is ranked all the same: rank_target_kernel scored it)
    if (a.excl_off) {
      __syncthreads();  // (the bitmap of the chunk before has been read)
      for (int i = tid; i < 4 * TK_TILE; i += 256) excl[i] = 0;
      __syncthreads();
      for (int ul = tid >> 5; ul < nu; ul += 8) {
        const int64_t hi = a.excl_off[u0 + ul + 1];
        for (int64_t e = a.excl_off[u0 + ul] + l32; e < hi; e += 32) {
          const int64_t d = (int64_t)a.excl_rows[e] - r0;
          if (d >= 0 && d < TK_TILE) atomicOr(&excl[(int)(d >> 5) * TK_TILE + ul], 1u << (d & 31));
        }
      }
      // (the barriers of the score tile stand between these writes and the reads below)
    }
    f32x16 acc[2][2];
    tk_score_tile<MLP, false>(a, r0, nullptr, u0, At, Bt, w2s, acc);
    // ---- what may be counted: the bias added as the selection adds it, everything else NaN
#pragma unroll
    for (int ub = 0; ub < 2; ++ub) {
      const int ul = uw + ub * 32 + l32;
      const uint32_t in = win.inside(ub, r0 + rw + half * 4);  // (inside the window: inside the table as well)
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        const uint32_t word = a.excl_off ? excl[((rw >> 5) + rb) * TK_TILE + ul] : 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int bit = (j >> 2) * 8 + half * 4 + (j & 3);
          const int64_t row = r0 + rw + rb * 32 + bit;
          const bool ok = ((in >> (rb * 16 + j)) & 1u) && row != a.pad_row && !((word >> bit) & 1u);
          acc[rb][ub][j] = ok ? acc[rb][ub][j] + bias : nan;
        }
      }
    }
    // ---- count
#pragma unroll
    for (int ub = 0; ub < 2; ++ub) {
      const int ul = uw + ub * 32 + l32;
      for (int64_t e = e_lo[ub]; e < e_hi[ub]; ++e) {
        const float st = a.scores[e];
        if (!(st == st)) continue;  // rank -1: no answer
        // the lane's row of element (rb, j) is below the target's row when 32 rb + 8 (j / 4) + j % 4 < d
        int64_t d64 = (int64_t)a.tgt_rows[e] - (r0 + rw + half * 4);
        const int d = d64 < 0 ? 0 : d64 > 64 ? 64 : (int)d64;
        int n = 0;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const float s = acc[rb][ub][j];
            n += (s > st) || (s == st && rb * 32 + (j >> 2) * 8 + (j & 3) < d);
          }
        if (n) {
          if (e - e_lo[ub] < RK_SLOTS) atomicAdd(&slot[(int)(e - e_lo[ub]) * TK_TILE + ul], n);
          else atomicAdd(&a.ranks[e], n);
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < RK_SLOTS * TK_TILE; i += 256)
    if (slot[i]) atomicAdd(&a.ranks[a.tgt_off[u0 + (i & (TK_TILE - 1))] + (i >> 7)], slot[i]);  // (counted: the user and the target exist)
}

int64_t tk_chunks_per_slice(int64_t B, int64_t n_rows) {
  const int64_t tiles = (B + TK_TILE - 1) / TK_TILE, chunks = (n_rows + TK_TILE - 1) / TK_TILE;
  if (tiles <= 0 || chunks <= 0) return 1;
  int64_t want = (TK_WGS + tiles - 1) / tiles;
  if (want > TK_MAX_SLICES) want = TK_MAX_SLICES;
  if (want > chunks) want = chunks;
  return (chunks + want - 1) / want;
}

bool tk_vec_ok(const float* p, int W) { return W % 4 == 0 && reinterpret_cast<uintptr_t>(p) % 16 == 0; }

struct TopkCall {
  const float* table;  // (n_rows, W): the vectors of the inner-product forms, P of the MLP form
  int64_t n_rows;
  int32_t W;
  int64_t B;
  const int64_t* excl_off;
  const int32_t* excl_rows;
  int32_t pad_row, k;
  int32_t *rows;
  float* scores;
  void* ws;
  size_t ws_bytes;
  int32_t proj_width;
  bool deep;  // xnrs_topk_deep*: k up to XNRS_TOPK_DEEP_MAX_K
  const int32_t *win_lo = nullptr, *win_hi = nullptr;  // xnrs_topk_deep*_win: both or neither
};

// the projected user side [B, proj_width] | k > XNRS_TOPK_MAX_K: the floor keys [B] | the partial lists [slices, B, k] of 64-bit keys
size_t tk_workspace_bytes(int64_t B, int64_t n_rows, int32_t proj_width, int32_t k, int32_t max_k) {
  if (B <= 0 || n_rows < 0 || proj_width < 0 || k < 1 || k > max_k) return 0;
  return carve_total({(size_t)B * proj_width * F32, k > XNRS_TOPK_MAX_K ? (size_t)B * sizeof(uint64_t) : 0,
                      (size_t)xnrs_topk_slices(B, n_rows) * B * k * sizeof(uint64_t)});
}

// the argument checks every entry point shares; XNRS_OK with *run = false: nothing to do
int32_t tk_check(const TopkCall& c, const float* u, bool* run) {
  *run = false;
  const int32_t max_k = c.deep ? XNRS_TOPK_DEEP_MAX_K : XNRS_TOPK_MAX_K;
  if (c.k < 1 || c.k > max_k || c.W <= 0 || c.B < 0 || c.n_rows < 0 || c.n_rows > 0x7fffffffLL) return XNRS_EINVAL;
  if (!c.win_lo != !c.win_hi) return XNRS_EINVAL;
  if (c.B == 0) return XNRS_OK;
  if (!c.rows || !c.scores || !u || (c.n_rows > 0 && !c.table) || (c.excl_off && !c.excl_rows)) return XNRS_EINVAL;
  const size_t need = tk_workspace_bytes(c.B, c.n_rows, c.proj_width, c.k, max_k);
  if (!c.ws || c.ws_bytes < need) return XNRS_EWORKSPACE;
  *run = true;
  return XNRS_OK;
}

// the launches; up:(B, W) the user side as the kernel reads it (u, v = u W[0], q = u W1u^T + b1).  k <= XNRS_TOPK_MAX_K runs
// the two kernels of xnrs_topk* whichever entry point was called.  A longer list runs their XNRS_TOPK_DEEP_MAX_K instantiations,
// which move a list of k keys through LDS on every merge: the inner-product forms therefore sweep the table twice.  The first
// sweep, with the kernels of xnrs_topk*, keeps kl = ceil(k / (slices - 1)) keys per slice -- one slice may be short -- and
// topk_floor_kernel turns them into a key that k rows of the user are known to reach; the second sweep starts its thresholds
// there, so that about k rows of the whole table pass instead of about k (1 + ln(slice rows / k)) per slice.  The floor only
// removes rows that cannot be among the k, so the result does not depend on it.  The MLP form sweeps once: its tanhf cost more
// than its merges.  The first sweep's lists lie where the second sweep's will (they are dead by then).
hipError_t tk_launch(const TopkCall& c, const float* up, const float* w2, const float* bias, hipStream_t stream) {
  const int64_t cps = tk_chunks_per_slice(c.B, c.n_rows);
  const int32_t slices = xnrs_topk_slices(c.B, c.n_rows);
  TopkArgs a{};
  a.table = c.table;
  a.u = up;
  a.w2 = w2;
  a.bias = bias;
  a.excl_off = c.excl_off;
  a.excl_rows = c.excl_rows;
  a.win_lo = c.win_lo;
  a.win_hi = c.win_hi;
  a.n_rows = c.n_rows;
  a.B = c.B;
  a.chunks_per_slice = cps;
  a.W = c.W;
  a.k = c.k;
  a.pad_row = c.pad_row;
  a.vec_t = tk_vec_ok(c.table, c.W);
  a.vec_u = tk_vec_ok(up, c.W);
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
    hipLaunchKernelGGL(topk_partial_kernel<false>, grid, dim3(256), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(topk_floor_kernel, dim3((unsigned)((c.B + 255) / 256)), dim3(256), 0, stream, a.part, slices, c.B, kl, c.k, floor);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    a.k = c.k;
    a.floor = floor;
  }
  if (deep && w2) hipLaunchKernelGGL((topk_partial_kernel<true, XNRS_TOPK_DEEP_MAX_K>), grid, dim3(256), 0, stream, a);
  else if (deep) hipLaunchKernelGGL((topk_partial_kernel<false, XNRS_TOPK_DEEP_MAX_K>), grid, dim3(256), 0, stream, a);
  else if (w2) hipLaunchKernelGGL(topk_partial_kernel<true>, grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(topk_partial_kernel<false>, grid, dim3(256), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 mgrid((unsigned)((c.B + 3) / 4));
  if (deep) hipLaunchKernelGGL(topk_merge_kernel<XNRS_TOPK_DEEP_MAX_K>, mgrid, dim3(256), 0, stream, a.part, slices, c.B, c.k, c.rows, c.scores);
  else hipLaunchKernelGGL(topk_merge_kernel<XNRS_TOPK_MAX_K>, mgrid, dim3(256), 0, stream, a.part, slices, c.B, c.k, c.rows, c.scores);
  return hipGetLastError();
}

// the bodies of xnrs_topk / _bilinear / _mlp and of their xnrs_topk_deep twins (c.deep)
int32_t tk_dot(const TopkCall& c, const float* u, hipStream_t stream) {
  bool run;
  XNRS_TRY_RC(tk_check(c, u, &run));
  if (run) XNRS_TRY(tk_launch(c, u, nullptr, nullptr, stream));
  return XNRS_OK;
}

int32_t tk_bilinear(const TopkCall& c, const float* u, const float* w, const float* bias, hipStream_t stream) {
  const int32_t E = c.W;
  bool run;
  XNRS_TRY_RC(tk_check(c, u, &run));
  if (!run) return XNRS_OK;
  if (!w) return XNRS_EINVAL;
  float* v = static_cast<float*>(c.ws);
  XNRS_TRY(sc_gemm(u, E, w, E, 1, nullptr, v, E, c.B, E, E, stream));  // v_b = W[0]^T u_b, as xnrs_score_csr_bilinear
  XNRS_TRY(tk_launch(c, v, nullptr, bias, stream));
  return XNRS_OK;
}

int32_t tk_mlp(const TopkCall& c, int32_t E, const float* u, const float* w1, const float* b1, const float* w2, const float* b2,
               hipStream_t stream) {
  const int32_t H = c.W;
  if (E <= 0) return XNRS_EINVAL;
  bool run;
  XNRS_TRY_RC(tk_check(c, u, &run));
  if (!run) return XNRS_OK;
  if (!w1 || !w2) return XNRS_EINVAL;
  float* q = static_cast<float*>(c.ws);
  XNRS_TRY(sc_gemm(u, E, w1, 2 * (int64_t)E, 0, b1, q, H, c.B, H, E, stream));  // q_b = W1u u_b + b1, as xnrs_score_csr_mlp
  XNRS_TRY(tk_launch(c, q, w2, b2, stream));
  return XNRS_OK;
}

struct RankCall {
  const float* table;
  int64_t n_rows;
  int32_t W;
  int64_t B;
  const int64_t *tgt_off, *excl_off;
  const int32_t *tgt_rows, *excl_rows;
  int32_t pad_row;
  int32_t* ranks;
  float* scores;
  void* ws;
  size_t ws_bytes;
  int32_t proj_width;
  const int32_t *win_lo = nullptr, *win_hi = nullptr;  // xnrs_rank*_win: both or neither
};

int32_t rk_check(const RankCall& c, const float* u, bool* run) {
  *run = false;
  if (c.W <= 0 || c.B < 0 || c.n_rows < 0 || c.n_rows > 0x7fffffffLL) return XNRS_EINVAL;
  if (!c.win_lo != !c.win_hi) return XNRS_EINVAL;
  if (c.B == 0) return XNRS_OK;
  if (!c.ranks || !c.scores || !c.tgt_off || !c.tgt_rows || !u || (c.n_rows > 0 && !c.table) || (c.excl_off && !c.excl_rows))
    return XNRS_EINVAL;
  const size_t need = xnrs_rank_workspace_bytes(c.B, c.proj_width);
  if (need && (!c.ws || c.ws_bytes < need)) return XNRS_EWORKSPACE;
  *run = true;
  return XNRS_OK;
}

// the two launches; up, w2, bias as tk_launch
hipError_t rk_launch(const RankCall& c, const float* up, const float* w2, const float* bias, hipStream_t stream) {
  RankArgs a{};
  a.table = c.table;
  a.u = up;
  a.w2 = w2;
  a.bias = bias;
  a.excl_off = c.excl_off;
  a.excl_rows = c.excl_rows;
  a.win_lo = c.win_lo;
  a.win_hi = c.win_hi;
  a.n_rows = c.n_rows;
  a.B = c.B;
  a.chunks_per_slice = tk_chunks_per_slice(c.B, c.n_rows);
  a.W = c.W;
  a.pad_row = c.pad_row;
  a.vec_t = tk_vec_ok(c.table, c.W);
  a.vec_u = tk_vec_ok(up, c.W);
  a.tgt_off = c.tgt_off;
  a.tgt_rows = c.tgt_rows;
  a.ranks = c.ranks;
  a.scores = c.scores;
  const int64_t tiles = (c.B + TK_TILE - 1) / TK_TILE;
  if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  if (w2) hipLaunchKernelGGL(rank_target_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(rank_target_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || c.n_rows == 0) return e;  // (an empty table: every query has its -1 / NaN)
  const dim3 grid((unsigned)tiles, (unsigned)xnrs_topk_slices(c.B, c.n_rows));
  if (w2) hipLaunchKernelGGL(rank_sweep_kernel<true>, grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(rank_sweep_kernel<false>, grid, dim3(256), 0, stream, a);
  return hipGetLastError();
}

// the bodies of xnrs_rank / _bilinear / _mlp and of their _win twins
int32_t rk_dot(const RankCall& c, const float* u, hipStream_t stream) {
  bool run;
  XNRS_TRY_RC(rk_check(c, u, &run));
  if (run) XNRS_TRY(rk_launch(c, u, nullptr, nullptr, stream));
  return XNRS_OK;
}

int32_t rk_bilinear(const RankCall& c, const float* u, const float* w, const float* bias, hipStream_t stream) {
  const int32_t E = c.W;
  bool run;
  XNRS_TRY_RC(rk_check(c, u, &run));
  if (!run) return XNRS_OK;
  if (!w) return XNRS_EINVAL;
  float* v = static_cast<float*>(c.ws);
  XNRS_TRY(sc_gemm(u, E, w, E, 1, nullptr, v, E, c.B, E, E, stream));  // v_b = W[0]^T u_b, as xnrs_topk_bilinear
  XNRS_TRY(rk_launch(c, v, nullptr, bias, stream));
  return XNRS_OK;
}

int32_t rk_mlp(const RankCall& c, int32_t E, const float* u, const float* w1, const float* b1, const float* w2, const float* b2,
               hipStream_t stream) {
  const int32_t H = c.W;
  if (E <= 0) return XNRS_EINVAL;
  bool run;
  XNRS_TRY_RC(rk_check(c, u, &run));
  if (!run) return XNRS_OK;
  if (!w1 || !w2) return XNRS_EINVAL;
  float* q = static_cast<float*>(c.ws);
  XNRS_TRY(sc_gemm(u, E, w1, 2 * (int64_t)E, 0, b1, q, H, c.B, H, E, stream));  // q_b = W1u u_b + b1, as xnrs_topk_mlp
  XNRS_TRY(rk_launch(c, q, w2, b2, stream));
  return XNRS_OK;
}

// ---- the full-table softmax ranking loss (xnrs_table_loss_fwd / _bwd): the training side of the two sweeps -----------------
// loss[e] = -log(e^p / (e^p + sum_n e^(s_bn))) for query e = (user b, target t), p = s_bt, n over b's NEGATIVES: the rows
// eligible for xnrs_rank*_win minus every target row of b.  Scores come from tk_score_tile and from nothing else.
//   forward : rank_target_kernel (the target scores) | loss_sweep_kernel: the grid, slices, windows, gaps and exclusion bitmap
//             of rank_sweep_kernel -- the user's targets go into the bitmap next to the list -- and per (user, chunk) a
//             stabilised partial (max, sum of exp(s - max)) | loss_combine_kernel: one thread per user folds the partials of
//             the chunks its window touches in ascending chunk order; a chunk without a negative is skipped, so the running
//             value's bits do not see it.
//   The in-chunk tree is fixed by the row's place in the chunk alone: the 32 elements of a lane in (rb, j) order, the two
//   lane halves, the two row halves of the chunk.  A masked element adds +0 to a non-negative sum.  So lse and loss of a
//   user do not depend on B, on the user's place in the batch, on the other users' windows or on the slicing, and a windowed
//   call equals the call with the complement rows on the exclusion list, bit for bit.
//   backward: loss_bwd_kernel<false> (d_up) and <true> (d_table) recompute the score tile, form ds = c_b exp(s - lse_b) in the
//             score registers, pass it through LDS to become the left operand of a second fp32 MFMA product with the table
//             chunk (d_up: 128 users x 256 features per pass) or the user tile (d_table: 128 rows x 256 features per pass),
//             and write per-slice / per-group partials that loss_reduce_kernel sums in order.  The target terms
//             -g_e (1 - p_e) are gathered by the reduce kernel (d_up) or added to ds in the tile (d_table: a chunk is
//             visited for a target as well as for a window).  The order of the sums follows the slicing: the gradients are
//             the same bits on every run, but may differ between batch sizes.
constexpr int TL_FB = 256;       // features per pass of a backward sweep: 8 accumulators of 32 x 32 per wave
constexpr int TL_KS = 32;        // contraction rows per LDS stage of the second product (TL_KS x TL_FB floats = the score stages)
constexpr int TL_DSP = TK_TILE + 1;  // pitch of the ds tile: conflict-free for the transposing writes of the d_table sweep
constexpr int TL_BWD_WGS = 256;  // workgroups that fill the chip in the backward: 256 CUs x 1 resident (100 KB of LDS, 8 accumulators)
static_assert(TL_KS * TL_FB <= 2 * TK_KT * TK_PITCH, "the second product's stage lies in the score tile's two stages");

struct LossArgs : RankArgs {
  float2* part;           // forward: part[chunk * B + user] = (max, sum of exp(s - max)) over the user's negatives of the chunk
  float *loss, *lse;      // the forward writes them; the backward reads lse
  const float* g;         // backward: the upstream gradient per query
  float* out;             // backward sweep: [gridDim.y][B or n_rows][W] partials, or the gradient itself when gridDim.y == 1
  int64_t tiles_per_group;  // d_table sweep: user tiles per blockIdx.y
};

// the chunk's bitmap of rank_sweep_kernel with the users' own targets next to their exclusion lists (ids are compared, never
// dereferenced).  All 256 threads; the barriers of the score tile stand between these writes and their readers.
__device__ __forceinline__ void tl_bitmap(const RankArgs& a, int64_t r0, int64_t u0, int nu, uint32_t* excl) {
  const int tid = threadIdx.x, l32 = tid & 31;
  __syncthreads();  // (the bitmap of the tile before has been read)
  for (int i = tid; i < 4 * TK_TILE; i += 256) excl[i] = 0;
  __syncthreads();
  for (int ul = tid >> 5; ul < nu; ul += 8) {
    if (a.excl_off) {
      const int64_t hi = a.excl_off[u0 + ul + 1];
      for (int64_t e = a.excl_off[u0 + ul] + l32; e < hi; e += 32) {
        const int64_t d = (int64_t)a.excl_rows[e] - r0;
        if (d >= 0 && d < TK_TILE) atomicOr(&excl[(int)(d >> 5) * TK_TILE + ul], 1u << (d & 31));
      }
    }
    const int64_t hi = a.tgt_off[u0 + ul + 1];
    for (int64_t e = a.tgt_off[u0 + ul] + l32; e < hi; e += 32) {
      const int64_t d = (int64_t)a.tgt_rows[e] - r0;
      if (d >= 0 && d < TK_TILE) atomicOr(&excl[(int)(d >> 5) * TK_TILE + ul], 1u << (d & 31));
    }
  }
}

// which of the lane's 32 score elements of user block ub are negatives of the user: bit rb * 16 + j, the order of TkWin::inside
__device__ __forceinline__ uint32_t tl_negatives(const TkOperands& a, const TkWin& win, const uint32_t* excl, int ub, int64_t r0,
                                                 int rw, int half, int ul) {
  uint32_t ok = 0;
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const uint32_t word = excl[((rw >> 5) + rb) * TK_TILE + ul];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int bit = (j >> 2) * 8 + half * 4 + (j & 3);
      const int64_t row = r0 + rw + rb * 32 + bit;
      ok |= (uint32_t)(row != a.pad_row && !((word >> bit) & 1u)) << (rb * 16 + j);
    }
  }
  return ok & win.inside(ub, r0 + rw + half * 4);  // (inside the window: inside the table as well)
}

__global__ __launch_bounds__(256, 2) void loss_sweep_kernel(LossArgs a) {
  __shared__ float At[TK_KT * TK_PITCH], Bt[TK_KT * TK_PITCH];
  __shared__ uint32_t excl[4 * TK_TILE];
  __shared__ float red_m[2 * TK_TILE], red_s[2 * TK_TILE];  // [row half of the chunk][user]
  __shared__ int rng[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, half = lane >> 5;
  const int rw = (wave >> 1) * 64, uw = (wave & 1) * 64;
  const int64_t u0 = (int64_t)blockIdx.x * TK_TILE;
  const int nu = a.B - u0 < TK_TILE ? (int)(a.B - u0) : TK_TILE;
  const float bias = a.bias ? a.bias[0] : 0.f;
  const float ninf = -__builtin_inff();
  TkWin win;
  int64_t c_lo, c_hi;
  tk_tile_range(a, u0, nu, rng, win, c_lo, c_hi);
  for (int64_t c = c_lo; c < c_hi; ++c) {
    const int64_t r0 = c * TK_TILE;
    if (win.gaps && !tk_chunk_live(win, r0)) continue;  // (no user of the tile reads this chunk's partial)
    tl_bitmap(a, r0, u0, nu, excl);
    f32x16 acc[2][2];
    tk_score_tile<false, false>(a, r0, nullptr, u0, At, Bt, nullptr, acc);
    float m[2];
#pragma unroll
    for (int ub = 0; ub < 2; ++ub) {
      const int ul = uw + ub * 32 + l32;
      const uint32_t neg = tl_negatives(a, win, excl, ub, r0, rw, half, ul);
      float mm = ninf;
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float s = ((neg >> (rb * 16 + j)) & 1u) ? acc[rb][ub][j] + bias : ninf;
          acc[rb][ub][j] = s;
          mm = fmaxf(mm, s);
        }
      mm = fmaxf(mm, __shfl_xor(mm, 32));
      if (half == 0) red_m[(wave >> 1) * TK_TILE + ul] = mm;
    }
    __syncthreads();
#pragma unroll
    for (int ub = 0; ub < 2; ++ub) {
      const int ul = uw + ub * 32 + l32;
      const float M = fmaxf(red_m[ul], red_m[TK_TILE + ul]);
      float s = 0.f;
      if (M > ninf) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
          for (int j = 0; j < 16; ++j) s += __expf(acc[rb][ub][j] - M);  // (a masked element: exp(-inf) = +0)
      }
      s += __shfl_xor(s, 32);
      if (half == 0) red_s[(wave >> 1) * TK_TILE + ul] = s;
      m[ub] = M;
    }
    __syncthreads();
    if (rw == 0 && half == 0) {
#pragma unroll
      for (int ub = 0; ub < 2; ++ub) {
        const int ul = uw + ub * 32 + l32;
        if (ul < nu) a.part[c * a.B + u0 + ul] = make_float2(m[ub], red_s[ul] + red_s[TK_TILE + ul]);
      }
    }
  }
}

// loss of a query from its score and the user's lse: logaddexp(s, lse) - s = softplus(lse - s); 0 without an answer or negatives
__device__ __forceinline__ float tl_loss(float s, float lse) {
  if (!(s == s) || !(lse > -__builtin_inff())) return 0.f;
  const float d = lse - s;
  return d > 0.f ? d + log1pf(expf(-d)) : log1pf(expf(d));
}
// g (1 - p) of a query, p = exp(s - logaddexp(s, lse)): 1 - p = sigmoid(lse - s); 0 without an answer or negatives
__device__ __forceinline__ float tl_coef(float s, float lse, float g) {
  if (!(s == s) || !(lse > -__builtin_inff())) return 0.f;
  const float d = lse - s;
  if (d > 0.f) return g / (1.f + expf(-d));
  const float t = expf(d);
  return g * (t / (1.f + t));
}

__global__ __launch_bounds__(256) void loss_combine_kernel(LossArgs a) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= a.B) return;
  const float ninf = -__builtin_inff();
  int64_t c0 = 0, c1 = (a.n_rows + TK_TILE - 1) / TK_TILE;
  if (a.win_lo) {  // the chunks that hold a row of the user's window, clamped as tk_tile_range clamps it: those were written
    int64_t lo = a.win_lo[b], hi = a.win_hi[b];
    lo = lo < 0 ? 0 : lo;
    hi = hi > a.n_rows ? a.n_rows : hi;
    if (lo >= hi) lo = hi = 0;
    c0 = lo / TK_TILE;
    c1 = (hi + TK_TILE - 1) / TK_TILE;
  }
  float M = ninf, S = 0.f;
  for (int64_t c = c0; c < c1; ++c) {
    const float2 p = a.part[c * a.B + b];
    if (!(p.x > ninf)) continue;  // no negative in this chunk: the running value keeps its bits
    if (!(M > ninf)) {
      M = p.x;
      S = p.y;
    } else {
      const float nm = fmaxf(M, p.x);
      S = S * expf(M - nm) + p.y * expf(p.x - nm);
      M = nm;
    }
  }
  const float lse = M > ninf ? M + logf(S) : ninf;
  a.lse[b] = lse;
  const int64_t e_hi = a.tgt_off[b + 1];
  for (int64_t e = a.tgt_off[b]; e < e_hi; ++e) a.loss[e] = tl_loss(a.scores[e], lse);
}

// what a lane of a backward sweep knows of its two users: c_b = sum_e g_e (1 - p_e), lse_b and the span of the targets
struct TlUsers {
  float c[2], lse[2];
  int64_t e_lo[2], e_hi[2];
};
__device__ __forceinline__ void tl_users(const LossArgs& a, int64_t u0, int nu, TlUsers& t) {
  const int tid = threadIdx.x, wave = tid >> 6, l32 = tid & 31, uw = (wave & 1) * 64;
#pragma unroll
  for (int ub = 0; ub < 2; ++ub) {
    const int ul = uw + ub * 32 + l32;
    t.c[ub] = 0.f;
    t.lse[ub] = -__builtin_inff();
    t.e_lo[ub] = t.e_hi[ub] = 0;
    if (ul < nu) {
      t.e_lo[ub] = a.tgt_off[u0 + ul];
      t.e_hi[ub] = a.tgt_off[u0 + ul + 1];
      t.lse[ub] = a.lse[u0 + ul];
      for (int64_t e = t.e_lo[ub]; e < t.e_hi[ub]; ++e) t.c[ub] += tl_coef(a.scores[e], t.lse[ub], a.g[e]);
    }
  }
}
// the lane's windows as tk_tile_range leaves them, for a sweep that takes its chunk from the grid (a user that does not exist: [0, 0))
__device__ __forceinline__ void tl_windows(const TkOperands& a, int64_t u0, int nu, TkWin& w) {
  const int tid = threadIdx.x, wave = tid >> 6, l32 = tid & 31, uw = (wave & 1) * 64;
#pragma unroll
  for (int ub = 0; ub < 2; ++ub) {
    const int ul = uw + ub * 32 + l32;
    int32_t lo = 0, hi = 0;
    if (ul < nu) {
      lo = a.win_lo ? a.win_lo[u0 + ul] : 0;
      hi = a.win_hi ? a.win_hi[u0 + ul] : (int32_t)a.n_rows;
      lo = lo < 0 ? 0 : lo;
      hi = hi > a.n_rows ? (int32_t)a.n_rows : hi;
      if (lo >= hi) lo = hi = 0;
    }
    w.lo[ub] = lo;
    w.hi[ub] = hi;
  }
  w.gaps = 1;
}

// rows [r0, r0 + TL_KS) x features [f0, f0 + TL_FB) of a row-major [n][W] matrix, eight float4 per thread; zero past n and W
struct TlStage {
  float4 v[8];
};
__device__ __forceinline__ void tl_load(TlStage& t, const float* x, int64_t n, int64_t r0, int W, int f0, int vec) {
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int idx = threadIdx.x + 256 * p;
    const int64_t r = r0 + (idx >> 6);
    const int k = f0 + (idx & 63) * 4;
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < n && k < W) {
      const float* s = x + r * W + k;
      if (vec) v = *reinterpret_cast<const float4*>(s);
      else {
        v.x = s[0];
        if (k + 1 < W) v.y = s[1];
        if (k + 2 < W) v.z = s[2];
        if (k + 3 < W) v.w = s[3];
      }
    }
    t.v[p] = v;
  }
}
__device__ __forceinline__ void tl_store(const TlStage& t, float* lds) {  // lds[row][feature], pitch TL_FB
#pragma unroll
  for (int p = 0; p < 8; ++p) *reinterpret_cast<float4*>(lds + (threadIdx.x + 256 * p) * 4) = t.v[p];
}

// DT == false, d_up: grid = user tiles x slices, a workgroup walks the chunks of its slice (tk_tile_range) and accumulates
//   d_up[user][f] += sum_row ds[row][user] table[row][f] over them.
// DT == true, d_table: grid = row chunks x user groups, a workgroup walks the user tiles of its group and accumulates
//   d_table[row][f] += sum_user ds[row][user] up[user][f], ds with the target terms.
// Either way: out[(blockIdx.y * n + m) * W + f], n = B or n_rows, every (m, f) of the workgroup written (zeros where nothing flows).
// The wave (mh, fh) = (wave & 1, wave >> 1) holds output rows mh * 64 + [0, 64) x the 32-feature blocks 2 i + fh, i < 4, of the pass.
template <bool DT>
__global__ __launch_bounds__(256, 1) void loss_bwd_kernel(LossArgs a) {
  __shared__ __attribute__((aligned(16))) float stage[2 * TK_KT * TK_PITCH];  // At | Bt of the score tile, then the second product's rows
  __shared__ float ds[TK_TILE * TL_DSP];                                      // ds[contraction index][output row]
  __shared__ uint32_t excl[4 * TK_TILE];
  __shared__ int rng[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, half = lane >> 5;
  const int rw = (wave >> 1) * 64, uw = (wave & 1) * 64;
  const int mw = (wave & 1) * 64, fh = wave >> 1;
  const float bias = a.bias ? a.bias[0] : 0.f;
  const int64_t tiles = (a.B + TK_TILE - 1) / TK_TILE;
  int64_t it_lo, it_hi, u0 = 0, r0 = 0;
  int nu = 0;
  TkWin win;
  TlUsers us;
  if (!DT) {
    u0 = (int64_t)blockIdx.x * TK_TILE;
    nu = a.B - u0 < TK_TILE ? (int)(a.B - u0) : TK_TILE;
    tk_tile_range(a, u0, nu, rng, win, it_lo, it_hi);
    tl_users(a, u0, nu, us);
  } else {
    r0 = (int64_t)blockIdx.x * TK_TILE;
    it_lo = (int64_t)blockIdx.y * a.tiles_per_group;
    it_hi = it_lo + a.tiles_per_group < tiles ? it_lo + a.tiles_per_group : tiles;
  }
  for (int f0 = 0; f0 < a.W; f0 += TL_FB) {
    f32x16 acc2[2][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc2[i >> 2][i & 3][j] = 0.f;
    for (int64_t it = it_lo; it < it_hi; ++it) {
      if (!DT) {
        r0 = it * TK_TILE;
        if (win.gaps && !tk_chunk_live(win, r0)) continue;
      } else {
        u0 = it * TK_TILE;
        nu = a.B - u0 < TK_TILE ? (int)(a.B - u0) : TK_TILE;
        tl_windows(a, u0, nu, win);
        tl_users(a, u0, nu, us);
        const int64_t r1 = r0 + TK_TILE;
        bool live = false;  // a window of the tile holds a row of the chunk, or an answered query of the tile points into it
#pragma unroll
        for (int ub = 0; ub < 2; ++ub) {
          live = live || (us.c[ub] != 0.f && win.lo[ub] < r1 && win.hi[ub] > r0);
          for (int64_t e = us.e_lo[ub]; e < us.e_hi[ub]; ++e) {
            const int64_t t = a.tgt_rows[e];
            live = live || (t >= r0 && t < r1 && a.scores[e] == a.scores[e]);
          }
        }
        if (!__syncthreads_or(live)) continue;
      }
      tl_bitmap(a, r0, u0, nu, excl);
      f32x16 acc[2][2];
      tk_score_tile<false, false>(a, r0, nullptr, u0, stage, stage + TK_KT * TK_PITCH, nullptr, acc);
      // ---- ds in the score registers, then through LDS: the contraction index of the second product leads
#pragma unroll
      for (int ub = 0; ub < 2; ++ub) {
        const int ul = uw + ub * 32 + l32;
        const uint32_t neg = tl_negatives(a, win, excl, ub, r0, rw, half, ul);
        const bool on = us.c[ub] != 0.f && us.lse[ub] > -__builtin_inff();
        const float c = us.c[ub], lse = us.lse[ub];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
          for (int j = 0; j < 16; ++j)
            acc[rb][ub][j] = on && ((neg >> (rb * 16 + j)) & 1u) ? c * __expf(acc[rb][ub][j] + bias - lse) : 0.f;
        if (DT) {
          for (int64_t e = us.e_lo[ub]; e < us.e_hi[ub]; ++e) {
            const int64_t rel = (int64_t)a.tgt_rows[e] - r0 - rw;
            if (rel < 0 || rel >= 64 || (int)((rel >> 2) & 1) != half) continue;
            const float q = tl_coef(a.scores[e], lse, a.g[e]);  // (0 for a query without an answer: the pad row inside the chunk)
            const int el = (int)(rel >> 5) * 16 + (int)((rel >> 3) & 3) * 4 + (int)(rel & 3);
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
              for (int j = 0; j < 16; ++j) acc[rb][ub][j] -= rb * 16 + j == el ? q : 0.f;
          }
        }
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const int row = rw + rb * 32 + (j >> 2) * 8 + half * 4 + (j & 3);
            ds[DT ? ul * TL_DSP + row : row * TL_DSP + ul] = acc[rb][ub][j];
          }
      }
      // ---- the second product: TL_KS contraction rows per stage
      const float* x = DT ? a.u : a.table;
      const int64_t xn = DT ? a.B : a.n_rows, x0 = DT ? u0 : r0;
      const int vec = DT ? a.vec_u : a.vec_t;
      TlStage st;
      tl_load(st, x, xn, x0, a.W, f0, vec);
      for (int ks = 0; ks < TK_TILE; ks += TL_KS) {
        __syncthreads();  // (the stage before, or the score tile's, has been read; ds is written)
        tl_store(st, stage);
        __syncthreads();
        if (ks + TL_KS < TK_TILE) tl_load(st, x, xn, x0 + ks + TL_KS, a.W, f0, vec);
        for (int kk = 0; kk < TL_KS; kk += 2) {
          const float* ap = ds + (ks + kk + half) * TL_DSP + mw + l32;
          const float a0 = ap[0], a1 = ap[32];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int fb = (2 * i + fh) * 32;
            if (f0 + fb < a.W) {  // (uniform over the wave)
              const float b = stage[(kk + half) * TL_FB + fb + l32];
              acc2[0][i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc2[0][i], 0, 0, 0);
              acc2[1][i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc2[1][i], 0, 0, 0);
            }
          }
        }
      }
    }
    // ---- element j of a lane: output row 8 (j / 4) + 4 half + j % 4 of its block, feature l32 of its block
    const int64_t n = DT ? a.n_rows : a.B, m0 = DT ? r0 : (int64_t)blockIdx.x * TK_TILE;
    float* out = a.out + (int64_t)blockIdx.y * n * a.W;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int f = f0 + (2 * i + fh) * 32 + l32;
        if (f >= a.W) continue;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int64_t m = m0 + mw + mb * 32 + (j >> 2) * 8 + half * 4 + (j & 3);
          if (m < n) out[m * a.W + f] = acc2[mb][i][j];
        }
      }
  }
}

// out[m][f] = sum over the `parts` partials, in their order, and -- tgt_off given (d_up) -- the target terms of user m behind them
__global__ __launch_bounds__(256) void loss_reduce_kernel(const float* part, int parts, int64_t n, int W, float* out, LossArgs a,
                                                          int targets) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * W) return;
  float s = 0.f;
  for (int p = 0; p < parts; ++p) s += part[(int64_t)p * n * W + i];
  if (targets) {
    const int64_t b = i / W;
    const int f = (int)(i - b * W);
    const float lse = a.lse[b];
    const int64_t e_hi = a.tgt_off[b + 1];
    for (int64_t e = a.tgt_off[b]; e < e_hi; ++e) {
      const float q = tl_coef(a.scores[e], lse, a.g[e]);
      const int64_t t = a.tgt_rows[e];
      if (q != 0.f && t >= 0 && t < a.n_rows) s = fmaf(-q, a.table[t * W + f], s);  // (an answered query: a row of the table)
    }
  }
  out[i] = s;
}

// the slices of the d_up sweep and the user groups of the d_table sweep: enough workgroups for the chip, no more (their
// partials are slices x B x E and groups x n_rows x E floats)
int64_t tl_split(int64_t outer, int64_t inner) {  // over how many parts the `inner` loop is split when the grid has `outer` columns
  if (outer <= 0 || inner <= 0) return 1;
  int64_t want = (TL_BWD_WGS + outer - 1) / outer;
  if (want > inner) want = inner;
  const int64_t per = (inner + want - 1) / want;
  return (inner + per - 1) / per;
}

struct LossCall {
  const float *table, *up, *bias;
  int64_t n_rows;
  int32_t W;
  int64_t B;
  const int64_t *tgt_off, *excl_off;
  const int32_t *tgt_rows, *excl_rows, *win_lo, *win_hi;
  int32_t pad_row;
  float *scores, *lse;
  void* ws;
  size_t ws_bytes;
};

size_t tl_workspace_bytes(int64_t B, int64_t n_rows, int32_t E, int32_t want_d_table) {
  if (B <= 0 || n_rows < 0 || E <= 0) return 0;
  const int64_t tiles = (B + TK_TILE - 1) / TK_TILE, chunks = (n_rows + TK_TILE - 1) / TK_TILE;
  const size_t fwd = carve_total({(size_t)chunks * B * sizeof(float2)});
  const int64_t groups = tl_split(chunks, tiles);
  const size_t bwd = carve_total({(size_t)tl_split(tiles, chunks) * B * E * F32,
                                  want_d_table && groups > 1 ? (size_t)groups * n_rows * E * F32 : 0});
  return fwd > bwd ? fwd : bwd;
}

int32_t tl_check(const LossCall& c, bool* run) {
  *run = false;
  if (c.W <= 0 || c.B < 0 || c.n_rows < 0 || c.n_rows > 0x7fffffffLL) return XNRS_EINVAL;
  if (!c.win_lo != !c.win_hi) return XNRS_EINVAL;
  if (c.B == 0) return XNRS_OK;
  if (!c.scores || !c.lse || !c.tgt_off || !c.tgt_rows || !c.up || (c.n_rows > 0 && !c.table) || (c.excl_off && !c.excl_rows))
    return XNRS_EINVAL;
  if ((c.B + TK_TILE - 1) / TK_TILE > 0x7fffffffLL) return XNRS_EINVAL;
  *run = true;
  return XNRS_OK;
}

LossArgs tl_args(const LossCall& c) {
  LossArgs a{};
  a.table = c.table;
  a.u = c.up;
  a.bias = c.bias;
  a.excl_off = c.excl_off;
  a.excl_rows = c.excl_rows;
  a.win_lo = c.win_lo;
  a.win_hi = c.win_hi;
  a.n_rows = c.n_rows;
  a.B = c.B;
  a.chunks_per_slice = tk_chunks_per_slice(c.B, c.n_rows);
  a.W = c.W;
  a.pad_row = c.pad_row;
  a.vec_t = tk_vec_ok(c.table, c.W);
  a.vec_u = tk_vec_ok(c.up, c.W);
  a.tgt_off = c.tgt_off;
  a.tgt_rows = c.tgt_rows;
  a.scores = c.scores;
  a.lse = c.lse;
  return a;
}

int32_t tl_fwd(const LossCall& c, float* loss, hipStream_t stream) {
  bool run;
  XNRS_TRY_RC(tl_check(c, &run));
  if (!run) return XNRS_OK;
  if (!loss) return XNRS_EINVAL;
  const size_t need = tl_workspace_bytes(c.B, c.n_rows, c.W, 0);
  if (need && (!c.ws || c.ws_bytes < need)) return XNRS_EWORKSPACE;
  LossArgs a = tl_args(c);
  a.loss = loss;
  a.part = static_cast<float2*>(c.ws);
  const unsigned tiles = (unsigned)((c.B + TK_TILE - 1) / TK_TILE);
  hipLaunchKernelGGL(rank_target_kernel<false>, dim3(tiles), dim3(256), 0, stream, a);
  XNRS_TRY(hipGetLastError());
  if (c.n_rows > 0) {
    hipLaunchKernelGGL(loss_sweep_kernel, dim3(tiles, (unsigned)xnrs_topk_slices(c.B, c.n_rows)), dim3(256), 0, stream, a);
    XNRS_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(loss_combine_kernel, dim3((unsigned)((c.B + 255) / 256)), dim3(256), 0, stream, a);
  XNRS_TRY(hipGetLastError());
  return XNRS_OK;
}

int32_t tl_bwd(const LossCall& c, const float* g, float* d_up, float* d_table, hipStream_t stream) {
  bool run;
  XNRS_TRY_RC(tl_check(c, &run));
  if (!run) return XNRS_OK;
  if (!g) return XNRS_EINVAL;
  const size_t need = tl_workspace_bytes(c.B, c.n_rows, c.W, d_table != nullptr);
  if (need && (!c.ws || c.ws_bytes < need)) return XNRS_EWORKSPACE;
  const int64_t tiles = (c.B + TK_TILE - 1) / TK_TILE, chunks = (c.n_rows + TK_TILE - 1) / TK_TILE;
  if ((c.n_rows * (int64_t)c.W + 255) / 256 > 0x7fffffffLL || (c.B * (int64_t)c.W + 255) / 256 > 0x7fffffffLL) return XNRS_EINVAL;
  LossArgs a = tl_args(c);
  a.g = g;
  Carver carve;
  if (d_up) {
    const int64_t slices = tl_split(tiles, chunks);
    float* part = at<float>(c.ws, carve.take((size_t)slices * c.B * c.W * F32));
    a.chunks_per_slice = chunks > 0 ? (chunks + slices - 1) / slices : 1;
    a.out = part;
    hipLaunchKernelGGL(loss_bwd_kernel<false>, dim3((unsigned)tiles, (unsigned)slices), dim3(256), 0, stream, a);
    XNRS_TRY(hipGetLastError());
    hipLaunchKernelGGL(loss_reduce_kernel, dim3((unsigned)((c.B * c.W + 255) / 256)), dim3(256), 0, stream, part, (int)slices, c.B,
                       c.W, d_up, a, 1);
    XNRS_TRY(hipGetLastError());
  } else {
    carve.take((size_t)tl_split(tiles, chunks) * c.B * c.W * F32);
  }
  if (d_table && c.n_rows > 0) {
    const int64_t groups = tl_split(chunks, tiles);
    float* part = groups > 1 ? at<float>(c.ws, carve.take((size_t)groups * c.n_rows * c.W * F32)) : d_table;
    a.tiles_per_group = (tiles + groups - 1) / groups;
    a.out = part;
    hipLaunchKernelGGL(loss_bwd_kernel<true>, dim3((unsigned)chunks, (unsigned)groups), dim3(256), 0, stream, a);
    XNRS_TRY(hipGetLastError());
    if (groups > 1) {
      hipLaunchKernelGGL(loss_reduce_kernel, dim3((unsigned)((c.n_rows * c.W + 255) / 256)), dim3(256), 0, stream, part, (int)groups,
                         c.n_rows, c.W, d_table, a, 0);
      XNRS_TRY(hipGetLastError());
    }
  }
  return XNRS_OK;
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
  return tk_dot({table, n_rows, E, B, excl_off, excl_rows, pad_row, k, rows, scores, ws, ws_bytes, 0, false}, u, (hipStream_t)stream);
}

int32_t xnrs_topk_bilinear(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const float* w,
                           const float* bias, const int64_t* excl_off, const int32_t* excl_rows, int32_t pad_row, int32_t k,
                           int32_t* rows, float* scores, void* ws, size_t ws_bytes, void* stream) {
  return tk_bilinear({table, n_rows, E, B, excl_off, excl_rows, pad_row, k, rows, scores, ws, ws_bytes, E, false}, u, w, bias,
                     (hipStream_t)stream);
}

int32_t xnrs_topk_mlp(const float* P, int64_t n_rows, int32_t E, int32_t H, const float* u, int64_t B, const float* w1,
                      const float* b1, const float* w2, const float* b2, const int64_t* excl_off, const int32_t* excl_rows,
                      int32_t pad_row, int32_t k, int32_t* rows, float* scores, void* ws, size_t ws_bytes, void* stream) {
  return tk_mlp({P, n_rows, H, B, excl_off, excl_rows, pad_row, k, rows, scores, ws, ws_bytes, H, false}, E, u, w1, b1, w2, b2,
                (hipStream_t)stream);
}

size_t xnrs_topk_deep_workspace_bytes(int64_t B, int64_t n_rows, int32_t proj_width, int32_t k) {
  return tk_workspace_bytes(B, n_rows, proj_width, k, XNRS_TOPK_DEEP_MAX_K);
}

int32_t xnrs_topk_deep(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const int64_t* excl_off,
                       const int32_t* excl_rows, int32_t pad_row, int32_t k, int32_t* rows, float* scores, void* ws,
                       size_t ws_bytes, void* stream) {
  return tk_dot({table, n_rows, E, B, excl_off, excl_rows, pad_row, k, rows, scores, ws, ws_bytes, 0, true}, u, (hipStream_t)stream);
}

int32_t xnrs_topk_deep_bilinear(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const float* w,
                                const float* bias, const int64_t* excl_off, const int32_t* excl_rows, int32_t pad_row, int32_t k,
                                int32_t* rows, float* scores, void* ws, size_t ws_bytes, void* stream) {
  return tk_bilinear({table, n_rows, E, B, excl_off, excl_rows, pad_row, k, rows, scores, ws, ws_bytes, E, true}, u, w, bias,
                     (hipStream_t)stream);
}

int32_t xnrs_topk_deep_mlp(const float* P, int64_t n_rows, int32_t E, int32_t H, const float* u, int64_t B, const float* w1,
                           const float* b1, const float* w2, const float* b2, const int64_t* excl_off, const int32_t* excl_rows,
                           int32_t pad_row, int32_t k, int32_t* rows, float* scores, void* ws, size_t ws_bytes, void* stream) {
  return tk_mlp({P, n_rows, H, B, excl_off, excl_rows, pad_row, k, rows, scores, ws, ws_bytes, H, true}, E, u, w1, b1, w2, b2,
                (hipStream_t)stream);
}

size_t xnrs_rank_workspace_bytes(int64_t B, int32_t proj_width) {
  if (B <= 0 || proj_width <= 0) return 0;
  return carve_total({(size_t)B * proj_width * F32});  // the projected user side [B, proj_width]
}

int32_t xnrs_rank(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const int64_t* tgt_off,
                  const int32_t* tgt_rows, const int64_t* excl_off, const int32_t* excl_rows, int32_t pad_row, int32_t* ranks,
                  float* scores, void* ws, size_t ws_bytes, void* stream) {
  return rk_dot({table, n_rows, E, B, tgt_off, excl_off, tgt_rows, excl_rows, pad_row, ranks, scores, ws, ws_bytes, 0}, u,
                (hipStream_t)stream);
}

int32_t xnrs_rank_bilinear(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const float* w,
                           const float* bias, const int64_t* tgt_off, const int32_t* tgt_rows, const int64_t* excl_off,
                           const int32_t* excl_rows, int32_t pad_row, int32_t* ranks, float* scores, void* ws, size_t ws_bytes,
                           void* stream) {
  return rk_bilinear({table, n_rows, E, B, tgt_off, excl_off, tgt_rows, excl_rows, pad_row, ranks, scores, ws, ws_bytes, E}, u, w,
                     bias, (hipStream_t)stream);
}

int32_t xnrs_rank_mlp(const float* P, int64_t n_rows, int32_t E, int32_t H, const float* u, int64_t B, const float* w1,
                      const float* b1, const float* w2, const float* b2, const int64_t* tgt_off, const int32_t* tgt_rows,
                      const int64_t* excl_off, const int32_t* excl_rows, int32_t pad_row, int32_t* ranks, float* scores,
                      void* ws, size_t ws_bytes, void* stream) {
  return rk_mlp({P, n_rows, H, B, tgt_off, excl_off, tgt_rows, excl_rows, pad_row, ranks, scores, ws, ws_bytes, H}, E, u, w1, b1,
                w2, b2, (hipStream_t)stream);
}

// ---- the row-window entry points: the argument lists of their parents with win_lo, win_hi behind excl_rows
int32_t xnrs_topk_deep_win(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const int64_t* excl_off,
                           const int32_t* excl_rows, const int32_t* win_lo, const int32_t* win_hi, int32_t pad_row, int32_t k,
                           int32_t* rows, float* scores, void* ws, size_t ws_bytes, void* stream) {
  return tk_dot({table, n_rows, E, B, excl_off, excl_rows, pad_row, k, rows, scores, ws, ws_bytes, 0, true, win_lo, win_hi}, u,
                (hipStream_t)stream);
}

int32_t xnrs_topk_deep_bilinear_win(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const float* w,
                                    const float* bias, const int64_t* excl_off, const int32_t* excl_rows, const int32_t* win_lo,
                                    const int32_t* win_hi, int32_t pad_row, int32_t k, int32_t* rows, float* scores, void* ws,
                                    size_t ws_bytes, void* stream) {
  return tk_bilinear({table, n_rows, E, B, excl_off, excl_rows, pad_row, k, rows, scores, ws, ws_bytes, E, true, win_lo, win_hi}, u,
                     w, bias, (hipStream_t)stream);
}

int32_t xnrs_topk_deep_mlp_win(const float* P, int64_t n_rows, int32_t E, int32_t H, const float* u, int64_t B, const float* w1,
                               const float* b1, const float* w2, const float* b2, const int64_t* excl_off,
                               const int32_t* excl_rows, const int32_t* win_lo, const int32_t* win_hi, int32_t pad_row, int32_t k,
                               int32_t* rows, float* scores, void* ws, size_t ws_bytes, void* stream) {
  return tk_mlp({P, n_rows, H, B, excl_off, excl_rows, pad_row, k, rows, scores, ws, ws_bytes, H, true, win_lo, win_hi}, E, u, w1,
                b1, w2, b2, (hipStream_t)stream);
}

int32_t xnrs_rank_win(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const int64_t* tgt_off,
                      const int32_t* tgt_rows, const int64_t* excl_off, const int32_t* excl_rows, const int32_t* win_lo,
                      const int32_t* win_hi, int32_t pad_row, int32_t* ranks, float* scores, void* ws, size_t ws_bytes,
                      void* stream) {
  return rk_dot({table, n_rows, E, B, tgt_off, excl_off, tgt_rows, excl_rows, pad_row, ranks, scores, ws, ws_bytes, 0, win_lo, win_hi},
                u, (hipStream_t)stream);
}

int32_t xnrs_rank_bilinear_win(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const float* w,
                               const float* bias, const int64_t* tgt_off, const int32_t* tgt_rows, const int64_t* excl_off,
                               const int32_t* excl_rows, const int32_t* win_lo, const int32_t* win_hi, int32_t pad_row,
                               int32_t* ranks, float* scores, void* ws, size_t ws_bytes, void* stream) {
  return rk_bilinear({table, n_rows, E, B, tgt_off, excl_off, tgt_rows, excl_rows, pad_row, ranks, scores, ws, ws_bytes, E, win_lo,
                      win_hi}, u, w, bias, (hipStream_t)stream);
}

int32_t xnrs_rank_mlp_win(const float* P, int64_t n_rows, int32_t E, int32_t H, const float* u, int64_t B, const float* w1,
                          const float* b1, const float* w2, const float* b2, const int64_t* tgt_off, const int32_t* tgt_rows,
                          const int64_t* excl_off, const int32_t* excl_rows, const int32_t* win_lo, const int32_t* win_hi,
                          int32_t pad_row, int32_t* ranks, float* scores, void* ws, size_t ws_bytes, void* stream) {
  return rk_mlp({P, n_rows, H, B, tgt_off, excl_off, tgt_rows, excl_rows, pad_row, ranks, scores, ws, ws_bytes, H, win_lo, win_hi},
                E, u, w1, b1, w2, b2, (hipStream_t)stream);
}

// ---- the full-table softmax ranking loss
size_t xnrs_table_loss_workspace_bytes(int64_t B, int64_t n_rows, int32_t E, int32_t want_d_table) {
  return tl_workspace_bytes(B, n_rows, E, want_d_table);
}

int32_t xnrs_table_loss_fwd(const float* table, int64_t n_rows, int32_t E, const float* up, const float* bias, int64_t B,
                            const int64_t* tgt_off, const int32_t* tgt_rows, const int64_t* excl_off, const int32_t* excl_rows,
                            const int32_t* win_lo, const int32_t* win_hi, int32_t pad_row, float* scores, float* loss, float* lse,
                            void* ws, size_t ws_bytes, void* stream) {
  return tl_fwd({table, up, bias, n_rows, E, B, tgt_off, excl_off, tgt_rows, excl_rows, win_lo, win_hi, pad_row, scores, lse, ws,
                 ws_bytes}, loss, (hipStream_t)stream);
}

int32_t xnrs_table_loss_bwd(const float* table, int64_t n_rows, int32_t E, const float* up, const float* bias, int64_t B,
                            const int64_t* tgt_off, const int32_t* tgt_rows, const int64_t* excl_off, const int32_t* excl_rows,
                            const int32_t* win_lo, const int32_t* win_hi, int32_t pad_row, const float* scores, const float* lse,
                            const float* g, float* d_up, float* d_table, void* ws, size_t ws_bytes, void* stream) {
  return tl_bwd({table, up, bias, n_rows, E, B, tgt_off, excl_off, tgt_rows, excl_rows, win_lo, win_hi, pad_row,
                 const_cast<float*>(scores), const_cast<float*>(lse), ws, ws_bytes}, g, d_up, d_table, (hipStream_t)stream);
}

}  // extern "C"
