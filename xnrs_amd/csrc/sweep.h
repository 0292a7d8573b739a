// What every sweep over a whole pre-encoded table shares -- the top-k selection (topk.hip), the rank of given rows (rank.hip)
// and the full-table softmax ranking loss (table_loss.hip): the score tile, the row windows, the chunk's exclusion bitmap and
// eligibility mask on the device; the call description, its argument check and the user-side projection on the host.
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
#pragma once
#include "host.h"

namespace xnrs {

constexpr int TK_TILE = 128;             // users per workgroup = table rows per chunk
constexpr int TK_KT = 32;                // features per LDS stage
constexpr int TK_PITCH = TK_TILE + 1;    // feature-major LDS tiles: conflict-free transposing writes (4 * pitch = 4 mod 32)
constexpr int TK_CB = 32;                // candidate buffer entries per user
constexpr int TK_WGS = 512;              // workgroups that fill the chip: 256 CUs x 2 resident (79 872 B of LDS each, 160 KB per CU)
// the most slices of a call (a single user tile is the only case that wants more): the merge kernel folds a user's slice lists
// one after the other, which with 512 lists takes longer than the partial kernel; 256 still gives every CU a workgroup
constexpr int TK_MAX_SLICES = 256;

using f32x16 = __attribute__((ext_vector_type(16))) float;

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
// ... and of the queries of the rank and of the loss: tgt_rows[tgt_off[b] .. tgt_off[b + 1]) are the targets of user b
struct RankArgs : TkOperands {
  const int64_t* tgt_off;
  const int32_t* tgt_rows;
  int32_t* ranks;
  float* scores;
};

// Where a thread stands in the 128 x 128 score tile of its workgroup (256 threads): wave `wave` holds rows rw + [0, 64) x
// users uw + [0, 64), a lane the users uw + l32 and uw + 32 + l32 (user blocks 0 and 1) and, of each 32-row block, the rows
// 8 (j / 4) + 4 half + j % 4, j < 16.
struct TkThread {
  int tid, lane, wave, l32, half, rw, uw;
  __device__ __forceinline__ TkThread()
      : tid(threadIdx.x), lane(tid & 63), wave(tid >> 6), l32(lane & 31), half(lane >> 5), rw((wave >> 1) * 64), uw((wave & 1) * 64) {}
  __device__ __forceinline__ int ul(int ub) const { return uw + ub * 32 + l32; }              // the lane's user of block ub, in the tile
  __device__ __forceinline__ int64_t first(int64_t r0) const { return r0 + rw + half * 4; }  // the lane's first row of chunk r0
};
// the users of tile i are u0 + [0, nu) of the batch
__device__ __forceinline__ int tk_tile_users(int64_t B, int64_t u0) { return B - u0 < TK_TILE ? (int)(B - u0) : TK_TILE; }

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

// the window [lo, hi) as every sweep sees it: clamped to [0, a.n_rows], an empty one as [0, 0).  lo and hi are assigned and
// read more than once: plain int32_t variables only, no expressions (why a macro: profiles/sweep_split_resource_usage.md)
#define TK_CLAMP_WINDOW(a, lo, hi)                      \
  do {                                                  \
    lo = lo < 0 ? 0 : lo;                               \
    hi = hi > (a).n_rows ? (int32_t)(a).n_rows : hi;    \
    if (lo >= hi) lo = hi = 0;                          \
  } while (0)

// The chunks [c_lo, c_hi) of the sweep that workgroup (tile blockIdx.x, slice blockIdx.y) walks, and the lane's windows.
// Without windows: the fixed share chunks_per_slice of the whole table.  With windows: the tile's users reduce their windows
// to the chunk range of their union (integer min / max in LDS, rng[4]: found on the device, no host synchronisation), and
// the gridDim.y slices split THAT range evenly -- slice s takes [n s / S, n (s + 1) / S) of its n chunks, so that no slice is
// idle while another holds two chunks more; with n < S some slices are empty (they write fillers / an empty list).  All
// 256 threads call it (two workgroup barriers).  A user's result does not depend on the split: the slices are disjoint and
// cover every chunk that holds a row of a window of the tile.
__device__ __forceinline__ void tk_tile_range(const TkOperands& a, int64_t u0, int nu, int* rng, TkWin& w, int64_t& c_lo, int64_t& c_hi) {
  const TkThread t;
  if (!a.win_lo) {
    w.lo[0] = w.lo[1] = 0;
    w.hi[0] = w.hi[1] = (int32_t)a.n_rows;
    w.gaps = 0;
    const int64_t chunks = (a.n_rows + TK_TILE - 1) / TK_TILE;
    c_lo = (int64_t)blockIdx.y * a.chunks_per_slice;
    c_hi = c_lo + a.chunks_per_slice < chunks ? c_lo + a.chunks_per_slice : chunks;
    return;
  }
  if (t.tid == 0) {
    rng[0] = rng[3] = 0x7fffffff;  // the least lo / TK_TILE, the least hi
    rng[1] = rng[2] = 0;           // the greatest ceil(hi / TK_TILE), the greatest lo
  }
  __syncthreads();
#pragma unroll
  for (int ub = 0; ub < 2; ++ub) {
    const int ul = t.ul(ub);
    int32_t lo = 0, hi = 0;
    if (ul < nu) {
      lo = a.win_lo[u0 + ul];
      hi = a.win_hi[u0 + ul];
      TK_CLAMP_WINDOW(a, lo, hi);
    }
    w.lo[ub] = lo;
    w.hi[ub] = hi;
    if (t.wave < 2 && hi > lo) {  // (waves 0 and 1 hold every user of the tile once)
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

// The score tile, the ONE definition of every kernel that ranks: acc <- the scores, before the bias, of table rows
// r0 + [0, 128) (GATHER: rows gather[0, 128)) x users u0 + [0, 128).  acc[row block][user block]: element j of a lane is row
// 8 (j / 4) + 4 half + j % 4 of the wave's row block, user l32 of its user block.  A (row, user) score depends on nothing but
// that pair: not on the other rows and users of the tile, nor on where in the tile the pair sits.  All 256 threads call it;
// it begins and ends between workgroup barriers of its own, and on return At / Bt / w2s may still be read by other waves.
template <bool MLP, bool GATHER>
__device__ __forceinline__ void tk_score_tile(const TkOperands& a, int64_t r0, const int32_t* gather, int64_t u0, float* At, float* Bt,
                                              float* w2s, f32x16 (&acc)[2][2]) {
  const TkThread t;
  const int tid = t.tid, l32 = t.l32, half = t.half, rw = t.rw, uw = t.uw;  // the wave's 64 x 64 part of the score tile
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

// Exclusions of a counting sweep: a bitmap of chunk r0, users x rows, in LDS -- bit r % 32 of excl[(r / 32) * 128 + user]: row r
// of the chunk is excluded -- filled by walking each user's exclusion list and, with TARGETS, the user's own targets next to
// it (half a wave per user; ids are compared, never dereferenced, duplicates set a set bit again).  All 256 threads; the
// barriers of the score tile stand between these writes and their readers.  TARGETS == false: the caller has tested a.excl_off.
__device__ __forceinline__ void tk_mark(const int64_t* off, const int32_t* rows, int64_t r0, int64_t u0, int ul, int l32, uint32_t* excl) {
  const int64_t hi = off[u0 + ul + 1];
  for (int64_t e = off[u0 + ul] + l32; e < hi; e += 32) {
    const int64_t d = (int64_t)rows[e] - r0;
    if (d >= 0 && d < TK_TILE) atomicOr(&excl[(int)(d >> 5) * TK_TILE + ul], 1u << (d & 31));
  }
}
template <bool TARGETS>
__device__ __forceinline__ void tk_bitmap(const RankArgs& a, int64_t r0, int64_t u0, int nu, uint32_t* excl) {
  const int tid = threadIdx.x, l32 = tid & 31;
  __syncthreads();  // (the bitmap of the chunk before has been read)
  for (int i = tid; i < 4 * TK_TILE; i += 256) excl[i] = 0;
  __syncthreads();
  for (int ul = tid >> 5; ul < nu; ul += 8) {
    if (!TARGETS || a.excl_off) tk_mark(a.excl_off, a.excl_rows, r0, u0, ul, l32, excl);
    if (TARGETS) tk_mark(a.tgt_off, a.tgt_rows, r0, u0, ul, l32, excl);
  }
}

// which of the lane's 32 score elements of user block ub may count for user ul of the tile -- inside the window (and so the
// table), not the pad row, not in the bitmap (excl NULL: no list): bit rb * 16 + j, the order of TkWin::inside
__device__ __forceinline__ uint32_t tk_eligible(const TkOperands& a, const TkWin& win, const uint32_t* excl, int ub, int64_t r0,
                                                int rw, int half, int ul) {
  uint32_t ok = 0;
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const uint32_t word = excl ? excl[((rw >> 5) + rb) * TK_TILE + ul] : 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int bit = (j >> 2) * 8 + half * 4 + (j & 3);
      const int64_t row = r0 + rw + rb * 32 + bit;
      ok |= (uint32_t)(row != a.pad_row && !((word >> bit) & 1u)) << (rb * 16 + j);
    }
  }
  return ok & win.inside(ub, r0 + rw + half * 4);  // (inside the window: inside the table as well)
}

// ---------------------------------------------------------------------------------------------------------------- host
inline int64_t tk_chunks_per_slice(int64_t B, int64_t n_rows) {
  const int64_t tiles = (B + TK_TILE - 1) / TK_TILE, chunks = (n_rows + TK_TILE - 1) / TK_TILE;
  if (tiles <= 0 || chunks <= 0) return 1;
  int64_t want = (TK_WGS + tiles - 1) / tiles;
  if (want > TK_MAX_SLICES) want = TK_MAX_SLICES;
  if (want > chunks) want = chunks;
  return (chunks + want - 1) / want;
}

inline bool tk_vec_ok(const float* p, int W) { return W % 4 == 0 && reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// what the entry points of every sweep are given; each feature adds its own outputs
struct SweepCall {
  const float* table;  // (n_rows, W): the vectors of the inner-product forms, P of the MLP form
  int64_t n_rows, B;
  int32_t W, pad_row;
  const int64_t* excl_off;
  const int32_t *excl_rows, *win_lo, *win_hi;  // win_lo, win_hi: both (xnrs_*_win) or neither
  void* ws;
  size_t ws_bytes;
  int32_t proj_width;  // the width of the projected user side at the head of the workspace (0: none)
  SweepCall(const float* table, int64_t n_rows, int32_t W, int64_t B, const int64_t* excl_off, const int32_t* excl_rows,
            const int32_t* win_lo, const int32_t* win_hi, int32_t pad_row, void* ws, size_t ws_bytes, int32_t proj_width)
      : table(table), n_rows(n_rows), B(B), W(W), pad_row(pad_row), excl_off(excl_off), excl_rows(excl_rows), win_lo(win_lo),
        win_hi(win_hi), ws(ws), ws_bytes(ws_bytes), proj_width(proj_width) {}
};

// the operands of the call; up:(B, W) the user side as the kernel reads it (u, v = u W[0], q = u W1u^T + b1)
inline void sweep_operands(const SweepCall& c, const float* up, const float* w2, const float* bias, TkOperands& a) {
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
}

// the argument checks every entry point shares (a feature checks its own pointers and its workspace behind them);
// XNRS_OK with *run = false: nothing to do
inline int32_t sweep_check(const SweepCall& c, const float* u, bool* run) {
  *run = false;
  if (c.W <= 0 || c.B < 0 || c.n_rows < 0 || c.n_rows > 0x7fffffffLL) return XNRS_EINVAL;
  if (!c.win_lo != !c.win_hi) return XNRS_EINVAL;
  if (c.B == 0) return XNRS_OK;
  if (!u || (c.n_rows > 0 && !c.table) || (c.excl_off && !c.excl_rows)) return XNRS_EINVAL;
  *run = true;
  return XNRS_OK;
}

// The scorer of a call: how the user side u becomes what the kernel reads, and what is added to the product.
struct Scorer {
  enum Form { DOT, BILINEAR, MLP } form = DOT;
  int32_t E = 0;                                                            // MLP: the width of u (the table's W is H)
  const float *w = nullptr, *b1 = nullptr, *w2 = nullptr, *bias = nullptr;  // w: W[0] (bilinear) or W1 (MLP); bias: added last
};
inline Scorer sc_bilinear(const float* w, const float* bias) {
  Scorer s;
  s.form = Scorer::BILINEAR, s.w = w, s.bias = bias;
  return s;
}
inline Scorer sc_mlp(int32_t E, const float* w1, const float* b1, const float* w2, const float* b2) {
  Scorer s;
  s.form = Scorer::MLP, s.E = E, s.w = w1, s.b1 = b1, s.w2 = w2, s.bias = b2;
  return s;
}

// check the call, project the user side with sc_gemm into the head of the workspace, launch: the one body of the dot,
// bilinear and MLP forms of every sweep that takes a scorer
template <class Call>
int32_t sweep_scored(const Call& c, const Scorer& s, const float* u, int32_t (*check)(const Call&, const float*, bool*),
                     hipError_t (*launch)(const Call&, const float*, const float*, const float*, hipStream_t), hipStream_t stream) {
  if (s.form == Scorer::MLP && s.E <= 0) return XNRS_EINVAL;
  bool run;
  XNRS_TRY_RC(check(c, u, &run));
  if (!run) return XNRS_OK;
  const float* up = u;
  if (s.form == Scorer::BILINEAR) {
    if (!s.w) return XNRS_EINVAL;
    XNRS_TRY(sc_gemm(u, c.W, s.w, c.W, 1, nullptr, static_cast<float*>(c.ws), c.W, c.B, c.W, c.W, stream));  // v_b = W[0]^T u_b, as xnrs_score_csr_bilinear
    up = static_cast<float*>(c.ws);
  } else if (s.form == Scorer::MLP) {
    if (!s.w || !s.w2) return XNRS_EINVAL;
    XNRS_TRY(sc_gemm(u, s.E, s.w, 2 * (int64_t)s.E, 0, s.b1, static_cast<float*>(c.ws), c.W, c.B, c.W, s.E, stream));  // q_b = W1u u_b + b1, as xnrs_score_csr_mlp
    up = static_cast<float*>(c.ws);
  }
  XNRS_TRY(launch(c, up, s.w2, s.bias, stream));
  return XNRS_OK;
}

// the target pass of the rank (rank.hip): scores[e] <- the score of query e, ranks[e] (nullable) <- 0, or -1 without an answer
hipError_t rank_target_scores(const RankArgs& a, bool mlp, hipStream_t stream);

}  // namespace xnrs
