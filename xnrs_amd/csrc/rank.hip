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
//            are compared, duplicates set a set bit again (tk_bitmap, sweep.h).
// The score tile, the row windows of xnrs_rank*_win and the eligibility mask: sweep.h.
#include "sweep.h"

namespace xnrs {

namespace {

constexpr int RK_SLOTS = 4;

template <bool MLP>
__global__ __launch_bounds__(256, MLP ? 1 : 2) void rank_target_kernel(RankArgs a) {
  __shared__ float At[TK_KT * TK_PITCH], Bt[TK_KT * TK_PITCH];
  __shared__ float w2s[TK_KT];
  __shared__ int64_t t_lo[TK_TILE], t_n[TK_TILE];
  __shared__ int32_t gather[TK_TILE];
  const TkThread t;
  const int64_t u0 = (int64_t)blockIdx.x * TK_TILE;
  const int nu = tk_tile_users(a.B, u0);
  const int tid = t.tid;
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
        const int32_t row = a.tgt_rows[t_lo[tid] + j];
        if (row >= 0 && row < a.n_rows && row != a.pad_row) g = row;
      }
      gather[tid] = g;
    }
    __syncthreads();
    f32x16 acc[2][2];
    tk_score_tile<MLP, true>(a, 0, gather, u0, At, Bt, w2s, acc);
    // the diagonal: row i of the tile is the target of user i.  It lies in the waves whose row half is their user half, in
    // block [b][b], in the lanes whose half holds row l32 of the block: 8 (j / 4) + 4 half + j % 4 == l32
    if (t.rw == t.uw && ((t.l32 >> 2) & 1) == t.half) {
      const int el = (t.l32 >> 3) * 4 + (t.l32 & 3);
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int ul = t.ul(b);
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
  __shared__ uint32_t excl[4 * TK_TILE];        // the chunk's exclusion bitmap (tk_bitmap)
  __shared__ int32_t slot[RK_SLOTS * TK_TILE];  // slot[i * 128 + user]: the slice's count for target i of the user
  __shared__ int rng[4];
  const TkThread t;
  const int64_t u0 = (int64_t)blockIdx.x * TK_TILE;
  const int nu = tk_tile_users(a.B, u0);
  for (int i = t.tid; i < RK_SLOTS * TK_TILE; i += 256) slot[i] = 0;
  int64_t e_lo[2], e_hi[2];  // the targets of the lane's two users
#pragma unroll
  for (int ub = 0; ub < 2; ++ub) {
    const int ul = t.ul(ub);
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
    if (a.excl_off) tk_bitmap<false>(a, r0, u0, nu, excl);
    f32x16 acc[2][2];
    tk_score_tile<MLP, false>(a, r0, nullptr, u0, At, Bt, w2s, acc);
    // ---- what may be counted: the bias added as the selection adds it, everything else NaN
#pragma unroll
    for (int ub = 0; ub < 2; ++ub) {
      const uint32_t ok = tk_eligible(a, win, a.excl_off ? excl : nullptr, ub, r0, t.rw, t.half, t.ul(ub));
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[rb][ub][j] = ((ok >> (rb * 16 + j)) & 1u) ? acc[rb][ub][j] + bias : nan;
    }
    // ---- count
#pragma unroll
    for (int ub = 0; ub < 2; ++ub) {
      const int ul = t.ul(ub);
      for (int64_t e = e_lo[ub]; e < e_hi[ub]; ++e) {
        const float st = a.scores[e];
        if (!(st == st)) continue;  // rank -1: no answer
        // the lane's row of element (rb, j) is below the target's row when 32 rb + 8 (j / 4) + j % 4 < d
        int64_t d64 = (int64_t)a.tgt_rows[e] - t.first(r0);
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
  for (int i = t.tid; i < RK_SLOTS * TK_TILE; i += 256)
    if (slot[i]) atomicAdd(&a.ranks[a.tgt_off[u0 + (i & (TK_TILE - 1))] + (i >> 7)], slot[i]);  // (counted: the user and the target exist)
}

struct RankCall : SweepCall {
  const int64_t* tgt_off;
  const int32_t* tgt_rows;
  int32_t* ranks;
  float* scores;
};

int32_t rk_check(const RankCall& c, const float* u, bool* run) {
  XNRS_TRY_RC(sweep_check(c, u, run));
  if (*run && (!c.ranks || !c.scores || !c.tgt_off || !c.tgt_rows)) return XNRS_EINVAL;
  const size_t need = xnrs_rank_workspace_bytes(c.B, c.proj_width);
  if (*run && need && (!c.ws || c.ws_bytes < need)) return XNRS_EWORKSPACE;
  return XNRS_OK;
}

// the two launches; up, w2, bias as sweep_operands takes them
hipError_t rk_launch(const RankCall& c, const float* up, const float* w2, const float* bias, hipStream_t stream) {
  RankArgs a{};
  sweep_operands(c, up, w2, bias, a);
  a.tgt_off = c.tgt_off;
  a.tgt_rows = c.tgt_rows;
  a.ranks = c.ranks;
  a.scores = c.scores;
  const int64_t tiles = (c.B + TK_TILE - 1) / TK_TILE;
  if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  hipError_t e = rank_target_scores(a, w2 != nullptr, stream);
  if (e != hipSuccess || c.n_rows == 0) return e;  // (an empty table: every query has its -1 / NaN)
  const dim3 grid((unsigned)tiles, (unsigned)xnrs_topk_slices(c.B, c.n_rows));
  if (w2) hipLaunchKernelGGL(rank_sweep_kernel<true>, grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(rank_sweep_kernel<false>, grid, dim3(256), 0, stream, a);
  return hipGetLastError();
}

// the one body of the six entry points: W the table's width (E, or H of the MLP form); win_lo, win_hi NULL without windows
int32_t rk_run(const Scorer& s, const float* table, int64_t n_rows, int32_t W, const float* u, int64_t B, const int64_t* tgt_off,
               const int32_t* tgt_rows, const int64_t* excl_off, const int32_t* excl_rows, const int32_t* win_lo, const int32_t* win_hi,
               int32_t pad_row, int32_t* ranks, float* scores, void* ws, size_t ws_bytes, void* stream) {
  const SweepCall sc(table, n_rows, W, B, excl_off, excl_rows, win_lo, win_hi, pad_row, ws, ws_bytes, s.form == Scorer::DOT ? 0 : W);
  const RankCall c{sc, tgt_off, tgt_rows, ranks, scores};
  return sweep_scored<RankCall>(c, s, u, rk_check, rk_launch, (hipStream_t)stream);
}

}  // namespace

hipError_t rank_target_scores(const RankArgs& a, bool mlp, hipStream_t stream) {  // (the caller has checked that the tiles fit a grid)
  const dim3 grid((unsigned)((a.B + TK_TILE - 1) / TK_TILE));
  if (mlp) hipLaunchKernelGGL(rank_target_kernel<true>, grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(rank_target_kernel<false>, grid, dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace xnrs

using namespace xnrs;

extern "C" {

size_t xnrs_rank_workspace_bytes(int64_t B, int32_t proj_width) {
  if (B <= 0 || proj_width <= 0) return 0;
  return carve_total({(size_t)B * proj_width * F32});  // the projected user side [B, proj_width]
}

// ---- the row-window entry points: the argument lists of their parents with win_lo, win_hi behind excl_rows
int32_t xnrs_rank_win(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const int64_t* tgt_off,
                      const int32_t* tgt_rows, const int64_t* excl_off, const int32_t* excl_rows, const int32_t* win_lo,
                      const int32_t* win_hi, int32_t pad_row, int32_t* ranks, float* scores, void* ws, size_t ws_bytes,
                      void* stream) {
  return rk_run({}, table, n_rows, E, u, B, tgt_off, tgt_rows, excl_off, excl_rows, win_lo, win_hi, pad_row, ranks, scores, ws, ws_bytes,
                stream);
}

int32_t xnrs_rank_bilinear_win(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const float* w,
                               const float* bias, const int64_t* tgt_off, const int32_t* tgt_rows, const int64_t* excl_off,
                               const int32_t* excl_rows, const int32_t* win_lo, const int32_t* win_hi, int32_t pad_row,
                               int32_t* ranks, float* scores, void* ws, size_t ws_bytes, void* stream) {
  return rk_run(sc_bilinear(w, bias), table, n_rows, E, u, B, tgt_off, tgt_rows, excl_off, excl_rows, win_lo, win_hi, pad_row, ranks,
                scores, ws, ws_bytes, stream);
}

int32_t xnrs_rank_mlp_win(const float* P, int64_t n_rows, int32_t E, int32_t H, const float* u, int64_t B, const float* w1,
                          const float* b1, const float* w2, const float* b2, const int64_t* tgt_off, const int32_t* tgt_rows,
                          const int64_t* excl_off, const int32_t* excl_rows, const int32_t* win_lo, const int32_t* win_hi,
                          int32_t pad_row, int32_t* ranks, float* scores, void* ws, size_t ws_bytes, void* stream) {
  return rk_run(sc_mlp(E, w1, b1, w2, b2), P, n_rows, H, u, B, tgt_off, tgt_rows, excl_off, excl_rows, win_lo, win_hi, pad_row, ranks,
                scores, ws, ws_bytes, stream);
}

// ---- xnrs_rank*: their _win twins without windows
int32_t xnrs_rank(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const int64_t* tgt_off,
                  const int32_t* tgt_rows, const int64_t* excl_off, const int32_t* excl_rows, int32_t pad_row, int32_t* ranks,
                  float* scores, void* ws, size_t ws_bytes, void* stream) {
  return xnrs_rank_win(table, n_rows, E, u, B, tgt_off, tgt_rows, excl_off, excl_rows, nullptr, nullptr, pad_row, ranks, scores, ws,
                       ws_bytes, stream);
}

int32_t xnrs_rank_bilinear(const float* table, int64_t n_rows, int32_t E, const float* u, int64_t B, const float* w,
                           const float* bias, const int64_t* tgt_off, const int32_t* tgt_rows, const int64_t* excl_off,
                           const int32_t* excl_rows, int32_t pad_row, int32_t* ranks, float* scores, void* ws, size_t ws_bytes,
                           void* stream) {
  return xnrs_rank_bilinear_win(table, n_rows, E, u, B, w, bias, tgt_off, tgt_rows, excl_off, excl_rows, nullptr, nullptr, pad_row,
                                ranks, scores, ws, ws_bytes, stream);
}

int32_t xnrs_rank_mlp(const float* P, int64_t n_rows, int32_t E, int32_t H, const float* u, int64_t B, const float* w1,
                      const float* b1, const float* w2, const float* b2, const int64_t* tgt_off, const int32_t* tgt_rows,
                      const int64_t* excl_off, const int32_t* excl_rows, int32_t pad_row, int32_t* ranks, float* scores,
                      void* ws, size_t ws_bytes, void* stream) {
  return xnrs_rank_mlp_win(P, n_rows, E, H, u, B, w1, b1, w2, b2, tgt_off, tgt_rows, excl_off, excl_rows, nullptr, nullptr, pad_row,
                           ranks, scores, ws, ws_bytes, stream);
}

}  // extern "C"
