// The full-table softmax ranking loss (xnrs_table_loss_fwd / _bwd): the training side of the two sweeps (topk.hip, rank.hip).
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
// The score tile, the row windows, the chunk's bitmap (tk_bitmap<true>) and the eligibility mask (tk_eligible): sweep.h.
#include "sweep.h"

namespace xnrs {

namespace {

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
    tk_bitmap<true>(a, r0, u0, nu, excl);
    f32x16 acc[2][2];
    tk_score_tile<false, false>(a, r0, nullptr, u0, At, Bt, nullptr, acc);
    float m[2];
#pragma unroll
    for (int ub = 0; ub < 2; ++ub) {
      const int ul = uw + ub * 32 + l32;
      const uint32_t neg = tk_eligible(a, win, excl, ub, r0, rw, half, ul);
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
    int32_t lo = a.win_lo[b], hi = a.win_hi[b];
    TK_CLAMP_WINDOW(a, lo, hi);
    c0 = lo / TK_TILE;
    c1 = ((int64_t)hi + TK_TILE - 1) / TK_TILE;
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
      TK_CLAMP_WINDOW(a, lo, hi);
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
      tk_bitmap<true>(a, r0, u0, nu, excl);
      f32x16 acc[2][2];
      tk_score_tile<false, false>(a, r0, nullptr, u0, stage, stage + TK_KT * TK_PITCH, nullptr, acc);
      // ---- ds in the score registers, then through LDS: the contraction index of the second product leads
#pragma unroll
      for (int ub = 0; ub < 2; ++ub) {
        const int ul = uw + ub * 32 + l32;
        const uint32_t neg = tk_eligible(a, win, excl, ub, r0, rw, half, ul);
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

struct LossCall : SweepCall {
  const float *up, *bias;
  const int64_t* tgt_off;
  const int32_t* tgt_rows;
  float *scores, *lse;  // (the forward writes them, the backward reads them)
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
  XNRS_TRY_RC(sweep_check(c, c.up, run));
  if (*run && (!c.scores || !c.lse || !c.tgt_off || !c.tgt_rows || (c.B + TK_TILE - 1) / TK_TILE > 0x7fffffffLL)) return XNRS_EINVAL;
  return XNRS_OK;
}

LossArgs tl_args(const LossCall& c) {
  LossArgs a{};
  sweep_operands(c, c.up, nullptr, c.bias, a);
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
  XNRS_TRY(rank_target_scores(a, false, stream));  // (a.ranks is NULL: the scores alone)
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

// what both entry points are given
LossCall tl_call(const float* table, int64_t n_rows, int32_t E, const float* up, const float* bias, int64_t B, const int64_t* tgt_off,
                 const int32_t* tgt_rows, const int64_t* excl_off, const int32_t* excl_rows, const int32_t* win_lo,
                 const int32_t* win_hi, int32_t pad_row, const float* scores, const float* lse, void* ws, size_t ws_bytes) {
  const SweepCall sc(table, n_rows, E, B, excl_off, excl_rows, win_lo, win_hi, pad_row, ws, ws_bytes, 0);
  return {sc, up, bias, tgt_off, tgt_rows, const_cast<float*>(scores), const_cast<float*>(lse)};
}

}  // namespace

}  // namespace xnrs

using namespace xnrs;

extern "C" {

size_t xnrs_table_loss_workspace_bytes(int64_t B, int64_t n_rows, int32_t E, int32_t want_d_table) {
  return tl_workspace_bytes(B, n_rows, E, want_d_table);
}

int32_t xnrs_table_loss_fwd(const float* table, int64_t n_rows, int32_t E, const float* up, const float* bias, int64_t B,
                            const int64_t* tgt_off, const int32_t* tgt_rows, const int64_t* excl_off, const int32_t* excl_rows,
                            const int32_t* win_lo, const int32_t* win_hi, int32_t pad_row, float* scores, float* loss, float* lse,
                            void* ws, size_t ws_bytes, void* stream) {
  return tl_fwd(tl_call(table, n_rows, E, up, bias, B, tgt_off, tgt_rows, excl_off, excl_rows, win_lo, win_hi, pad_row, scores, lse, ws,
                        ws_bytes), loss, (hipStream_t)stream);
}

int32_t xnrs_table_loss_bwd(const float* table, int64_t n_rows, int32_t E, const float* up, const float* bias, int64_t B,
                            const int64_t* tgt_off, const int32_t* tgt_rows, const int64_t* excl_off, const int32_t* excl_rows,
                            const int32_t* win_lo, const int32_t* win_hi, int32_t pad_row, const float* scores, const float* lse,
                            const float* g, float* d_up, float* d_table, void* ws, size_t ws_bytes, void* stream) {
  return tl_bwd(tl_call(table, n_rows, E, up, bias, B, tgt_off, tgt_rows, excl_off, excl_rows, win_lo, win_hi, pad_row, scores, lse, ws,
                        ws_bytes), g, d_up, d_table, (hipStream_t)stream);
}

}  // extern "C"
