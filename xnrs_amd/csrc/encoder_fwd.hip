// Forward orchestration of the sequence encoders: the padded pipeline (seq_encode), the host-compacted and the
// device-compacted padding-free pipelines, the folded out-projection they share, and their extern "C" entry points.
// No device allocation and no sync: everything is enqueued on the caller's stream into the caller's workspace
// (hipGraph-capturable).
//
// Sequence-encoder pipeline (TextEncoder news_encoding.py:34-60 / UserEncoder user_encoding.py:50-81),
// per chunk of sequences:
//   [att]   QKV = x.[Wq|Wk|Wv]^T + b   (one 3-segment MFMA GEMM, optional id-gather on the rows)
//           O   = softmax(rowmask(QK^T/sqrt(dk))) V          (mha_core, per sequence/head/q-tile)
//           Y   = O.Wo^T + bo                                  (MFMA GEMM)
//   [pool]  T   = tanh(Y.W1^T + b1)                            (MFMA GEMM, tanh epilogue)
//           p   = sum_i a_i Y_i,  a = exp(T.w2+b2)*m / (sum+1e-8)   (additive_pool)  | masked mean
//   [head]  y   = W4 relu(W3 p + b3) + b4                      (two MFMA GEMMs over all sequences)
// Short sequences (L <= 32, D <= 320: BASELINE configs[1]) take [att] + [pool] as ONE launch (news_fused.hip).
//
// The three pipelines must stay bit for bit equal (tested).  Every stage they share is therefore described ONCE, by the
// builders below (fc1_pair, qkv_projection, mha_core_args, fc1_product, additive_pool_args, pooled_tail); a pipeline sets
// only what differs: where its rows come from, where the row count lives, its output block.
#include <vector>

#include "host.h"

using namespace xnrs;

namespace xnrs {

// workspace carve for one chunk
Plan make_plan(int64_t n_seq, int L, int D, int A, int E, bool att, bool additive, bool head, bool pooled, int64_t chunk,
               bool train, int n_heads, bool widen) {
  Plan p{};
  if (train) chunk = n_seq > 0 ? n_seq : 1;  // the saved activations of the whole batch live in one carve
  if (chunk <= 0) chunk = 65536 / L;  // <= 64k token rows per pass: 512 full 128-row GEMM tiles (whole rounds of workgroups)
  if (chunk > n_seq) chunk = n_seq;
  if (chunk < 1) chunk = 1;
  p.chunk = chunk;
  const size_t rows = (size_t)chunk * L;
  Carver c;
  p.off_qkv = c.take_if(att, rows * 3 * (size_t)D * F32);
  p.off_o = c.take_if(att, rows * (size_t)D * F32);
  p.off_y = c.take_if(att && pooled, rows * (size_t)D * F32);  // att output when a pooler follows
  p.off_t = c.take_if(pooled && additive, rows * (size_t)A * F32);
  // pooled vectors / head hidden of ALL sequences: the head runs once after the chunk loop (two GEMMs over
  // n_seq rows instead of 2 x n_chunks launches of ~20 workgroups each)
  p.off_p = c.take_if(pooled && head, (size_t)n_seq * D * F32);
  p.off_h = c.take_if(pooled && head, (size_t)n_seq * E * F32);
  p.off_stats = c.take_if(train && att, (size_t)chunk * n_heads * L * 2 * F32);
  p.off_a = c.take_if(train && additive, rows * F32);
  // always reserved (15 MB at D = 768), so the plan does not depend on the GEMM mode of the moment
  size_t pl = 0;
  if (att) pl += 4 * align_up(split_planes_bytes(D, D));
  if (pooled && additive) pl += align_up(split_planes_bytes(A, D));
  p.off_planes = c.take(pl);
  // fused short-sequence path (news_fused.hip): reserved whenever the shape is eligible, whatever the knobs say
  // (a size query does not know the head count: it reserves the bound over all of them)
  NewsFusedPlan nf{};
  size_t nfb = 0;
  if (att && additive && !train) {
    if (n_heads <= 0) nfb = news_fused_img_bound_bytes(L, D, A);
    else if (news_fused_plan(L, D, n_heads, A, &nf)) nfb = nf.img_bytes;
  }
  p.off_nf = c.take_if(nfb != 0, nfb);
  p.off_nfo = c.take_if(nfb != 0, news_fused_scratch_bytes(L, D));  // its O rows while the out-projection is folded away
  // live row tiles of the dense passes (launch_live_tiles; a few KB): reserved for every pooled inference plan with an
  // attention tower, whatever the knobs and the batch size say
  const bool lt = att && pooled && !train;
  const size_t passes = (size_t)(((n_seq > 0 ? n_seq : 1) + chunk - 1) / chunk);
  p.off_lt_alive = c.take_if(lt, (size_t)(n_seq > 0 ? n_seq : 1));
  p.off_lt_n = c.take_if(lt, passes * sizeof(int64_t));
  p.off_lt_tiles = c.take_if(lt, passes * (size_t)live_tiles_cap(chunk, L, LIVE_TILE_BM) * sizeof(int32_t));
  // ... and their live rows (launch_dense_row_lists: 8 bytes per token row of the call, 11 MB at the benchmark's history call),
  // in the pass's row space and in the gathered table's; {live rows, -, -} per pass
  const bool lr = lt && L <= 64;
  p.off_lr_loc = c.take_if(lr, passes * rows * sizeof(int32_t));
  p.off_lr_src = c.take_if(lr, passes * rows * sizeof(int32_t));
  p.off_lr_cnt = c.take_if(lr, passes * 3 * sizeof(int64_t));
  // folded out-projection ("fold" below): reserved whenever the shape is eligible, whatever the knob says
  // (training keeps W', b', the pooled O rows and the weight sums for the backward)
  p.fold = carve_fold(c, att && additive, n_seq, D, A);
  // bf16 table: one pass of widened rows and mask rows, whatever route the call takes (behind every other region: the
  // offsets of an fp32 call's carve are those of the plan without it)
  p.off_x32 = c.take_if(widen, rows * (size_t)D * F32);
  p.off_m32 = c.take_if(widen, rows * F32);
  p.total = c.total();
  return p;
}

bool device_counts_ok(const float* x, int D, int A, const xnrs_mha_params* att, const xnrs_additive_params* pool) {
  if (!knobs().gemm_buf || gemm_mode() != 0 || D % 4 != 0 || D < 4 || (A > 0 && A % 4 != 0)) return false;
  // (w1_folded: the fc1 weight such a product reads instead of w1 when the call folds -- fc1_pair.  Asked about whether or not
  // THIS call folds: a pair that is given but unused and sits off a 16-byte boundary costs the route, never a result -- the
  // predicate stays a function of the operands alone, as its callers in both directions and the Python mirror have it)
  if (!aligned16(x) || (pool && !(aligned16(pool->w1) && aligned16(pool->w1_folded)))) return false;
  if (att && !(aligned16(att->wq) && aligned16(att->wk) && aligned16(att->wv) && aligned16(att->wo))) return false;
  return (int64_t)D * D * 4 <= (1ll << 30) && (int64_t)A * D * 4 <= (1ll << 30);
}

}  // namespace xnrs

namespace {

constexpr int64_t LINEAR_BF16_WIDEN_ROWS = 1024;  // rows per pass of xnrs_linear_fwd_bf16's widening route

// ---- "fold": the out-projection behind the pooling (inference).
// The pooler never needs the attention OUTPUT rows Y_i = Wo O_i + bo one by one (layers.py:154 -> layers.py:60-65):
//   fc1(Y_i)           = W1 (Wo O_i + bo) + b1 = (W1 Wo) O_i + (W1 bo + b1)            -> scores straight from the O rows
//   sum_i a_i Y_i      = Wo (sum_i a_i O_i) + bo (sum_i a_i)                             -> ONE out-projection per sequence
// so the rows x D x D out-projection GEMM (12.4 of 57 ms of the benchmark step) becomes an n_seq x D x D one, plus an
// A x D x D product for the folded weight per call (0.3 GFLOP; the ABI keeps no state between calls).  Exact algebra for
// every input -- only the rounding order differs from the reference's (observed <= 2e-6 on the scores, bar 1e-4); the
// training forward keeps Y (the backward needs it).  XNRS_FOLD_OUT=0 keeps the per-token out-projection.
// The folded weight is rebuilt per call (the ABI keeps no state): a split-K product over 8 slices and a wave-per-row bias
// kernel, ~20 us per call at D = 768 -- three short launches.  One impression (1 250 + 250 token rows, three encoder calls)
// pays ~0.05 ms for that (a single unsliced product cost twice as much); from a few thousand token rows on the fold wins,
// +25 % at the benchmark batch.  The choice deliberately never depends on the batch size (only the short-title dispatch
// below does: fused kernel or pipeline by news count) -- a news item's vector must not change in the last bit with the batch
// it is encoded in (chunking, id gather, skip_empty and the padding-free path are all tested bitwise against the plain
// path).  Knob (fold_wanted): 0 never, anything else always.

// C[M][D] = X[M][D] . Wo[D][D]: a weight folded behind the out-projection (W1 -> W1.Wo, the head's W0 -> W0.Wo)
hipError_t fold_product(const float* X, int M, const float* wo, int D, float* C, float* slabs, hipStream_t stream) {
  GemmArgs g = gemm_kmajor_b(X, D, wo, D, C, D, M, D, D);
  if (D >= 64 * FOLD_SPLITS) {  // enough contraction to slice: 8 x the workgroups, fixed-order reduce (bitwise reproducible)
    g.slabs = slabs;
    g.nsplit = FOLD_SPLITS;
  }
  return launch_gemm_f32(g, stream);
}

// wf = W1 . Wo, bf = W1 . bo + b1.  Returns the fc1 bias to use (nullptr if there is none).
const float* fold_out_projection(const xnrs_mha_params* att, const xnrs_additive_params* pool, int D, int A, float* wf,
                                 float* bf, float* slabs, hipStream_t stream, hipError_t* err) {
  *err = fold_product(pool->w1, A, att->wo, D, wf, slabs, stream);
  if (*err != hipSuccess || !att->bo) return pool->b1;
  *err = launch_fold_bias(pool->w1, att->bo, pool->b1, bf, A, D, stream);  // bf = W1 . bo + b1
  return bf;
}

// The pooler's first layer as a call runs it: the module's own pair, or -- fold -- the caller's copy of the folded pair
// (xnrs_fold_weights: nothing to rebuild; training: the backward call is then given the same pair, the saved blob's copy
// stays unwritten), or the folded pair rebuilt into the workspace.
struct Fc1 {
  const float* w;
  const float* b;
};
int32_t fc1_pair(bool fold, const xnrs_mha_params* att, const xnrs_additive_params* pool, int D, void* ws, const FoldRegions& fr,
                 hipStream_t stream, Fc1* fc1) {
  *fc1 = Fc1{pool ? pool->w1 : nullptr, pool ? pool->b1 : nullptr};
  if (!fold) return XNRS_OK;
  if (pool->w1_folded) {
    if (att->bo && !pool->b1_folded) return XNRS_EINVAL;
    *fc1 = Fc1{pool->w1_folded, att->bo ? pool->b1_folded : pool->b1};
    return XNRS_OK;
  }
  hipError_t fe = hipSuccess;
  fc1->w = at(ws, fr.fw);
  fc1->b = fold_out_projection(att, pool, D, pool->hidden, at(ws, fr.fw), at(ws, fr.fb), at(ws, fr.fsl), stream, &fe);
  return hip_rc(fe);
}

// the fused row dots ride on the raw-buffer-load forward kernel: 16-byte aligned operands
// (w1 and the caller's w1_folded both, whichever the call will multiply by: see device_counts_ok)
bool fc1_rowdot_ok(const float* x, bool att, const xnrs_additive_params* pool, int D) {
  // (rows of any count / any gather: beyond the 1-GB descriptor window or with row ids the launcher takes the
  // pointer-gather variant of the same kernel)
  return knobs().fc1_rowdot && knobs().gemm_buf && gemm_mode() == 0 && pool && pool->w2 && D % 4 == 0 && D >= 4 &&
         aligned16(pool->w1) && aligned16(pool->w1_folded) && (att || aligned16(x)) && (int64_t)pool->hidden * D * 4 <= (1ll << 30);
}
inline int n_epart(int A) { return (A + 31) / 32; }  // partial fc2 dots per row: one per 32 hidden columns

// ---- the stages every pipeline shares
// the padding-free pipelines' attention runs on the LDS-staged kernel with compact queries
int32_t compact_attention_rc(const xnrs_mha_params* att, int S, int D) {
  if (att->n_heads <= 0 || D % att->n_heads != 0) return XNRS_EHEADS;
  if (S > 64 || D / att->n_heads > 64 || (D / att->n_heads) % 4 != 0 || D % 4 != 0) return XNRS_EUNSUPPORTED;
  return XNRS_OK;
}

// [Q|]K|V = x . [Wq|]Wk|Wv^T + b as ONE multi-segment product into the row-major image C of pitch ldc (first = 0: Q|K|V,
// 1: K|V only).  planes (nullable): the pre-split weights {q, k, v} of the bf16-split modes.
GemmArgs qkv_projection(const float* x, RowIds rows, const xnrs_mha_params* att, int first, float* C, int64_t ldc, int64_t M,
                        int D, const unsigned short* const* planes = nullptr) {
  const float* W[3] = {att->wq, att->wk, att->wv};
  const float* b[3] = {att->bq, att->bk, att->bv};
  GemmArgs g = gemm_base(x, D, nullptr, D, C, ldc, M, D, D);
  g.gather_ids = rows.ids;
  g.gather_S = rows.S;
  for (int s = first; s < 3; ++s) {
    g.W[s - first] = W[s];
    g.bias[s - first] = b[s];
    g.Wp[s - first] = planes ? planes[s] : nullptr;
  }
  g.ldp = split_plane_ld(D);
  g.nseg = 3 - first;
  return g;
}

// Attention over the K | V columns of a row-major image (k = its K columns, pitch ld; V follows D columns on), one S-row
// block per sequence.  The caller sets the query source (q; compact queries: q_off / ldq / kv_block), the mask, the
// dropout seeds, stats and skip_dead.
// Q/K/V stay a row-major image.  A head-major image (every (sequence, head) block one contiguous S x d_k run) was
// measured: attention -4 %, but the projection's scattered 64-B stores cost it +2 % -- a net loss at the shipped shape, so
// it was dropped.
MhaCoreArgs mha_core_args(const float* k, int64_t ld, const xnrs_mha_params* att, float* out, int64_t n_seq, int S, int D) {
  MhaCoreArgs ma{};
  ma.k = k;
  ma.v = k + D;
  ma.ld = ld;
  ma.seq_stride = (int64_t)S * ld;
  ma.head_stride = D / att->n_heads;
  ma.out = out;
  ma.ldo = D;
  ma.n_seq = n_seq;
  ma.S = S;
  ma.n_heads = att->n_heads;
  ma.d_k = D / att->n_heads;
  ma.scaled = att->scaled;
  return ma;
}

// T = tanh(rows . W1^T + b1) over M rows; rowdot: the fc2 dot per 32 hidden columns straight from the epilogue instead
// (GemmArgs::rowdot_out; tanh(fc1 x) is never stored, the T region then holds n_epart(A) partial dots per row)
GemmArgs fc1_product(const float* seq, RowIds rows, Fc1 fc1, float* t, int64_t M, int D, int A, bool rowdot,
                     const xnrs_additive_params* pool, const unsigned short* planes = nullptr) {
  GemmArgs g = gemm_linear(seq, rows, D, fc1.w, fc1.b, t, A, M, A, D, XNRS_ACT_TANH, planes);
  if (rowdot) {
    g.rowdot_w = pool->w2;
    g.rowdot_out = t;
    g.ldrd = n_epart(A);
  }
  return g;
}

// the additive pooler over what fc1_product left in t; the caller sets the row layout (mask / gathers, or row_off /
// row_ids / poison for compact rows) and the outputs
AdditivePoolArgs additive_pool_args(const float* t, bool rowdot, const xnrs_additive_params* pool, const float* x, int64_t n_seq,
                                    int N, int D, int A) {
  AdditivePoolArgs pa{};
  pa.t = rowdot ? nullptr : t;
  pa.epart = rowdot ? t : nullptr;
  pa.n_epart = n_epart(A);
  pa.w2 = pool->w2;
  pa.b2 = pool->b2;
  pa.x = x;
  pa.ldx = D;
  pa.n_seq = n_seq;
  pa.N = N;
  pa.D = D;
  pa.A = A;
  return pa;
}

// dst[n] = Wo po[n] + bo s[n]: the out-projection behind the pooling.  fp32 GEMM mode: the bias term rides in the GEMM's
// epilogue (fmaf(s, bo, acc): the same bits as the separate pass, one launch less); split modes keep the separate pass.
hipError_t pooled_out_projection(const float* po, const float* s, const xnrs_mha_params* att, float* dst, int64_t n, int D,
                                 const unsigned short* planes, hipStream_t stream) {
  GemmArgs g = gemm_linear(po, {}, D, att->wo, nullptr, dst, D, n, D, D, XNRS_ACT_NONE, planes);
  const bool in_epilogue = att->bo && gemm_mode() == 0;
  if (in_epilogue) {
    g.rowscale = s;
    g.rowscale_vec = att->bo;
  }
  hipError_t e = launch_gemm_f32(g, stream);
  if (e != hipSuccess || !att->bo || in_epilogue) return e;
  return launch_add_rowscaled_bias(dst, D, s, att->bo, n, D, stream);
}

// The tail of a pooled encoder call: [out-projection behind the pooling] -> [head].
//   fold && head && head->w0_folded (inference, fp32 GEMM mode): the out-projection is folded INTO the head's first layer,
//     W0 (Wo po + bo s) + b0 = (W0 Wo) po + (W0 bo) s + b0 -- the caller's cached pair (xnrs_fold_head_weights) -- and the
//     n x D x D product disappears (0.31 of the 44.4 ms benchmark step, 13 of the 299 us of configs[1]); the rank-1 term
//     rides in the GEMM's epilogue like bo s did.  Exact algebra, another rounding order (~1e-6).
//   otherwise: pooled = Wo po + bo s, then the head's two layers as written (news_encoding.py:27-31).
int32_t pooled_tail(bool fold, const float* pob, const float* asum, const xnrs_mha_params* att, const xnrs_head_params* head,
                    float* pb, float* hb, float* y, int64_t n, int D, int E, const unsigned short* wo_planes, bool train,
                    hipStream_t stream) {
  const bool fold_head = fold && head && !train && head->w0_folded && gemm_mode() == 0 && (!att->bo || head->b0_rowvec);
  if (fold && !fold_head) {
    ProfScope ps(2, 2.0 * n * (double)D * D, stream);
    XNRS_TRY(pooled_out_projection(pob, asum, att, head ? pb : y, n, D, wo_planes, stream));
  }
  if (head) {
    ProfScope ps(5, 2.0 * n * ((double)D * E + (double)E * E), stream);
    GemmArgs g1 = gemm_linear(fold_head ? pob : pb, {}, D, fold_head ? head->w0_folded : head->w0, head->b0, hb, E, n, E, D,
                              head->activation);
    if (fold_head && att->bo) {
      g1.rowscale = asum;
      g1.rowscale_vec = head->b0_rowvec;
    }
    XNRS_TRY(launch_gemm_f32(g1, stream));
    XNRS_TRY(launch_gemm_f32(gemm_linear(hb, {}, E, head->w2, head->b2, y, E, n, E, E), stream));
  }
  return XNRS_OK;
}

// where the pooled vectors of a call go: the fold buffer (pooled_tail follows), else the head's input, else the caller's y
inline float* pooled_dst(bool fold, float* pob, const xnrs_head_params* head, float* pb, float* y) { return fold ? pob : (head ? pb : y); }
// This product runs over a row list IN PLACE: A rows gathered through `src` (one row per id), C rows (or row dots) scattered
// through `dst` (nullptr: `src`); n = the list's length (its CAPACITY with the length on the device, n_dev), fill = its expected share
inline void over_row_list(GemmArgs* g, const int32_t* src, const int32_t* dst, int64_t n, const int64_t* n_dev, float fill) {
  g->gather_ids = src; g->gather_S = 1; g->c_scatter = 1; g->c_scatter_ids = dst;
  g->M = n; g->m_dev = n_dev; g->m_fill_hint = fill;
}
inline void over_live_tiles(GemmArgs* g, const int64_t* n, const int32_t* tiles) { g->live_n = n; g->live_tiles = tiles; }
constexpr float LR_FILL = 0.3f;  // tile choice only: the share of a pass's rows expected on the list (ragged titles x empty slots)

// ---- the padded pipeline (seq_encode): check -> plan -> route -> weights -> (one-launch kernel | pass loop) -> tail
inline bool is_additive(const SeqEncode& r) { return r.pooled && r.pool_kind == XNRS_POOL_ADDITIVE; }
inline int hidden_of(const SeqEncode& r) { return is_additive(r) ? r.pool->hidden : 0; }
inline int width_of(const SeqEncode& r) { return (r.pooled && r.head) ? r.head->out_features : r.D; }
// the argument checks of a padded call, in the order the tests pin (which code a bad call returns)
int32_t check_seq_encode(const SeqEncode& r) {
  if (r.n_seq < 0 || r.L <= 0 || r.D <= 0 || (!r.x && !r.x16) || !r.y) return XNRS_EINVAL;
  if (r.x16 && (r.x || !r.ids || !r.m || !r.pooled || r.train || r.a_out)) return XNRS_EINVAL;  // a bf16 TABLE, inference: never dense rows
  if (r.att) {
    if (r.att->n_heads <= 0 || !r.att->wq || !r.att->wk || !r.att->wv || !r.att->wo) return XNRS_EINVAL;
    if (r.D % r.att->n_heads != 0) return XNRS_EHEADS;
    if (r.L > 128) return XNRS_EUNSUPPORTED;
    if (r.train && r.D / r.att->n_heads > 128) return XNRS_EUNSUPPORTED;  // the backward kernels' limit (mha_bwd.hip MAX_FT)
  }
  if (r.pooled) {
    if (r.pool_kind != XNRS_POOL_ADDITIVE && r.pool_kind != XNRS_POOL_MEAN) return XNRS_EINVAL;
    if (is_additive(r) && (!r.pool || !r.pool->w1 || !r.pool->w2 || r.pool->hidden <= 0)) return XNRS_EINVAL;
    if (r.pool_kind == XNRS_POOL_MEAN && !r.m) return XNRS_EINVAL;
    if (r.L > 512) return XNRS_EUNSUPPORTED;
    if (r.head && (!r.head->w0 || !r.head->w2 || r.head->out_features <= 0 || r.head->activation < 0 || r.head->activation > 2))
      return XNRS_EINVAL;
  }
  return (r.ids && !r.m && r.pooled && r.pool_kind == XNRS_POOL_MEAN) ? XNRS_EINVAL : XNRS_OK;
}

// ---- Route: every decision of a padded call, each taken ONCE, in make_route, from arguments, plan, knobs, GEMM mode and the timer's
// stage mask -- never from data (hipGraph).  qkv_given, live, kvl require train, every other one !train.  Per stage, first match:
struct Route {
  bool fused, afused;  // the whole call as ONE kernel: news_fused.hip, additive_fused.hip
  // project: image given | training lists (kvl: K|V over a list too) | live rows ("lr_qkv"; tail: the launch carries the
  //   previous fc1) | dense (lt_qkv: live row tiles; direct: from the bf16 rows, a16: their weight planes are wanted)
  bool qkv_given, live, kvl, lr_qkv, tail, lt_qkv, direct, a16;
  bool fold;  // out-project: folded away ("fold") | training lists (live) | dense
  // fc1: training lists (live) | live rows (lr_fc1; tail: deferred) | dense (lt_fc1: live row tiles; rowdot: fc2 in the epilogue)
  bool lr_fc1, lt_fc1, rowdot;
  bool skip_dead, read_counts;  // attend: zeros for an all-masked sequence; timer: the list counts of every pass are read back once
  bool o_live;  // attend: the O row of a masked query is not stored at all (every reader of O walks the live rows)
};

// Short sequences: attention + additive pooling of ALL sequences in one launch (news_fused.hip); only the pooled
// vectors leave the CU.  Inference only (nothing is saved for a backward), fp32 arithmetic only.
// Dispatch (measured, tools/bench_news_fused.py at D = 320; profiles/r02_news_fused_dispatch_sweep.txt): a workgroup owns
// news padded to 32 token rows each, so the kernel wins from ~26 tokens (<= 19 % padding) upwards and once there are
// enough news to fill the CUs -- with 1 news per workgroup (two workgroups per CU) from ~200, with 2 news per workgroup
// (every weight fragment feeds 4 row tiles) from 512: 256 x 30 tokens 116 vs 149 us for the pipeline, 512 x 30: 177 vs
// 217 us, 1024 x 30: 325 vs 329 us.  From ~1500 news on the pipeline is ahead again since it folds the out-projection
// behind the pooling (fold_out_projection above; the fused kernel computes it per token): 2048 x 30: 623 vs 592 us,
// 28 160 x 30: 8.2 vs 7.1 ms; 64 x 30: 111 vs 104 us, 1024 x 20: 318 vs 255 us.  XNRS_NEWS_FUSED=2 forces the kernel
// for every eligible shape (tests), 0 turns it off.
// Short sequences go through the fused kernel; everything else folds the out-projection behind the pooling.
// The predicate covers EVERY precondition of the launch (shape, 16-byte aligned operands, 160 KB of dynamic LDS on the
// current device: news_fused_ready), so a batch the kernel cannot take runs on the pipeline instead of failing.
bool news_fused_route(const SeqEncode& r, const Plan& p, int A, bool fold, NewsFusedArgs* f) {
  const xnrs_mha_params* att = r.att;
  const int L = r.L, D = r.D;
  if (!(att && is_additive(r) && !r.train && !r.a_out && att->dropout_p == 0.f && gemm_mode() == 0 && knobs().news_fused &&
        news_fused_plan(L, D, att->n_heads, A, nullptr) && (D / att->n_heads) * att->n_heads == D &&
        (knobs().news_fused == 2 || (L >= 26 && r.n_seq >= 192))))
    return false;
  f->x = r.x; f->ids = r.ids; f->mask = r.m;
  f->wq = att->wq; f->bq = att->bq; f->wk = att->wk; f->bk = att->bk; f->wv = att->wv; f->bv = att->bv;
  f->wo = att->wo; f->bo = att->bo;
  f->w1 = r.pool->w1; f->b1 = r.pool->b1; f->w2 = r.pool->w2; f->b2 = r.pool->b2;
  f->img = at(r.ws, p.off_nf);
  f->p = pooled_dst(fold, at(r.ws, p.fold.po), r.head, at(r.ws, p.off_p), r.y);
  f->ldp = D; f->hm = r.m ? r.hm : nullptr; f->n_seq = r.n_seq;
  f->S = L; f->D = D; f->n_heads = att->n_heads; f->d_k = D / att->n_heads; f->A = A; f->scaled = att->scaled;
  f->npw = knobs().news_fused_npw ? knobs().news_fused_npw : (r.n_seq < 512 ? 1 : 2);
  if (fold) {  // the kernel pools the attention rows; Wo is applied once per news (pooled_tail)
    f->fold = 1; f->o_scratch = at(r.ws, p.off_nfo); f->asum = at(r.ws, p.fold.as);
  }
  if (r.x16) {  // bf16 table: the kernel runs pass by pass on the widened rows and the gathered mask rows (run_one_launch)
    f->x = at(r.ws, p.off_x32); f->ids = nullptr; f->mask = at(r.ws, p.off_m32);
  }
  // (fold with the caller's folded pair: prepare_weights hands the kernel THAT w1 -- its alignment is asked about here, before
  // the route is taken, not by the launch)
  if (fold && r.pool->w1_folded && !aligned16(r.pool->w1_folded)) return false;
  return p.off_nf != 0 && news_fused_ready(*f);
}

// Additive-only towers (no self-attention: StandardRec / BaseRec / NAML / LSTUR news encoders) from a batch that fills
// the chip: fc1 + tanh + fc2 + exp + mask + normalise + weighted sum as ONE persistent launch (additive_fused.hip).  Its
// result equals the GEMM + pooling pipeline's bit for bit (same MFMA fragments and k order, same reduction orders), so
// the choice may depend on the batch size without a news vector ever changing: from two 256-row tiles per CU on the
// fused launch wins (tools/bench_af.py, settled clocks: 2 560 news x 50 x 768 -- two tiles per CU -- 0.447 vs 0.469 ms for
// the pipeline; 12 800 news -- ten per CU -- 2.13 vs 2.33 ms, i.e. 0.98 of the plain fc1 GEMM of the same shape with the
// pooling included); below that the pipeline's smaller tiles fill the chip better.
bool additive_fused_route(const SeqEncode& r, const Plan& p, int A, bool rowdot, AdditiveFusedArgs* af) {
  if (!(!r.att && is_additive(r) && !r.train && !r.a_out && gemm_mode() == 0 && knobs().additive_fused &&
        additive_fused_plan(r.L, r.D, A, nullptr, nullptr) && rowdot &&
        (knobs().additive_fused == 2 || additive_fused_tiles(r.n_seq, r.L) >= 512)))
    return false;
  af->x = r.x16 ? at(r.ws, p.off_x32) : r.x; af->ids = r.x16 ? nullptr : r.ids; af->mask = r.x16 ? at(r.ws, p.off_m32) : r.m;
  af->w1 = r.pool->w1; af->b1 = r.pool->b1; af->w2 = r.pool->w2; af->b2 = r.pool->b2;
  af->y = pooled_dst(false, nullptr, r.head, at(r.ws, p.off_p), r.y);
  af->ldy = r.D; af->hm = r.m ? r.hm : nullptr; af->n_seq = r.n_seq;
  af->S = r.L; af->D = r.D; af->A = A;
  return additive_fused_ready(*af);
}
// the pre-split planes of Wq, Wk, Wv, Wo (i = 0..3), then W1, in the plan's planes region (prepare_weights fills them)
inline unsigned short* weight_plane(const SeqEncode& r, const Plan& p, int i) {
  return at<unsigned short>(r.ws, p.off_planes + (size_t)i * align_up(split_planes_bytes(r.D, r.D)));
}

// *nf / *af: the arguments of the one-launch kernel the route names (w1 / b1: prepare_weights puts the folded pair there)
Route make_route(const SeqEncode& r, const Plan& p, NewsFusedArgs* nf, AdditiveFusedArgs* af) {
  const xnrs_row_lists rl = r.rl ? *r.rl : xnrs_row_lists{};
  const int L = r.L, D = r.D, A = hidden_of(r);
  const bool additive = is_additive(r);
  const int64_t n_rows = r.n_seq * (int64_t)L;
  Route rt{};
  // (training) the Q|K|V image of another forward over the same input and weights: read it, project nothing (xnrs_row_lists)
  rt.qkv_given = r.train && r.att && rl.qkv_shared;
  // Training forward over the UNMASKED token rows (optional, exact): a masked token row has pooling weight exp(e) * 0, so
  // its query projection, its out-projection row and its fc1 row never reach the output or any gradient (K and V stay
  // dense: padded tokens are keys, layers.py:142-144).  Those three products run over the live rows in place (A rows
  // gathered, C rows scattered through the same list); the dead rows of Q, Y and T are ZEROED first, which keeps every
  // later consumer -- attention core, pooling, and the backward kernels that read the saved activations -- finite and
  // exactly as if the rows had been computed and then multiplied by the zero weight.
  // An attention-FREE additive tower (StandardRec, NAML's views) takes the same list for its one row-parallel product:
  // fc1 runs over the live token rows of x, T of the masked rows is zero.
  rt.live = r.train && additive && r.m && rl.live_rows && (rl.counts_dev || (rl.n_live >= 0 && rl.n_live < n_rows)) &&
            !(r.ids && !rl.live_src_rows);
  // ... and K|V over the token rows of the NON-EMPTY news only (kv_rows, optional, exact): the keys and values of a news
  // are read by that news' own queries alone, and an all-masked news has no live query, so its K and V rows (zeroed
  // here: its attention rows then come out as finite zeros) reach neither the output nor a gradient.
  rt.kvl = rt.live && rl.kv_rows && (rl.counts_dev || (rl.n_kv >= 0 && rl.n_kv < n_rows)) && !(r.ids && !rl.kv_src_rows);
  rt.fold = r.att && additive && fold_wanted(r.train ? knobs().fold_train : knobs().fold_out);  // ("fold", above)
  rt.fused = news_fused_route(r, p, A, rt.fold, nf);
  // inference, fp32 GEMM mode, 16-byte-aligned shapes the buffer-load kernel serves, no gathered rows: the pooler's fc2
  // dot is taken in the fc1 epilogue (fc1_product)
  // (every input path -- dense rows, id gather, padding-free -- takes it, so they stay bitwise equal)
  // (x16: the pooler of an attention-free tower reads the widened rows, 256-byte aligned in the workspace)
  const float* xal = r.x16 ? at(r.ws, p.off_x32) : r.x;  // the rows whose alignment the predicates ask about
  rt.rowdot = additive && !r.train && !rt.fused && fc1_rowdot_ok(xal, r.att != nullptr, r.pool, r.D);
  rt.afused = additive_fused_route(r, p, A, rt.rowdot, af);
  // (bf16 table: the direct route multiplies the bf16 rows with the planes of Wq | Wk | Wv in EVERY mode)
  rt.a16 = r.x16 && r.att && additive && !rt.fused && knobs().gemm_a16;
  // bf16 table, direct route: Q|K|V of every pass is ONE gemm_a16 product over the bf16 rows.  Decided once per call, from
  // the shape of its first (largest) pass; a shape the kernel refuses takes the widening route.
  const unsigned short* pl[3] = {weight_plane(r, p, 0), weight_plane(r, p, 1), weight_plane(r, p, 2)};
  const int64_t rows0 = (r.n_seq < p.chunk ? r.n_seq : p.chunk) * r.L;
  rt.direct = rt.a16 && gemm_a16_ok(qkv_projection(nullptr, {r.ids, r.L}, r.att, 0, at(r.ws, p.off_qkv), 3 * (int64_t)r.D, rows0, r.D, pl), r.x16);
  // Live row tiles (inference, the news encoder's pooled calls with a mask; XNRS_GEMM_LIVE_TILES=0: off).  An all-masked
  // sequence -- an empty history slot, 49.5 % of the benchmark's -- has a result that needs none of its rows: every query
  // row is masked, the pooler multiplies every row by 0, the pooled vector is 0.  Its rows are contiguous, so whole
  // 128-row GEMM tiles hold nothing else: the two row-parallel products of a pass walk the tiles that hold a row of a live
  // sequence (GemmArgs::live_tiles; the list of every pass is built by ONE launch per call, rows stay where they are).
  //   Q|K|V: only while the attention kernel of this shape leaves a dead sequence before reading its rows
  //          (mha_core_skips_dead: the skipped rows of the image are never written);
  //   fc1:   with the fc2 dot in its epilogue; the pooler then leaves a dead sequence before reading its scores.
  // By size: the list costs one short launch per call (a workgroup per pass; measured 33 us at 20 passes), which must not
  // show where a call is latency-bound (one impression: 2 750 token rows) -- from live_tiles_min_rows token rows per call
  // on (default 16 384 = 128 tiles: the list then pays for itself from ~9 dead tiles, 3.6 us each at D = 768 for the two
  // products).
  // The choice never depends on the data (hipGraph) and changes no bit: a live sequence's rows are computed as before.
  const bool lt = r.live_tiles && knobs().gemm_live_tiles && !r.train && r.pooled && r.m && r.att && !rt.fused && !rt.afused &&
                  n_rows >= knobs().gemm_live_tiles_min_rows &&
                  device_counts_ok(xal, D, A, r.att, additive ? r.pool : nullptr);
  MhaCoreArgs probe{};
  if (lt && knobs().mha_skip_masked) {
    probe = mha_core_args(at(r.ws, p.off_qkv) + D, 3 * (int64_t)D, r.att, at(r.ws, p.off_o), p.chunk, L, D);
    probe.q = at(r.ws, p.off_qkv); probe.mask = r.m; probe.skip_dead = 1;
  }
  rt.lt_qkv = probe.skip_dead && mha_core_skips_dead(probe);
  rt.lt_fc1 = lt && additive && rt.rowdot;
  // Live rows (the second half of the same saving; XNRS_GEMM_LIVE_ROWS=0: off).  A masked token row of a LIVE sequence stays
  // a key and a value (the mask is a query-row mask, layers.py:142-144), but its Q row feeds only its own attention row and
  // its fc1 row only its own score -- and both poolers multiply that row by exactly 0.  So wherever a product walks the
  // live row tiles, its query / score half walks the ascending list of the pass's unmasked token rows instead (mask != 0:
  // the dense path's own rule, any mask value keeps its meaning), rows gathered and results scattered IN PLACE:
  //   Q|K|V: K|V over the live row tiles as before (N = 2D), Q over the live rows (N = D) into the same image; the Q rows
  //          of masked tokens stay UNWRITTEN -- the attention kernel does not read a masked query's row (mha_core.hip);
  //   fc1:   the fc2 dots of the live rows, scattered to their own rows of the score image; the pooler does not read a
  //          masked token's score (AdditivePoolArgs::skip_masked), so its summation order -- and every bit -- is unchanged.
  // The lists of every pass come from the ONE list launch of the call (launch_dense_row_lists writes the tile lists too);
  // the grids are sized for every row, the counts stay on the device (GemmArgs::m_dev): nothing depends on the data.
  const bool lr = lt && knobs().gemm_live_rows && p.off_lr_cnt != 0 && L <= 64 && n_rows <= 0x7fffffffLL &&
                  n_rows >= knobs().gemm_live_rows_min_rows;
  // (bf16 table, direct route: Q|K|V stays one product over the live row tiles -- no live-row Q list, no one-launch grid)
  rt.lr_qkv = lr && rt.lt_qkv && !rt.direct;
  rt.lr_fc1 = lr && rt.lt_fc1;
  // fc1 in the tail (XNRS_GEMM_FC1_IN_TAIL=0: off).  Where a pass takes the one-launch projection and its fc1 walks the
  // live-row list over the O rows (folded out-projection), fc1 + pooling of pass i-1 wait until pass i has been projected:
  //   launch{ K|V(i), Q(i), fc1(i-1) }  ->  pool(i-1)  ->  mha(i)          (after the last pass: fc1 and pool on their own)
  // fc1 fills the tail of the projection grid instead of being a short launch of its own (gemm_f32.hip).  No new buffer:
  // o and t of pass i-1 are read before mha(i) overwrites o, the image of pass i is written after mha(i-1) has read it, the
  // row lists of every pass are in the workspace already.  Decided from shapes and knobs alone; a call with ids, a bf16
  // table or the stage-3 timer on (an fc1 without a launch of its own has no time to report) keeps the sequence above.
  rt.tail = rt.lr_qkv && rt.lr_fc1 && rt.fold && r.pooled && !r.ids && !r.x16 && knobs().gemm_fc1_in_tail && !prof_on(3);
  // launch timer on: the live-tile (and live-row) counts of every pass, read back ONCE per call (the timer is a measurement
  // aid that synchronises anyway; nothing is read while it is off) -- stages 0 and 3 then report EXECUTED FLOPs
  rt.read_counts = (rt.lt_qkv && prof_on(0)) || (rt.lt_fc1 && prof_on(3));
  // an all-masked sequence: zeros instead of attention over keys nobody weights (kernels.h).  Training over row lists,
  // and (round 4) every POOLED call with a mask: both poolers multiply a masked row by exactly 0 (layers.py:33,62-65), so
  // the pooled vector is bit for bit the same whether such a row holds the uniform average of V or zeros -- the empty
  // history slots of the benchmark batch (49.5 % of its news) cost the attention core nothing.  MultiHeadAttention
  // alone (pooled == false) returns its masked rows to the caller and computes them.
  rt.skip_dead = rt.live || (r.pooled && r.m && knobs().mha_skip_masked);
  // O rows nobody reads (XNRS_MHA_LIVE_O=0: off).  With the out-projection folded away the pooler works on the O rows, and
  // on the live-row route O has exactly two readers: fc1 walks the pass's live-row list (fc1_live_rows_args), and the pooler
  // leaves an all-masked sequence behind its mask and then reads the rows with a non-zero weight only -- a masked row's
  // weight is its mask value, 0 (pool_score.hip: skip_masked, s_idx).  So the attention kernel stores NOTHING for a masked
  // query (MhaCoreArgs::o_live_only): at the benchmark's history passes 49.5 % of the news are empty slots and a title fills
  // 27.5 of its 50 rows, i.e. ~145 MB of zeros and averages per pass that went to HBM to be overwritten by the next pass.
  // Only where the attention launch goes to the kernel that honours skip_dead (lt_qkv: decided by mha_core_skips_dead above).
  // A dense reader of O keeps every write: the out-projection GEMM (XNRS_FOLD_OUT=0), the live-TILE fc1 without the row list
  // (lt_fc1 alone: its tiles hold masked rows), MultiHeadAttention alone (the caller reads the rows), training (the backward).
  // (and never with dropout: the kernel's dropout instantiations do not take the flag)
  rt.o_live = rt.lr_fc1 && rt.lt_qkv && rt.fold && r.pooled && !r.train && rt.skip_dead && r.att->dropout_p == 0.f && knobs().mha_live_o;
  return rt;
}

// ---- the context of one call: what its stages share, resolved once (prepare_weights and run_passes complete it)
struct Call {
  const SeqEncode& r;
  hipStream_t stream;
  const Plan p;
  const Route rt;
  NewsFusedArgs nf; AdditiveFusedArgs af;  // the launch of Route::fused / afused
  const int L = r.L, D = r.D, A = hidden_of(r);
  const xnrs_mha_params* att = r.att;
  // training lists (xnrs_row_lists; lvx, kvx: as rows of x, table rows with ids).  Counts on the device (counts_dev): the list
  // lengths are then CAPACITIES (every row), the products over a list read their row count on the device (GemmArgs::m_dev)
  const xnrs_row_lists rl = r.rl ? *r.rl : xnrs_row_lists{};
  const int32_t *lvx = rt.live ? (r.ids ? rl.live_src_rows : rl.live_rows) : nullptr, *kvx = rt.kvl ? (r.ids ? rl.kv_src_rows : rl.kv_rows) : nullptr;
  const int64_t* cnt = rl.counts_dev;
  const int64_t n_live = cnt ? r.n_seq * L : rl.n_live, n_kv = cnt ? r.n_seq * L : rl.n_kv;
  float *qkv = rt.qkv_given ? const_cast<float*>(rl.qkv_shared) : at(r.ws, p.off_qkv), *o = at(r.ws, p.off_o), *yb = at(r.ws, p.off_y);
  float *t = at(r.ws, p.off_t), *pb = at(r.ws, p.off_p), *hb = at(r.ws, p.off_h), *pob = at(r.ws, p.fold.po), *asum = at(r.ws, p.fold.as);
  float *stats = (r.train && att) ? at(r.ws, p.off_stats) : nullptr, *a_save = (r.train && is_additive(r)) ? at(r.ws, p.off_a) : nullptr;
  float *x32 = at(r.ws, p.off_x32), *m32 = at(r.ws, p.off_m32);
  const int64_t lt_cap = live_tiles_cap(p.chunk, L, LIVE_TILE_BM);
  uint8_t* lt_alive = at<uint8_t>(r.ws, p.off_lt_alive);
  int64_t *lt_n = at<int64_t>(r.ws, p.off_lt_n), *lr_cnt = at<int64_t>(r.ws, p.off_lr_cnt);
  int32_t *lt_tiles = at<int32_t>(r.ws, p.off_lt_tiles), *lr_loc = at<int32_t>(r.ws, p.off_lr_loc), *lr_src = at<int32_t>(r.ws, p.off_lr_src);
  std::vector<int64_t> lt_host{}, lr_host{};  // launch timer: host copies of the counts (empty: not read)
  Fc1 fc1{};
  const unsigned short *pqkv[3] = {nullptr, nullptr, nullptr}, *po = nullptr, *p1 = nullptr;
};

// plane i of the region <- the split of W [N][D]; nullptr if the split did not launch (a product then does without the plane)
const unsigned short* split_plane(const Call& c, const float* W, int N, int i) {
  return launch_split_weights(W, N, c.D, weight_plane(c.r, c.p, i), c.stream) == hipSuccess ? weight_plane(c.r, c.p, i) : nullptr;
}
// The weights of a call: the fold-weight build, then -- it reads fc1.w -- the split planes.
int32_t prepare_weights(Call* c) {
  const Route& rt = c->rt;
  XNRS_TRY_RC(fc1_pair(rt.fold, c->att, is_additive(c->r) ? c->r.pool : nullptr, c->D, c->r.ws, c->p.fold, c->stream, &c->fc1));
  if (rt.fold && rt.fused) {  // the fused kernel's fc1 image is built from the folded pair
    c->nf.w1 = c->fc1.w; c->nf.b1 = c->fc1.b;
  }
  // bf16-split GEMM modes: split the weights ONCE per call (the pass loop reuses them ~20 times per step)
  if (gemm_mode() == 0 && !rt.a16) return XNRS_OK;
  if (c->att) {  // (direct route: launch_gemm_a16 refuses a product whose plane is missing)
    const float* W[3] = {c->att->wq, c->att->wk, c->att->wv};
    for (int i = 0; i < 3; ++i) c->pqkv[i] = split_plane(*c, W[i], c->D, i);
    if (gemm_mode() != 0) c->po = split_plane(*c, c->att->wo, c->D, 3);
  }
  if (c->A && gemm_mode() != 0) c->p1 = split_plane(*c, c->fc1.w, c->A, c->att ? 4 : 0);
  return XNRS_OK;
}

// ---- Pass: the view of the sequences [c0, c0 + nc) of a call (make_pass)
struct Pass {
  int64_t c0, nc, rows;
  const float *cx, *cm;        // the pass's token rows (the whole table when gathering) and mask rows
  const int32_t *cids, *xids;  // gather for the mask rows; gather for the token rows
  // what the pooler sees, and the gather for it: the token rows, behind an attention tower its output (out_project)
  const float* seq; const int32_t* seq_ids;
  // its live row tiles (count, list; timer: the rows they hold) and live rows (in its own row space, in x's, count; timer: its value)
  const int64_t *ltn, *lrn;
  const int32_t *ltl, *lrl, *lrs;
  double lt_rows, lr_rows;
};

// The pass from sequence c0 on (`step` sequences, fewer in the last).  bf16 table: every route but the direct one runs on its WIDENED
// rows, enqueued here -- before anything reads x32 / m32, which the next pass reuses (a one-launch kernel: and its gathered mask rows)
int32_t make_pass(const Call& c, int64_t c0, int64_t step, Pass* ps) {
  const SeqEncode& r = c.r;
  const int64_t i = c0 / c.p.chunk;
  ps->c0 = c0; ps->nc = (r.n_seq - c0 < step) ? (r.n_seq - c0) : step; ps->rows = ps->nc * c.L;
  ps->ltn = c.lt_n + i; ps->ltl = c.lt_tiles + i * c.lt_cap;
  ps->lt_rows = (double)LIVE_TILE_BM * (double)(c.lt_host.empty() ? (ps->rows + LIVE_TILE_BM - 1) / LIVE_TILE_BM : c.lt_host[(size_t)i]);
  ps->lrl = c.lr_loc + i * c.p.chunk * c.L; ps->lrs = c.lr_src + i * c.p.chunk * c.L; ps->lrn = c.lr_cnt + 3 * i;
  ps->lr_rows = c.lr_host.empty() ? (double)ps->rows : (double)c.lr_host[(size_t)(3 * i)];
  ps->cids = r.ids ? r.ids + c0 : nullptr; ps->xids = ps->cids;  // gathers for the mask rows and the token rows
  ps->cx = r.ids ? r.x : r.x + c0 * (int64_t)c.L * c.D;  // table stays whole when gathering
  ps->cm = r.m ? (r.ids ? r.m : r.m + c0 * (int64_t)c.L) : nullptr;
  if (r.x16) {  // bf16 table: the direct route reads it in the projection alone; every other call runs on the widened rows
    ps->cx = c.rt.direct ? nullptr : c.x32; ps->xids = c.rt.direct ? ps->cids : nullptr;
    if (!c.rt.direct) XNRS_TRY(launch_gather_rows_bf16(r.x16, r.ids + c0, 1, c.x32, ps->nc, (int64_t)c.L * c.D, c.stream));
    if (c.rt.fused || c.rt.afused) XNRS_TRY(launch_gather_rows(r.m, r.ids + c0, c.m32, ps->nc, c.L, c.stream));
  }
  ps->seq = ps->cx; ps->seq_ids = ps->xids;
  return XNRS_OK;
}

// The whole call as one kernel (Route::fused / afused).  bf16 table: pass by pass on the widened rows (the same bits).
int32_t run_one_launch(const Call& c) {
  const double L = c.L, D = c.D, A = c.A;
  const double fl = c.rt.fused ? (double)c.r.n_seq * ((c.nf.fold ? 6.0 : 8.0) * L * D * D + 4.0 * L * L * D + 2.0 * L * D * A + 2.0 * L * (A + D))
                               : (double)c.r.n_seq * (2.0 * L * D * A + 2.0 * L * (A + D));
  ProfScope ps(c.rt.fused ? 6 : 3, fl, c.stream);
  const int64_t step = c.r.x16 ? c.p.chunk : c.r.n_seq;
  Pass pass;
  for (int64_t c0 = 0; c0 < c.r.n_seq; c0 += step) {
    XNRS_TRY_RC(make_pass(c, c0, step, &pass));
    if (c.rt.fused) {
      NewsFusedArgs f = c.nf;
      f.n_seq = pass.nc; f.p = c.nf.p + c0 * c.nf.ldp;
      f.hm = c.nf.hm ? c.nf.hm + c0 : nullptr; f.asum = c.nf.asum ? c.nf.asum + c0 : nullptr;
      XNRS_TRY(launch_news_fused(f, c.stream));
    } else {
      AdditiveFusedArgs a = c.af;
      a.n_seq = pass.nc; a.y = c.af.y + c0 * (int64_t)c.D; a.hm = c.af.hm ? c.af.hm + c0 : nullptr;
      XNRS_TRY(launch_additive_fused(a, c.stream));
    }
  }
  return XNRS_OK;
}

// ---- pool: what fc1 left in t -> pooled vector, history mask | masked mean
int32_t pool_additive(const Call& c, const Pass& pass) {
  AdditivePoolArgs pa = additive_pool_args(c.t, c.rt.rowdot, c.r.pool, pass.seq, pass.nc, c.L, c.D, c.A);
  pa.skip_dead = c.rt.lt_fc1 ? 1 : 0; pa.skip_masked = c.rt.lr_fc1 ? 1 : 0;
  pa.mask = pass.cm; pa.mask_gather_ids = pass.cids; pa.x_gather_ids = pass.seq_ids;
  pa.y = pooled_dst(c.rt.fold, c.pob, c.r.head, c.pb, c.r.y) + pass.c0 * (int64_t)c.D;
  pa.asum_out = c.rt.fold ? c.asum + pass.c0 : nullptr;
  pa.a_out = c.a_save ? c.a_save : (c.r.a_out ? c.r.a_out + pass.c0 * (int64_t)c.L : nullptr);
  pa.hm_out = (pass.cm && c.r.hm) ? c.r.hm + pass.c0 : nullptr;
  {
    ProfScope ps(4, 2.0 * (double)pass.rows * (double)(c.A + c.D), c.stream);
    XNRS_TRY(launch_additive_pool(pa, c.stream));
  }
  if (c.a_save && c.r.a_out)  // (after the pool)
    XNRS_TRY(hipMemcpyAsync(c.r.a_out, c.a_save, (size_t)pass.rows * sizeof(float), hipMemcpyDeviceToDevice, c.stream));
  return XNRS_OK;
}
int32_t pool_mean(const Call& c, const Pass& pass) {
  MeanPoolArgs mp{};
  mp.x = pass.seq; mp.ldx = c.D; mp.x_gather_ids = pass.seq_ids;
  mp.mask = pass.cm; mp.mask_gather_ids = pass.cids;
  mp.y = pooled_dst(false, nullptr, c.r.head, c.pb, c.r.y) + pass.c0 * (int64_t)c.D;
  mp.hm_out = c.r.hm ? c.r.hm + pass.c0 : nullptr;
  mp.n_seq = pass.nc; mp.N = c.L; mp.D = c.D;
  ProfScope ps(4, 2.0 * pass.rows * (double)c.D, c.stream);
  return hip_rc(launch_mean_pool(mp, c.stream));
}

// ---- fc1 in the tail (Route::tail): the deferred fc1 + pooling of the previous pass,
//   launch{ K|V(i), Q(i), fc1(i-1) }  ->  pool(i-1)  ->  mha(i)          (after the last pass: fc1 and pool on their own)
struct DeferredFc1 {
  bool on = false;  // fc1 + pooling of a pass are outstanding
  GemmArgs fg; Pass pass;  // its fc1 goes out with the next pass's projection, its pooling right behind it
  void defer(const GemmArgs& g, const Pass& of) { on = true; fg = g; pass = of; }
  // rode: the projection launch carried fc1, its scores are out -- pool the pass before the next attention overwrites its O
  // rows.  Else fc1 and pooling on their own: the last pass of a call, or a successor that does not take the merged launch
  int32_t flush(const Call& c, bool rode) {
    if (!on) return XNRS_OK;
    on = false;
    if (!rode) XNRS_TRY(launch_gemm_f32(fg, c.stream));
    return pool_additive(c, pass);
  }
};

// ---- project: [Q|]K|V of a pass into the image c.qkv
// (training lists) K|V of every row (kvl: of the rows of the non-empty news), Q of the live rows only (dead rows = 0)
int32_t project_train_lists(const Call& c, const Pass& pass) {
  const int D = c.D;
  const int64_t ld3 = 3 * (int64_t)D;
  const double nl = (double)prof_count(0, c.cnt, 0, c.n_live, c.stream), nkv = (double)prof_count(0, c.cnt, 1, c.n_kv, c.stream);
  ProfScope ps(0, 2.0 * (c.rt.kvl ? nkv : pass.rows) * 2.0 * D * D + 2.0 * nl * (double)D * D, c.stream);
  GemmArgs g = qkv_projection(pass.cx, {pass.xids, c.L}, c.att, 1, c.qkv + D, ld3, pass.rows, D, c.pqkv);
  if (c.rt.kvl) {
    XNRS_TRY(launch_zero_dead_qkv(c.qkv, pass.cm, pass.cids, pass.nc, c.L, D, c.stream));
    over_row_list(&g, c.kvx, c.rl.kv_rows, c.n_kv, c.cnt ? c.cnt + 1 : nullptr, 0.6f);
    if (c.n_kv > 0) XNRS_TRY(launch_gemm_f32(g, c.stream));
  } else {
    XNRS_TRY(launch_gemm_f32(g, c.stream));
    XNRS_TRY(launch_zero_cols(c.qkv, ld3, D, pass.rows, c.stream));
  }
  if (c.n_live <= 0) return XNRS_OK;
  GemmArgs q = gemm_linear(pass.cx, {}, D, c.att->wq, c.att->bq, c.qkv, ld3, 0, D, D, XNRS_ACT_NONE, c.pqkv[0]);
  over_row_list(&q, c.lvx, c.rl.live_rows, c.n_live, c.cnt, 0.4f);
  return hip_rc(launch_gemm_f32(q, c.stream));
}
// (live rows, "lr_qkv") K|V of the live row tiles, Q of the live rows: a masked token's Q row stays unwritten, nobody reads it
int32_t project_live_rows(const Call& c, const Pass& pass, DeferredFc1* prev) {
  const int D = c.D;
  GemmArgs g = qkv_projection(pass.cx, {pass.xids, c.L}, c.att, 1, c.qkv + D, 3 * (int64_t)D, pass.rows, D, c.pqkv);
  over_live_tiles(&g, pass.ltn, pass.ltl);
  GemmArgs q = gemm_linear(pass.cx, {}, D, c.att->wq, c.att->bq, c.qkv, 3 * (int64_t)D, 0, D, D);
  over_row_list(&q, pass.xids ? pass.lrs : pass.lrl, pass.lrl, pass.rows, pass.lrn, LR_FILL);
  // the two read the same x and write disjoint columns of the image: ONE grid, the Q tiles behind the K|V tiles, leaves
  // one partly filled last round of workgroups instead of two and a launch boundary (XNRS_GEMM_QKV_ONE_LAUNCH=0: two
  // launches; the same bits either way, and the same choice for every pass of the call whatever the data)
  const bool one = gemm_qkv_one_launch_ok(g, q);
  // (fc1 in the tail) the outstanding fc1 rides in this launch if it can; otherwise it and its pooling run first, as before
  const bool merged = c.rt.tail && one && (!prev->on || gemm_fc1_in_tail_ok(prev->fg));
  if (!merged) XNRS_TRY_RC(prev->flush(c, false));
  {
    // (on the merged route the stage's time includes the fc1 tiles in the launch's tail; its FLOPs stay those of K|V + Q)
    ProfScope ps(0, 2.0 * pass.lt_rows * 2.0 * D * D + 2.0 * pass.lr_rows * (double)D * D, c.stream);
    if (merged) {
      XNRS_TRY(launch_gemm_qkv_fc1(g, q, prev->on ? &prev->fg : nullptr, c.stream));
      if (prev->on) fc1_in_tail_add(1);
    } else if (one) {
      XNRS_TRY(launch_gemm_qkv_one(g, q, c.stream));
    } else {
      XNRS_TRY(launch_gemm_f32(g, c.stream));
      XNRS_TRY(launch_gemm_f32(q, c.stream));
    }
    qkv_launches_add(one ? 1 : 2);
  }
  return prev->flush(c, true);
}
int32_t project(const Call& c, const Pass& pass, DeferredFc1* prev) {
  if (c.rt.qkv_given) return XNRS_OK;  // nothing to project
  if (c.rt.live) return project_train_lists(c, pass);
  if (c.rt.lr_qkv) return project_live_rows(c, pass, prev);
  // (dense) Q|K|V as one product
  GemmArgs g = qkv_projection(pass.cx, {pass.xids, c.L}, c.att, 0, c.qkv, 3 * (int64_t)c.D, pass.rows, c.D, c.pqkv);
  if (c.rt.lt_qkv) over_live_tiles(&g, pass.ltn, pass.ltl);  // dead tiles stay unwritten: the attention kernel never reads their rows
  ProfScope ps(0, 2.0 * (c.rt.lt_qkv ? pass.lt_rows : (double)pass.rows) * 3.0 * c.D * c.D, c.stream);
  return hip_rc(c.rt.direct ? launch_gemm_a16(g, c.r.x16, c.stream) : launch_gemm_f32(g, c.stream));
}

// ---- attend: O = softmax(rowmask(QK^T/sqrt(dk))) V over the image
int32_t attend(const Call& c, const Pass& pass) {
  MhaCoreArgs ma = mha_core_args(c.qkv + c.D, 3 * (int64_t)c.D, c.att, c.o, pass.nc, c.L, c.D);
  ma.q = c.qkv; ma.mask = pass.cm; ma.mask_gather_ids = pass.cids; ma.dropout_p = c.att->dropout_p;
  // the kernels count (sequence, head) pairs from the launch's first sequence (kernels.h drop_uniform): a pass that starts
  // at sequence c0 continues the counter at pair c0 * heads, so sequence c0 + i draws what it draws in an unchunked call.
  ma.seed = c.att->seed + (uint64_t)pass.c0 * (uint64_t)c.att->n_heads * 0x9E3779B97F4A7C15ull;
  ma.seed_dev = c.att->seed_dev; ma.stats = c.stats; ma.skip_dead = c.rt.skip_dead ? 1 : 0;
  // (Route::o_live) fc1 and the pooler read the O rows of unmasked tokens only: the others are not stored
  ma.o_live_only = c.rt.o_live ? 1 : 0;
  if (c.rt.lt_qkv && !mha_core_skips_dead(ma)) return XNRS_EUNSUPPORTED;  // (never: the two are decided by one rule)
  ProfScope ps(1, 4.0 * pass.rows * (double)c.L * c.D, c.stream);
  XNRS_TRY(launch_mha_core(ma, c.stream));
  if (c.rt.o_live) mha_live_o_add(1);
  return XNRS_OK;
}

// ---- out-project: Y = O.Wo^T + bo; what the pooler sees from here on (pass->seq)
// (training lists) over the live rows in place, the dead rows zeroed
int32_t out_project_train_lists(const Call& c, const Pass& pass, float* dst) {
  const int D = c.D;
  ProfScope ps(2, 2.0 * (double)prof_count(2, c.cnt, 0, c.n_live, c.stream) * (double)D * D, c.stream);
  XNRS_TRY(hipMemsetAsync(dst, 0, (size_t)pass.rows * D * sizeof(float), c.stream));
  if (c.n_live <= 0) return XNRS_OK;
  GemmArgs og = gemm_linear(c.o, {}, D, c.att->wo, c.att->bo, dst, D, 0, D, D, XNRS_ACT_NONE, c.po);
  over_row_list(&og, c.rl.live_rows, nullptr, c.n_live, c.cnt, 0.4f);
  return hip_rc(launch_gemm_f32(og, c.stream));
}
int32_t out_project(const Call& c, Pass* pass) {
  // fold: the pooler works on the O rows (fold_out_projection); masked rows of O are finite and carry weight 0
  float* dst = c.rt.fold ? c.o : (c.r.pooled ? c.yb : c.r.y + pass->c0 * (int64_t)c.L * c.D);
  pass->seq = dst; pass->seq_ids = nullptr;
  if (c.rt.fold) return XNRS_OK;
  if (c.rt.live) return out_project_train_lists(c, *pass, dst);
  ProfScope ps(2, 2.0 * pass->rows * (double)c.D * c.D, c.stream);
  return hip_rc(launch_gemm_f32(gemm_linear(c.o, {}, c.D, c.att->wo, c.att->bo, dst, c.D, pass->rows, c.D, c.D, XNRS_ACT_NONE, c.po), c.stream));
}

// ---- fc1: T = tanh(seq.W1^T + b1), or the fc2 dots of its rows (rowdot)
// (training lists) with attention seq is the dense attention output; without, the rows of x (table rows with ids: lvx)
int32_t fc1_train_lists(const Call& c, const Pass& pass) {
  ProfScope ps(3, 2.0 * (double)prof_count(3, c.cnt, 0, c.n_live, c.stream) * (double)c.D * c.A, c.stream);
  XNRS_TRY(hipMemsetAsync(c.t, 0, (size_t)pass.rows * c.A * sizeof(float), c.stream));
  if (c.n_live <= 0) return XNRS_OK;
  GemmArgs fg = fc1_product(pass.seq, {}, c.fc1, c.t, 0, c.D, c.A, false, c.r.pool, c.p1);
  over_row_list(&fg, c.att ? c.rl.live_rows : c.lvx, c.rl.live_rows, c.n_live, c.cnt, 0.4f);
  return hip_rc(launch_gemm_f32(fg, c.stream));
}
// (live rows, "lr_fc1") the scores of the live rows, in place; the pooler reads no other
GemmArgs fc1_live_rows_args(const Call& c, const Pass& pass) {
  GemmArgs fg = fc1_product(pass.seq, {}, c.fc1, c.t, 0, c.D, c.A, true, c.r.pool, c.p1);
  over_row_list(&fg, pass.seq_ids ? pass.lrs : pass.lrl, pass.lrl, pass.rows, pass.lrn, LR_FILL);
  return fg;
}
int32_t fc1_stage(const Call& c, const Pass& pass) {
  if (c.rt.live) return fc1_train_lists(c, pass);
  if (c.rt.lr_fc1) {
    ProfScope ps(3, 2.0 * pass.lr_rows * (double)c.D * c.A, c.stream);
    return hip_rc(launch_gemm_f32(fc1_live_rows_args(c, pass), c.stream));
  }
  // (dense) every row
  GemmArgs fg = fc1_product(pass.seq, {pass.seq_ids, c.L}, c.fc1, c.t, pass.rows, c.D, c.A, c.rt.rowdot, c.r.pool, c.p1);
  if (c.rt.lt_fc1) over_live_tiles(&fg, pass.ltn, pass.ltl);  // their scores stay unwritten: the pooler leaves their sequences first
  ProfScope ps(3, 2.0 * (c.rt.lt_fc1 ? pass.lt_rows : (double)pass.rows) * (double)c.D * c.A, c.stream);
  return hip_rc(launch_gemm_f32(fg, c.stream));
}

// ---- the pass loop: the pipeline diagram at the top of this file, once per pass
int32_t run_passes(Call* call) {
  const Call& c = *call;
  const SeqEncode& r = c.r;
  if (c.rt.lr_qkv || c.rt.lr_fc1)
    XNRS_TRY(launch_dense_row_lists(r.m, r.ids, r.n_seq, c.p.chunk, r.L, LIVE_TILE_BM, c.lr_loc, c.lr_src, c.lr_cnt, c.lt_alive, c.lt_n,
                                    c.lt_tiles, c.stream));
  else if (c.rt.lt_qkv || c.rt.lt_fc1)
    XNRS_TRY(launch_live_tiles(r.m, r.ids, r.n_seq, c.p.chunk, r.L, LIVE_TILE_BM, c.lt_alive, c.lt_n, c.lt_tiles, c.stream));
  if (c.rt.read_counts) {
    call->lt_host.resize((size_t)((r.n_seq + c.p.chunk - 1) / c.p.chunk));
    if (hipStreamSynchronize(c.stream) != hipSuccess ||
        hipMemcpy(call->lt_host.data(), c.lt_n, c.lt_host.size() * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess)
      call->lt_host.clear();
    if (c.rt.lr_qkv || c.rt.lr_fc1) {
      call->lr_host.resize(3 * c.lt_host.size());
      if (c.lt_host.empty() || hipMemcpy(call->lr_host.data(), c.lr_cnt, c.lr_host.size() * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess)
        call->lr_host.clear();
    }
  }
  DeferredFc1 prev;  // (fc1 in the tail)
  Pass pass;
  for (int64_t c0 = 0; c0 < r.n_seq; c0 += c.p.chunk) {
    XNRS_TRY_RC(make_pass(c, c0, c.p.chunk, &pass));
    if (c.att) {
      XNRS_TRY_RC(project(c, pass, &prev));  // (fc1 in the tail: ... with fc1 of the previous pass, then its pooling)
      XNRS_TRY_RC(attend(c, pass));
      XNRS_TRY_RC(out_project(c, &pass));
    }
    if (!r.pooled) continue;
    if (!is_additive(r)) {
      XNRS_TRY_RC(pool_mean(c, pass));
    } else if (c.rt.tail) {
      prev.defer(fc1_live_rows_args(c, pass), pass);
    } else {
      XNRS_TRY_RC(fc1_stage(c, pass));
      XNRS_TRY_RC(pool_additive(c, pass));
    }
  }
  return prev.flush(c, false);  // (fc1 in the tail) the last pass
}

}  // namespace

int32_t xnrs::seq_encode(const SeqEncode& r, hipStream_t stream) {
  if (r.n_seq == 0) return XNRS_OK;
  XNRS_TRY_RC(check_seq_encode(r));
  const Plan p = make_plan(r.n_seq, r.L, r.D, hidden_of(r), width_of(r), r.att != nullptr, is_additive(r), r.pooled && r.head, r.pooled,
                           r.chunk, r.train, r.att ? r.att->n_heads : 0, r.x16 != nullptr);
  if (p.total > r.ws_bytes || (p.total > 0 && !r.ws)) return XNRS_EWORKSPACE;
  NewsFusedArgs nf{}; AdditiveFusedArgs af{};
  const Route rt = make_route(r, p, &nf, &af);
  Call c{r, stream, p, rt, nf, af};
  if (c.cnt && rt.live && !device_counts_ok(r.x, r.D, c.A, r.att, r.pool)) return XNRS_EUNSUPPORTED;
  XNRS_TRY_RC(prepare_weights(&c));
  XNRS_TRY_RC((rt.fused || rt.afused) ? run_one_launch(c) : run_passes(&c));
  // pooled = Wo (sum_i a_i O_i) + bo (sum_i a_i): one out-projection per sequence (or folded into the head), then the head
  return pooled_tail(rt.fold, c.pob, c.asum, r.att, r.pooled ? r.head : nullptr, c.pb, c.hb, r.y, r.n_seq, r.D, width_of(r), c.po,
                     r.train, stream);
}

namespace {

// ---- unpadded news encoder (inference): workspace carve
struct UnpadPlan {
  size_t off_kv, off_q, off_o, off_y, off_t, off_p, off_h;
  FoldRegions fold;
  size_t total;
};
UnpadPlan make_unpad_plan(int64_t n_news, int64_t n_valid, int S, int D, int A, int E, bool att, bool head) {
  UnpadPlan p{};
  Carver c;
  const size_t nv = (size_t)(n_valid > 0 ? n_valid : 1);
  p.off_kv = c.take_if(att, (size_t)n_news * S * 2 * D * F32);
  p.off_q = c.take_if(att, nv * D * F32);
  p.off_o = c.take_if(att, nv * D * F32);
  p.off_y = c.take_if(att, nv * D * F32);
  p.off_t = c.take(nv * A * F32);
  p.off_p = c.take_if(head, (size_t)n_news * D * F32);
  p.off_h = c.take_if(head, (size_t)n_news * E * F32);
  p.fold = carve_fold(c, att, n_news, D, A);
  p.total = c.total();
  return p;
}

// ---- the padding-free encoder with the row lists built ON THE DEVICE (no host sync: hipGraph-capturable)
struct CompactPlan {
  int64_t chunk;
  size_t off_kv, off_q, off_o, off_t, off_roff, off_live, off_kvs, off_kvb, off_cnt, off_p, off_h;
  FoldRegions fold;
  size_t total;
};
CompactPlan make_compact_plan(int64_t n_news, int S, int D, int A, int E, bool att, bool head, int64_t chunk) {
  CompactPlan p{};
  // default pass: ~262 k token rows (3.2 GB of worst-case scratch at D = 768 -- sized for 288 GB of HBM).  Four times the
  // padded path's pass: the row counts are only known on the device, so every pass pays the latency of its five launches
  // even when most of its rows are dead (tools/bench_compact_chunk.py: 95 % empty news 6.1 -> 3.6 ms per 25 600 news,
  // 50 %: 20.4 -> 18.5 ms; beyond ~10 k news per pass the one-workgroup-per-pass compaction kernel becomes the cost)
  if (chunk <= 0) chunk = 262144 / S;
  if (chunk > n_news) chunk = n_news;
  if (chunk < 1) chunk = 1;
  p.chunk = chunk;
  Carver c;
  const size_t rows = (size_t)chunk * S;  // worst case of a pass: every token live
  p.off_kv = c.take_if(att, rows * 2 * D * F32);
  p.off_q = c.take_if(att, rows * D * F32);
  p.off_o = c.take_if(att, rows * D * F32);
  p.off_t = c.take(rows * (size_t)n_epart(A) * F32);
  const size_t passes = (size_t)((n_news + chunk - 1) / chunk);
  p.off_roff = c.take(passes * ((size_t)chunk + 1) * 8);  // the row lists of EVERY pass (one compaction launch per call)
  p.off_live = c.take(passes * rows * 4);
  p.off_kvs = c.take(passes * rows * 4);
  p.off_kvb = c.take(passes * (size_t)chunk * 4);
  p.off_cnt = c.take(passes * 3 * 8);  // {live rows, K|V rows, bad-mask flag} per pass
  p.off_p = c.take_if(head, (size_t)n_news * D * F32);
  p.off_h = c.take_if(head, (size_t)n_news * E * F32);
  p.fold = carve_fold(c, att, n_news, D, A);
  p.total = c.total();
  return p;
}

SeqEncode padded_call(const float* x, const float* m, int64_t n_seq, int L, int D, float* y, void* ws, size_t ws_bytes) {
  SeqEncode r{};
  r.x = x; r.m = m; r.n_seq = n_seq; r.L = L; r.D = D; r.y = y; r.ws = ws; r.ws_bytes = ws_bytes;
  return r;
}
int32_t news_encode(SeqEncode r, const int32_t* ids, const xnrs_mha_params* att, int32_t pool_kind, const xnrs_additive_params* pool,
                    const xnrs_head_params* head, float* hm, int64_t chunk, void* stream) {
  r.ids = ids; r.att = att; r.pooled = true; r.pool_kind = pool_kind; r.pool = pool; r.head = head; r.hm = hm; r.chunk = chunk;
  r.live_tiles = true;  // empty history slots are news: whole row tiles of a pass may hold nothing else
  return seq_encode(r, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int32_t xnrs_linear_fwd(const float* x, const int32_t* gather_ids, int32_t gather_S, const float* w, const float* bias,
                        float* y, int64_t M, int32_t N, int32_t K, int32_t act, void* stream) {
  if (!x || !w || !y || M < 0 || N <= 0 || K <= 0 || act < 0 || act > 2) return XNRS_EINVAL;
  if (gather_ids && gather_S <= 0) return XNRS_EINVAL;
  return hip_rc(launch_gemm_f32(gemm_linear(x, {gather_ids, gather_S}, K, w, bias, y, N, M, N, K, act), (hipStream_t)stream));
}

size_t xnrs_mha_workspace_bytes(int64_t B, int32_t S, int32_t D) {
  return make_plan(B, S, D, 0, D, true, false, false, false, 0).total;
}

int32_t xnrs_mha_fwd(const float* x, const float* m, const xnrs_mha_params* p, float* y, int64_t B, int32_t S, int32_t D,
                     void* ws, size_t ws_bytes, void* stream) {
  if (!p) return XNRS_EINVAL;
  SeqEncode r = padded_call(x, m, B, S, D, y, ws, ws_bytes);
  r.att = p;
  return seq_encode(r, (hipStream_t)stream);
}

size_t xnrs_additive_workspace_bytes(int64_t B, int32_t N, int32_t D, int32_t A) {
  return make_plan(B, N, D, A, D, false, true, false, true, 0).total;
}

int32_t xnrs_additive_attention_fwd(const float* x, const float* m, const xnrs_additive_params* p, float* y, float* a_out,
                                    int64_t B, int32_t N, int32_t D, void* ws, size_t ws_bytes, void* stream) {
  if (!p) return XNRS_EINVAL;
  SeqEncode r = padded_call(x, m, B, N, D, y, ws, ws_bytes);
  r.pooled = true; r.pool_kind = XNRS_POOL_ADDITIVE; r.pool = p; r.a_out = a_out;
  return seq_encode(r, (hipStream_t)stream);
}

int32_t xnrs_masked_mean_fwd(const float* x, const float* m, float* y, int64_t B, int32_t N, int32_t D, void* stream) {
  SeqEncode r = padded_call(x, m, B, N, D, y, nullptr, 0);
  r.pooled = true; r.pool_kind = XNRS_POOL_MEAN;
  return seq_encode(r, (hipStream_t)stream);
}

size_t xnrs_text_encoder_workspace_bytes(int64_t n_news, int32_t S, int32_t D, int32_t A, int32_t E, int32_t has_att,
                                         int32_t pool_kind, int32_t has_head, int64_t chunk) {
  return make_plan(n_news, S, D, A, E, has_att != 0, pool_kind == XNRS_POOL_ADDITIVE, has_head != 0, true, chunk).total;
}

int32_t xnrs_text_encoder_fwd(const float* x, const float* m, const int32_t* ids, int64_t n_news, int32_t S, int32_t D,
                              const xnrs_mha_params* att, int32_t pool_kind, const xnrs_additive_params* pool,
                              const xnrs_head_params* head, float* y, float* hm, int64_t chunk, void* ws, size_t ws_bytes,
                              void* stream) {
  if (n_news == 0) return XNRS_OK;
  if (!m) return XNRS_EINVAL;  // TextEncoder always receives a token mask (news_encoding.py:41-50)
  return news_encode(padded_call(x, m, n_news, S, D, y, ws, ws_bytes), ids, att, pool_kind, pool, head, hm, chunk, stream);
}

size_t xnrs_text_encoder_bf16_workspace_bytes(int64_t n_news, int32_t S, int32_t D, int32_t A, int32_t E, int32_t has_att,
                                              int32_t pool_kind, int32_t has_head, int64_t chunk) {
  return make_plan(n_news, S, D, A, E, has_att != 0, pool_kind == XNRS_POOL_ADDITIVE, has_head != 0, true, chunk, false, 0, true).total;
}

int32_t xnrs_text_encoder_fwd_bf16(const uint16_t* x_bf16, const float* m, const int32_t* ids, int64_t n_news, int32_t S, int32_t D,
                                   const xnrs_mha_params* att, int32_t pool_kind, const xnrs_additive_params* pool,
                                   const xnrs_head_params* head, float* y, float* hm, int64_t chunk, void* ws, size_t ws_bytes,
                                   void* stream) {
  if (!ids || !x_bf16 || !m) return XNRS_EINVAL;  // a TABLE and its mask, gathered by id: dense bf16 activations are not a feature
  if (n_news == 0) return XNRS_OK;
  SeqEncode r = padded_call(nullptr, m, n_news, S, D, y, ws, ws_bytes);
  r.x16 = x_bf16;
  return news_encode(r, ids, att, pool_kind, pool, head, hm, chunk, stream);
}

size_t xnrs_linear_bf16_workspace_bytes(int32_t N, int32_t K) {
  if (N <= 0 || K <= 0) return 0;
  return carve_total({split_planes_bytes(N, K), (size_t)LINEAR_BF16_WIDEN_ROWS * (size_t)K * F32});
}

int32_t xnrs_linear_fwd_bf16(const uint16_t* x_bf16, const int32_t* gather_ids, int32_t gather_S, const float* w, const float* bias,
                             float* y, int64_t M, int32_t N, int32_t K, int32_t act, void* ws, size_t ws_bytes, void* stream) {
  if (!x_bf16 || !w || !y || M < 0 || N <= 0 || K <= 0 || act < 0 || act > 2) return XNRS_EINVAL;
  if (gather_ids && gather_S <= 0) return XNRS_EINVAL;
  if (M == 0) return XNRS_OK;
  if (!ws || ws_bytes < xnrs_linear_bf16_workspace_bytes(N, K)) return XNRS_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  Carver c;
  unsigned short* planes = at<unsigned short>(ws, c.take(split_planes_bytes(N, K)));
  float* x32 = at(ws, c.take((size_t)LINEAR_BF16_WIDEN_ROWS * (size_t)K * F32));
  GemmArgs g = gemm_linear(nullptr, {gather_ids, gather_S}, K, w, bias, y, N, M, N, K, act, planes);
  if (gemm_a16_ok(g, x_bf16)) {
    XNRS_TRY(launch_split_weights(w, N, K, planes, st));
    return hip_rc(launch_gemm_a16(g, x_bf16, st));
  }
  // widening route: the rows as fp32, LINEAR_BF16_WIDEN_ROWS at a time, through the fp32 launcher (a row's bits do not
  // depend on the rows beside it)
  for (int64_t r0 = 0; r0 < M; r0 += LINEAR_BF16_WIDEN_ROWS) {
    const int64_t nr = M - r0 < LINEAR_BF16_WIDEN_ROWS ? M - r0 : LINEAR_BF16_WIDEN_ROWS;
    XNRS_TRY(launch_gather_rows_bf16(x_bf16, gather_ids, gather_ids ? gather_S : 1, x32, nr, K, st, r0));
    XNRS_TRY(launch_gemm_f32(gemm_linear(x32, {}, K, w, bias, y + r0 * (int64_t)N, N, nr, N, K, act), st));
  }
  return XNRS_OK;
}

size_t xnrs_user_encoder_workspace_bytes(int64_t B, int32_t H, int32_t E, int32_t A, int32_t has_att, int32_t pool_kind,
                                         int32_t has_head) {
  return make_plan(B, H, E, A, E, has_att != 0, pool_kind == XNRS_POOL_ADDITIVE, has_head != 0, true, 0).total;
}

int32_t xnrs_user_encoder_fwd(const float* x, const float* m, int64_t B, int32_t H, int32_t E, const xnrs_mha_params* att,
                              int32_t pool_kind, const xnrs_additive_params* pool, const xnrs_head_params* head, float* y,
                              float* a_out, void* ws, size_t ws_bytes, void* stream) {
  SeqEncode r = padded_call(x, m, B, H, E, y, ws, ws_bytes);
  r.att = att; r.pooled = true; r.pool_kind = pool_kind; r.pool = pool; r.head = head; r.a_out = a_out;
  return seq_encode(r, (hipStream_t)stream);
}

size_t xnrs_text_encoder_unpadded_workspace_bytes(int64_t n_news, int64_t n_valid, int32_t S, int32_t D, int32_t A,
                                                  int32_t E, int32_t has_att, int32_t has_head) {
  return make_unpad_plan(n_news, n_valid, S, D, A, E, has_att != 0, has_head != 0).total;
}

int32_t xnrs_text_encoder_fwd_unpadded(const float* x, const int32_t* ids, int64_t n_news, int32_t S, int32_t D,
                                       const int32_t* rows, const int64_t* row_off, int64_t n_valid,
                                       const xnrs_mha_params* att, const xnrs_additive_params* pool,
                                       const xnrs_head_params* head, float* y, float* hm, void* ws, size_t ws_bytes,
                                       void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_news == 0) return XNRS_OK;
  if (!x || !row_off || !pool || !y || n_news < 0 || n_valid < 0 || S <= 0 || D <= 0 || (n_valid > 0 && !rows))
    return XNRS_EINVAL;
  if (S > 512) return XNRS_EUNSUPPORTED;
  const int A = pool->hidden, E = head ? head->out_features : D;
  if (att) XNRS_TRY_RC(compact_attention_rc(att, S, D));
  const UnpadPlan p = make_unpad_plan(n_news, n_valid, S, D, A, E, att != nullptr, head != nullptr);
  if (p.total > 0 && (!ws || ws_bytes < p.total)) return XNRS_EWORKSPACE;
  float *kv = at(ws, p.off_kv), *qc = at(ws, p.off_q), *oc = at(ws, p.off_o), *yc = at(ws, p.off_y), *tc = at(ws, p.off_t);
  float *pb = at(ws, p.off_p), *hb = at(ws, p.off_h), *pob = at(ws, p.fold.po), *asum = at(ws, p.fold.as);
  const int64_t rows_all = n_news * (int64_t)S;

  const float* vals = x;          // what the pooler weights: compact y rows, or x rows through `rows`
  const int32_t* val_ids = rows;
  const bool fold = att && fold_wanted(knobs().fold_out);
  Fc1 fc1{};
  XNRS_TRY_RC(fc1_pair(fold, att, pool, D, ws, p.fold, stream, &fc1));
  if (att) {
    {  // K and V of EVERY token row: padded tokens stay keys (QUERY-row mask, layers.py:142-144)
      ProfScope ps(0, 2.0 * rows_all * 2.0 * D * D + 2.0 * n_valid * (double)D * D, stream);
      XNRS_TRY(launch_gemm_f32(qkv_projection(x, {ids, S}, att, 1, kv, 2 * (int64_t)D, rows_all, D), stream));
      // Q of the live rows only (row gather through `rows`)
      if (n_valid > 0) XNRS_TRY(launch_gemm_f32(gemm_linear(x, {rows, 1}, D, att->wq, att->bq, qc, D, n_valid, D, D), stream));
    }
    if (n_valid > 0) {
      MhaCoreArgs ma = mha_core_args(kv, 2 * (int64_t)D, att, oc, n_news, S, D);
      ma.q = qc;
      ma.q_off = row_off;
      ma.ldq = D;
      {
        ProfScope ps(1, 4.0 * n_valid * (double)S * D, stream);
        XNRS_TRY(launch_mha_core(ma, stream));
      }
      if (!fold) {
        ProfScope ps(2, 2.0 * n_valid * (double)D * D, stream);
        XNRS_TRY(launch_gemm_f32(gemm_linear(oc, {}, D, att->wo, att->bo, yc, D, n_valid, D, D), stream));
      }
    }
    vals = fold ? oc : yc;
    val_ids = nullptr;
  }
  const bool rowdot = fc1_rowdot_ok(x, att != nullptr, pool, D);
  if (n_valid > 0) {
    ProfScope ps(3, 2.0 * n_valid * (double)D * A, stream);
    XNRS_TRY(launch_gemm_f32(fc1_product(vals, {val_ids, 1}, fc1, tc, n_valid, D, A, rowdot, pool), stream));
  }
  AdditivePoolArgs pa = additive_pool_args(tc, rowdot, pool, vals, n_news, S, D, A);
  pa.row_off = row_off;
  pa.row_ids = val_ids;
  pa.y = pooled_dst(fold, pob, head, pb, y);
  pa.asum_out = fold ? asum : nullptr;
  pa.hm_out = hm;
  {
    ProfScope ps(4, 2.0 * n_valid * (double)(A + D), stream);
    XNRS_TRY(launch_additive_pool(pa, stream));
  }
  return pooled_tail(fold, pob, asum, att, head, pb, hb, y, n_news, D, E, nullptr, false, stream);
}

size_t xnrs_text_encoder_compact_workspace_bytes(int64_t n_news, int32_t S, int32_t D, int32_t A, int32_t E, int32_t has_att,
                                                 int32_t has_head, int64_t chunk) {
  return make_compact_plan(n_news, S, D, A, E, has_att != 0, has_head != 0, chunk).total;
}

int32_t xnrs_text_encoder_fwd_compact(const float* x, const float* m, const int32_t* ids, int64_t n_news, int32_t S, int32_t D,
                                      const xnrs_mha_params* att, const xnrs_additive_params* pool, const xnrs_head_params* head,
                                      float* y, float* hm, int64_t chunk, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_news == 0) return XNRS_OK;
  if (!x || !m || !pool || !pool->w1 || !pool->w2 || !y || n_news < 0 || S <= 0 || D <= 0 || pool->hidden <= 0) return XNRS_EINVAL;
  if (S > 512) return XNRS_EUNSUPPORTED;
  const int A = pool->hidden, E = head ? head->out_features : D;
  if (att) {
    XNRS_TRY_RC(compact_attention_rc(att, S, D));
    if (att->dropout_p != 0.f) return XNRS_EUNSUPPORTED;  // inference only
  }
  // the device row counts ride on the fp32 forward kernel with the fc2 dot in its epilogue (what the padded and the
  // host-compacted paths run too: the three stay bitwise equal)
  if (gemm_mode() != 0 || !fc1_rowdot_ok(x, att != nullptr, pool, D)) return XNRS_EUNSUPPORTED;
  // ... and so do the projections: a product that reads its row count on the device has no scalar-load instantiation, its
  // launch would fail on rows or a projection weight off a 16-byte boundary (the padded entry point serves those)
  if (att && !(aligned16(x) && aligned16(att->wq) && aligned16(att->wk) && aligned16(att->wv))) return XNRS_EUNSUPPORTED;
  const CompactPlan p = make_compact_plan(n_news, S, D, A, E, att != nullptr, head != nullptr, chunk);
  if (!ws || ws_bytes < p.total) return XNRS_EWORKSPACE;
  float *kv = at(ws, p.off_kv), *qc = at(ws, p.off_q), *oc = at(ws, p.off_o), *tc = at(ws, p.off_t);
  int64_t *roff0 = at<int64_t>(ws, p.off_roff), *cnt0 = at<int64_t>(ws, p.off_cnt);
  int32_t *live0 = at<int32_t>(ws, p.off_live), *kvs0 = at<int32_t>(ws, p.off_kvs), *kvb0 = at<int32_t>(ws, p.off_kvb);
  float *pb = at(ws, p.off_p), *hb = at(ws, p.off_h), *pob = at(ws, p.fold.po), *asum = at(ws, p.fold.as);
  const bool fold = att && fold_wanted(knobs().fold_out);
  Fc1 fc1{};
  XNRS_TRY_RC(fc1_pair(fold, att, pool, D, ws, p.fold, stream, &fc1));
  if (att && !fold) return XNRS_EUNSUPPORTED;  // (the per-token out-projection order: use the host-compacted entry point)
  XNRS_TRY(launch_compact_rows(m, ids, n_news, p.chunk, S, roff0, live0, kvs0, kvb0, cnt0, stream));
  for (int64_t c0 = 0; c0 < n_news; c0 += p.chunk) {
    const int64_t nc = (n_news - c0 < p.chunk) ? (n_news - c0) : p.chunk;
    const int64_t rows = nc * S;  // worst case
    const int64_t pass = c0 / p.chunk;
    const int64_t* cnt = cnt0 + 3 * pass;
    const int64_t* roff = roff0 + pass * (p.chunk + 1);
    const int32_t* live = live0 + pass * p.chunk * S;
    const int32_t* kvs = kvs0 + pass * p.chunk * S;
    const int32_t* kvb = kvb0 + pass * p.chunk;
    const float* vals = x;           // what the pooler weights: compact O rows, or x rows through `live`
    const int32_t* val_ids = live;
    if (att) {
      {  // K and V of every token of the news that have a live token: rows gathered through the device list, written as
         // consecutive S-row blocks (the attention kernel finds a news' block through kv_block: no row scatter)
        GemmArgs g = qkv_projection(x, {kvs, 1}, att, 1, kv, 2 * (int64_t)D, rows, D);
        g.m_dev = cnt + 1;
        ProfScope ps(0, 2.0 * rows * 3.0 * D * D, stream);  // (worst case: the row counts live on the device)
        XNRS_TRY(launch_gemm_f32(g, stream));
        GemmArgs q = gemm_linear(x, {live, 1}, D, att->wq, att->bq, qc, D, rows, D, D);
        q.m_dev = cnt;
        XNRS_TRY(launch_gemm_f32(q, stream));
      }
      MhaCoreArgs ma = mha_core_args(kv, 2 * (int64_t)D, att, oc, nc, S, D);
      ma.q = qc;
      ma.q_off = roff;
      ma.ldq = D;
      ma.kv_block = kvb;
      {
        ProfScope ps(1, 4.0 * rows * (double)S * D, stream);
        XNRS_TRY(launch_mha_core(ma, stream));
      }
      vals = oc;
      val_ids = nullptr;
    }
    {
      ProfScope ps(3, 2.0 * rows * (double)D * A, stream);
      GemmArgs fg = fc1_product(vals, {val_ids, 1}, fc1, tc, rows, D, A, true, pool);
      fg.m_dev = cnt;
      XNRS_TRY(launch_gemm_f32(fg, stream));
    }
    AdditivePoolArgs pa = additive_pool_args(tc, true, pool, vals, nc, S, D, A);
    pa.row_off = roff;
    pa.row_ids = val_ids;
    pa.poison = cnt + 2;  // a mask value other than 0 / 1: NaN out, not a silently different result
    pa.y = pooled_dst(fold, pob, head, pb, y) + c0 * (int64_t)D;
    pa.asum_out = fold ? asum + c0 : nullptr;
    pa.hm_out = hm ? hm + c0 : nullptr;
    {
      ProfScope ps(4, 2.0 * rows * (double)(A + D), stream);
      XNRS_TRY(launch_additive_pool(pa, stream));
    }
  }
  XNRS_TRY_RC(pooled_tail(fold, pob, asum, att, head, pb, hb, y, n_news, D, E, nullptr, false, stream));
  // a mask value other than 0 / 1 in any pass: NaN over the whole result (a ReLU head would swallow a NaN fed in earlier)
  const int n_pass = (int)((n_news + p.chunk - 1) / p.chunk);
  XNRS_TRY(launch_poison(y, n_news * (int64_t)E, cnt0 + 2, n_pass, 3, stream));
  if (hm) XNRS_TRY(launch_poison(hm, n_news, cnt0 + 2, n_pass, 3, stream));
  return XNRS_OK;
}

size_t xnrs_fold_weights_workspace_bytes(int32_t D, int32_t A) {
  return D > 0 && A > 0 ? align_up((size_t)FOLD_SPLITS * A * D * sizeof(float)) : 0;
}

int32_t xnrs_fold_weights(const xnrs_mha_params* att, const xnrs_additive_params* pool, int32_t D, float* w1f, float* b1f,
                          void* ws, size_t ws_bytes, void* stream) {
  if (!att || !pool || !att->wo || !pool->w1 || pool->hidden <= 0 || D <= 0 || !w1f || !b1f) return XNRS_EINVAL;
  if (ws_bytes < xnrs_fold_weights_workspace_bytes(D, pool->hidden) || !ws) return XNRS_EWORKSPACE;
  hipError_t fe = hipSuccess;
  const float* b = fold_out_projection(att, pool, D, pool->hidden, w1f, b1f, static_cast<float*>(ws), (hipStream_t)stream, &fe);
  XNRS_TRY(fe);
  if (b != b1f) {  // no out-projection bias: b1 as it is (or zeros)
    if (pool->b1) XNRS_TRY(hipMemcpyAsync(b1f, pool->b1, (size_t)pool->hidden * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    else XNRS_TRY(hipMemsetAsync(b1f, 0, (size_t)pool->hidden * sizeof(float), (hipStream_t)stream));
  }
  return XNRS_OK;
}

size_t xnrs_fold_head_weights_workspace_bytes(int32_t D, int32_t E) {  // (unaligned, unlike xnrs_fold_weights_workspace_bytes)
  return (D > 0 && E > 0) ? (size_t)FOLD_SPLITS * (size_t)E * (size_t)D * sizeof(float) : 0;
}

int32_t xnrs_fold_head_weights(const xnrs_mha_params* att, const xnrs_head_params* head, int32_t D, float* w0f, float* b0v,
                               void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!att || !head || !att->wo || !head->w0 || !w0f || D <= 0 || head->out_features <= 0) return XNRS_EINVAL;
  if (att->bo && !b0v) return XNRS_EINVAL;
  const int E = head->out_features;
  if (ws_bytes < xnrs_fold_head_weights_workspace_bytes(D, E) || !ws) return XNRS_EWORKSPACE;
  XNRS_TRY(fold_product(head->w0, E, att->wo, D, w0f, static_cast<float*>(ws), stream));  // w0f = W0 . Wo
  if (att->bo) XNRS_TRY(launch_fold_bias(head->w0, att->bo, nullptr, b0v, E, D, stream));  // b0v = W0 . bo
  return XNRS_OK;
}

}  // extern "C"
