/*
 * xnrs_hip.h -- C ABI of libxnrs_hip.so: the MI355X (gfx950) implementation of the xnrs
 * user-news scoring hot path (news encode -> user encode -> dot-product score).
 *
 * The reference (tan9zj/xnrs) is 100% Python/PyTorch and defines NO FFI of its own; its interface
 * for this path is the `xnrs.models.components` module API.  Every entry point below therefore
 * cites the reference *method* it replaces (file:line relative to the reference repo root); the
 * Python host side (xnrs_amd/models/...) keeps the reference's class names, constructor
 * signatures and state_dict keys and binds these symbols with ctypes.
 *
 * Conventions
 *   - all tensors are contiguous row-major fp32 DEVICE pointers unless stated; masks are fp32 0/1
 *     exactly like the reference (news_encoding.py:34-50); ids are int32 device pointers.
 *   - nn.Linear weights keep the reference layout W[out][in] (K-contiguous), bias[out] or NULL.
 *   - no device-memory allocation and no host sync: the caller supplies the workspace (size from the
 *     *_workspace_bytes query) and a hipStream_t (as void*; NULL = default stream).  Safe to capture
 *     into a hipGraph.  Every result of a call is ordered on THAT stream when the call returns; the
 *     backward entry points may fork weight-gradient launches onto a library-owned stream and join
 *     them back by events inside the call (one stream + 32 events per device, created at the first
 *     eager backward; XNRS_BWD_SIDE_STREAM=0: never).
 *   - alignment: an operand pointer (inputs, weights, outputs, gradients) needs the 4 bytes of its element type and no
 *     more (2 for bf16 rows); the launchers look at every address and take scalar loads and stores, or the unfused route,
 *     where an operand is not on a 16-byte boundary -- slower, the same results (tests/test_hip_pointer_alignment.py).
 *     A WORKSPACE is different: every `ws` and `saved` pointer, and every pointer derived from one with a *_offset query
 *     (xnrs_row_lists::qkv_shared), must be 256-byte aligned.  The library carves these buffers into regions aligned
 *     relative to their base and its 16-byte vector kernels rely on that; the base itself is not checked.
 *   - process-global state (documented at its entry points, nothing else exists): the forward-GEMM
 *     arithmetic mode (xnrs_set_gemm_mode), the development knobs (xnrs_reload_knobs), the optional
 *     launch timer (xnrs_profile_*), the status word (xnrs_set_status_word) and that side stream.  Encode / score calls on different streams may run from different
 *     threads; changing one of the three while another thread launches is the caller's race.
 *   - return value: 0 = ok; >0 = hipError_t of the failed launch; <0 = XNRS_E* argument error.
 *     xnrs_error_string() explains either.
 */
#ifndef XNRS_HIP_H
#define XNRS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XNRS_ABI_VERSION 6

#define XNRS_OK 0
#define XNRS_EINVAL (-1)     /* bad shape / NULL pointer */
#define XNRS_EHEADS (-2)     /* d_model % n_heads != 0 (reference raises RuntimeError, layers.py:111,133) */
#define XNRS_EWORKSPACE (-3) /* workspace too small */
#define XNRS_EUNSUPPORTED (-4)

/* activation fused into a Linear's epilogue */
#define XNRS_ACT_NONE 0
#define XNRS_ACT_RELU 1
#define XNRS_ACT_TANH 2

/* pooler kinds */
#define XNRS_POOL_ADDITIVE 0 /* layers.AdditiveAttention (layers.py:40-69) */
#define XNRS_POOL_MEAN 1     /* layers.MaskedMean        (layers.py:19-37) */

/* layers.MultiHeadAttention parameters (layers.py:106-118): four Linear(D,D) */
typedef struct {
  const float *wq, *bq, *wk, *bk, *wv, *bv, *wo, *bo;
  int32_t n_heads;
  int32_t scaled;   /* 1: scores / sqrt(d_k) (layers.py:139-140) */
  float dropout_p;  /* attention-probability dropout (layers.py:117,148); 0 in eval mode */
  uint64_t seed;    /* counter-based RNG seed for dropout; ignored when dropout_p == 0 */
  /* ABI 6, optional: a DEVICE word added to `seed` by the kernels (forward and backward read it; the caller must not change
   * it between a training forward and its backward).  A grad step captured in a hipGraph bakes `seed` into the graph; with
   * this word -- incremented by the caller inside the captured step -- every replay draws a fresh attention-dropout mask
   * (layers.py:148 draws one per call).  NULL: seed alone. */
  const uint64_t *seed_dev;
} xnrs_mha_params;

/* layers.AdditiveAttention parameters (layers.py:42-45): fc1 Linear(D,A), fc2 Linear(A,1).
 * w1_folded / b1_folded (optional; ABI version 3; the training entry points take them too since round 4 -- the backward
 * call must then be given the same pair as its forward): fc1 folded behind the out-projection of
 * the attention stage passed IN THE SAME CALL -- W1.Wo [A,D] and W1.bo + b1 [A], as xnrs_fold_weights computes them
 * (DESIGN.md section 4.6).  The library keeps no state between calls, so without them every call rebuilds the pair
 * (three short launches, ~20 us); a caller that encodes with the same weights again and again computes them once
 * (xnrs_amd/hip.py caches them per module and weight version).  NULL = rebuilt per call; the bits are the same. */
typedef struct {
  const float *w1, *b1, *w2, *b2;
  int32_t hidden; /* A */
  const float *w1_folded, *b1_folded;
} xnrs_additive_params;

/* nn.Sequential(Linear(in,out), activation, Linear(out,out)) head
 * (news_encoding.py:25-31, user_encoding.py:30-34); biases may be NULL (bias=False).
 * activation: XNRS_ACT_RELU (the reference's default nn.ReLU()), XNRS_ACT_TANH or XNRS_ACT_NONE -- the three the GEMM
 * epilogue and its backward implement; the Python mirror refuses any other `activation` module (ABI version 2 added
 * this field). */
typedef struct {
  const float *w0, *b0, *w2, *b2;
  int32_t out_features;
  int32_t activation;
  /* ABI 6, optional, inference entry points with an attention stage + additive pooler in the same call: the head's first
   * layer folded behind the out-projection (layers.py:154 under news_encoding.py:27-31),
   *   w0_folded [E, D] = W0 . Wo      b0_rowvec [E] = W0 . bo      (xnrs_fold_head_weights; exact algebra)
   * so that the per-news out-projection product disappears: head_1 = act((W0 Wo) po + (W0 bo) s + b0) with po the pooled
   * attention rows and s the sum of the pooling weights.  NULL = out-projection, then the head as written. */
  const float *w0_folded, *b0_rowvec;
} xnrs_head_params;

int32_t xnrs_abi_version(void);
/* Hash of the sources this binary was built from (every .hip file of xnrs_amd/csrc, kernels.h, this header; the Makefile computes
 * it): lets a reader tell the measured binary from the tree without a rebuild (tests/test_abi.py, bench.py). */
const char *xnrs_build_id(void);
const char *xnrs_error_string(int32_t code);

/* ---- nn.Linear (layers.py:60,128-130,154; news_encoding.py:27-31) --------------------------
 * y[M,N] = act(x[M,K] . w[N,K]^T + bias[N]).  If gather_ids != NULL, logical row m of x is row
 * gather_ids[m / gather_S] * gather_S + m % gather_S of the table `x` (device-resident news-token
 * table [n_news,S,D] + id gather fused into the load: SURVEY.md section 8 a0). */
int32_t xnrs_linear_fwd(const float *x, const int32_t *gather_ids, int32_t gather_S, const float *w,
                        const float *bias, float *y, int64_t M, int32_t N, int32_t K, int32_t act,
                        void *stream);

/* ---- layers.MultiHeadAttention.forward (layers.py:120-156) ---------------------------------
 * x:(B,S,D), m:(B,S) fp32 0/1 or NULL -> y:(B,S,D).  Row-mask semantics of layers.py:142-144. */
size_t xnrs_mha_workspace_bytes(int64_t B, int32_t S, int32_t D);
int32_t xnrs_mha_fwd(const float *x, const float *m, const xnrs_mha_params *p, float *y, int64_t B,
                     int32_t S, int32_t D, void *ws, size_t ws_bytes, void *stream);

/* ---- layers.AdditiveAttention.forward (layers.py:47-69) ------------------------------------
 * x:(B,N,D), m:(B,N) or NULL -> y:(B,D); a_out:(B,N) optional attention weights (return_weights). */
size_t xnrs_additive_workspace_bytes(int64_t B, int32_t N, int32_t D, int32_t A);
int32_t xnrs_additive_attention_fwd(const float *x, const float *m, const xnrs_additive_params *p,
                                    float *y, float *a_out, int64_t B, int32_t N, int32_t D, void *ws,
                                    size_t ws_bytes, void *stream);

/* ---- layers.MaskedMean.forward (layers.py:26-37) : y = sum(x*m)/(sum(m)+1e-8) -------------- */
int32_t xnrs_masked_mean_fwd(const float *x, const float *m, float *y, int64_t B, int32_t N, int32_t D,
                             void *stream);

/* ---- xnrs.utils.collaps_mask (utils.py:74-75): hm = clamp(sum_S m, 0, 1) ------------------- */
int32_t xnrs_collapse_mask(const float *m, float *hm, int64_t n_rows, int32_t S, void *stream);

/* ---- TextEncoder.forward (news_encoding.py:34-60) -------------------------------------------
 * x:(n_news,S,D) [or table + ids, see xnrs_linear_fwd], m:(n_news,S) -> y:(n_news,E'), hm:(n_news).
 * att == NULL: no self-attention stage; head == NULL: y is the pooled D-vector (E' = D).
 * If ids != NULL, x and m are the TABLE ([n_table,S,D], [n_table,S]) and n_news = len(ids).
 * `chunk` = news per internal pass (bounds the workspace; 0 = library default).
 * With an attention stage and the additive pooler the out-projection (layers.py:154) is applied once per news behind
 * the pooling (exact algebra); <= 32 tokens and D <= 320 run as one fused kernel (section 4.4). */
size_t xnrs_text_encoder_workspace_bytes(int64_t n_news, int32_t S, int32_t D, int32_t A, int32_t E,
                                         int32_t has_att, int32_t pool_kind, int32_t has_head,
                                         int64_t chunk);
int32_t xnrs_text_encoder_fwd(const float *x, const float *m, const int32_t *ids, int64_t n_news,
                              int32_t S, int32_t D, const xnrs_mha_params *att, int32_t pool_kind,
                              const xnrs_additive_params *pool, const xnrs_head_params *head, float *y,
                              float *hm, int64_t chunk, void *ws, size_t ws_bytes, void *stream);

/* ---- a news table STORED in bf16 (NewsStore.astype(torch.bfloat16)) -----------------------
 * bf16 values are passed as const uint16_t * (the high half of the fp32 value; widening is bits << 16, exact).
 *
 * xnrs_linear_fwd_bf16: the twin of xnrs_linear_fwd over bf16 rows x (pitch K elements; gather_ids / gather_S as there),
 * w, bias and y in fp32.  With K % 8 == 0, a 16-byte aligned x and a launch of at least XNRS_GEMM_SPLIT_MIN_TILES 128 x 128
 * tiles (and XNRS_GEMM_A16 != 0) the product runs on the bf16 matrix cores against the exact three-way bf16 split of w --
 * x.w = x.wh + x.wm + x.wl with fp32 accumulation: fp32-grade, whatever xnrs_set_gemm_mode says; one tile shape, so a row's
 * bits do not depend on the batch.  Otherwise the rows are widened to fp32, 1024 at a time, and take xnrs_linear_fwd's route.
 * ws: xnrs_linear_bf16_workspace_bytes(N, K) of scratch (the weight planes and the widening buffer). */
size_t xnrs_linear_bf16_workspace_bytes(int32_t N, int32_t K);
int32_t xnrs_linear_fwd_bf16(const uint16_t *x_bf16, const int32_t *gather_ids, int32_t gather_S, const float *w,
                             const float *bias, float *y, int64_t M, int32_t N, int32_t K, int32_t act, void *ws,
                             size_t ws_bytes, void *stream);

/* xnrs_text_encoder_fwd over a bf16 TABLE: x is [n_table,S,D] bf16, m the table's fp32 mask, ids required (NULL ids:
 * XNRS_EINVAL, nothing is written -- dense bf16 activations are not a feature).  Two routes:
 *   direct    an attention tower with the additive pooler on the GEMM pipeline projects Q|K|V of every pass straight from the
 *             bf16 rows (the product of xnrs_linear_fwd_bf16, over the live row tiles where the fp32 call would walk them);
 *             everything behind the projection is the fp32 call's.  Results agree with the fp32 call on the widened table to
 *             fp32 rounding (the bf16x3 bar).  XNRS_GEMM_A16=0, or a shape the kernel refuses: the widening route.
 *   widening  everything else (attention-free towers, mean pooling, the fused short-title kernels): the rows of each pass are
 *             widened into the workspace and the fp32 route runs on them -- bit for bit xnrs_text_encoder_fwd on the
 *             widened table with the same ids.
 * The whole table is never converted.  Workspace: xnrs_text_encoder_bf16_workspace_bytes (the fp32 call's plus one pass of
 * fp32 rows and mask rows). */
size_t xnrs_text_encoder_bf16_workspace_bytes(int64_t n_news, int32_t S, int32_t D, int32_t A, int32_t E,
                                              int32_t has_att, int32_t pool_kind, int32_t has_head, int64_t chunk);
int32_t xnrs_text_encoder_fwd_bf16(const uint16_t *x_bf16, const float *m, const int32_t *ids, int64_t n_news,
                                   int32_t S, int32_t D, const xnrs_mha_params *att, int32_t pool_kind,
                                   const xnrs_additive_params *pool, const xnrs_head_params *head, float *y,
                                   float *hm, int64_t chunk, void *ws, size_t ws_bytes, void *stream);

/* The folded fc1 of an (attention stage, additive pooler) pair, for xnrs_additive_params.w1_folded / b1_folded:
 *   w1f [A, D] = W1 . Wo      b1f [A] = W1 . bo + b1      (layers.py:154 behind layers.py:60, exact algebra)
 * ws: xnrs_fold_weights_workspace_bytes(D, A) of scratch. */
size_t xnrs_fold_weights_workspace_bytes(int32_t D, int32_t A);
int32_t xnrs_fold_weights(const xnrs_mha_params *att, const xnrs_additive_params *pool, int32_t D, float *w1f, float *b1f,
                          void *ws, size_t ws_bytes, void *stream);

/* The folded first head layer for xnrs_head_params.w0_folded / b0_rowvec (b0v may be NULL when att->bo is NULL).
 * ws: xnrs_fold_head_weights_workspace_bytes(D, E) of scratch. */
size_t xnrs_fold_head_weights_workspace_bytes(int32_t D, int32_t E);
int32_t xnrs_fold_head_weights(const xnrs_mha_params *att, const xnrs_head_params *head, int32_t D, float *w0f, float *b0v,
                               void *ws, size_t ws_bytes, void *stream);

/* ---- TextEncoder.forward without the padding work (inference) --------------------------------
 * Same result as xnrs_text_encoder_fwd for 0/1 masks, computing only what can reach the output
 * (news_encoding.py:34-60 + layers.py:47-69,120-156): a masked token row has pooling weight exp(e)*0, so its
 * query projection, attention row, output projection and fc1 row are dead; as a KEY it is alive (the reference
 * masks query rows only, layers.py:142-144), so K and V are still projected for every row.
 *   rows    : int32 [n_valid]   source token row (row of x viewed as [*, D]) of every unmasked token, in order
 *   row_off : int64 [n_news+1]  news n owns the compact rows row_off[n] .. row_off[n+1]; row_off[n_news] = n_valid
 * x is (n_news,S,D), or the table when ids != NULL (ids: table row of each news, used for K/V; `rows` then holds
 * table token rows).  att may be NULL (additive-only towers); the pooler is the additive one.  One pass (the
 * caller bounds n_news per call); hm[n] = (row_off[n+1] > row_off[n]).  Requires S <= 64 and d_k <= 64, d_k % 4 == 0
 * when att != NULL (XNRS_EUNSUPPORTED otherwise -- use the padded entry point). */
size_t xnrs_text_encoder_unpadded_workspace_bytes(int64_t n_news, int64_t n_valid, int32_t S, int32_t D, int32_t A,
                                                  int32_t E, int32_t has_att, int32_t has_head);
int32_t xnrs_text_encoder_fwd_unpadded(const float *x, const int32_t *ids, int64_t n_news, int32_t S, int32_t D,
                                       const int32_t *rows, const int64_t *row_off, int64_t n_valid,
                                       const xnrs_mha_params *att, const xnrs_additive_params *pool,
                                       const xnrs_head_params *head, float *y, float *hm, void *ws, size_t ws_bytes,
                                       void *stream);

/* ---- the same, with the row lists built ON THE DEVICE (ABI version 3) --------------------------------
 * xnrs_text_encoder_fwd_unpadded needs the compact row lists and their count from the host (one device->host read of the
 * counts per call).  This entry point takes the padded inputs of xnrs_text_encoder_fwd (x / m, or a table + ids) and
 * compacts on the device: per pass of `chunk` news a single-workgroup kernel builds the CSR offsets, the live-row list
 * and the list of token rows of the non-empty news (an all-masked news has no live query, so its K / V are never read
 * and are not projected either); the GEMMs are launched over the worst-case row count and read the real one from
 * device memory (tiles past it return at once).  No host sync, no data-dependent launch: the whole call can be captured
 * in a hipGraph.  0/1 masks are a PRECONDITION here (not checked: that would be the host read this entry point exists to
 * avoid); inference, additive pooler, fp32 GEMM mode, S <= 512 -- and with an attention stage S <= 64, head width <= 64 and
 * a multiple of 4 (XNRS_EUNSUPPORTED otherwise: use xnrs_text_encoder_fwd).  Results equal xnrs_text_encoder_fwd bit for
 * bit for prefix masks, at every S up to 512 (tests/test_hip_length_limits.py holds it beyond 64 tokens). */
size_t xnrs_text_encoder_compact_workspace_bytes(int64_t n_news, int32_t S, int32_t D, int32_t A, int32_t E,
                                                 int32_t has_att, int32_t has_head, int64_t chunk);
int32_t xnrs_text_encoder_fwd_compact(const float *x, const float *m, const int32_t *ids, int64_t n_news, int32_t S,
                                      int32_t D, const xnrs_mha_params *att, const xnrs_additive_params *pool,
                                      const xnrs_head_params *head, float *y, float *hm, int64_t chunk, void *ws,
                                      size_t ws_bytes, void *stream);

/* ---- UserEncoder.forward (user_encoding.py:50-81) -------------------------------------------
 * x:(B,H,E), m:(B,H) -> y:(B,E) [, a_out:(B,H) when the pooler is additive and a_out != NULL]. */
size_t xnrs_user_encoder_workspace_bytes(int64_t B, int32_t H, int32_t E, int32_t A, int32_t has_att,
                                         int32_t pool_kind, int32_t has_head);
int32_t xnrs_user_encoder_fwd(const float *x, const float *m, int64_t B, int32_t H, int32_t E,
                              const xnrs_mha_params *att, int32_t pool_kind,
                              const xnrs_additive_params *pool, const xnrs_head_params *head, float *y,
                              float *a_out, void *ws, size_t ws_bytes, void *stream);

/* ---- DotScoring.forward (scoring.py:12-23) --------------------------------------------------
 * u:(B,E), c:(B,C,E) -> r:(B,C); normalize != 0 applies the L2 normalisation of scoring.py:20-22. */
int32_t xnrs_dot_scoring_fwd(const float *u, const float *c, float *r, int64_t B, int32_t C, int32_t E,
                             int32_t normalize, void *stream);

/* ---- training: forward that keeps its activations + backward --------------------------------
 * Autograd of the sequence-encoder pipeline (TextEncoder news_encoding.py:34-60, UserEncoder
 * user_encoding.py:50-81, and their parts when pool_kind == XNRS_POOL_NONE / att == NULL), as needed by
 * the grad step (training.py:402-431: loss.backward()) and by integrated gradients (explain.py:160-166,
 * which needs d score / d x).
 *   fwd_train : same arithmetic as xnrs_text_encoder_fwd / xnrs_user_encoder_fwd, one pass (no chunking),
 *               intermediates are kept in the caller's `saved` buffer (xnrs_seq_encoder_saved_bytes).
 *   bwd       : dy:(n_seq,E') [pool_kind == XNRS_POOL_NONE: (n_seq,L,D)] -> parameter gradients (each
 *               pointer of the *_grads structs may be NULL = not wanted; values are WRITTEN, not
 *               accumulated) and, if dx != NULL, the input gradient dx:(n_seq,L,D) (not available with
 *               ids: a gathered table gets no gradient).  Deterministic: no float atomics. */
#define XNRS_POOL_NONE (-1) /* no pooler: y = att(x), the MultiHeadAttention module alone */
typedef struct {
  float *wq, *bq, *wk, *bk, *wv, *bv, *wo, *bo;
} xnrs_mha_grads;
typedef struct {
  float *w1, *b1, *w2, *b2;
} xnrs_additive_grads;
typedef struct {
  float *w0, *b0, *w2, *b2;
} xnrs_head_grads;

size_t xnrs_seq_encoder_saved_bytes(int64_t n_seq, int32_t L, int32_t D, int32_t A, int32_t E, int32_t n_heads,
                                    int32_t pool_kind, int32_t has_head);
int32_t xnrs_seq_encoder_fwd_train(const float *x, const float *m, const int32_t *ids, int64_t n_seq, int32_t L,
                                   int32_t D, const xnrs_mha_params *att, int32_t pool_kind,
                                   const xnrs_additive_params *pool, const xnrs_head_params *head, float *y,
                                   float *a_out, float *hm, void *saved, size_t saved_bytes, void *stream);
/* The same forward computing only what can reach the output or a gradient (optional; identical results): with
 * live_rows / live_src_rows / n_live as in xnrs_seq_encoder_bwd_live below, the query projection, the output projection
 * and fc1 run over the unmasked token rows in place and the masked rows of Q, Y and T are stored as zeros (a masked
 * row's pooling weight is exp(e) * 0: nothing downstream, forward or backward, depends on its values; K and V stay
 * dense because the reference masks query rows only, layers.py:142-144).  Used with additive pooling + a mask: with an
 * attention tower as described; without one (StandardRec, NAML's views) fc1 runs over the live rows of x and T of the
 * masked rows is zero.  live_rows == NULL = xnrs_seq_encoder_fwd_train. */
int32_t xnrs_seq_encoder_fwd_train_live(const float *x, const float *m, const int32_t *ids, int64_t n_seq, int32_t L,
                                        int32_t D, const xnrs_mha_params *att, int32_t pool_kind,
                                        const xnrs_additive_params *pool, const xnrs_head_params *head, float *y,
                                        float *a_out, float *hm, void *saved, size_t saved_bytes,
                                        const int32_t *live_rows, const int32_t *live_src_rows, int64_t n_live,
                                        void *stream);
size_t xnrs_seq_encoder_bwd_workspace_bytes(int64_t n_seq, int32_t L, int32_t D, int32_t A, int32_t E,
                                            int32_t n_heads, int32_t pool_kind, int32_t has_head);
int32_t xnrs_seq_encoder_bwd(const float *x, const float *m, const int32_t *ids, int64_t n_seq, int32_t L, int32_t D,
                             const xnrs_mha_params *att, int32_t pool_kind, const xnrs_additive_params *pool,
                             const xnrs_head_params *head, const void *saved, size_t saved_bytes, const float *dy,
                             float *dx, const xnrs_mha_grads *g_att, const xnrs_additive_grads *g_pool,
                             const xnrs_head_grads *g_head, void *ws, size_t ws_bytes, void *stream);
/* The same backward over the unmasked token rows only (optional speed-up of the grad step; identical gradients up to
 * summation order).  A masked token row has pooling weight exp(e)*0, so every gradient that flows through it is
 * exactly zero; with live_rows (int32 [n_live]: indices of the unmasked rows in the padded [n_seq*L] row space, in
 * order) the row-parallel products of the attention tower -- fc1, output projection, Q projection -- run over those
 * rows in place; K / V gradients stay dense (padded tokens are keys, layers.py:142-144).  live_src_rows: the rows of
 * the live tokens in x when ids != NULL (table rows), NULL otherwise.  Used with additive pooling + a mask (without an
 * attention tower: dW1 and the input gradient's fc1 term over the live rows); ignored (= xnrs_seq_encoder_bwd) otherwise. */
int32_t xnrs_seq_encoder_bwd_live(const float *x, const float *m, const int32_t *ids, int64_t n_seq, int32_t L, int32_t D,
                                  const xnrs_mha_params *att, int32_t pool_kind, const xnrs_additive_params *pool,
                                  const xnrs_head_params *head, const void *saved, size_t saved_bytes, const float *dy,
                                  float *dx, const xnrs_mha_grads *g_att, const xnrs_additive_grads *g_pool,
                                  const xnrs_head_grads *g_head, const int32_t *live_rows,
                                  const int32_t *live_src_rows, int64_t n_live, void *ws, size_t ws_bytes, void *stream);

/* Both row lists of the grad step in one argument (ABI 4).  live_* as above.  kv_rows (int32 [n_kv], optional, rides on
 * the live-row path): the token rows -- masked ones included -- of the news that have at least one unmasked token, in
 * order.  The keys and values of a news are read by that news' own queries only, and an all-masked news (an empty history
 * slot, dataset.py:82-85) has no live query: its K and V rows reach neither the output nor a gradient, and its dK / dV
 * rows are exactly zero.  With the list the K|V projection of the forward and the dWk / dWv products of the backward run
 * over those rows only (K and V of the other rows are stored as zeros).  kv_src_rows: the same tokens' rows in x when
 * ids != NULL.  Identical results up to summation order; a NULL list pointer = the plain entry points. */
typedef struct {
  const int32_t *live_rows, *live_src_rows;
  int64_t n_live;
  const int32_t *kv_rows, *kv_src_rows;
  int64_t n_kv;
  /* ABI 5, optional: the Q|K|V image ([n_seq*L, 3D] fp32) of ANOTHER training forward over the same input, ids, mask,
   * row lists and projection weights -- the address of its saved blob + xnrs_seq_encoder_saved_qkv_offset().  The
   * reference's train step encodes the history twice (training.py:406,409) and, with input dropout 0 (every shipped
   * config), the two encodes differ only in their attention-dropout draws: the second forward then skips its Q/K/V
   * projection and reads the first one's image, and so does its backward (which still computes its own dQ|dK|dV and weight
   * gradients).  Identical results, bit for bit.  The caller keeps the other blob alive until this forward's backward
   * has run.  NULL: project as usual. */
  const float *qkv_shared;
  /* ABI 6, optional: the two counts as DEVICE scalars, int64 counts_dev[2] = {n_live, n_kv} (xnrs_build_row_lists writes
   * them).  n_live / n_kv above are then only the capacities of the lists (n_seq * L); every product over a list reads
   * its row count on the device, so the caller never reads the counts back: no host synchronisation in the grad step, and
   * its launch sequence does not depend on the data (hipGraph-capturable).  fp32 GEMM mode, 16-byte aligned operands and
   * D, A multiples of 4 (XNRS_EUNSUPPORTED otherwise: pass host counts). */
  const int64_t *counts_dev;
  /* ABI 6, optional, backward only: ONE weight-gradient product per projection for two backward calls over the same
   * Q|K|V image (qkv_shared above: the reference's two history encodes, training.py:406,409) --
   *   dW = (dQKV_1 + dQKV_2)^T . X   instead of   dQKV_1^T . X + dQKV_2^T . X   (layers.py:128-130 under autograd).
   * dqkv_image: caller-owned [n_seq*L, 3D] fp32.  dqkv_mode XNRS_DQKV_DEFER: this call leaves its dQ|dK|dV there and
   * computes NO gradient of wq/bq/wk/bk/wv/bv (and no input gradient); XNRS_DQKV_MERGE: this call ADDS its dQ|dK|dV to
   * the image and computes those gradients from the sum.  Both calls must pass the same row lists.  Rows of all-masked
   * sequences / masked queries that the lists never reach may stay unwritten. */
  float *dqkv_image;
  int32_t dqkv_mode;
} xnrs_row_lists;
#define XNRS_DQKV_OWN 0
#define XNRS_DQKV_DEFER 1
#define XNRS_DQKV_MERGE 2

/* The row lists of xnrs_row_lists built on the device from the mask (m: (n_seq, L) fp32, or the table's mask with ids):
 * live_rows / kv_rows: int32 [n_seq * L] each (capacity; the first counts[0] / counts[1] entries are written, in row
 * order -- what torch.nonzero gives); live_src_rows / kv_src_rows: the same tokens' rows in the table (required with ids,
 * NULL otherwise); counts: int64 [2] = {n_live, n_kv}.  ws: xnrs_row_lists_workspace_bytes(n_seq).  Two short launches,
 * no host synchronisation.  A token is live when its mask value is != 0 (as the host bookkeeping had it). */
size_t xnrs_row_lists_workspace_bytes(int64_t n_seq);
int32_t xnrs_build_row_lists(const float *m, const int32_t *ids, int64_t n_seq, int32_t L, int32_t *live_rows,
                             int32_t *live_src_rows, int32_t *kv_rows, int32_t *kv_src_rows, int64_t *counts, void *ws,
                             size_t ws_bytes, void *stream);
/* byte offset of the Q|K|V image inside the saved blob of a training forward with these shapes (0 without attention) */
size_t xnrs_seq_encoder_saved_qkv_offset(int64_t n_seq, int32_t L, int32_t D, int32_t A, int32_t E, int32_t n_heads,
                                         int32_t pool_kind, int32_t has_head);
int32_t xnrs_seq_encoder_fwd_train_rows(const float *x, const float *m, const int32_t *ids, int64_t n_seq, int32_t L,
                                        int32_t D, const xnrs_mha_params *att, int32_t pool_kind,
                                        const xnrs_additive_params *pool, const xnrs_head_params *head, float *y,
                                        float *a_out, float *hm, void *saved, size_t saved_bytes,
                                        const xnrs_row_lists *rows, void *stream);
int32_t xnrs_seq_encoder_bwd_rows(const float *x, const float *m, const int32_t *ids, int64_t n_seq, int32_t L, int32_t D,
                                  const xnrs_mha_params *att, int32_t pool_kind, const xnrs_additive_params *pool,
                                  const xnrs_head_params *head, const void *saved, size_t saved_bytes, const float *dy,
                                  float *dx, const xnrs_mha_grads *g_att, const xnrs_additive_grads *g_pool,
                                  const xnrs_head_grads *g_head, const xnrs_row_lists *rows, void *ws, size_t ws_bytes,
                                  void *stream);

/* autograd of nn.Linear (xnrs_linear_fwd): dx = dy.W, dw = dy^T.x, db = colsum(dy), each nullable (db alone: a
 * stand-alone column sum; with dw: summed by the product's own launch).  gather_ids as in the forward (then dx must be NULL).
 * M == 0, here and in the two xnrs_embedding_linear_bwd* below: every output that was asked for is written as zeros and
 * nothing else is touched; x / ids / dy and the workspace may be NULL. */
size_t xnrs_linear_bwd_workspace_bytes(int64_t M, int32_t N, int32_t K);
int32_t xnrs_linear_bwd(const float *x, const int32_t *gather_ids, int32_t gather_S, const float *w, const float *dy,
                        float *dx, float *dw, float *db, int64_t M, int32_t N, int32_t K, void *ws, size_t ws_bytes,
                        void *stream);

/* autograd of fc(embedder(idx)) (naml.py:82-86; forward = xnrs_linear_fwd with gather_S = 1):
 * dw:(N,K) = dy^T . table[ids], db:(N) = colsum(dy), d_table:(n_rows,K) = scatter-add of dy.W by ids
 * (deterministic).  Every output nullable.  ws: xnrs_embedding_linear_bwd_workspace_bytes. */
size_t xnrs_embedding_linear_bwd_workspace_bytes(int64_t M, int32_t N, int32_t K);
int32_t xnrs_embedding_linear_bwd(const float *table, const int32_t *ids, const float *w, const float *dy, float *d_table,
                                  float *dw, float *db, int64_t M, int32_t N, int32_t K, int32_t n_rows, void *ws,
                                  size_t ws_bytes, void *stream);

/* autograd of DotScoring.forward with normalize == 0 (scoring.py:23): du:(B,E), dc:(B,C,E), either nullable */
int32_t xnrs_dot_scoring_bwd(const float *u, const float *c, const float *dr, float *du, float *dc, int64_t B,
                             int32_t C, int32_t E, void *stream);
/* the same with normalize == 1 (scoring.py:20-22: u and c L2-normalised before the product); E <= 1024 */
int32_t xnrs_dot_scoring_norm_bwd(const float *u, const float *c, const float *dr, float *du, float *dc, int64_t B,
                                  int32_t C, int32_t E, void *stream);

/* ---- NewsRecDataset.__getitem__ look-ups + torch.cat (xnrs/data/dataset.py:63-85,97-109) as a device copy ----
 * out[i, :] = table[ids[i], :], i < n, rows of row_floats fp32 (a whole news block: S*D token floats, or S mask
 * floats).  For consumers that need the dense batch (input gradients of the explainer, explain.py:160-166); the
 * encoders gather inside their first load and never call this.  HBM-bound; 16-byte streaming accesses when
 * row_floats % 4 == 0 and both pointers are 16-byte aligned. */
int32_t xnrs_gather_rows(const float *table, const int32_t *ids, float *out, int64_t n, int64_t row_floats,
                         void *stream);

/* ---- input dropout of the towers (news_encoding.py:51, user_encoding.py:69: nn.Dropout(p) on the token rows / the
 * history vectors), optionally fused with the row gather above ----
 * out[i, j] = keep(i, j) ? x[src(i), j] * (1/(1-p)) : 0      i < n, j < row_floats
 * src(i) = ids ? ids[i] : i      (ids: the contract of xnrs_gather_rows; NULL = dense, and then out may alias x)
 * The backward of a dense call is the same call on dy with the same (p, seed, seed_dev).
 *
 * The draw is the attention dropout's counter-based generator (xnrs_mha_params::seed) with one "head": the 64-bit state of
 * row i is one splitmix64 of (seed + (seed_dev ? *seed_dev : 0), i) -- i is the row's position IN THIS CALL, never the
 * table row, so two occurrences of one news get two masks as nn.Dropout gives them -- and element j's uniform u is the
 * 32-bit finaliser of that state and j.  keep = u < 1.f - p in fp32; a kept element is ONE fp32 multiply by 1.f / (1.f - p);
 * a dropped element is the literal 0.f, not x * 0: an inf or NaN in a dropped slot gives 0 where torch gives NaN.
 * p <= 0: plain copy / gather, no draw.  p == 1: zeros.  p NaN or outside [0, 1], row_floats >= 2^32 (j is a
 * 32-bit index), NULL x or out, n < 0, row_floats <= 0: XNRS_EINVAL.  n == 0: XNRS_OK.
 * One launch, no allocation, no host sync, capturable.  16-byte streaming accesses when row_floats % 4 == 0 and both
 * pointers are 16-byte aligned, scalar accesses otherwise. */
int32_t xnrs_dropout_rows(const float *x, const int32_t *ids, float *out, int64_t n, int64_t row_floats, float p,
                          uint64_t seed, const uint64_t *seed_dev, void *stream);

/* The two calls above from a table stored in bf16 (row_elems bf16 values per row), widened on the way (bits << 16): out is fp32.
 * xnrs_gather_rows_bf16 has the contract of xnrs_gather_rows; 16-byte loads of 8 elements and 16-byte stores when
 * row_elems % 8 == 0 and both pointers are 16-byte aligned.  xnrs_dropout_rows_bf16 gathers, widens and drops in ONE launch:
 * ids is required, and the keep mask is that of xnrs_dropout_rows for the same (seed, seed_dev, row i of the call, column j),
 * so it equals xnrs_dropout_rows on the widened table bit for bit.  The other rules (p, n, row_elems) are the same. */
int32_t xnrs_gather_rows_bf16(const uint16_t *table, const int32_t *ids, float *out, int64_t n, int64_t row_elems,
                              void *stream);
int32_t xnrs_dropout_rows_bf16(const uint16_t *table, const int32_t *ids, float *out, int64_t n, int64_t row_elems,
                               float p, uint64_t seed, const uint64_t *seed_dev, void *stream);

/* ---- integrated gradients with ONE Q|K|V projection (explain.py:152-173) ----
 * The scaled tokens of interpolation step i are a_i x, and an attention tower reads its tokens through the Q|K|V
 * projection alone: QKV_i = a_i P + b with P = x [Wq; Wk; Wv]^T, and sum_i d s_i / d (a_i x) = (sum_i dQKV_i) [Wq; Wk; Wv].
 * Two streaming kernels turn the one product into the n images and the n gradient images into the operand of one product.
 *
 * xnrs_ig_expand: p:(rows, W), bias:(W) or NULL (= 0), alphas:(n) fp32 ON THE DEVICE -> out:(n * rows, W),
 *   out[i * rows + r][c] = fmaf(alphas[i], p[r][c], bias[c])      (one fused multiply-add, nothing else)
 * xnrs_ig_reduce: g:(n * rows, W) -> out:(rows, W).  Per element s = g[0] + g[1] + ... + g[n-1], ONE fp32 chain in
 *   ascending i; out = scale * s (accumulate == 0) or out = out + scale * s (accumulate == 1), the product and every sum
 *   rounded on their own (no contraction).  No atomics; the bits do not depend on the launch geometry.
 * Both: one launch, no allocation, no host sync, capturable; int64 offsets (n * rows * W may pass 2^31).  16-byte accesses
 * when W % 4 == 0 and p / g and out are 16-byte aligned (bias: any fp32 address), scalar accesses otherwise -- the same bits.
 * n < 0, rows < 0, W <= 0, accumulate outside {0, 1}: XNRS_EINVAL.  n == 0 or rows == 0: XNRS_OK, nothing written.
 * NULL p / alphas / g / out: XNRS_EINVAL.  Errors are found before any launch. */
int32_t xnrs_ig_expand(const float *p, const float *bias, const float *alphas, int64_t n, int64_t rows, int32_t W,
                       float *out, void *stream);
int32_t xnrs_ig_reduce(const float *g, int64_t n, int64_t rows, int32_t W, float scale, float *out, int32_t accumulate,
                       void *stream);

/* ---- device-side batch assembly and evaluation -----------------------
 * Click histories / positives / negatives live on the device as CSR arrays of ROWS into the resident news
 * table ([n_rows,S,D] + mask; `pad_row` = the empty slot: all-zero tokens and mask, dataset.py:82-85).
 *
 * xnrs_assemble_train_batch: NewsRecDataset.__getitem__ 'train' mode + custom_collate_fn
 *   (xnrs/data/dataset.py:54-57,77-85,97-109,147; xnrs/utils.py:190-204) -> hist_rows:(B,l_hist) (the LAST
 *   l_hist clicks, padding behind), cand_rows:(B,1+n_neg) (one random positive, n_neg negatives drawn WITH
 *   replacement); targets are the constant [1,0,..].  Draws: splitmix64(seed, session, slot) % n -- a
 *   counter-based stream (Python's `random` cannot be matched), restated bit for bit by the oracle.
 * xnrs_assemble_eval_batch: 'eval' mode (dataset.py:58-61,149): all positives then all negatives;
 *   cand_off:(B+1) is supplied by the caller (prefix sum of the per-session counts).
 * xnrs_score_csr: r[e] = <vecs[cand_rows[e]], u[cand_sess[e]]> (+ReLU, training.py:392) against news
 *   vectors pre-encoded once per epoch (scoring.py:23 per impression, training.py:194-203).
 * xnrs_rank_metrics: xnrs/evaluation/metrics.py:9-64 per impression after np.nan_to_num
 *   (training.py:210-211); out:(B,9) = ndcg@5, ndcg@10, rr, ctr@1, ctr@10, auc, acc, rec, prec.
 *   Ties in the ranking are broken "higher original index first". */
int32_t xnrs_assemble_train_batch(const int64_t *sess, int64_t B, const int64_t *hist_off, const int32_t *hist_val,
                                  const int64_t *pos_off, const int32_t *pos_val, const int64_t *neg_off,
                                  const int32_t *neg_val, int32_t l_hist, int32_t n_neg, int32_t pad_row, uint64_t seed,
                                  int32_t *hist_rows, int32_t *cand_rows, void *stream);
int32_t xnrs_assemble_eval_batch(const int64_t *sess, int64_t B, const int64_t *hist_off, const int32_t *hist_val,
                                 const int64_t *pos_off, const int32_t *pos_val, const int64_t *neg_off,
                                 const int32_t *neg_val, int32_t l_hist, int32_t pad_row, const int64_t *cand_off,
                                 int32_t *hist_rows, int32_t *cand_rows, int32_t *cand_sess, float *targets, void *stream);
int32_t xnrs_score_csr(const float *vecs, const int32_t *cand_rows, const int32_t *cand_sess, const float *u, float *r,
                       int64_t n_cand, int32_t E, int32_t relu, void *stream);
int32_t xnrs_rank_metrics(const float *scores, const float *targets, const int64_t *cand_off, float *out, int64_t B,
                          void *stream);

/* ---- in-batch InfoNCE (ContrastiveRankingTrainer._compute_contrastive_loss, training.py:433-472) ----
 * emb:(B,E) user embeddings, labels:(B) int64 -> loss:(1).  Same epsilons as the reference: F.normalize
 * eps 1e-12, denominator + 1e-12, mean over rows with >= 1 positive / (count + 1e-8).  `saved`
 * (xnrs_infonce_saved_bytes) carries the normalised embeddings and row sums to the backward, which returns
 * d loss / d emb scaled by the upstream scalar gradient *gout (device pointer).  E <= 1024. */
size_t xnrs_infonce_saved_bytes(int64_t B, int32_t E);
int32_t xnrs_infonce_fwd(const float *emb, const int64_t *labels, int64_t B, int32_t E, float temperature, float *loss,
                         void *saved, size_t saved_bytes, void *stream);
int32_t xnrs_infonce_bwd(const int64_t *labels, int64_t B, int32_t E, float temperature, const void *saved,
                         size_t saved_bytes, const float *gout, float *demb, void *stream);

/* ---- measurement aid (no reference counterpart) ----------------------------------------------
 * When enabled, the sequence-encoder pipeline brackets each kernel launch of the selected stages
 * with hipEvents on the caller's stream (process-global, mutex-guarded; off by default; not
 * hipGraph-capturable while on).  stage_mask bit i selects stage i:
 *   0 qkv GEMM | 1 attention core | 2 out-proj GEMM | 3 fc1+tanh GEMM | 4 pooling | 5 head GEMMs
 *   6 fused short-sequence encoder (stages 0-4 in one launch: S <= 32, D <= 320, news_fused.hip)
 *   7 weight-gradient GEMMs of the backward (dW = dY^T . X) | 8 input-gradient GEMMs (dX = dY . W)
 *   9 attention-core backward
 * (stage 3 also counts the one-launch additive encoder, additive_fused.hip: fc1 + pooling, stage 4 then stays empty)
 * (stage 0 on the "fc1 in the tail" route, XNRS_GEMM_FC1_IN_TAIL below: its FLOPs are those of K|V + Q as ever, its time
 * includes the fc1 tiles of the previous pass in the tail of the merged launch; while stage 3 is selected that route is
 * not taken)
 * xnrs_profile_read synchronises the recorded events and returns, per stage, the summed launch
 * duration (ms), the number of launches and the summed ALGORITHMIC flops of those launches
 * (arrays of XNRS_PROFILE_STAGES entries), then clears the record. */
#define XNRS_PROFILE_STAGES 10
int32_t xnrs_profile_enable(uint32_t stage_mask);
int32_t xnrs_profile_read(double *ms, int64_t *launches, double *flops);

/* ---- Q and K|V of a dense live-row pass in one launch (knob XNRS_GEMM_QKV_ONE_LAUNCH; no reference counterpart) ----
 * Which route did a call take?  The launch timer cannot tell: stage 0 brackets the pass and reports the same executed
 * FLOPs either way.  xnrs_qkv_launch_count returns the number of GEMM launches the live-row Q|K|V branch of the sequence
 * encoder has issued since the last reset (process-global, relaxed atomic): one per pass on the one-launch route, two
 * per pass otherwise (the knob at 0, and every call with ids: the one-launch entry serves dense rows only), none where the
 * branch does not engage; reset != 0 clears it after reading.
 * xnrs_qkv_one_launch_map is the kernel's block -> work rule, evaluated on the host (pure; tests enumerate it): for
 * `block` of a grid sized for kv_row_tiles x kv_col_tiles K|V tiles and ceil(q_rows / q_tile_rows) x q_col_tiles Q tiles,
 * given the device counts live_tiles and live_rows, it writes the section (0 K|V, 1 Q, -1 none) and the workgroup's
 * index inside the section (both pointers nullable together) and returns the grid size (< 0: XNRS_EINVAL).  The K|V
 * tiles come first and their section is rounded up to a multiple of 8 blocks, so both sections keep the XCD of the
 * hardware's round-robin in the low three bits of their own index. */
int32_t xnrs_qkv_launch_count(int32_t reset);
int32_t xnrs_qkv_one_launch_map(int64_t block, int64_t live_tiles, int64_t live_rows, int32_t kv_row_tiles,
                                int32_t kv_col_tiles, int64_t q_rows, int32_t q_tile_rows, int32_t q_col_tiles,
                                int32_t *section, int32_t *index);

/* ---- fc1 of the previous pass in the tail of that launch (knob XNRS_GEMM_FC1_IN_TAIL; no reference counterpart) ----
 * Where a dense call takes the one-launch projection AND the pooler's fc1 walks the live-row list behind a folded
 * out-projection (fp32 rows without ids, 33 <= S <= 64, inference, XNRS_FOLD_OUT on), the fc1 product of pass i-1 goes
 * out as a third section of the projection launch of pass i; only the last pass of a call keeps an fc1 launch of its own.
 * The same bits either way.  xnrs_fc1_in_tail_count returns the number of fc1 products that went out inside a projection
 * launch since the last reset (process-global, relaxed atomic; the launch timer's FLOPs cannot tell the routes apart):
 * passes - 1 per call on that route, 0 otherwise; reset != 0 clears it after reading.  xnrs_qkv_launch_count counts one
 * per pass on this route too.
 * Launch timer: stage 0 brackets the merged launch and reports the K|V + Q FLOPs as before, so its TIME on this route
 * includes the fc1 tiles in the launch's tail (rates derived from it are slightly conservative).  A call made while
 * stage 3 is selected takes the separate launches: an fc1 without a launch of its own has no time to report.
 * xnrs_qkv_fc1_launch_map is the kernel's block -> work rule on the host (pure; tests enumerate it): the arguments of
 * xnrs_qkv_one_launch_map plus the third section's device count (fc1_live_rows), its capacity (fc1_rows), tile height and
 * column tiles.  Sections 0 and 1 are those of xnrs_qkv_one_launch_map for the same arguments; section 2 (fc1) starts at
 * the end of the Q section rounded up to a multiple of 8 blocks.  Returns the grid size (< 0: XNRS_EINVAL). */
int32_t xnrs_fc1_in_tail_count(int32_t reset);
int32_t xnrs_qkv_fc1_launch_map(int64_t block, int64_t live_tiles, int64_t live_rows, int64_t fc1_live_rows,
                                int32_t kv_row_tiles, int32_t kv_col_tiles, int64_t q_rows, int32_t q_tile_rows,
                                int32_t q_col_tiles, int64_t fc1_rows, int32_t fc1_tile_rows, int32_t fc1_col_tiles,
                                int32_t *section, int32_t *index);

/* ---- attention rows nobody reads are not stored (knob XNRS_MHA_LIVE_O; no reference counterpart) -----------------
 * Where the fc1 of a dense inference pass walks the live-row list over the attention rows (folded out-projection,
 * 33 <= S <= 64: dense rows, ids, a bf16 table's direct route), fc1 and the pooler are the only readers of those rows and
 * both read the rows of unmasked tokens alone.  The attention core then stores nothing for a masked query: not the zeros
 * of an all-masked news or query tile, not the uniform average of V of a masked query next to live ones.  The same bits
 * in every output either way.  xnrs_mha_live_o_count returns the number of attention launches that ran that way since the
 * last reset (process-global, relaxed atomic): one per pass on that route, 0 otherwise; reset != 0 clears it after reading. */
int32_t xnrs_mha_live_o_count(int32_t reset);

/* Does the TRAINING forward fold the out-projection behind the pooling right now (knob XNRS_FOLD_TRAIN)?
 * The saved-activation blob of xnrs_seq_encoder_fwd_train* is laid out by that decision and xnrs_seq_encoder_bwd* reads it
 * under the decision of ITS call time: a caller that may reload the knobs between the two (tests, A/B tools) records this
 * value at the forward and refuses the backward when it has changed (xnrs_amd/autograd.py does).  1 / 0. */
int32_t xnrs_train_fold_enabled(void);

/* ---- sticky device status word (ABI 6; no reference counterpart) ------------------------------------------
 * Entry points that never synchronise cannot return an error for a precondition only the device can see.  They OR a bit
 * into ONE caller-owned int32 device word instead (and keep their outputs recognisably wrong: NaN), which the caller reads
 * at its next natural synchronisation point.  xnrs_set_status_word registers the word (process-global like the knobs, and
 * bound to the device that is current at the call: launches on another device ignore it; NULL: none -- the NaN outputs
 * are then the only signal); the caller zeroes it.  xnrs_status_string explains a value.
 *   XNRS_STATUS_NONBINARY_MASK  xnrs_text_encoder_fwd_compact met a mask value other than 0 / 1
 *   XNRS_STATUS_ROW_RANGE       (set by the Python host layer, NewsStore.gather) a table row id outside the table; the
 *                               id was clamped so that no kernel read out of bounds
 *   XNRS_STATUS_QUERY_RANGE     xnrs_personalized_fwd* met a q_idx outside [0, n_q) (that sequence's outputs are NaN), or
 *                               (set by the Python host layer, NPA.queries) a user id outside the user table (clamped) */
#define XNRS_STATUS_NONBINARY_MASK 1
#define XNRS_STATUS_ROW_RANGE 2
#define XNRS_STATUS_QUERY_RANGE 4
int32_t xnrs_set_status_word(int32_t *device_word);
const char *xnrs_status_string(int32_t word);

/* ---- arithmetic mode of the forward GEMMs (nn.Linear call sites listed at xnrs_linear_fwd) ----------
 *   XNRS_GEMM_F32     (0, default) v_mfma_f32_32x32x2_f32: an exact fp32 fmaf chain.
 *   XNRS_GEMM_BF16X3  (1) each fp32 operand is split exactly into three bf16 pieces and the product is
 *                     rebuilt from six v_mfma_f32_32x32x16_bf16 with fp32 accumulation: dropped terms are
 *                     <= 2^-26 |a||b| per product.  Measured against an fp64 product: as close as mode 0 on
 *                     N(0,1) operands (7.6e-7 vs 9.5e-7 normwise), about 2x mode 0's error on operands
 *                     with a wide dynamic range (5.5e-7 vs 2.4e-7; tests/test_hip_split_gemm.py bounds it
 *                     at 1e-6); same distance to the CPU oracle as mode 0 on the full workload.
 *   XNRS_GEMM_BF16X2  (2) two pieces, three products: ~1e-5 relative per product; an opt-in speed knob.
 * Process-wide; the initial value comes from the environment variable XNRS_GEMM_MODE.  It covers every GEMM
 * that runs on the forward-layout kernel: the nn.Linear forwards and the input-gradient products dX = dY . W of
 * the backward (computed against a transposed weight copy); the weight-gradient products dW = dY^T . X always
 * run in mode 0, and so does any launch of fewer than 512 128x128 tiles (the fp32 kernel's smaller tiles win
 * there): in modes 1/2 a row's result can therefore differ by fp32 rounding noise between two batch sizes,
 * whereas mode 0 is bitwise independent of the batch.  Returns the previous mode; values outside 0..2 select 0. */
#define XNRS_GEMM_F32 0
#define XNRS_GEMM_BF16X3 1
#define XNRS_GEMM_BF16X2 2
int32_t xnrs_set_gemm_mode(int32_t mode);
int32_t xnrs_get_gemm_mode(void);

/* ---- development knobs (no reference counterpart) ---------------------------------------------
 * Kernel-selection switches for A/B measurements and tests (XNRS_GEMM_PIPE, _BK, _BUF, _GROUP, _TILE,
 * XNRS_GEMM_SPLIT_MIN_TILES, XNRS_GEMM_DW, XNRS_MHA_LDS, XNRS_MHA_HEADWAVE, XNRS_MHA_PAIR, XNRS_MHA_BWD_FUSED,
 * XNRS_NEWS_FUSED, XNRS_NEWS_FUSED_NPW, XNRS_FOLD_OUT, XNRS_FOLD_TRAIN, XNRS_FC1_ROWDOT, XNRS_MHA_SKIP_MASKED, XNRS_GEMM_QKV_ONE_LAUNCH, XNRS_BWD_SIDE_STREAM, XNRS_BWD_SIDE_MIN_ROWS; DESIGN.md section 6 -- and XNRS_GRU_LAYOUT).  The library reads
 * them from the environment ONCE when it is loaded -- no launch calls getenv -- and again only when this function is
 * called.  None changes a result beyond summation / association order (XNRS_FOLD_*: whether the attention
 * out-projection is applied per token row, as the reference writes it, or once per sequence behind the additive
 * pooling; XNRS_FOLD_TRAIN must not change between a training forward and its backward). */
int32_t xnrs_reload_knobs(void);

/* ---- BilinScoring / FCScoring (scoring.py:41-102), u:(B,E), c:(B,N,E) -> s:(B,N) --------------------------
 * Factorised: bilinear v_b = W[0]^T u^_b (one GEMM per call), s = v_b . c^_bn + bias, with u^ / c^ = u / ||u||, c / ||c||
 * when normalize (no epsilon, scoring.py:58-60) and u / c otherwise; MLP (hidden H, tanh): q_b = W1u u_b + b1 (once per
 * impression), p_bn = W1c c_bn, s = w2 . tanh(q_b + p_bn) + b2, where W1 = [W1u | W1c] is fc1.weight (H, 2E).
 * w: nn.Bilinear weight (1,E,E); w1 (H,2E), w2 (1,H); every bias nullable (bias=False).  `saved`
 * (xnrs_*_scoring_saved_bytes) is written by the forward and read by the backward: bilinear v [| u^], MLP q | p.
 * Backward: every gradient output nullable, and only what is asked for is computed (an input-gradient pass launches no
 * weight-gradient product and the other way round); dw1 is written as [dW1u | dW1c] into its (H, 2E) rows.  All sums in
 * a fixed order (no atomics).  Launches: forward <= 3, backward <= 6.  B == 0 or N == 0: nothing to score (no launch;
 * a backward writes zero weight gradients).  B > 2^31 - 1 or B*N >= 2^31: XNRS_EUNSUPPORTED. */
size_t xnrs_bilinear_scoring_saved_bytes(int64_t B, int32_t E, int32_t normalize);
int32_t xnrs_bilinear_scoring_fwd(const float *u, const float *c, const float *w, const float *bias, float *s, int64_t B,
                                  int32_t N, int32_t E, int32_t normalize, void *saved, size_t saved_bytes, void *stream);
size_t xnrs_bilinear_scoring_bwd_workspace_bytes(int64_t B, int32_t E, int32_t normalize);
int32_t xnrs_bilinear_scoring_bwd(const float *u, const float *c, const float *w, const void *saved, size_t saved_bytes,
                                  const float *ds, float *du, float *dc, float *dw, float *dbias, int64_t B, int32_t N,
                                  int32_t E, int32_t normalize, void *ws, size_t ws_bytes, void *stream);
size_t xnrs_mlp_scoring_saved_bytes(int64_t B, int32_t N, int32_t H);
int32_t xnrs_mlp_scoring_fwd(const float *u, const float *c, const float *w1, const float *b1, const float *w2,
                             const float *b2, float *s, int64_t B, int32_t N, int32_t E, int32_t H, void *saved,
                             size_t saved_bytes, void *stream);
size_t xnrs_mlp_scoring_bwd_workspace_bytes(int64_t B, int32_t N, int32_t H);
int32_t xnrs_mlp_scoring_bwd(const float *u, const float *c, const float *w1, const float *w2, const void *saved,
                             size_t saved_bytes, const float *ds, float *du, float *dc, float *dw1, float *db1, float *dw2,
                             float *db2, int64_t B, int32_t N, int32_t E, int32_t H, void *ws, size_t ws_bytes,
                             void *stream);
/* p:(rows,H) = c:(rows,E) . W1c^T -- the news-side half of fc1 (evaluation: once per epoch over the news table) */
int32_t xnrs_mlp_scoring_news_proj(const float *c, int64_t rows, int32_t E, const float *w1, int32_t H, float *p,
                                   void *stream);
/* Evaluation against news vectors pre-encoded once per epoch (as xnrs_score_csr), u:(n_sess,E):
 *   xnrs_score_csr_bilinear: r[e] = relu?(v[sess[e]] . vecs[rows[e]] + bias), v = u W[0] (one GEMM into ws)
 *   xnrs_score_csr_mlp:      r[e] = relu?(w2 . tanh(q[sess[e]] + P[rows[e]]) + b2), q = u W1u^T + b1 (one GEMM into ws),
 *                            P = xnrs_mlp_scoring_news_proj of the table
 * ws: xnrs_score_csr_scorer_workspace_bytes(n_sess, E) (bilinear) / (n_sess, H) (MLP).  A normalised bilinear scorer
 * passes vectors normalised with xnrs_l2_normalize_rows. */
size_t xnrs_score_csr_scorer_workspace_bytes(int64_t n_sess, int32_t width);
int32_t xnrs_score_csr_bilinear(const float *vecs, const int32_t *cand_rows, const int32_t *cand_sess, const float *u,
                                int64_t n_sess, const float *w, const float *bias, float *r, int64_t n_cand, int32_t E,
                                int32_t relu, void *ws, size_t ws_bytes, void *stream);
int32_t xnrs_score_csr_mlp(const float *P, const int32_t *cand_rows, const int32_t *cand_sess, const float *u,
                           int64_t n_sess, const float *w1, const float *b1, const float *w2, const float *b2, float *r,
                           int64_t n_cand, int32_t E, int32_t H, int32_t relu, void *ws, size_t ws_bytes, void *stream);
/* y[r,:] = x[r,:] / ||x[r,:]|| (no epsilon, scoring.py:20-22); y may equal x */
int32_t xnrs_l2_normalize_rows(const float *x, float *y, int64_t rows, int32_t E, void *stream);

/* ---- top-k rows of a pre-encoded news table per user (recommendation; csrc/topk.hip) -------------------------------------
 * rows:(B,k) int32, scores:(B,k) fp32 <- for every user the k eligible table rows of highest score, without a (B, n_rows)
 * score matrix: a partial kernel ranks the score tiles of (user tile x table slice) while it forms them, a merge kernel
 * merges the slices.  The three entry points mirror xnrs_score_csr / _bilinear / _mlp -- the same user-side GEMM into ws,
 * the same meaning of table / P (already L2-normalised by the caller where the scorer normalises):
 *   xnrs_topk          s = <table[n], u[b]>
 *   xnrs_topk_bilinear s = <table[n], v[b]> + bias, v = u W[0]
 *   xnrs_topk_mlp      s = w2 . tanh(q[b] + P[n]) + b2, q = u W1u^T + b1, P:(n_rows,H) = xnrs_mlp_scoring_news_proj of the table
 * Order: higher score first; equal scores (==, so +0 and -0 tie) lower row first; a NaN score is never selected; -inf is a
 * legal score.  The ranking is by the RAW score: there is no ReLU here (the evaluation's relu would tie every negative score).
 * Eligible rows: [0, n_rows) minus pad_row (when >= 0) minus the user's exclusion list.  With fewer than k eligible rows the
 * tail holds fillers -- row -1, score -inf -- behind every real entry.
 * Exclusions: excl_off:(B+1) int64 and excl_rows: int32 form a CSR over the users, the offsets ABSOLUTE into excl_rows (a
 * slice of a longer offset array works without a copy).  A list may be unsorted, hold duplicates and hold ids outside the
 * table (compared, never dereferenced), at any length.  excl_off == NULL: no exclusions.
 * Arithmetic: the inner-product forms are one fp32 fma chain over ascending feature index from 0 (the fp32 MFMA), the bias
 * added last; the MLP form sums over h in ascending order.  A user's result therefore does not depend on B, on the user's
 * position in the batch or on the slicing, and is bit for bit the same on every run.
 * Limits: 1 <= k <= XNRS_TOPK_MAX_K, n_rows <= 2^31 - 1, any E, H >= 1, any B >= 0.  B == 0: XNRS_OK, nothing written;
 * n_rows == 0: fillers.  Argument errors (XNRS_EINVAL) and a short workspace (XNRS_EWORKSPACE) are found on the host before
 * any launch and write nothing.  ws: xnrs_topk_workspace_bytes(B, n_rows, proj_width, k), proj_width = 0 (xnrs_topk), E
 * (bilinear), H (MLP).  xnrs_topk_slices: the number of table slices a call of this size uses, chosen from (B, n_rows) alone
 * so that user tiles x slices fills the chip (a pure host call; 1 for a table of one 128-row chunk). */
#define XNRS_TOPK_MAX_K 128
size_t xnrs_topk_workspace_bytes(int64_t B, int64_t n_rows, int32_t proj_width, int32_t k);
int32_t xnrs_topk_slices(int64_t B, int64_t n_rows);
int32_t xnrs_topk(const float *table, int64_t n_rows, int32_t E, const float *u, int64_t B, const int64_t *excl_off,
                  const int32_t *excl_rows, int32_t pad_row, int32_t k, int32_t *rows, float *scores, void *ws,
                  size_t ws_bytes, void *stream);
int32_t xnrs_topk_bilinear(const float *table, int64_t n_rows, int32_t E, const float *u, int64_t B, const float *w,
                           const float *bias, const int64_t *excl_off, const int32_t *excl_rows, int32_t pad_row, int32_t k,
                           int32_t *rows, float *scores, void *ws, size_t ws_bytes, void *stream);
int32_t xnrs_topk_mlp(const float *P, int64_t n_rows, int32_t E, int32_t H, const float *u, int64_t B, const float *w1,
                      const float *b1, const float *w2, const float *b2, const int64_t *excl_off, const int32_t *excl_rows,
                      int32_t pad_row, int32_t k, int32_t *rows, float *scores, void *ws, size_t ws_bytes, void *stream);

/* ---- deep top-k: the same lists up to k = 1024 (candidate generation; csrc/topk.hip) ---------------------------------------
 * xnrs_topk_deep / _bilinear / _mlp take the argument lists of xnrs_topk / _bilinear / _mlp and keep their contract word for
 * word -- order, fillers, eligibility, the exclusion CSR with absolute offsets, pad_row, the NaN / +-inf / +-0 rules, the
 * arithmetic, refusals on the host before any launch that write nothing, no host synchronisation, hipGraph-capturable, no
 * allocation, no float atomics -- with the limit 1 <= k <= XNRS_TOPK_DEEP_MAX_K.  On top of it:
 *   same bits : scores are formed by the score-tile function of xnrs_topk* and by nothing else; for k <= XNRS_TOPK_MAX_K a call
 *               runs the two launches of xnrs_topk* and returns their rows and scores bit for bit.
 *   prefix    : deep(k)[:, :j] == deep(j) for every j <= k, so deep(1024)[:, :128] == xnrs_topk*(128).
 *   rank      : for an eligible row t of user b, xnrs_rank* over the same arguments gives ranks < k exactly when deep(k) lists
 *               t, at position ranks with the bits of scores.
 *   A user's result does not depend on B, on the user's position in the batch or on the slicing, and is the same on every run.
 * For k > XNRS_TOPK_MAX_K the launches are the user-side GEMM where the scorer has one, then the partial and the merge kernel
 * of xnrs_topk* instantiated for lists of up to 1024 keys: the partial kernel stages a list in LDS (8 KB per half-wave, 135 KB
 * per workgroup: one workgroup per CU) and moves only the keys a list holds so far, the merge kernel holds three lists per
 * wave (96 KB per workgroup).  The inner-product
 * forms sweep the table twice: a first sweep with the kernels of xnrs_topk* keeps ceil(k / (slices - 1)) keys per slice, a
 * one-thread-per-user kernel turns them into a key that k rows of the user are known to reach, and the second sweep starts its
 * thresholds there (the floor removes only rows that cannot be among the k: the result does not depend on it).  Results cross
 * from launch to launch at kernel boundaries only.
 * ws: xnrs_topk_deep_workspace_bytes(B, n_rows, proj_width, k) = align(B * proj_width * 4) + align(B * 8) + align(slices * B *
 * k * 8), align = up to 256 B, slices = xnrs_topk_slices(B, n_rows) <= 256: it grows with n_rows through the slice count alone
 * and never holds a (B, n_rows) array; for k <= XNRS_TOPK_MAX_K it is xnrs_topk_workspace_bytes (no B * 8 term).  A pure host
 * call; 0 for k outside the limit. */
#define XNRS_TOPK_DEEP_MAX_K 1024
size_t xnrs_topk_deep_workspace_bytes(int64_t B, int64_t n_rows, int32_t proj_width, int32_t k);
int32_t xnrs_topk_deep(const float *table, int64_t n_rows, int32_t E, const float *u, int64_t B, const int64_t *excl_off,
                       const int32_t *excl_rows, int32_t pad_row, int32_t k, int32_t *rows, float *scores, void *ws,
                       size_t ws_bytes, void *stream);
int32_t xnrs_topk_deep_bilinear(const float *table, int64_t n_rows, int32_t E, const float *u, int64_t B, const float *w,
                                const float *bias, const int64_t *excl_off, const int32_t *excl_rows, int32_t pad_row,
                                int32_t k, int32_t *rows, float *scores, void *ws, size_t ws_bytes, void *stream);
int32_t xnrs_topk_deep_mlp(const float *P, int64_t n_rows, int32_t E, int32_t H, const float *u, int64_t B, const float *w1,
                           const float *b1, const float *w2, const float *b2, const int64_t *excl_off,
                           const int32_t *excl_rows, int32_t pad_row, int32_t k, int32_t *rows, float *scores, void *ws,
                           size_t ws_bytes, void *stream);

/* ---- where given rows rank within the whole table per user (full-corpus evaluation; csrc/rank.hip) ------------------------
 * The sweep of xnrs_topk* that counts instead of selects, again without a (B, n_rows) score matrix.  table / P, u, the
 * weights, the exclusion CSR and pad_row mean what they mean for xnrs_topk*: the same tensors serve both calls.
 * Queries: tgt_off:(B+1) int64 and tgt_rows: int32 form a CSR of target rows over the users, the offsets ABSOLUTE into
 * tgt_rows like excl_off.  ranks: int32 and scores: fp32 are indexed like tgt_rows; a call writes positions
 * [tgt_off[0], tgt_off[B]) and nothing else.  A user may have zero, one or any number of targets; duplicate targets are
 * separate queries with the same answer.  For query e = (user b, row t):
 *   scores[e] = the raw score of (b, t): the very bits xnrs_topk* forms for that pair (one score-tile function, the same
 *               instruction, for the targets and for the sweep)
 *   ranks[e]  = the number of eligible rows n != t that come before (b, t) in the order of xnrs_topk: a higher score, or an
 *               equal score (==, so -0 ties +0) in a lower row.  A NaN-scored row is never counted; -inf is a legal score.
 * Eligible rows are those of xnrs_topk: [0, n_rows) minus pad_row minus the user's exclusion list (unsorted, duplicates,
 * foreign ids, any length; compared, never dereferenced; a duplicate is not counted twice).  THE TARGET ITSELF IS RANKED
 * EVEN WHEN IT IS ON ITS OWN USER'S EXCLUSION LIST: the list removes competitors, not the query.  So for an eligible target
 * ranks[e] < k exactly when xnrs_topk* with the same arguments returns t, and it returns t at position ranks[e] with
 * scores[e].  Rank -1 and score NaN: t outside [0, n_rows) (never dereferenced), t == pad_row, a NaN score.
 * A query's result does not depend on B, on the user's position in the batch or on the slicing, and is the same on every
 * run (integer counts; no float atomics).  No host synchronisation: the target counts are read on the device only.
 * Limits as xnrs_topk: n_rows <= 2^31 - 1, any E, H >= 1, any B >= 0.  B == 0 or an empty target span: XNRS_OK, nothing
 * written; n_rows == 0: every query -1 / NaN.  Argument errors (XNRS_EINVAL) and a short workspace (XNRS_EWORKSPACE) are
 * found on the host before any launch and write nothing.  ws: xnrs_rank_workspace_bytes(B, proj_width) -- the projected
 * user side only -- proj_width = 0 (xnrs_rank: no workspace, ws may be NULL), E (bilinear), H (MLP); a pure host call.  The
 * grid of the sweep is user tiles x xnrs_topk_slices(B, n_rows). */
size_t xnrs_rank_workspace_bytes(int64_t B, int32_t proj_width);
int32_t xnrs_rank(const float *table, int64_t n_rows, int32_t E, const float *u, int64_t B, const int64_t *tgt_off,
                  const int32_t *tgt_rows, const int64_t *excl_off, const int32_t *excl_rows, int32_t pad_row,
                  int32_t *ranks, float *scores, void *ws, size_t ws_bytes, void *stream);
int32_t xnrs_rank_bilinear(const float *table, int64_t n_rows, int32_t E, const float *u, int64_t B, const float *w,
                           const float *bias, const int64_t *tgt_off, const int32_t *tgt_rows, const int64_t *excl_off,
                           const int32_t *excl_rows, int32_t pad_row, int32_t *ranks, float *scores, void *ws,
                           size_t ws_bytes, void *stream);
int32_t xnrs_rank_mlp(const float *P, int64_t n_rows, int32_t E, int32_t H, const float *u, int64_t B, const float *w1,
                      const float *b1, const float *w2, const float *b2, const int64_t *tgt_off, const int32_t *tgt_rows,
                      const int64_t *excl_off, const int32_t *excl_rows, int32_t pad_row, int32_t *ranks, float *scores,
                      void *ws, size_t ws_bytes, void *stream);

/* ---- a per-user row window for the two sweeps (time-aware recommendation and evaluation; csrc/sweep.h) ---------------------
 * xnrs_topk_deep*_win and xnrs_rank*_win take the argument lists of xnrs_topk_deep* / xnrs_rank* with two int32 device arrays
 * of length B, win_lo and win_hi, behind excl_rows: user b sees the table rows [win_lo[b], win_hi[b]) only.  With the table
 * ordered by publication time that is "the news that existed at the session's time and was still fresh".
 * THE RESULT OF A WINDOWED CALL EQUALS THE PARENT'S RESULT WITH EVERY ROW OUTSIDE THE USER'S WINDOW APPENDED TO THE USER'S
 * EXCLUSION LIST -- rows, ranks and score bits.  Everything else of the parents' contract holds word for word: order, fillers,
 * the exclusion CSR, pad_row, the NaN / +-inf / +-0 rules, the arithmetic (a window changes which scores are looked at, never
 * a score's bits), refusals on the host before any launch that write nothing, no host synchronisation, hipGraph-capturable, no
 * allocation, no float atomics, results crossing launches at kernel boundaries only, and: a user's result does not depend
 * on B, on the user's position in the batch, on the OTHER users' windows or on the slicing, and is the same on every run.
 *   Eligible : row n is eligible for user b when it is eligible for the parent (inside [0, n_rows), not pad_row, not on b's
 *              exclusion list, score not NaN) and win_lo[b] <= n < win_hi[b].
 *   Bounds   : clamped to [0, n_rows] on the device; compared, never dereferenced.  win_lo[b] >= win_hi[b]: no row is eligible
 *              -- fillers only, rank 0 for a scored target.
 *   NULL     : both pointers NULL: the call IS the parent call, bit for bit (the same launches over the same slices).  Exactly
 *              one NULL: XNRS_EINVAL.
 *   top-k    : 1 <= k <= XNRS_TOPK_DEEP_MAX_K; k <= XNRS_TOPK_MAX_K runs the two launches of xnrs_topk* with their bits, so
 *              there is no separate shallow entry.  prefix: win(k)[:, :j] == win(j).
 *   rank     : as with the exclusion list the window removes competitors, not the query: A TARGET OUTSIDE ITS USER'S WINDOW IS
 *              STILL SCORED AND RANKED among the eligible rows.  For a target that is eligible, ranks[e] < k exactly when
 *              xnrs_topk_deep*_win with the same arguments lists it, at position ranks[e] with the bits of scores[e].
 *   Work     : rows outside the windows are not scored.  A workgroup reduces the windows of its (up to 128) users to the chunk
 *              range of their union on the device (128-row chunks) and the xnrs_topk_slices(B, n_rows) slices of the grid
 *              split that range evenly instead of the whole table; a chunk of the union that no window of the tile touches
 *              is skipped.  The cost of a tile therefore follows the UNION of its users' windows: sessions sorted by time
 *              give narrow unions, shuffled sessions with narrow windows still sweep nearly the whole table per tile.
 *   Floor    : the first sweep of the deep inner-product forms (k > XNRS_TOPK_MAX_K) sees the same windows and the same
 *              slices, so a full slice list still proves that many eligible rows of the user; a user whose window holds fewer
 *              than k rows, or touches too few slices, gets no floor and is swept from the filler.
 * ws: the parents' xnrs_topk_deep_workspace_bytes / xnrs_rank_workspace_bytes; the windows need none. */
int32_t xnrs_topk_deep_win(const float *table, int64_t n_rows, int32_t E, const float *u, int64_t B, const int64_t *excl_off,
                           const int32_t *excl_rows, const int32_t *win_lo, const int32_t *win_hi, int32_t pad_row, int32_t k,
                           int32_t *rows, float *scores, void *ws, size_t ws_bytes, void *stream);
int32_t xnrs_topk_deep_bilinear_win(const float *table, int64_t n_rows, int32_t E, const float *u, int64_t B, const float *w,
                                    const float *bias, const int64_t *excl_off, const int32_t *excl_rows, const int32_t *win_lo,
                                    const int32_t *win_hi, int32_t pad_row, int32_t k, int32_t *rows, float *scores, void *ws,
                                    size_t ws_bytes, void *stream);
int32_t xnrs_topk_deep_mlp_win(const float *P, int64_t n_rows, int32_t E, int32_t H, const float *u, int64_t B, const float *w1,
                               const float *b1, const float *w2, const float *b2, const int64_t *excl_off,
                               const int32_t *excl_rows, const int32_t *win_lo, const int32_t *win_hi, int32_t pad_row,
                               int32_t k, int32_t *rows, float *scores, void *ws, size_t ws_bytes, void *stream);
int32_t xnrs_rank_win(const float *table, int64_t n_rows, int32_t E, const float *u, int64_t B, const int64_t *tgt_off,
                      const int32_t *tgt_rows, const int64_t *excl_off, const int32_t *excl_rows, const int32_t *win_lo,
                      const int32_t *win_hi, int32_t pad_row, int32_t *ranks, float *scores, void *ws, size_t ws_bytes,
                      void *stream);
int32_t xnrs_rank_bilinear_win(const float *table, int64_t n_rows, int32_t E, const float *u, int64_t B, const float *w,
                               const float *bias, const int64_t *tgt_off, const int32_t *tgt_rows, const int64_t *excl_off,
                               const int32_t *excl_rows, const int32_t *win_lo, const int32_t *win_hi, int32_t pad_row,
                               int32_t *ranks, float *scores, void *ws, size_t ws_bytes, void *stream);
int32_t xnrs_rank_mlp_win(const float *P, int64_t n_rows, int32_t E, int32_t H, const float *u, int64_t B, const float *w1,
                          const float *b1, const float *w2, const float *b2, const int64_t *tgt_off, const int32_t *tgt_rows,
                          const int64_t *excl_off, const int32_t *excl_rows, const int32_t *win_lo, const int32_t *win_hi,
                          int32_t pad_row, int32_t *ranks, float *scores, void *ws, size_t ws_bytes, void *stream);

/* ---- sampled top-k: a list DRAWN from the scores instead of the k best (stochastic ranking; csrc/topk.hip) ------------------
 * xnrs_topk_sample*_win take the argument lists of xnrs_topk_deep*_win with temperature, seed and user_keys behind k.  The
 * list of user b is a sample WITHOUT replacement from the Plackett-Luce distribution over b's eligible rows: the first place
 * is row n with probability proportional to exp(s_bn / temperature), the second is drawn the same way from the rest, and so
 * on.  It is computed as Gumbel top-k -- the k largest of the perturbed keys
 *     key_bn = fl(fl(s_bn * (1 / temperature)) + g_bn),    g_bn = -log(-log(1 - w)),  w = min((x + 1/2) 2^-32, 1 - 2^-24)
 * (fp32; product and sum rounded separately), x the 32-bit word of the dropout stream of xnrs_dropout_rows for seed `seed`,
 * row user_keys[b] and element n (one splitmix64 per (seed, user key), one murmur3 fmix32 per table row; csrc/kernels.h:
 * drop_word, drop_gumbel).  The uniform keeps an fp32's relative precision towards 0, the tail the winners of a large table
 * come from; there are 2^32 draws per (seed, user key), and g lies in [-2.8116, 22.874].  s_bn is the score of xnrs_topk*,
 * formed by its score tile, bias included.
 *   rows     : (B,k) int32, best perturbed key first; scores: (B,k) fp32 holds the PERTURBED KEYS, not the raw scores (score
 *              the returned rows with xnrs_score_csr* where those are wanted).  Fillers: row -1, key -inf.
 *   Order    : of the keys as xnrs_topk* orders scores: higher key first, equal keys lower row first.  A NaN score never
 *              wins; a -inf score keeps the key -inf, behind every finite key and before the fillers; +inf stays +inf.
 *   Pure     : key_bn depends on (seed, user_keys[b], n, s_bn, temperature) and nothing else -- not on B, on the user's position
 *              in the batch, on the other users, on the windows, on the slicing, on k or on the run.  So a call repeats bit
 *              for bit, sample(k)[:, :j] == sample(j), and a user called alone with its key gets the list it got in a batch.
 *   user_keys: (B,) int64 on the device, any values (a session id); NULL: the user's index in the call, 0 .. B-1.  Two users
 *              with one key and one score vector draw the same list.
 *   Limits   : 1 <= k <= XNRS_TOPK_DEEP_MAX_K; temperature finite, > 0 and with a finite 1 / temperature, else XNRS_EINVAL
 *              before any launch.  As temperature -> 0 the list tends to xnrs_topk_deep*_win's (once the gaps of s / temperature
 *              exceed the range of g, 25.69, it IS that list); as it grows the list tends to a uniform draw.
 * Everything else is the contract of xnrs_topk_deep*_win word for word: eligibility, the exclusion CSR, pad_row, the windows
 * (both NULL: none; exactly one: XNRS_EINVAL), refusals on the host that write nothing, no host synchronisation,
 * hipGraph-capturable, no allocation, no float atomics.  Launches: those of xnrs_topk_deep* with the sampled instantiations of
 * the partial kernel (both sweeps of a k > XNRS_TOPK_MAX_K inner-product call draw the same noise); a score whose
 * fl(fl(s / temperature) + 22.874) is below the user's current threshold is dropped without its draw.
 * ws: xnrs_topk_deep_workspace_bytes(B, n_rows, proj_width, k). */
int32_t xnrs_topk_sample_win(const float *table, int64_t n_rows, int32_t E, const float *u, int64_t B, const int64_t *excl_off,
                             const int32_t *excl_rows, const int32_t *win_lo, const int32_t *win_hi, int32_t pad_row,
                             int32_t k, float temperature, uint64_t seed, const int64_t *user_keys, int32_t *rows,
                             float *scores, void *ws, size_t ws_bytes, void *stream);
int32_t xnrs_topk_sample_bilinear_win(const float *table, int64_t n_rows, int32_t E, const float *u, int64_t B, const float *w,
                                      const float *bias, const int64_t *excl_off, const int32_t *excl_rows,
                                      const int32_t *win_lo, const int32_t *win_hi, int32_t pad_row, int32_t k,
                                      float temperature, uint64_t seed, const int64_t *user_keys, int32_t *rows, float *scores,
                                      void *ws, size_t ws_bytes, void *stream);
int32_t xnrs_topk_sample_mlp_win(const float *P, int64_t n_rows, int32_t E, int32_t H, const float *u, int64_t B,
                                 const float *w1, const float *b1, const float *w2, const float *b2, const int64_t *excl_off,
                                 const int32_t *excl_rows, const int32_t *win_lo, const int32_t *win_hi, int32_t pad_row,
                                 int32_t k, float temperature, uint64_t seed, const int64_t *user_keys, int32_t *rows,
                                 float *scores, void *ws, size_t ws_bytes, void *stream);

/* ---- the full-table softmax ranking loss: the training side of the two sweeps (csrc/table_loss.hip) ------------------------
 * The reference's ranking_loss(p, n) = -log(e^p / (e^p + sum e^n)) (xnrs/utils.py:117-131) with EVERY eligible news of the
 * table as a negative, forward and backward, again without a (B, n_rows) score matrix.  The operands are those of
 * xnrs_rank_win: table:(n_rows,E), the user side up:(B,E) as the score reads it (u, or v = u W[0] of the bilinear scorer),
 * bias: one float on the device or NULL, the target CSR tgt_off / tgt_rows (one query per entry), the exclusion CSR (NULL:
 * none), win_lo / win_hi (both or neither; exactly one: XNRS_EINVAL) and pad_row.  Scores s_bn = <table[n], up[b]> (+ bias)
 * are formed by the score tile of xnrs_topk* / xnrs_rank* and by nothing else.
 *   Negatives of user b: the rows eligible for xnrs_rank*_win (inside the table, not pad_row, not on b's exclusion list,
 *              inside b's window) minus EVERY target row of b: another positive of the same session is not a negative.
 *   Forward  : lse[b] = log sum_{n in negatives} exp(s_bn), max-stabilised (no overflow for finite scores), -inf when the
 *              user has no negatives.  For query e = (b, t): scores[e] = the raw score, the bits xnrs_rank writes;
 *              loss[e] = logaddexp(s_bt, lse[b]) - s_bt = ranking_loss(p = s_bt, n = all negatives).
 *   No answer: the rank -1 queries of xnrs_rank (t outside the table, t == pad_row): scores[e] = NaN, loss[e] = 0, no
 *              gradient.  As with rank, a target on its own exclusion list or outside its window is still a query.
 *   No negatives: loss = 0 exactly and every gradient of the user 0; no NaN.
 *   Backward : g[e] the upstream gradient per query, p_e = exp(s_bt - logaddexp(s_bt, lse[b])), c_b = sum_{e of b} g_e (1 - p_e):
 *              d s_bt = -g_e (1 - p_e); d s_bn = c_b exp(s_bn - lse[b]) per negative; d_up[b] = sum_n d s_bn table[n];
 *              d_table[n] = sum_b d s_bn up[b].  Duplicate targets are separate queries and both contribute.  d_up:(B,E) and
 *              d_table:(n_rows,E) are OVERWRITTEN (zero rows where nothing flows); either may be NULL, and a NULL gradient's
 *              sweep is not launched.  scores and lse are what the forward call over the same operands wrote.
 *   Precondition: table and up are finite; the results for non-finite inputs are unspecified.
 * Launches: forward 3 (target scores; the sweep -- user tiles x xnrs_topk_slices(B, n_rows), per (user, 128-row chunk) a
 * partial (max, sum exp(s - max)); the combine, one thread per user).  d_up 2 (the sweep recomputes the score tile and feeds
 * d s through LDS into a second fp32 MFMA product with the table chunk, 128 users x 256 features per pass; a reduce sums
 * the slice partials in slice order and adds the target terms).  d_table 1 or 2 (the transposed sweep over row chunks, and
 * over user groups when the table has fewer than 256 chunks; then a reduce in group order).
 * Determinism: lse, loss and scores of a user do not depend on B, on the user's position in the batch, on the other users'
 * windows or on the slicing and are the same bits on every run: chunk partials are folded in ascending chunk order, the
 * in-chunk tree is fixed by the row's place in its chunk, and a chunk without a negative leaves the running value's bits
 * untouched -- so A WINDOWED CALL EQUALS, BIT FOR BIT, THE CALL WITH EVERY OUT-OF-WINDOW ROW ON THE EXCLUSION LIST, and both
 * window pointers NULL is the call without them.  d_up and d_table are the same bits on every run of the same call; their
 * summation order follows the slicing, so they MAY differ in the last bits between batch sizes and batch positions.
 * No float atomics, results cross launches at kernel boundaries only, no host synchronisation, no allocation, hipGraph-
 * capturable.  XNRS_EINVAL and XNRS_EWORKSPACE are found on the host before any launch and write nothing.  B == 0: XNRS_OK,
 * nothing written; an empty target span writes lse alone; n_rows == 0: lse = -inf, every query NaN / 0.  n_rows <= 2^31 - 1,
 * any E >= 1 (E % 4 != 0 or an unaligned base takes scalar loads).
 * ws: xnrs_table_loss_workspace_bytes(B, n_rows, E, want_d_table), one size for both calls, a pure host call, never a
 * (B, n_rows) array: the larger of
 *   forward : 8 ceil(n_rows / 128) B bytes                                            (1/64 of the score matrix)
 *   backward: 4 S B E + (want_d_table and G > 1 ? 4 G n_rows E : 0) bytes, S = the slices of the d_up sweep = min(chunks,
 *             ceil(256 / user tiles)) and G = the user groups of the d_table sweep = min(user tiles, ceil(256 / chunks)),
 *             both rounded to even shares: the partials are bounded by 256 workgroups x 128 x E floats (+ one tile row),
 * each region rounded up to 256 B. */
size_t xnrs_table_loss_workspace_bytes(int64_t B, int64_t n_rows, int32_t E, int32_t want_d_table);
int32_t xnrs_table_loss_fwd(const float *table, int64_t n_rows, int32_t E, const float *up, const float *bias, int64_t B,
                            const int64_t *tgt_off, const int32_t *tgt_rows, const int64_t *excl_off, const int32_t *excl_rows,
                            const int32_t *win_lo, const int32_t *win_hi, int32_t pad_row, float *scores, float *loss,
                            float *lse, void *ws, size_t ws_bytes, void *stream);
int32_t xnrs_table_loss_bwd(const float *table, int64_t n_rows, int32_t E, const float *up, const float *bias, int64_t B,
                            const int64_t *tgt_off, const int32_t *tgt_rows, const int64_t *excl_off, const int32_t *excl_rows,
                            const int32_t *win_lo, const int32_t *win_hi, int32_t pad_row, const float *scores,
                            const float *lse, const float *g, float *d_up, float *d_table, void *ws, size_t ws_bytes,
                            void *stream);

/* ---- the softmax ranking loss over per-user row LISTS: training against mined negatives (csrc/list_loss.hip) -----------------
 * The same ranking_loss(p, n) with the L rows a caller LISTS per user as the negatives -- the lists xnrs_topk_deep returns
 * (the m hardest negatives), sampled rows, stale lists -- forward and backward, without a (B, L, E) copy of the listed rows.
 * The operands are the user side of xnrs_table_loss_*: table:(n_rows,E), up:(B,E) as the score reads it (u, or v = u W[0] of
 * the bilinear scorer), bias: one float on the device or NULL, the target CSR tgt_off / tgt_rows (one query per entry; T =
 * the entries of tgt_rows, T >= tgt_off[B]) and pad_row; plus neg_rows:(B,L) int32, row-major.  Scores s = <table[r], up[b]>
 * (+ bias).
 *   Negatives of user b: every slot j whose row neg_rows[b][j] is inside [0, n_rows), is not pad_row and equals no target row
 *              of b (a user's own click is never their negative, as in the table loss).  Every other slot is EMPTY: the -1
 *              fillers of xnrs_topk_deep, ids outside the table, the pad row, a target; such a row is compared, never
 *              dereferenced.  neg_scores[b][j] = the score of a negative, NaN for an empty slot.  A ROW LISTED TWICE BY ONE
 *              USER COUNTS TWICE: this is the reference's loss over a gathered list, and it differs here from the table
 *              loss, where a row is a negative once.
 *   Forward  : lse[b] = log sum_{filled slots} exp(s_bj), max-stabilised, -inf when the user has no negatives.  For query
 *              e = (b, t): scores[e] = the raw score, loss[e] = logaddexp(s_bt, lse[b]) - s_bt.  Entries of scores / loss
 *              outside [tgt_off[0], tgt_off[B]) are not written.
 *   No answer: t outside the table or t == pad_row: scores[e] = NaN, loss[e] = 0, no gradient.
 *   No negatives: loss = 0 exactly and every gradient of the user 0; no NaN.  L == 0: every user is one.
 *   Backward : the formulas of the table loss above with "negative" = a filled slot: g[e] the upstream gradient per query,
 *              c_b = sum_{e of b} g_e (1 - p_e); d s_bt = -g_e (1 - p_e); d s_bj = c_b exp(s_bj - lse[b]) per filled slot;
 *              d_up[b] = sum over b's slots and queries of d s * table[row]; d_table[n] = sum over every slot and query
 *              whose row is n of d s * up[b].  d_up:(B,E) and d_table:(n_rows,E) are OVERWRITTEN (rows that nothing lists
 *              are exactly zero); either may be NULL, and then its launches are skipped.  scores, lse and neg_scores are
 *              what the forward call over the same operands wrote.
 *   order    : (B L + T) int32, NULL iff d_table is NULL (one without the other: XNRS_EINVAL): a permutation of the entries
 *              -- slot (b, j) is entry b L + j, query e is entry B L + e -- sorted ascending by row, ties in ascending
 *              entry index, with every entry that has no row to give a gradient to (an empty slot, a query without an
 *              answer: NaN in neg_scores / scores) behind all others.  A query of a user WITHOUT NEGATIVES has a score and
 *              is sorted by its row like any other; it adds exactly 0 to that row.  The caller builds it (a stable sort of the row keys; xnrs_amd/ops.py: list_loss_backward); the
 *              kernel walks the runs of equal rows in its first B L + tgt_off[B] positions.  A value outside [0, B L + T) is
 *              skipped and never dereferenced.  An order that is NOT grouped by row gives unspecified gradients for the
 *              rows concerned and nothing worse: no access outside the operands.
 *   Precondition: table and up are finite; B (L + 1) <= 2^31 - 1 and n_rows <= 2^31 - 1 (else XNRS_EINVAL).
 * Launches: forward 1 (a workgroup of four waves per user: a wave gathers four listed rows at a time against the user
 * vector in LDS, then the workgroup folds max and sum exp over the slots and scores the user's queries).  d_up 1 (the same
 * walk, d s * table[row] summed per wave in slot order, the four waves in wave order).  d_table 4 (c_b per user; the zero
 * fill; the walk: the sorted positions are cut into G <= 8192 equal spans, a wave takes its span 64 positions at
 * a time, decodes them with a lane per position and adds d s * up[b] in sorted order -- a run of equal rows inside a span is stored at
 * once, the first and the last run of a span go to the workspace; the join adds the parts of a run that crosses span
 * bounds in ascending span order).  A row that every user lists is summed by as many waves as its run touches spans.
 * Determinism: scores, neg_scores, lse, loss and d_up of a user are the same bits on every run and depend neither on B
 * nor on the user's position in the batch: one workgroup owns the user and every reduction tree is fixed by the slot
 * position.  d_table is the same bits on every run of the same call; its summation order follows the sorted order and the
 * span cut, so it MAY differ in the last bits between batches.  The 16-byte and the scalar load forms add the same elements
 * in the same order: the alignment of an operand does not change a bit.  No float atomics, results cross launches at
 * kernel boundaries only, no host synchronisation, no allocation, hipGraph-capturable.  XNRS_EINVAL (L < 0, E < 1, a NULL
 * required pointer, order and d_table not NULL together) and XNRS_EWORKSPACE are found on the host before any launch and
 * write nothing.  B == 0: XNRS_OK, nothing written.  Any E >= 1, any operand alignment its element type allows (E % 4 != 0
 * or a base off the 16-byte boundary takes scalar loads).
 * ws: xnrs_list_loss_workspace_bytes(B, L, T, E, want_d_table), a pure host call: 0 for the forward and for d_up alone (ws
 * may then be NULL); with d_table 4 B + 8 G E + 8 G bytes, G = min(8192, ceil(B (L + 1) / 64)), each region rounded up to
 * 256 B -- 1/32 of the (B, L, E) copy or less.  (T does not enter: the spans are cut on the device.) */
size_t xnrs_list_loss_workspace_bytes(int64_t B, int32_t L, int64_t T, int32_t E, int32_t want_d_table);
int32_t xnrs_list_loss_fwd(const float *table, int64_t n_rows, int32_t E, const float *up, const float *bias, int64_t B,
                           const int64_t *tgt_off, const int32_t *tgt_rows, const int32_t *neg_rows, int32_t L,
                           int32_t pad_row, float *scores, float *loss, float *lse, float *neg_scores, void *ws,
                           size_t ws_bytes, void *stream);
int32_t xnrs_list_loss_bwd(const float *table, int64_t n_rows, int32_t E, const float *up, const float *bias, int64_t B,
                           const int64_t *tgt_off, const int32_t *tgt_rows, const int32_t *neg_rows, int32_t L,
                           int32_t pad_row, const float *scores, const float *lse, const float *neg_scores, const float *g,
                           const int32_t *order, float *d_up, float *d_table, void *ws, size_t ws_bytes, void *stream);

/* ---- the soft-target loss over per-user row LISTS: distilling a re-ranker, graded labels (csrc/list_loss.hip) ---------------
 * The listwise loss whose target is a DISTRIBUTION over the listed rows instead of one click: the cross-entropy between
 * the per-slot weights a caller gives (the softmax of a teacher's scores: distillation; graded labels: ListNet) and the
 * softmax of the user's own scores over the same slots.  Forward and backward, without a (B, L, E) copy of the listed rows.
 * Operands: table:(n_rows,E), up:(B,E) as the score reads it, bias: one float on the device or NULL, pad_row -- as
 * xnrs_list_loss_* -- plus rows:(B,L) int32 and weights:(B,L) fp32, both row-major.  There are no queries.
 *   Filled slot: slot (b, j) is FILLED when 0 <= rows[b][j] < n_rows and the row is not pad_row.  Every other slot is EMPTY:
 *              the -1 fillers of xnrs_topk_deep, ids outside the table, the pad row; its row is compared, never
 *              dereferenced, its weight is ignored (it may be anything, NaN included), slot_scores holds NaN there.  A ROW
 *              LISTED TWICE IS TWO SLOTS.  Unlike xnrs_list_loss_* nothing else empties a slot: a click is a row like any other.
 *   Weights  : must be finite on the filled slots; they need not sum to 1 and may be 0 (or negative).
 *   Forward  : s_bj = <table[row], up[b]> (+ bias), the dot chain of xnrs_list_loss_fwd; slot_scores[b][j] = s_bj.
 *              lse[b] = log sum_{filled} exp(s_bj), max-stabilised, -inf when b has no filled slot.  With W_b = sum_{filled}
 *              w_bj: loss[b] = sum_{filled} w_bj (lse[b] - s_bj), summed in THIS form term by term (never W_b lse - sum w s,
 *              which cancels at large scores), in the fixed slot tree of the sum exp; a term's lse[b] - s_bj is evaluated as
 *              (m - s_bj) + log sum exp(s - m), m the largest score, so the rounding of lse to the ulp of m does not enter;
 *              and that log as log(c) + log1p(r / c), c the number of slots at the maximum and r the sum over the others, so a
 *              sum of 1 + a little is not rounded to the ulp of 1 (the loss of a confident user IS that little).
 *              With W_b = 1 it is the cross-entropy of the target distribution against softmax(s).
 *   Zero cases: a user with no filled slot, or with all weights 0, has loss = 0 exactly and every gradient exactly 0; no NaN.
 *              L == 0: every user is one.
 *   Backward : g:(B) the upstream gradient per user, p_bj = exp(s_bj - lse[b]); d s_bj = g[b] (W_b p_bj - w_bj) per filled
 *              slot; d_up[b] = sum_j d s_bj * table[row]; d_table[n] = sum over the slots whose row is n of d s_bj * up[b].
 *              d_up:(B,E) and d_table:(n_rows,E) are OVERWRITTEN (rows that nothing lists are exactly zero); either may be
 *              NULL, and then its launches are skipped.  lse and slot_scores are what the forward call over the same
 *              operands wrote.  bias shifts every score of a user alike and gets no gradient.
 *   order    : (B L) int32, NULL iff d_table is NULL (one without the other: XNRS_EINVAL): the slots -- slot (b, j) is entry
 *              b L + j -- sorted ascending by row, ties in ascending entry index, the empty slots (NaN in slot_scores) behind
 *              all others: the order of xnrs_list_loss_bwd with no queries (xnrs_amd/ops.py: list_xent_order).  A value
 *              outside [0, B L) is skipped and never dereferenced.  An order that is NOT grouped by row gives unspecified
 *              gradients for the rows concerned and nothing worse: no access outside the operands.
 *   Precondition: table and up are finite; B L <= 2^31 - 1 and n_rows <= 2^31 - 1 (else XNRS_EINVAL).
 * Launches: forward 1 (a workgroup of four waves per user: the gather walk of xnrs_list_loss_fwd, then max, sum exp and the
 * weighted sum over the slots).  d_up 1 (W_b in the slot tree, then the same walk, d s * table[row] summed per wave in slot
 * order, the four waves in wave order).  d_table 4 (W_b per user; the zero fill; the walk and the join of
 * xnrs_list_loss_bwd -- the same two kernels, only the decode of a sorted position into (row, user, d s) differs).
 * Determinism: loss, lse, slot_scores and d_up of a user are the same bits on every run and depend neither on B nor on the
 * user's position in the batch: one workgroup owns the user and every reduction tree is fixed by the slot position.
 * d_table is the same bits on every run of the same call; its summation order follows the sorted order and the span cut, so
 * it MAY differ in the last bits between batches.  The 16-byte and the scalar load forms add the same elements in the same
 * order: the alignment of an operand does not change a bit.  No float atomics, results cross launches at kernel boundaries
 * only, no host synchronisation, no allocation, hipGraph-capturable.  XNRS_EINVAL (L < 0, E < 1, a NULL required pointer,
 * order and d_table not NULL together) and XNRS_EWORKSPACE are found on the host before any launch and write nothing.
 * B == 0: XNRS_OK, nothing written.  Any E >= 1, any operand alignment its element type allows (E % 4 != 0 or a base off the
 * 16-byte boundary takes scalar loads).  The user vector sits in LDS up to 4096 floats and is read from global memory beyond.
 * ws: xnrs_list_xent_workspace_bytes(B, L, E, want_d_table), a pure host call: 0 for the forward and for d_up alone (ws may
 * then be NULL); with d_table 4 B + 8 G E + 8 G bytes, G = max(1, min(8192, ceil(B L / 64))), each of the five regions (W_b,
 * head rows, tail rows, head row ids, tail row ids) rounded up to 256 B. */
size_t xnrs_list_xent_workspace_bytes(int64_t B, int32_t L, int32_t E, int32_t want_d_table);
int32_t xnrs_list_xent_fwd(const float *table, int64_t n_rows, int32_t E, const float *up, const float *bias, int64_t B,
                           const int32_t *rows, const float *weights, int32_t L, int32_t pad_row, float *loss, float *lse,
                           float *slot_scores, void *ws, size_t ws_bytes, void *stream);
int32_t xnrs_list_xent_bwd(const float *table, int64_t n_rows, int32_t E, const float *up, const float *bias, int64_t B,
                           const int32_t *rows, const float *weights, int32_t L, int32_t pad_row, const float *lse,
                           const float *slot_scores, const float *g, const int32_t *order, float *d_up, float *d_table,
                           void *ws, size_t ws_bytes, void *stream);

/* ---- diverse lists: MMR re-ranking and intra-list distance over the table's own vectors (csrc/diversity.hip) ---------------
 * Beyond-accuracy measures of a recommended list, and the re-ranking that trades relevance for variety.  Both rest on ONE
 * similarity of two rows a, b of table:(n_rows,E) fp32 (the encoded news vectors, not a scorer's prepared table):
 *   inv[r]    = 1 / sqrt(sum_e x[r][e]^2), 0 when the sum is 0        (xnrs_row_inv_norms, once per encoded table)
 *   cos(a, b) = (sum_e x[a][e] x[b][e]) * inv[a] * inv[b]
 * one device function: a lane's fp32 fma chain over the elements [4 l, 4 l + 4) + 256 j in ascending j, a butterfly over the 64
 * lanes, then the two products.  The order is a function of E alone -- not of B, P, k, the session's place in the batch or an
 * operand's alignment (E % 4 != 0 or a table off the 16-byte boundary takes scalar loads of the same elements in the same
 * order).  A zero row has inv = 0: its cosines are 0, never NaN.  table must be finite.
 *
 * xnrs_row_inv_norms: inv_out:(n_rows,) fp32; one wave per row, one read of the table, no copy of it.
 *
 * xnrs_mmr_rerank: greedy maximal marginal relevance over a candidate list per session, e.g. the rows and scores of
 * xnrs_topk_deep*.  pool_rows:(B,P) int32, pool_scores:(B,P) fp32.  A place i is VALID when 0 <= pool_rows[b][i] < n_rows and
 * its score is finite; every other place (the -1 fillers, ids outside the table, NaN, +-inf) is ignored, its row compared and
 * never dereferenced.  A row listed at two places is two candidates.
 *   relevance r_i : XNRS_MMR_REL_RAW: the score s_i; XNRS_MMR_REL_MINMAX: (s_i - s_min) / (s_max - s_min) over the session's
 *                   valid places, 0 when s_max == s_min (s_max - s_min must be finite).
 *   for t = 0 .. k-1: among the valid places not yet selected pick the largest obj_i = lam * r_i - (1 - lam) * m_i, m_i = the
 *                   largest cos(row_i, row_j) over the places j selected so far, m_i = 0 at t = 0; the two products and the
 *                   difference are each rounded to fp32 (at lam = 1 the objective is r_i exactly).  Equal objectives (==, so
 *                   -0 and +0 tie) go to the lower place.
 *   out_rows[b][t] = the row, out_scores[b][t] = the pool's score, ITS OWN BITS (never recomputed), out_pos[b][t] = the place
 *                   (int32).  Once the valid places run out: -1 / -inf / -1.
 * Hence: at lam = 1 a pool in the order of xnrs_topk_deep* comes back as its own first k places; mmr(k)[:, :j] == mmr(j);
 * a session's outputs depend on nothing but its own pool -- not on B or its position in the batch -- and are the same bits on
 * every run.  One launch, one workgroup per session with the session's state in LDS (relevance, m, the alive flags and the row
 * selected last); the pool's rows are streamed again every step, about k P E 4 bytes per session.  No workspace, no float
 * atomics, no host synchronisation, no allocation, hipGraph-capturable.
 * Limits: 1 <= k <= P <= XNRS_TOPK_DEEP_MAX_K, 0 <= lam <= 1 (NaN refused), 1 <= E <= XNRS_DIVERSITY_MAX_E (the row in LDS),
 * n_rows <= 2^31 - 1, rel_mode one of the two.  A violation returns XNRS_EINVAL on the host before any launch and writes
 * nothing.  B == 0: XNRS_OK, nothing written.
 *
 * xnrs_list_diversity: rows:(B,k) int32 lists (of xnrs_topk*, xnrs_mmr_rerank, anything); a place is valid when its row is
 * inside [0, n_rows).  Per session b:
 *   out_n[b]       = the number of valid places n (int32)
 *   out_ild[b]     = pair_sum / n_pairs, ONE fp32 division of the fp32 sum of 1 - cos(row_i, row_j) over the valid pairs i < j
 *                    by n (n - 1) / 2; 0 when n < 2.  A row listed twice is two places (their distance is 1 - cos of the row
 *                    with itself).  The order of the sum is a function of (k, E) alone.
 *   with row_cat:(n_rows,) int32 not NULL (else out_ncat / out_diffcat are not written and may be NULL; n_cat is still checked):
 *   out_ncat[b]    = the number of distinct categories among the valid places
 *   out_diffcat[b] = the number of valid pairs i < j whose categories differ
 *                    a category outside [0, n_cat) takes its place out of both counts.
 * Limits: 1 <= k <= XNRS_TOPK_MAX_K, 0 <= n_cat <= XNRS_DIVERSITY_MAX_CATEGORIES (an LDS histogram, integer atomics), E as
 * above; refusals, B == 0 and the launch properties as xnrs_mmr_rerank.  A session's outputs do not depend on the batch. */
#define XNRS_MMR_REL_RAW 0
#define XNRS_MMR_REL_MINMAX 1
#define XNRS_DIVERSITY_MAX_E 4096
#define XNRS_DIVERSITY_MAX_CATEGORIES 4096
int32_t xnrs_row_inv_norms(const float *table, int64_t n_rows, int32_t E, float *inv_out, void *stream);
int32_t xnrs_mmr_rerank(const float *table, const float *inv, int64_t n_rows, int32_t E, const int32_t *pool_rows,
                        const float *pool_scores, int64_t B, int32_t P, int32_t k, float lam, int32_t rel_mode,
                        int32_t *out_rows, float *out_scores, int32_t *out_pos, void *stream);
int32_t xnrs_list_diversity(const float *table, const float *inv, int64_t n_rows, int32_t E, const int32_t *rows, int64_t B,
                            int32_t k, const int32_t *row_cat, int32_t n_cat, float *out_ild, int32_t *out_n,
                            int32_t *out_ncat, int32_t *out_diffcat, void *stream);

/* ---- calibrated lists: re-ranking towards a target category mix, and the miscalibration of a list (csrc/calibration.hip) ---
 * Does a user whose history is 70 % sports get a list in that proportion?  (Steck, "Calibrated Recommendations", RecSys
 * 2018.)  Only the categories of the listed rows are read, never a news vector.
 *   row_cat:(n_rows,) int32; a value outside [0, n_cat) is "no category".
 *   target:(B,n_cat) fp32 weights; w_c COUNTS when it is finite and > 0, anything else is 0.  W = the fp32 sum of the counting
 *   weights (it must stay finite), p_c = w_c / W (one fp32 division; a p_c that rounds to 0 is 0).  W == 0: the session has NO
 *   TARGET.
 *   KL(n, N) = sum over c with p_c > 0 of t_c(n_c, N),  t_c(n, N) = p_c * logf(p_c / ((1 - alpha) * (n / N) + alpha * p_c)),
 *   n / N = 0 at N == 0; every operation rounded to fp32 on its own, logf of OCML (<= 1 ulp), 1 - alpha one fp32 subtraction.
 *   0 <= KL <= -ln(alpha).  ORDER of every sum over categories (W, KL): thread t of 256 adds its terms c = t, t + 256, ... in
 *   ascending c from 0, a butterfly (xor 32, 16, .., 1) adds the 64 chains of a wave, the four wave sums are added as
 *   (w0 + w1) + (w2 + w3): a function of n_cat alone.  KL is ONE device function, shared by the two entry points below.
 *
 * xnrs_csr_category_counts: per list b of a CSR (off:(B+1) int64, rows int32 -- the shape of the exclusion CSR),
 * counts_out[b][c] = the number of its rows of category c.  A row outside [0, n_rows), pad_row (-1: none) or a row without a
 * category counts nowhere.  One workgroup per list, an LDS histogram with integer atomics, every output word written.
 *
 * xnrs_calibrated_rerank: pool_rows:(B,P) int32, pool_scores:(B,P) fp32, e.g. of xnrs_topk_deep*.  VALID places and the
 * relevance r_i (rel_mode XNRS_MMR_REL_RAW / XNRS_MMR_REL_MINMAX) are those of xnrs_mmr_rerank; a row outside the table is
 * never dereferenced, not in row_cat either; a row listed twice is two candidates.  State: the counts n_c of the categorised
 * picks so far, N = sum n_c.
 *   pen(c) for a candidate of category c = KL(n + e_c, N + 1), formed as (S1 - t_c(n_c, N + 1)) + t_c(n_c + 1, N + 1) with
 *          S1 = KL(n, N + 1) summed once per step in the order above; a candidate without a category: pen = KL(n, N);
 *          a session without a target: pen = 0 for every candidate.
 *   for t = 0 .. k-1: among the valid places not yet picked take the largest obj_i = lam * r_i - (1 - lam) * pen(cat_i), the
 *          two products and the difference each rounded to fp32 (at lam = 1 the objective is r_i exactly).  Equal objectives
 *          (==) go to the lower place.
 *   out_rows / out_scores (the pool's OWN BITS) / out_pos as xnrs_mmr_rerank; -1 / -inf / -1 once the valid places run out.
 *   out_kl[b] = KL(n, N) of the final counts, 0 without a target: what xnrs_list_calibration says of out_rows, bit for bit.
 * Hence: lam = 1, or no target at any lam, returns the first k valid places of a pool in the order of xnrs_topk_deep*;
 * cal(k)[:, :j] == cal(j); a session's outputs depend on its own pool and target only -- not on B, its position in the batch
 * or an operand's address (every load is of one element; there is no second code path) -- and are the same bits on every
 * run.  One launch, one workgroup of four waves per session, the state in LDS; row_cat[pool_rows] is read once and nothing
 * else of the table.  No workspace, no float atomics, no host synchronisation, no allocation, hipGraph-capturable.
 *
 * xnrs_list_calibration: rows:(B,k) int32 lists (of xnrs_topk*, xnrs_mmr_rerank, xnrs_calibrated_rerank, anything); a place
 * is valid when its row is inside [0, n_rows).  out_counts[b][c] (nullable) = the valid places of category c, out_n[b] = N =
 * their sum, out_kl[b] = KL(counts, N) (about -ln alpha at N == 0), 0 without a target.
 *
 * Limits: 1 <= k <= P <= XNRS_TOPK_DEEP_MAX_K (xnrs_list_calibration: 1 <= k <= XNRS_TOPK_DEEP_MAX_K), 1 <= n_cat <=
 * XNRS_DIVERSITY_MAX_CATEGORIES, 0 <= lam <= 1, 0 < alpha < 1 (NaN refused for both), n_rows <= 2^31 - 1, rel_mode one of the
 * two.  A violation returns XNRS_EINVAL on the host before any launch and writes nothing.  B == 0: XNRS_OK, nothing written. */
int32_t xnrs_csr_category_counts(const int64_t *off, const int32_t *rows, int64_t B, const int32_t *row_cat, int64_t n_rows,
                                 int32_t n_cat, int32_t pad_row, int32_t *counts_out, void *stream);
int32_t xnrs_calibrated_rerank(const int32_t *pool_rows, const float *pool_scores, int64_t B, int32_t P, int32_t k,
                               const int32_t *row_cat, int64_t n_rows, int32_t n_cat, const float *target, float lam,
                               float alpha, int32_t rel_mode, int32_t *out_rows, float *out_scores, int32_t *out_pos,
                               float *out_kl, void *stream);
int32_t xnrs_list_calibration(const int32_t *rows, int64_t B, int32_t k, const int32_t *row_cat, int64_t n_rows, int32_t n_cat,
                              const float *target, float alpha, float *out_kl, int32_t *out_n, int32_t *out_counts,
                              void *stream);

/* ---- layers.PersonalizedAttention (layers.py:72-102) and NPA's news encoder (npa.py:63-69) ------------------------------
 *   t_i = tanh(x_fc x_i)   e_i = q . t_i   s_i = exp(e_i) m_i   a_i = s_i / (sum_j s_j + 1e-8)   p = sum_i a_i x_i
 * (no max-stabilisation, the mask after the exp, an all-masked sequence pools to 0), then the optional head
 * y = W2 act(W0 p + b0) + b2.  The query is per sequence: sequence s scores with row q_idx[s] of q, the user's projected
 * embedding q_fc(user_embedder(uid)) -- q_idx = s / n_per_user replaces repeat_interleave (npa.py:67,80), q_idx = the
 * impression of a CSR candidate list serves evaluation.  x:(n_seq,L,D), m:(n_seq,L) fp32 or NULL; with ids, x and m are the
 * table ([n_table,L,D], [n_table,L]) and sequence s is its row ids[s].  y:(n_seq,E) (E = D without a head), a_out:(n_seq,L)
 * and hm:(n_seq) = clamp(sum m, 0, 1) nullable.  L <= 4096.
 *   fwd        ws: xnrs_personalized_saved_bytes of scratch
 *   fwd_train  the same arithmetic; `saved` (xnrs_personalized_saved_bytes) keeps tanh(x_fc x), a, p and the head's hidden
 *              layer for the backward
 *   bwd        dy:(n_seq,E) -> dwx / dbx (x_fc), dq:(n_q, hidden) = d loss / d q per QUERY ROW (the sequences sharing a row
 *              are summed in sequence order), the head's gradients, and dx:(n_seq,L,D) = a_i dp + (dpre . Wx)_i (the user
 *              tower's input; not with ids).  Every output nullable, written (not accumulated), no float atomics. */
typedef struct {
  const float *wx, *bx;   /* x_fc: Linear(D, hidden) weight [hidden][D], bias [hidden] (nullable) */
  const float *q;         /* projected queries, row r at q + r * q_ld */
  const int32_t *q_idx;   /* [n_seq] int32 device array: the query row of every sequence */
  int32_t hidden;
  int32_t q_ld;           /* row stride of q in floats (0 = hidden): two projections side by side in one GEMM output */
  int32_t n_q;            /* rows of q.  A sequence whose q_idx is outside [0, n_q) reads no query: its outputs are NaN, it
                           * passes no gradient, and XNRS_STATUS_QUERY_RANGE is set in the status word */
} xnrs_personalized_params;

size_t xnrs_personalized_saved_bytes(int64_t n_seq, int32_t L, int32_t D, int32_t A, int32_t E, int32_t has_head);
int32_t xnrs_personalized_fwd(const float *x, const float *m, const int32_t *ids, int64_t n_seq, int32_t L, int32_t D,
                              const xnrs_personalized_params *p, const xnrs_head_params *head, float *y, float *a_out,
                              float *hm, void *ws, size_t ws_bytes, void *stream);
int32_t xnrs_personalized_fwd_train(const float *x, const float *m, const int32_t *ids, int64_t n_seq, int32_t L, int32_t D,
                                    const xnrs_personalized_params *p, const xnrs_head_params *head, float *y, float *a_out,
                                    float *hm, void *saved, size_t saved_bytes, void *stream);
size_t xnrs_personalized_bwd_workspace_bytes(int64_t n_seq, int32_t L, int32_t D, int32_t A, int32_t E, int32_t has_head);
int32_t xnrs_personalized_bwd(const float *x, const int32_t *ids, int64_t n_seq, int32_t L, int32_t D,
                              const xnrs_personalized_params *p, const xnrs_head_params *head, const void *saved,
                              size_t saved_bytes, const float *dy, float *dx, float *dwx, float *dbx, float *dq, int64_t n_q,
                              const xnrs_head_grads *g_head, void *ws, size_t ws_bytes, void *stream);

/* nn.Embedding backward at table scale (npa.py:12-15: 703 790 rows, NO padding row): d_table:(n_rows,K) = zeros except
 * row ids[m] += d_rows[m] -- one 16-byte-store zero fill, then one workgroup per id; the workgroup of an id's first
 * occurrence sums all its occurrences in batch order (no atomics).  Cost: the ids, not the table.  Ids outside
 * [0, n_rows) are skipped. */
int32_t xnrs_embedding_grad_sparse(const float *d_rows, const int32_t *ids, int64_t M, int32_t K, float *d_table,
                                   int32_t n_rows, void *stream);
/* xnrs_embedding_linear_bwd with that table gradient (fc(embedder(ids)) with a large table: NPA's stacked q_fc
 * projections): the same arguments, workspace size and M == 0 rule; the two sum an id's occurrences in different orders. */
size_t xnrs_embedding_linear_bwd_sparse_workspace_bytes(int64_t M, int32_t N, int32_t K);
int32_t xnrs_embedding_linear_bwd_sparse(const float *table, const int32_t *ids, const float *w, const float *dy,
                                         float *d_table, float *dw, float *db, int64_t M, int32_t N, int32_t K, int32_t n_rows,
                                         void *ws, size_t ws_bytes, void *stream);

/* ---- nn.GRU, one layer, batch_first (LSTUR's short-term user tower, lstur.py:113-154) --------------------------------------
 * x:(B,T,E) the first T history vectors of every user, m: fp32 0/1 history mask, row b at m + b * ldm (ldm >= T; NULL: every
 * row is full), h0:(B,Hd) or NULL (zeros) -> y:(B,Hd), the hidden state after step len_b - 1 with len_b = sum_t m[b][t].  The
 * GRU reads the FIRST len_b slots of a row wherever the mask's ones are (pack_padded_sequence, lstur.py:141-145); len_b is
 * computed on the device (no host read).  A row with len_b == 0 returns its initial state (the reference raises there).
 * Weights in nn.GRU's layout: w_ih [3Hd][E], w_hh [3Hd][Hd], b_ih / b_hh [3Hd] (nullable), gate order r, z, n:
 *   r = s(W_ir x + b_ir + W_hr h + b_hr)   z = s(W_iz x + b_iz + W_hz h + b_hz)   n = tanh(W_in x + b_in + r (W_hn h + b_hn))
 *   h' = (1 - z) n + z h
 * The input projection of all B*T rows is one dense GEMM; the recurrence runs one launch per step (or one launch in all:
 * knob XNRS_GRU_LAYOUT=1); no atomics, no grid-wide barrier, no host synchronisation: hipGraph-capturable, bit-identical
 * run to run.
 *   fwd        ws: xnrs_gru_workspace_bytes of scratch
 *   fwd_train  the same arithmetic; `saved` (xnrs_gru_saved_bytes) keeps the gates r | z | n, W_hn h + b_hn and the state
 *              before every step
 *   bwd        dy:(B,Hd) -> dx:(B,T,E), dh0:(B,Hd) and the four parameter gradients, every output nullable, written (not
 *              accumulated).  BPTT over the steps in reverse (dh_{t-1} = dGh_t . W_hh + z dh_t), then ONE product each over
 *              the stacked B*T rows: dW_hh = dGh^T . H_prev, dW_ih = dGi^T . X, dX = dGi . W_ih; bias gradients = column sums.
 *              ws: xnrs_gru_bwd_workspace_bytes. */
typedef struct {
  const float *w_ih, *w_hh, *b_ih, *b_hh;
  int32_t hidden; /* Hd */
} xnrs_gru_params;
typedef struct {
  float *w_ih, *w_hh, *b_ih, *b_hh;
} xnrs_gru_grads;
size_t xnrs_gru_workspace_bytes(int64_t B, int32_t T, int32_t E, int32_t Hd);
size_t xnrs_gru_saved_bytes(int64_t B, int32_t T, int32_t E, int32_t Hd);
int32_t xnrs_gru_fwd(const float *x, const float *m, int32_t ldm, const float *h0, const xnrs_gru_params *p, float *y,
                     int64_t B, int32_t T, int32_t E, void *ws, size_t ws_bytes, void *stream);
int32_t xnrs_gru_fwd_train(const float *x, const float *m, int32_t ldm, const float *h0, const xnrs_gru_params *p, float *y,
                           int64_t B, int32_t T, int32_t E, void *saved, size_t saved_bytes, void *stream);
size_t xnrs_gru_bwd_workspace_bytes(int64_t B, int32_t T, int32_t E, int32_t Hd);
int32_t xnrs_gru_bwd(const float *x, const xnrs_gru_params *p, const void *saved, size_t saved_bytes, const float *dy,
                     float *dx, float *dh0, const xnrs_gru_grads *g, int64_t B, int32_t T, int32_t E, void *ws,
                     size_t ws_bytes, void *stream);

/* ---- CAUM's candidate-aware user tower (xnrs/models/full_models/caum.py:31-111) -------------------------------------------
 * Additive to ABI 6.  P = B * C (user, candidate) pairs, row (b, i, j) = pair p = b * C + i, history slot j.
 *
 * Long attention: unmasked softmax(Q K^T / sqrt(d_k)) V per head over a packed Q|K|V image at ANY length (caum.py:92 runs
 * nn.MultiheadAttention without batch_first on a (P, H, E) view: the attended axis is P, hundreds to thousands long).
 *   qkv : element (l, nb, col) at qkv[l * seq_stride + nb * batch_stride + col], l < L, nb < Nb; q | k | v at columns
 *         0 | E | 2E, head h at columns [h d_k, (h + 1) d_k) of each (nn.MultiheadAttention's in_proj layout); a contiguous
 *         seq-first (L, Nb, 3E) image has seq_stride = Nb * 3E, batch_stride = 3E
 *   o   : (l, nb, col) at o[l * o_seq_stride + nb * o_batch_stride + col], heads concatenated (the out_proj input)
 * Any L >= 1, Nb >= 1, d_k = E / n_heads from 1 to 128 (XNRS_EHEADS when E % n_heads != 0, XNRS_EUNSUPPORTED above 128).
 * Online softmax over 32-key tiles: the L x L scores never reach memory.
 *   fwd_train  also keeps the log-sum-exp of every score row in `saved` (xnrs_attn_long_saved_bytes)
 *   bwd        d_o (addressed like o) -> dqkv (addressed like qkv, every element written); the probabilities are recomputed
 *              from `saved`.  ws: xnrs_attn_long_workspace_bytes.  No float atomics: bit-identical run to run. */
size_t xnrs_attn_long_saved_bytes(int64_t L, int64_t Nb, int32_t E, int32_t n_heads);
size_t xnrs_attn_long_workspace_bytes(int64_t L, int64_t Nb, int32_t E, int32_t n_heads);
int32_t xnrs_attn_long_fwd(const float *qkv, int64_t seq_stride, int64_t batch_stride, float *o, int64_t o_seq_stride,
                           int64_t o_batch_stride, int64_t L, int64_t Nb, int32_t E, int32_t n_heads, void *stream);
int32_t xnrs_attn_long_fwd_train(const float *qkv, int64_t seq_stride, int64_t batch_stride, float *o, int64_t o_seq_stride,
                                 int64_t o_batch_stride, int64_t L, int64_t Nb, int32_t E, int32_t n_heads, void *saved,
                                 size_t saved_bytes, void *stream);
int32_t xnrs_attn_long_bwd(const float *qkv, int64_t seq_stride, int64_t batch_stride, const float *o, const float *d_o,
                           int64_t o_seq_stride, int64_t o_batch_stride, const void *saved, size_t saved_bytes, float *dqkv,
                           int64_t L, int64_t Nb, int32_t E, int32_t n_heads, void *ws, size_t ws_bytes, void *stream);

/* Pair broadcast / combine (caum.py:70-89 without its (B, C, H, 4E) and (B, C, H, 2E) concatenations).  With
 * linear1.weight = [Wl | Wm | Wr | Wc] and linear2.weight = [W2c | W2h]:
 *   hp:(B*H, 4E) = h' . [Wl; Wm; Wr; W2h]^T      cp: row p at cp + p * ld_cp, columns 0:E = Wc c' + b1, E:2E = W2c c' + b2
 *   h_cnn[b,i,j] = hp[b, (j-1) mod H, 0:E] + hp[b, j, E:2E] + hp[b, (j+1) mod H, 2E:3E] + cp[b,i, 0:E]        (B*C*H, E)
 *   z[b,i,j]     = hp[b, j, 3E:4E] + cp[b,i, E:2E]                                                            (B*C*H, E)
 * bwd: d_hp = sums over the candidates with the shifts inverted, d_cp (row pitch ld_dcp, columns 0:2E) = sums over the
 * slots; each nullable, fixed order, no atomics.  H = 1: left, middle and right are the same slot. */
int32_t xnrs_caum_pair_fwd(const float *hp, const float *cp, int64_t ld_cp, float *h_cnn, float *z, int64_t B, int32_t C,
                           int32_t H, int32_t E, void *stream);
int32_t xnrs_caum_pair_bwd(const float *d_hcnn, const float *d_z, float *d_hp, float *d_cp, int64_t ld_dcp, int64_t B,
                           int32_t C, int32_t H, int32_t E, void *stream);

/* t[p*H + j, :] = tanh(pre[p*H + j, :] + cb[p, :]) -- the candidate half of dense_att.linear (layers.py:163,170 under
 * caum.py:100-101) added per row; cb: row p at cb + p * ld_cb.  bwd: dpre = dt (1 - t^2), dcb:(P, E) = sum_j dpre (nullable). */
int32_t xnrs_caum_bias_tanh_fwd(const float *pre, const float *cb, int64_t ld_cb, float *t, int64_t P, int32_t H, int32_t E,
                                void *stream);
int32_t xnrs_caum_bias_tanh_bwd(const float *t, const float *dt, float *dpre, float *dcb, int64_t P, int32_t H, int32_t E,
                                void *stream);
/* dpre[i] = dy[i] f'(y[i]) for an activation fused into xnrs_linear_fwd (y = act(pre)): tanh 1 - y^2, relu (y > 0), none 1 */
int32_t xnrs_act_bwd(const float *y, const float *dy, float *dpre, int64_t n, int32_t act, void *stream);

/* Candidate pooling (caum.py:101-109): s_j = w3 . t2[p, j] + b3, a = softmax_j(s) over the H slots of pair p (NO mask),
 * u[p] = sum_j a_j h_all[p, j].  t2:(P*H, A) the activated second layer of dense_att, w3:(A), b3:(1) nullable,
 * h_all:(P*H, E) -> u:(P, E), a_out:(P, H) nullable (the backward needs it).  H <= 8192.
 * bwd: du:(P, E) -> d_t2, d_w3:(A), d_b3:(1), d_hall, each nullable; d_b3 is the sum of the score gradients, which cancels
 * analytically (a bias in front of a softmax): each pair's share is summed in double around the weighted mean of its
 * score gradients, so what is written is the rounding of that mean, far below the reference's own summation noise.
 * ws: xnrs_caum_pool_bwd_workspace_bytes. */
int32_t xnrs_caum_pool_fwd(const float *t2, const float *w3, const float *b3, const float *h_all, float *u, float *a_out,
                           int64_t P, int32_t H, int32_t A, int32_t E, void *stream);
size_t xnrs_caum_pool_bwd_workspace_bytes(int64_t P, int32_t H, int32_t A);
int32_t xnrs_caum_pool_bwd(const float *t2, const float *w3, const float *h_all, const float *a, const float *du, float *d_t2,
                           float *d_w3, float *d_b3, float *d_hall, int64_t P, int32_t H, int32_t A, int32_t E, void *ws,
                           size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XNRS_HIP_H */
