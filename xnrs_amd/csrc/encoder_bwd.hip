// Training: the forward that keeps its activations (thin wrappers over seq_encode), the backward of the sequence
// encoders with its side lane, the weight / input gradient products (gemm_dw, gemm_dx) and the linear-layer backward.
#include <mutex>

#include "host.h"

using namespace xnrs;

namespace {

// ---- side lane of the backward (round 4).  A backward call is two dependency chains: the input-gradient chain (dX products,
// pooling and attention backward -- the critical path) and the weight-gradient products hanging off it (dW GEMM + split-K
// reduction + bias sums: 3-4 launches of 7-25 us per parameter pair, most of them far too small to fill 256 CUs).  Issued on
// one stream they serialise: 230 launches under 30 us made up 2.1 of the 8.1 ms of the NRMS grad step.  The weight-gradient
// launches go to ONE library-owned stream per device instead, ordered behind their producers by events (fork) and joined
// back into the caller's stream before the entry point returns -- so for the caller the call is still "everything enqueued
// on my stream": what follows on that stream sees every result, workspaces may be reused right after the call, and a
// hipGraph capture of the caller's stream captures the fork / join as graph edges.  No host synchronisation.  Results are
// bitwise the same (the same launches, no atomics).  Off: XNRS_BWD_SIDE_STREAM=0, and while the launch timer is on (its stage
// times would overlap).
struct SideLane {
  hipStream_t side = nullptr;
  hipEvent_t ev[32] = {};
  unsigned next = 0;
  bool ok = false, tried = false;
};
constexpr int MAX_LANES = 64;
SideLane g_lanes[MAX_LANES];
std::mutex g_lane_mu;

SideLane* side_lane(hipStream_t main) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_LANES) return nullptr;
  SideLane& l = g_lanes[dev];
  std::lock_guard<std::mutex> lk(g_lane_mu);
  if (!l.tried) {
    // (never created under a stream capture -- resource creation is not a capturable call: a capture whose warm-up did not
    // run a backward simply keeps one stream)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(main, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;
    l.tried = true;
    bool good = hipStreamCreateWithFlags(&l.side, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; good && i < 32; ++i) good = hipEventCreateWithFlags(&l.ev[i], hipEventDisableTiming) == hipSuccess;
    l.ok = good;
  }
  return l.ok ? &l : nullptr;
}

class Fork {
 public:
  Fork(hipStream_t main, bool want) : main_(main) {
    if (want && knobs().bwd_side_stream && g_prof_mask == 0) lane_ = side_lane(main);
  }
  // the stream for work that depends on everything issued on the caller's stream SO FAR (the caller's stream itself when the
  // lane is off or an event call fails)
  hipStream_t after_main() {
    if (!lane_) return main_;
    hipEvent_t e = next_event();
    if (hipEventRecord(e, main_) != hipSuccess || hipStreamWaitEvent(lane_->side, e, 0) != hipSuccess) {
      join();
      lane_ = nullptr;
      return main_;
    }
    used_ = true;
    return lane_->side;
  }
  // the caller's stream waits for the lane (idempotent; the destructor calls it on every return path)
  void join() {
    if (!lane_ || !used_) return;
    hipEvent_t e = next_event();
    if (hipEventRecord(e, lane_->side) == hipSuccess) (void)hipStreamWaitEvent(main_, e, 0);
    used_ = false;
  }
  ~Fork() { join(); }
  Fork(const Fork&) = delete;
  Fork& operator=(const Fork&) = delete;

 private:
  hipEvent_t next_event() {
    std::lock_guard<std::mutex> lk(g_lane_mu);
    return lane_->ev[lane_->next++ & 31u];
  }
  hipStream_t main_;
  SideLane* lane_ = nullptr;
  bool used_ = false;
};

struct BwdPlan {
  size_t off_dh, off_dp, off_dseq, off_dpre, off_de, off_docat, off_dqkv, off_delta, off_slabs, off_colsum, off_wt;
  // folded out-projection (training): g = dp.Wo, c = dp.bo, dW', db'
  size_t off_g, off_c, off_dwf, off_dbf;
  size_t total;
};

size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

BwdPlan make_bwd_plan(int64_t n_seq, int L, int D, int A, int E, int n_heads, bool additive, bool head, bool pooled) {
  BwdPlan p{};
  const bool att = n_heads > 0;
  const size_t rows = (size_t)n_seq * L;
  Carver c;
  p.off_dh = c.take_if(pooled && head, (size_t)n_seq * E * F32);
  p.off_dp = c.take_if(pooled && head, (size_t)n_seq * D * F32);
  p.off_dseq = c.take_if(pooled, rows * D * F32);
  p.off_dpre = c.take_if(additive, rows * A * F32);
  p.off_de = c.take_if(additive, rows * F32);
  p.off_docat = c.take_if(att, rows * D * F32);
  p.off_dqkv = c.take_if(att, rows * 3 * D * F32);
  p.off_delta = c.take_if(att, (size_t)n_seq * n_heads * L * F32);
  const bool foldable = att && additive;
  p.off_g = c.take_if(foldable, (size_t)n_seq * D * F32);
  p.off_c = c.take_if(foldable, (size_t)n_seq * F32);
  p.off_dwf = c.take_if(foldable, (size_t)A * D * F32);
  p.off_dbf = c.take_if(foldable, (size_t)A * F32);
  // split-K slabs: the largest dW this pipeline produces
  size_t slabs = 0;
  if (att) slabs = max_sz(slabs, gemm_splitk_workspace_bytes(2 * (int64_t)D, D, rows));  // (dWk | dWv as one product)
  if (additive) slabs = max_sz(slabs, gemm_splitk_workspace_bytes(A, D, rows));
  if (foldable) slabs = max_sz(slabs, gemm_splitk_workspace_bytes(D, D, (int64_t)n_seq));  // dWo = dp^T po (+ W1^T dW')
  if (pooled && head) {
    slabs = max_sz(slabs, gemm_splitk_workspace_bytes(E, D, n_seq));
    slabs = max_sz(slabs, gemm_splitk_workspace_bytes(E, E, n_seq));
  }
  p.off_slabs = c.take(slabs);
  int maxn = 3 * D;
  if (A > maxn) maxn = A;
  if (E > maxn) maxn = E;
  p.off_colsum = c.take(colsum_workspace_bytes(maxn + 1));  // (+ 1: launch_colsum_wsum's column of ones)
  // one transposed weight at a time (gemm_dx): the largest of D x D, A x D, E x D, E x E
  size_t wdim = (size_t)D;
  if ((size_t)A > wdim) wdim = (size_t)A;
  if ((size_t)E > wdim) wdim = (size_t)E;
  p.off_wt = c.take(wdim * wdim * F32);
  p.total = c.total();
  return p;
}

// AdditivePoolBwdArgs over the saved activations; the caller sets the pooled gradient (dp, shift_*) and the value rows
AdditivePoolBwdArgs additive_pool_bwd_args(const float* x, const float* a, const float* t, const xnrs_additive_params* pool,
                                           float* dx, float* dpre, float* de, int64_t n_seq, int L, int D, int A) {
  AdditivePoolBwdArgs pa{};
  pa.x = x;
  pa.ldx = D;
  pa.a = a;
  pa.t = t;
  pa.w2 = pool->w2;
  pa.dx = dx;
  pa.lddx = D;
  pa.dpre = dpre;
  pa.de = de;
  pa.n_seq = n_seq;
  pa.N = L;
  pa.D = D;
  pa.A = A;
  return pa;
}

xnrs_row_lists live_lists(const int32_t* live_rows, const int32_t* live_src_rows, int64_t n_live) {
  xnrs_row_lists r{};
  r.live_rows = live_rows;
  r.live_src_rows = live_src_rows;
  r.n_live = n_live;
  return r;
}

}  // namespace

// dW[N,K] = dY^T[N,M] . X[M,K]   (A k-major = dY, B k-major = X), split-K over the M rows.
// x_rows: row gather on X (dense contraction); live: contract over listed rows only (LiveRows; it replaces x_rows).
// bias (optional): the bias gradient db[N] = sum_rows dY, produced by the same launch (the kernel adds up the dY chunks
// it stages; a separate column-sum pass re-read every dY from HBM: 8.6 % of the train step).
// second (optional): the product covers TWO parameters (DwSecond; dY columns side by side, the same contraction rows):
// one launch instead of two (needs split-K; else two calls)
hipError_t xnrs::gemm_dw(const float* dY, int64_t lddy, const float* X, RowIds x_rows, int64_t ldx, float* dW, int64_t M, int N,
                         int K, float* slabs, hipStream_t stream, LiveRows live, DwBias bias, int accumulate, DwSecond second) {
  const int64_t M_all = M;
  float *db = bias.db, *csum = bias.csum;
  if (live.rows) {
    M = live.n;
    if (M <= 0) {
      if (db) {
        hipError_t e0 = hipMemsetAsync(db, 0, (size_t)N * sizeof(float), stream);
        if (e0 != hipSuccess) return e0;
      }
      return hipMemsetAsync(dW, 0, (size_t)N * K * sizeof(float), stream);
    }
  }
  GemmArgs g = gemm_kmajor_ab(dY, lddy, X, ldx, dW, K, N, K, M);
  g.gather_ids = live.rows;
  g.gather_S = live.rows ? 1 : 0;
  g.b_gather_ids = live.rows ? live.x_rows : x_rows.ids;
  g.b_gather_S = live.rows ? 1 : x_rows.S;
  g.k_dev = live.rows ? live.n_dev : nullptr;  // the list's length on the device (M is then its capacity)
  g.accumulate = accumulate;
  const int ns = gemm_pick_splits(N, K, M, knobs().gemm_dw && gemm_dw_eligible(g));
  if (ns > 1) {
    g.slabs = slabs;
    g.nsplit = ns;
  }
  const bool fuse_db = db && csum && (lddy % 4 == 0) && (N % 4 == 0);  // the k-major vector path stages dY as 16-byte chunks
  if (second.dW2) {
    const int64_t per = ((M + ns - 1) / ns + 31) / 32 * 32;  // (the launcher's slice rule: is there really more than one?)
    if (ns <= 1 || (M + per - 1) / per <= 1 || (db && !fuse_db) || (!db != !second.db2)) {  // no split-K reduction to route the rows: two products
      hipError_t e1 = gemm_dw(dY, lddy, X, x_rows, ldx, dW, M_all, second.n1, K, slabs, stream, live, bias, accumulate);
      if (e1 != hipSuccess) return e1;
      return gemm_dw(dY + second.n1, lddy, X, x_rows, ldx, second.dW2, M_all, N - second.n1, K, slabs, stream, live,
                     {second.db2, csum}, accumulate);
    }
    g.C2 = second.dW2;
    g.c2_row0 = second.n1;
    g.colsum_out2 = second.db2;
  }
  if (fuse_db) {  // partials per K slice; the split-K reduction launch adds them up into db (GemmArgs::colsum_out)
    g.colsum = csum;
    g.colsum_out = db;
  }
  // M = the rows actually contracted (the live ones)
  ProfScope ps(7, 2.0 * (double)prof_count(7, g.k_dev, 0, M, stream) * N * K, stream);
  hipError_t e = launch_gemm_f32(g, stream);
  if (e != hipSuccess) return e;
  if (db && !fuse_db) return launch_colsum(dY, lddy, nullptr, M_all, N, db, csum, stream);  // all rows (the non-live ones are zero)
  return hipSuccess;
}

// dX[M,K] (+)= (dY[M,N] . W[N,K]) (*) f'(aux)
// With a scratch buffer (>= N*K floats) and enough rows, W is transposed first (a few MB, microseconds) so that
// the product runs on the forward-layout kernel -- both operands k-contiguous, raw buffer loads, 4 workgroups per
// CU: ~133 TF -- instead of the k-major variant (87 TF on the 80 000-row dX GEMMs of the NRMS train step).
// live (optional): the listed rows of dY and dX only, in place (the other rows of dY are zero; dX's are left as they are)
hipError_t xnrs::gemm_dx(const float* dY, int64_t lddy, const float* W, float* dX, int64_t lddx, int64_t M, int N, int K,
                         hipStream_t stream, float* wt_scratch, int accumulate, LiveRows live, DxAct act) {
  if (live.rows) {
    if (live.n <= 0) return hipSuccess;
    M = live.n;
  }
  const int64_t* m_dev = live.rows ? live.n_dev : nullptr;  // the list's length on the device (live.n is then its capacity)
  ProfScope ps(8, 2.0 * (double)prof_count(8, m_dev, 0, M, stream) * N * K, stream);
  if (m_dev && !wt_scratch) return hipErrorInvalidValue;  // device row counts: forward-layout kernel only
  const bool transposed = wt_scratch && (M >= 4096 || m_dev);
  if (transposed) {
    hipError_t e = launch_transpose(W, wt_scratch, N, K, stream);  // Wt[K][N]
    if (e != hipSuccess) return e;
  }
  GemmArgs g = transposed ? gemm_linear(dY, {}, lddy, wt_scratch, nullptr, dX, lddx, M, K, N)
                          : gemm_kmajor_b(dY, lddy, W, K, dX, lddx, M, K, N);
  if (live.rows) {
    g.gather_ids = live.rows;
    g.gather_S = 1;
    g.c_scatter = 1;
    g.m_dev = m_dev;
    g.m_fill_hint = 0.4f;
  }
  g.aux = act.aux;
  g.ldaux = act.ldaux;
  g.aux_mode = act.mode;
  g.accumulate = accumulate;
  return launch_gemm_f32(g, stream);
}

extern "C" {

size_t xnrs_seq_encoder_saved_bytes(int64_t n_seq, int32_t L, int32_t D, int32_t A, int32_t E, int32_t n_heads,
                                    int32_t pool_kind, int32_t has_head) {
  const bool pooled = pool_kind != XNRS_POOL_NONE;
  return make_plan(n_seq, L, D, A, E, n_heads > 0, pool_kind == XNRS_POOL_ADDITIVE, pooled && has_head, pooled, 0, true,
                   n_heads)
      .total;
}

size_t xnrs_seq_encoder_saved_qkv_offset(int64_t n_seq, int32_t L, int32_t D, int32_t A, int32_t E, int32_t n_heads,
                                         int32_t pool_kind, int32_t has_head) {
  const bool pooled = pool_kind != XNRS_POOL_NONE;
  return make_plan(n_seq, L, D, A, E, n_heads > 0, pool_kind == XNRS_POOL_ADDITIVE, pooled && has_head, pooled, 0, true, n_heads)
      .off_qkv;
}

int32_t xnrs_seq_encoder_fwd_train(const float* x, const float* m, const int32_t* ids, int64_t n_seq, int32_t L, int32_t D,
                                   const xnrs_mha_params* att, int32_t pool_kind, const xnrs_additive_params* pool,
                                   const xnrs_head_params* head, float* y, float* a_out, float* hm, void* saved,
                                   size_t saved_bytes, void* stream) {
  return xnrs_seq_encoder_fwd_train_live(x, m, ids, n_seq, L, D, att, pool_kind, pool, head, y, a_out, hm, saved, saved_bytes,
                                         nullptr, nullptr, 0, stream);
}

int32_t xnrs_seq_encoder_fwd_train_live(const float* x, const float* m, const int32_t* ids, int64_t n_seq, int32_t L, int32_t D,
                                        const xnrs_mha_params* att, int32_t pool_kind, const xnrs_additive_params* pool,
                                        const xnrs_head_params* head, float* y, float* a_out, float* hm, void* saved,
                                        size_t saved_bytes, const int32_t* live_rows, const int32_t* live_src_rows,
                                        int64_t n_live, void* stream) {
  const xnrs_row_lists r = live_lists(live_rows, live_src_rows, n_live);
  return xnrs_seq_encoder_fwd_train_rows(x, m, ids, n_seq, L, D, att, pool_kind, pool, head, y, a_out, hm, saved, saved_bytes,
                                         live_rows ? &r : nullptr, stream);
}

int32_t xnrs_seq_encoder_fwd_train_rows(const float* x, const float* m, const int32_t* ids, int64_t n_seq, int32_t L, int32_t D,
                                        const xnrs_mha_params* att, int32_t pool_kind, const xnrs_additive_params* pool,
                                        const xnrs_head_params* head, float* y, float* a_out, float* hm, void* saved,
                                        size_t saved_bytes, const xnrs_row_lists* r, void* stream) {
  const bool pooled = pool_kind != XNRS_POOL_NONE;
  xnrs_row_lists none{};
  if (!r) r = &none;
  if (r->kv_rows && !r->live_rows) return XNRS_EINVAL;  // the K|V list rides on the live-row path
  // a gathered table needs the table rows of the listed tokens
  if (ids && ((r->live_rows && !r->live_src_rows) || (r->kv_rows && !r->kv_src_rows))) return XNRS_EINVAL;
  SeqEncode q{};
  q.x = x; q.m = m; q.ids = ids; q.n_seq = n_seq; q.L = L; q.D = D;
  q.att = att; q.pooled = pooled; q.pool_kind = pool_kind; q.pool = pool; q.head = pooled ? head : nullptr;
  q.y = y; q.a_out = a_out; q.hm = hm;
  q.ws = saved; q.ws_bytes = saved_bytes; q.train = true; q.rl = r;
  return seq_encode(q, (hipStream_t)stream);
}

size_t xnrs_seq_encoder_bwd_workspace_bytes(int64_t n_seq, int32_t L, int32_t D, int32_t A, int32_t E, int32_t n_heads,
                                            int32_t pool_kind, int32_t has_head) {
  const bool pooled = pool_kind != XNRS_POOL_NONE;
  return make_bwd_plan(n_seq, L, D, A, E, n_heads, pool_kind == XNRS_POOL_ADDITIVE, pooled && has_head, pooled).total;
}

int32_t xnrs_seq_encoder_bwd(const float* x, const float* m, const int32_t* ids, int64_t n_seq, int32_t L, int32_t D,
                             const xnrs_mha_params* att, int32_t pool_kind, const xnrs_additive_params* pool,
                             const xnrs_head_params* head, const void* saved, size_t saved_bytes, const float* dy, float* dx,
                             const xnrs_mha_grads* g_att, const xnrs_additive_grads* g_pool, const xnrs_head_grads* g_head,
                             void* ws, size_t ws_bytes, void* stream_) {
  return xnrs_seq_encoder_bwd_live(x, m, ids, n_seq, L, D, att, pool_kind, pool, head, saved, saved_bytes, dy, dx, g_att,
                                   g_pool, g_head, nullptr, nullptr, 0, ws, ws_bytes, stream_);
}

int32_t xnrs_seq_encoder_bwd_live(const float* x, const float* m, const int32_t* ids, int64_t n_seq, int32_t L, int32_t D,
                                  const xnrs_mha_params* att, int32_t pool_kind, const xnrs_additive_params* pool,
                                  const xnrs_head_params* head, const void* saved, size_t saved_bytes, const float* dy,
                                  float* dx, const xnrs_mha_grads* g_att, const xnrs_additive_grads* g_pool,
                                  const xnrs_head_grads* g_head, const int32_t* live_rows, const int32_t* live_src_rows,
                                  int64_t n_live, void* ws, size_t ws_bytes, void* stream_) {
  const xnrs_row_lists r = live_lists(live_rows, live_src_rows, n_live);
  return xnrs_seq_encoder_bwd_rows(x, m, ids, n_seq, L, D, att, pool_kind, pool, head, saved, saved_bytes, dy, dx, g_att, g_pool,
                                   g_head, live_rows ? &r : nullptr, ws, ws_bytes, stream_);
}

int32_t xnrs_seq_encoder_bwd_rows(const float* x, const float* m, const int32_t* ids, int64_t n_seq, int32_t L, int32_t D,
                                  const xnrs_mha_params* att, int32_t pool_kind, const xnrs_additive_params* pool,
                                  const xnrs_head_params* head, const void* saved, size_t saved_bytes, const float* dy,
                                  float* dx, const xnrs_mha_grads* g_att, const xnrs_additive_grads* g_pool,
                                  const xnrs_head_grads* g_head, const xnrs_row_lists* rl, void* ws, size_t ws_bytes,
                                  void* stream_) {
  xnrs_row_lists none{};
  if (!rl) rl = &none;
  const int32_t* live_rows = rl->live_rows;
  const int32_t* live_src_rows = rl->live_src_rows;
  // counts on the device (xnrs_row_lists::counts_dev): n_live / n_kv are then the lists' capacities (every row)
  const int64_t* cnt = rl->counts_dev;
  const int64_t n_live = cnt ? n_seq * L : rl->n_live, n_kv = cnt ? n_seq * L : rl->n_kv;
  if (rl->kv_rows && !live_rows) return XNRS_EINVAL;
  if (rl->dqkv_mode != XNRS_DQKV_OWN && (rl->dqkv_mode < 0 || rl->dqkv_mode > XNRS_DQKV_MERGE || !att || !rl->dqkv_image || dx))
    return XNRS_EINVAL;
  if (ids && rl->kv_rows && !rl->kv_src_rows) return XNRS_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  if (n_seq == 0) return XNRS_OK;
  if (n_seq < 0 || L <= 0 || D <= 0 || !x || !dy) return XNRS_EINVAL;
  if (ids && dx) return XNRS_EINVAL;
  const bool pooled = pool_kind != XNRS_POOL_NONE;
  const bool additive = pool_kind == XNRS_POOL_ADDITIVE;
  if (!pooled) head = nullptr;
  if (att && att->n_heads <= 0) return XNRS_EINVAL;
  if (att && D % att->n_heads != 0) return XNRS_EHEADS;
  // the forward's limits (seq_encode), checked here before the first launch: launch_mha_bwd and launch_additive_pool_bwd
  // refuse the same shapes, but only after the head's products have been enqueued
  if (att && (L > 128 || D / att->n_heads > 128)) return XNRS_EUNSUPPORTED;
  if (pooled && L > 512) return XNRS_EUNSUPPORTED;
  if (additive && !pool) return XNRS_EINVAL;
  if (pool_kind == XNRS_POOL_MEAN && !m) return XNRS_EINVAL;
  const int A = additive ? pool->hidden : 0;
  const int E = head ? head->out_features : D;
  const int nh = att ? att->n_heads : 0;
  const Plan sp = make_plan(n_seq, L, D, A, E, att != nullptr, additive, head != nullptr, pooled, 0, true, nh);
  if (sp.total > saved_bytes || (sp.total > 0 && !saved)) return XNRS_EWORKSPACE;
  const BwdPlan bp = make_bwd_plan(n_seq, L, D, A, E, nh, additive, head != nullptr, pooled);
  if (bp.total > ws_bytes || (bp.total > 0 && !ws)) return XNRS_EWORKSPACE;
  const float* qkv = (att && rl->qkv_shared) ? rl->qkv_shared : at(saved, sp.off_qkv);
  const float *o = at(saved, sp.off_o), *yatt = at(saved, sp.off_y), *t = at(saved, sp.off_t), *pb = at(saved, sp.off_p);
  const float *hb = at(saved, sp.off_h), *stats = at(saved, sp.off_stats), *a_sv = at(saved, sp.off_a);
  float *dh = at(ws, bp.off_dh), *dp = at(ws, bp.off_dp), *dseq = at(ws, bp.off_dseq), *dpre = at(ws, bp.off_dpre);
  float *de = at(ws, bp.off_de), *docat = at(ws, bp.off_docat), *delta = at(ws, bp.off_delta);
  // (dqkv_mode: the caller's image shared by the two backward calls over one Q|K|V image, xnrs_row_lists)
  float* dqkv = rl->dqkv_mode != XNRS_DQKV_OWN ? rl->dqkv_image : at(ws, bp.off_dqkv);
  float *slabs = at(ws, bp.off_slabs), *csum = at(ws, bp.off_colsum), *wt = at(ws, bp.off_wt);
  const int64_t rows = n_seq * L;
  // Live rows (optional): the unmasked token rows.  A masked row has pooling weight 0, so every gradient that passes
  // through it is exactly zero (dy_i = a_i dp = 0, dpre_i = 0, dO_i = 0, dS_i = 0): the row-parallel GEMMs of the
  // attention tower run over the live rows only, in place.  K and V gradients stay dense (padded rows are keys).
  const bool live = live_rows && pooled && additive && m && (cnt || (n_live >= 0 && n_live < rows));
  if (cnt && live && !device_counts_ok(x, D, A, att, pool)) return XNRS_EUNSUPPORTED;
  const int64_t* cnt_live = (cnt && live) ? cnt : nullptr;
  const int32_t* lv = live ? live_rows : nullptr;
  const int32_t* lvx = live ? (live_src_rows ? live_src_rows : live_rows) : nullptr;
  if (live_rows && ids && !live_src_rows) return XNRS_EINVAL;  // a gathered table needs the table rows of the live tokens
  // K / V gradients over the token rows of the non-empty news (the forward's kv list): an all-masked news has no live query,
  // so its dK and dV rows are exactly zero
  const bool kvl = live && rl->kv_rows && (cnt || (n_kv >= 0 && n_kv < rows));
  const int64_t* cnt_kv = (cnt && kvl) ? cnt + 1 : nullptr;
  const int32_t* kvr = kvl ? rl->kv_rows : nullptr;
  const int32_t* kvx = kvl ? (rl->kv_src_rows ? rl->kv_src_rows : rl->kv_rows) : nullptr;
  // the row sets of the products below; each is dense (every row) while its list is off
  const LiveRows live_in{lv, lv, n_live, cnt_live};    // rows of a gradient image (dW: against the same rows of an activation image)
  const LiveRows live_inx{lv, lvx, n_live, cnt_live};  // ... against the live rows of x (table rows with ids)
  const LiveRows kv_inx{kvr, kvx, n_kv, cnt_kv};
  const bool fold = att && pooled && additive && fold_wanted(knobs().fold_train);  // = the forward's decision

  // weight-gradient launches go to the side lane (SideLane above in this file): `sw` = that stream, re-ordered behind the caller's stream
  // (after_main) wherever the input-gradient chain has produced what the next weight gradients read.  slabs / csum are
  // touched by lane launches only, wt by the chain only.
  // Where it pays (tools/bench_side_lane.py, B = 64 grad steps): the NRMS step, GPU-bound at ~30 us per launch, 7.93 -> 7.64
  // ms; the attention-free towers of StandardRec / NAML (1.4 / 3.3 ms steps of ~100 launches: the HOST is the limit there and
  // the fork / join calls only add to it) +6 % / +2 % -- so the lane serves towers with an attention stage and at least
  // XNRS_BWD_SIDE_MIN_ROWS token rows.
  Fork fk(stream, att != nullptr && rows >= knobs().bwd_side_min_rows);
  hipStream_t sw = stream;

  // gradient w.r.t. the sequence rows that fed the pooler (att output, or x itself)
  const float* dseq_src = nullptr;  // [rows, D]
  if (pooled) {
    // ---- head: y = W2 relu(W0 p + b0) + b2
    const float* dpool = dy;  // [n_seq, D]
    if (head) {
      sw = fk.after_main();  // (dy: produced on the caller's stream before this call)
      if (g_head && g_head->w2)
        XNRS_TRY(gemm_dw(dy, E, hb, {}, E, g_head->w2, n_seq, E, E, slabs, sw, {}, {g_head->b2, csum}));
      else if (g_head && g_head->b2) XNRS_TRY(launch_colsum(dy, E, nullptr, n_seq, E, g_head->b2, csum, sw));
      // f'(saved activation): relu' (aux mode 2), tanh' = 1 - t^2 (1), identity (0)
      const int hmode = head->activation == XNRS_ACT_RELU ? 2 : (head->activation == XNRS_ACT_TANH ? 1 : 0);
      XNRS_TRY(gemm_dx(dy, E, head->w2, dh, E, n_seq, E, E, stream, wt, 0, {}, {hmode ? hb : nullptr, E, hmode}));
      sw = fk.after_main();  // dh
      if (g_head && g_head->w0)
        XNRS_TRY(gemm_dw(dh, E, pb, {}, D, g_head->w0, n_seq, E, D, slabs, sw, {}, {g_head->b0, csum}));
      else if (g_head && g_head->b0) XNRS_TRY(launch_colsum(dh, E, nullptr, n_seq, E, g_head->b0, csum, sw));
      XNRS_TRY(gemm_dx(dh, E, head->w0, dp, D, n_seq, E, D, stream, wt));
      dpool = dp;
    }
    // ---- pooler
    if (fold) {
      // Folded out-projection (seq_encode "fold"; the forward saved O, tanh(W' O + b'), a, the pooled O rows and sum a):
      //   p = Wo po + bo s,  po = sum_i a_i O_i,  s = sum_i a_i;   pre_i = W' O_i + b',  W' = W1 Wo,  b' = W1 bo + b1
      //   g = Wo^T dp, c = dp . bo:  da_i = g . O_i + c,  dO_i = a_i g + dpre_i W'
      //   dW' = dpre^T O, db' = sum dpre:  dW1 = dW' Wo^T + db' (x) bo,  db1 = db'
      //   dWo = dp^T po + W1^T dW',  dbo = sum_n s_n dp_n + W1^T db'      (one stacked product / column sum each)
      // The three rows x D x D products of the per-token order (forward out-projection, dO = dY Wo, dWo = dY^T O) are gone.
      const float* wf = pool->w1_folded ? pool->w1_folded : at(saved, sp.fold.fw);  // (as the forward was given)
      const float *pob = at(saved, sp.fold.po), *asum = at(saved, sp.fold.as);
      float *gvec = at(ws, bp.off_g), *dwf = at(ws, bp.off_dwf);
      // db' IS db1 (see the algebra above): produced in place when the caller wants it (a device copy per call before)
      float* dbf = (g_pool && g_pool->b1) ? g_pool->b1 : at(ws, bp.off_dbf);
      XNRS_TRY(gemm_dx(dpool, D, att->wo, gvec, D, n_seq, D, D, stream, wt));

      // dO_i = a_i g into docat (every row written; masked rows get 0)
      AdditivePoolBwdArgs pa = additive_pool_bwd_args(o, a_sv, t, pool, docat, dpre, de, n_seq, L, D, A);
      pa.dp = gvec;
      pa.shift_u = att->bo ? dpool : nullptr;  // c_n = dp_n . bo, taken inside the kernel
      pa.shift_v = att->bo;
      XNRS_TRY(launch_additive_pool_bwd(pa, stream));
      sw = fk.after_main();  // dpool (dp), dpre, de
      XNRS_TRY(gemm_dx(dpre, A, wf, docat, D, rows, A, D, stream, wt, /*accumulate*/ 1, live_in));
      if (g_pool && g_pool->w2 && g_pool->b2) XNRS_TRY(launch_colsum_wsum(t, A, de, rows, A, g_pool->w2, g_pool->b2, csum, sw));
      else if (g_pool && g_pool->w2) XNRS_TRY(launch_colsum(t, A, de, rows, A, g_pool->w2, csum, sw));
      else if (g_pool && g_pool->b2) XNRS_TRY(launch_colsum(de, 1, nullptr, rows, 1, g_pool->b2, csum, sw));
      XNRS_TRY(gemm_dw(dpre, A, o, {}, D, dwf, rows, A, D, slabs, sw, live_in, {dbf, csum}));
      if (g_pool && g_pool->w1) {
        GemmArgs g1 = gemm_linear(dwf, {}, D, att->wo, nullptr, g_pool->w1, D, A, D, D);
        if (att->bo) {  // + db' (x) bo in the epilogue: fmaf(db'[a], bo[d], acc), the bits of the separate pass it replaces
          g1.rowscale = dbf;
          g1.rowscale_vec = att->bo;
        }
        XNRS_TRY(launch_gemm_f32(g1, sw));
      }
      // dWo = dp^T po + W1^T dW' as two products (the second accumulates), dbo = sum_n s_n dp_n + sum_a db'_a W1[a,:] as ONE
      // column sum over the two row blocks (round 3 staged [dp; W1] and [po; dW'] with six device copies per call)
      if (g_att && g_att->wo) {
        XNRS_TRY(gemm_dw(dpool, D, pob, {}, D, g_att->wo, n_seq, D, D, slabs, sw));
        XNRS_TRY(gemm_dw(pool->w1, D, dwf, {}, D, g_att->wo, A, D, D, slabs, sw, LiveRows{}, DwBias{}, /*accumulate*/ 1));
      }
      if (g_att && g_att->bo) XNRS_TRY(launch_colsum2(dpool, D, asum, n_seq, pool->w1, D, dbf, A, D, g_att->bo, csum, sw));

    } else {
    const float* seq = att ? yatt : x;
    const int32_t* seq_ids = att ? nullptr : ids;
    const bool need_dseq = att || dx;
    float* dseq_dst = att ? dseq : dx;  // no attention stage: the sequence rows ARE x
    if (additive) {
      AdditivePoolBwdArgs pa = additive_pool_bwd_args(seq, a_sv, t, pool, need_dseq ? dseq_dst : nullptr, dpre, de, n_seq, L, D, A);
      pa.dp = dpool;
      pa.x_gather_ids = seq_ids;
      XNRS_TRY(launch_additive_pool_bwd(pa, stream));
      sw = fk.after_main();  // dpre, de
      if (g_pool && g_pool->w2 && g_pool->b2) XNRS_TRY(launch_colsum_wsum(t, A, de, rows, A, g_pool->w2, g_pool->b2, csum, sw));
      else if (g_pool && g_pool->w2) XNRS_TRY(launch_colsum(t, A, de, rows, A, g_pool->w2, csum, sw));
      else if (g_pool && g_pool->b2) XNRS_TRY(launch_colsum(de, 1, nullptr, rows, 1, g_pool->b2, csum, sw));
      if (g_pool && g_pool->w1)  // live: rows of dpre through lv; rows of seq through lv (yatt) or lvx (x / table rows)
        XNRS_TRY(gemm_dw(dpre, A, seq, {seq_ids, L}, D, g_pool->w1, rows, A, D, slabs, sw, att ? live_in : live_inx, {g_pool->b1, csum}));
      else if (g_pool && g_pool->b1) XNRS_TRY(launch_colsum(dpre, A, nullptr, rows, A, g_pool->b1, csum, sw));
      if (need_dseq)
        XNRS_TRY(gemm_dx(dpre, A, pool->w1, dseq_dst, D, rows, A, D, stream, wt, /*accumulate*/ 1, live_in));
    } else if (need_dseq) {
      XNRS_TRY(launch_mean_pool_bwd(dpool, m, ids, dseq_dst, D, n_seq, L, D, stream));
    }
    dseq_src = dseq_dst;
    }
  } else {
    dseq_src = dy;  // MultiHeadAttention alone: dy is the gradient of the attention output
  }
  if (!att) return XNRS_OK;

  // ---- out projection: yatt = O Wo^T + bo   (folded: docat and the Wo / bo gradients are complete already)
  if (!fold) {
    sw = fk.after_main();  // the sequence-row gradient is complete (pooler: its fc1 dX product accumulated into it)
    if (g_att && g_att->wo)
      XNRS_TRY(gemm_dw(dseq_src, D, o, {}, D, g_att->wo, rows, D, D, slabs, sw, live_in, {g_att->bo, csum}));
    else if (g_att && g_att->bo) XNRS_TRY(launch_colsum(dseq_src, D, nullptr, rows, D, g_att->bo, csum, sw));
    if (live) XNRS_TRY(hipMemsetAsync(docat, 0, (size_t)rows * D * sizeof(float), stream));  // dO of a masked row is zero
    XNRS_TRY(gemm_dx(dseq_src, D, att->wo, docat, D, rows, D, D, stream, wt, 0, live_in));
  }
  // ---- attention core
  MhaBwdArgs mb{};
  mb.q = qkv;
  mb.k = qkv + D;
  mb.v = qkv + 2 * (int64_t)D;
  mb.ld = 3 * (int64_t)D;
  mb.mask = m;
  mb.mask_gather_ids = ids;
  mb.o = o;
  mb.ldo = D;
  mb.d_o = docat;
  mb.lddo = D;
  mb.stats = stats;
  mb.delta = delta;
  mb.dq = dqkv;
  mb.dk = dqkv + D;
  mb.dv = dqkv + 2 * (int64_t)D;
  mb.ldd = 3 * (int64_t)D;
  mb.n_seq = n_seq;
  mb.S = L;
  mb.n_heads = nh;
  mb.d_k = D / nh;
  mb.scaled = att->scaled;
  mb.dropout_p = att->dropout_p;
  mb.seed = att->seed;
  mb.seed_dev = att->seed_dev;
  mb.masked_do_is_zero = (pooled && m) ? 1 : 0;  // both poolers give masked rows a zero gradient
  // an all-masked news has dQ = dK = dV = 0: written without reading (1), or -- when every consumer goes through the row
  // lists and no input gradient is asked for -- not even written (2)
  // (a deferring call: the merging call that consumes its image reads it through the same lists -- the caller's contract)
  const bool lists_only = kvl && !dx && (rl->dqkv_mode == XNRS_DQKV_DEFER || (g_att && g_att->wq && g_att->wk && g_att->wv));  // (a bias-only gradient sums dense rows)
  mb.dead_seq_mode = live ? (lists_only ? 2 : 1) : 0;
  mb.accumulate = rl->dqkv_mode == XNRS_DQKV_MERGE ? 1 : 0;
  {
    ProfScope ps(9, 10.0 * rows * (double)L * D, stream);  // S, dP, dV, dK, dQ: five S x S x d_k products per head
    XNRS_TRY(launch_mha_bwd(mb, stream));
  }
  if (rl->dqkv_mode == XNRS_DQKV_DEFER) return XNRS_OK;  // the merging call computes the projection gradients from the sum
  sw = fk.after_main();  // dQ | dK | dV
  // ---- Q/K/V projections
  float* gw[3] = {g_att ? g_att->wq : nullptr, g_att ? g_att->wk : nullptr, g_att ? g_att->wv : nullptr};
  float* gb[3] = {g_att ? g_att->bq : nullptr, g_att ? g_att->bk : nullptr, g_att ? g_att->bv : nullptr};
  const float* wqkv[3] = {att->wq, att->wk, att->wv};
  // dWk | dWv as ONE product when both are wanted and contract over the same rows: the K and V columns of the image lie side
  // by side (A = the 2D columns from D on), X is staged once per tile for both, the split-K reduction routes the two halves
  // (and their bias sums) to the two parameters -- half the launches and K loops twice as long per workgroup
  bool kv_merged = false;
  if (gw[1] && gw[2] && !dx && (!gb[1] == !gb[2])) {
    XNRS_TRY(gemm_dw(dqkv + D, 3 * (int64_t)D, x, {ids, L}, D, gw[1], rows, 2 * D, D, slabs, sw, kv_inx, {gb[1], csum}, 0,
                     {gw[2], gb[2], D}));
    kv_merged = true;
  }
  for (int s3 = 0; s3 < 3; ++s3) {
    const float* dpart = dqkv + (int64_t)s3 * D;
    if (kv_merged && s3 > 0) continue;
    if (gw[s3]) {
      // dQ is zero on masked rows (live list); dK / dV are not (padded tokens are keys) except on the rows of an all-masked
      // news (kv list)
      XNRS_TRY(gemm_dw(dpart, 3 * (int64_t)D, x, {ids, L}, D, gw[s3], rows, D, D, slabs, sw, s3 == 0 ? live_inx : kv_inx,
                       {gb[s3], csum}));
    } else if (gb[s3]) {
      XNRS_TRY(launch_colsum(dpart, 3 * (int64_t)D, nullptr, rows, D, gb[s3], csum, sw));
    }
    if (dx) XNRS_TRY(gemm_dx(dpart, 3 * (int64_t)D, wqkv[s3], dx, D, rows, D, D, stream, wt, /*accumulate*/ s3 > 0 ? 1 : 0));
  }
  return XNRS_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- nn.Linear and fc(embedder(ids)) backward
// The gradients of an empty batch (M == 0) are zeros: every output that was asked for is written, nothing else is touched.
static int32_t zero_grads(float* dw, float* db, float* d_table, int N, int K, int n_rows, hipStream_t stream) {
  if (dw) XNRS_TRY(hipMemsetAsync(dw, 0, (size_t)N * K * F32, stream));
  if (db) XNRS_TRY(hipMemsetAsync(db, 0, (size_t)N * F32, stream));
  if (d_table) XNRS_TRY(hipMemsetAsync(d_table, 0, (size_t)n_rows * K * F32, stream));
  return XNRS_OK;
}

// dw, db = xnrs_linear_bwd over the gathered rows; d_table = the rows dy . W scattered by ids, summed per table row by
// launch_embedding_grad (one workgroup per TABLE row: small tables) or by xnrs_embedding_grad_sparse (one per ID: large ones)
int32_t xnrs::embedding_linear_bwd(const float* table, const int32_t* ids, const float* w, const float* dy, float* d_table,
                                   float* dw, float* db, int64_t M, int N, int K, int n_rows, void* ws, size_t ws_bytes,
                                   hipStream_t stream, bool sparse_table) {
  if (!table || !w || M < 0 || N <= 0 || K <= 0 || n_rows <= 0) return XNRS_EINVAL;
  if (M == 0) return zero_grads(dw, db, d_table, N, K, n_rows, stream);
  if (!ids || !dy) return XNRS_EINVAL;
  const size_t s1 = xnrs_linear_bwd_workspace_bytes(M, N, K);
  if (xnrs_embedding_linear_bwd_workspace_bytes(M, N, K) > ws_bytes || !ws) return XNRS_EWORKSPACE;
  if (dw || db) XNRS_TRY_RC(xnrs_linear_bwd(table, ids, 1, w, dy, nullptr, dw, db, M, N, K, ws, s1, stream));
  if (d_table) {
    float* d_rows = at(ws, s1);
    XNRS_TRY(gemm_dx(dy, N, w, d_rows, K, M, N, K, stream));
    if (sparse_table) XNRS_TRY_RC(xnrs_embedding_grad_sparse(d_rows, ids, M, K, d_table, n_rows, stream));
    else XNRS_TRY(launch_embedding_grad(d_rows, ids, M, K, d_table, n_rows, stream));
  }
  return XNRS_OK;
}

extern "C" {

size_t xnrs_linear_bwd_workspace_bytes(int64_t M, int32_t N, int32_t K) {
  return carve_total({gemm_splitk_workspace_bytes(N, K, M), colsum_workspace_bytes(N)});  // split-K slabs | column-sum partials
}

int32_t xnrs_linear_bwd(const float* x, const int32_t* gather_ids, int32_t gather_S, const float* w, const float* dy,
                        float* dx, float* dw, float* db, int64_t M, int32_t N, int32_t K, void* ws, size_t ws_bytes,
                        void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (M < 0 || N <= 0 || K <= 0) return XNRS_EINVAL;
  if (M == 0) return zero_grads(dw, db, nullptr, N, K, 0, stream);  // (dx has no rows)
  if (!x || !w || !dy) return XNRS_EINVAL;
  if (gather_ids && (dx || gather_S <= 0)) return XNRS_EINVAL;
  if (xnrs_linear_bwd_workspace_bytes(M, N, K) > ws_bytes || !ws) return XNRS_EWORKSPACE;
  Carver c;
  float *slabs = at(ws, c.take(gemm_splitk_workspace_bytes(N, K, M))), *csum = at(ws, c.take(colsum_workspace_bytes(N)));
  if (dw) XNRS_TRY(gemm_dw(dy, N, x, {gather_ids, gather_S}, K, dw, M, N, K, slabs, stream, {}, {db, csum}));
  else if (db) XNRS_TRY(launch_colsum(dy, N, nullptr, M, N, db, csum, stream));
  if (dx) XNRS_TRY(gemm_dx(dy, N, w, dx, K, M, N, K, stream));
  return XNRS_OK;
}

size_t xnrs_embedding_linear_bwd_workspace_bytes(int64_t M, int32_t N, int32_t K) {  // linear backward | the dense rows dy . W
  return carve_total({xnrs_linear_bwd_workspace_bytes(M, N, K), (size_t)M * K * F32});
}

int32_t xnrs_embedding_linear_bwd(const float* table, const int32_t* ids, const float* w, const float* dy, float* d_table,
                                  float* dw, float* db, int64_t M, int32_t N, int32_t K, int32_t n_rows, void* ws,
                                  size_t ws_bytes, void* stream) {
  return embedding_linear_bwd(table, ids, w, dy, d_table, dw, db, M, N, K, n_rows, ws, ws_bytes, (hipStream_t)stream, false);
}

}  // extern "C"
