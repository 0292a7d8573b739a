// Host-side helpers shared by the translation units that hold extern "C" entry points: error propagation, the launch
// timer's scope, the workspace carver, GEMM descriptor builders, the folded out-projection's regions and product, and the
// declarations of the orchestration functions one file defines and another calls.  Host code only (no kernel sees this).
#pragma once
#include <initializer_list>

#include "../../include/xnrs_hip.h"
#include "kernels.h"

namespace xnrs {

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

inline int32_t hip_rc(hipError_t e) { return e == hipSuccess ? XNRS_OK : (int32_t)e; }

// return from an int32_t entry point on a failed HIP call / on a failed XNRS_* call
#define XNRS_TRY(expr)                       \
  do {                                       \
    hipError_t _e = (expr);                  \
    if (_e != hipSuccess) return hip_rc(_e); \
  } while (0)
#define XNRS_TRY_RC(expr)           \
  do {                              \
    int32_t _rc = (expr);           \
    if (_rc != XNRS_OK) return _rc; \
  } while (0)

// ---------------------------------------------------------------- workspace carve
// Every region of every workspace / saved blob is 256-B aligned; sizes in BYTES.
struct Carver {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off += align_up(bytes);
    return o;
  }
  size_t take_if(bool wanted, size_t bytes) { return wanted ? take(bytes) : 0; }
  size_t total() const { return off; }
};
inline size_t carve_total(std::initializer_list<size_t> regions) {  // the bytes of a carve of these regions, in order
  Carver c;
  for (size_t r : regions) c.take(r);
  return c.total();
}
template <class T = float>
inline T* at(void* base, size_t off) {  // the region at byte offset `off`
  return reinterpret_cast<T*>(static_cast<char*>(base) + off);
}
template <class T = float>
inline const T* at(const void* base, size_t off) {
  return reinterpret_cast<const T*>(static_cast<const char*>(base) + off);
}
constexpr size_t F32 = sizeof(float);

// ---------------------------------------------------------------- optional per-launch event timing (xnrs_profile_*)
// The records and their mutex live in api.hip; a scope is a single load and compare while the timer is off (the default).
struct ProfRec {
  hipEvent_t beg, end;
  int stage;
  double flops;
};
extern uint32_t g_prof_mask;
inline bool prof_on(int stage) { return (g_prof_mask >> stage) & 1u; }
bool prof_begin(ProfRec* r, hipStream_t stream);
void prof_end(const ProfRec& r, hipStream_t stream);
struct ProfScope {
  bool on;
  hipStream_t st;
  ProfRec r{};
  ProfScope(int stage, double flops, hipStream_t s) : on(prof_on(stage)), st(s) {
    r.stage = stage;
    r.flops = flops;
    if (on) on = prof_begin(&r, st);
  }
  ~ProfScope() {
    if (on) prof_end(r, st);
  }
};
// a row count for the launch timer's FLOP figure: the host value, or -- counts on the device, timer on for this stage --
// read back (the timer is a measurement aid that synchronises anyway; no read happens while it is off)
int64_t prof_count(int stage, const int64_t* cnt, int which, int64_t host_value, hipStream_t stream);

// ---------------------------------------------------------------- GEMM descriptors
// logical row m of an operand is physical row ids[m / S] * S + m % S ({} = the rows as they lie)
struct RowIds {
  const int32_t* ids = nullptr;
  int S = 0;
};
// the fields every layout shares: C[M, N] (pitch ldc) from A (pitch lda) and ONE weight segment W (pitch ldw), contraction K
inline GemmArgs gemm_base(const float* A, int64_t lda, const float* W, int64_t ldw, float* C, int64_t ldc, int64_t M, int N,
                          int64_t K) {
  GemmArgs g{};
  g.A = A;
  g.lda = lda;
  g.W[0] = W;
  g.ldw = ldw;
  g.nseg = 1;
  g.Nseg = N;
  g.C = C;
  g.ldc = ldc;
  g.M = M;
  g.K = K;
  return g;
}
// C[M, N] = act(A[M, K] . W[N, K]^T + b): W in nn.Linear layout (pitch K; bf16-split modes: its pre-split planes)
inline GemmArgs gemm_linear(const float* A, RowIds a_rows, int64_t lda, const float* W, const float* b, float* C, int64_t ldc,
                            int64_t M, int N, int64_t K, int act = XNRS_ACT_NONE, const unsigned short* planes = nullptr) {
  GemmArgs g = gemm_base(A, lda, W, K, C, ldc, M, N, K);
  g.gather_ids = a_rows.ids;
  g.gather_S = a_rows.S;
  g.Wp[0] = planes;
  g.ldp = split_plane_ld(K);
  g.bias[0] = b;
  g.act = act;
  return g;
}
// C[M, N] = A[M, K] . B[K, N]: B k-major (its row index is the contraction index), pitch ldb
inline GemmArgs gemm_kmajor_b(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N,
                              int64_t K) {
  GemmArgs g = gemm_base(A, lda, B, ldb, C, ldc, M, N, K);
  g.b_kn = 1;
  return g;
}
// C[M, N] = At[K, M]^T . B[K, N]: both operands k-major (dW = dY^T . X, contraction over the rows)
inline GemmArgs gemm_kmajor_ab(const float* At, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N,
                               int64_t K) {
  GemmArgs g = gemm_base(At, lda, B, ldb, C, ldc, M, N, K);
  g.a_col = g.b_kn = 1;
  return g;
}

// the dense projections of the scorers (scorers.hip, sweep.h)
// C[M, N] = A[M, K] . op(W) (+ bias): W row-major [N][K] at pitch ldw (w_kn = 0: nn.Linear layout) or [K][N] at pitch ldw
// (w_kn = 1); one launch, no split-K
inline hipError_t sc_gemm(const float* A, int64_t lda, const float* W, int64_t ldw, int w_kn, const float* bias, float* C, int64_t ldc,
                   int64_t M, int N, int64_t K, hipStream_t stream) {
  GemmArgs g = w_kn ? gemm_kmajor_b(A, lda, W, ldw, C, ldc, M, N, K) : gemm_linear(A, {}, lda, W, bias, C, ldc, M, N, K);
  g.bias[0] = bias;
  g.ldw = ldw;
  return launch_gemm_f32(g, stream);
}

// ---------------------------------------------------------------- folded out-projection (encoder_fwd.hip "fold")
constexpr int FOLD_SPLITS = 8;  // K slices of the folded-weight product X . Wo (slabs: FOLD_SPLITS x M x D floats)
inline bool fold_wanted(int knob) { return knob != 0; }  // knob: 0 never, anything else always
// W1.Wo, W1.bo + b1, pooled O rows, sum of weights, split-K slabs of the weight product
struct FoldRegions {
  size_t fw, fb, po, as, fsl;
};
inline FoldRegions carve_fold(Carver& c, bool wanted, int64_t n_seq, int D, int A) {
  FoldRegions f{};
  f.fw = c.take_if(wanted, (size_t)A * D * F32);
  f.fb = c.take_if(wanted, (size_t)A * F32);
  f.po = c.take_if(wanted, (size_t)n_seq * D * F32);
  f.as = c.take_if(wanted, (size_t)n_seq * F32);
  f.fsl = c.take_if(wanted, (size_t)FOLD_SPLITS * A * D * F32);
  return f;
}

// ---------------------------------------------------------------- the padded encoder (encoder_fwd.hip)
struct Plan {
  int64_t chunk;  // sequences per pass
  size_t off_qkv, off_o, off_y, off_t, off_p, off_h;
  size_t off_stats, off_a;  // training only: softmax row statistics, pooling weights
  size_t off_planes;        // bf16-split GEMM modes: pre-split weight planes (wq, wk, wv, wo, w1)
  size_t off_nf, off_nfo;   // fused short-sequence encoder: fragment-ordered weight images, O-row scratch (fold)
  size_t off_lt_alive, off_lt_n, off_lt_tiles;  // live row tiles of the dense passes (launch_live_tiles)
  size_t off_lr_loc, off_lr_src, off_lr_cnt;    // live rows of the dense passes (launch_dense_row_lists); 0 = not reserved (L > 64)
  FoldRegions fold;
  size_t off_x32, off_m32;  // bf16 table (SeqEncode::x16): one pass of widened fp32 token rows and of gathered mask rows
  size_t total;
};
// workspace (train: saved-activation) carve for one chunk; widen: the rows come from a bf16 table (SeqEncode::x16)
Plan make_plan(int64_t n_seq, int L, int D, int A, int E, bool att, bool additive, bool head, bool pooled, int64_t chunk,
               bool train = false, int n_heads = 0, bool widen = false);

// x:(n_seq,L,D) [or table + ids], m:(n_seq,L) [or table mask] -> y
//   pooled == false: y:(n_seq,L,D) = att(x)            (MultiHeadAttention alone)
//   pooled == true : y:(n_seq,E')  = head(pool(att(x)))
struct SeqEncode {
  const float *x, *m;
  const int32_t* ids;
  int64_t n_seq;
  int L, D;
  const xnrs_mha_params* att;
  bool pooled;
  int pool_kind;
  const xnrs_additive_params* pool;
  const xnrs_head_params* head;
  float *y, *a_out, *hm;  // a_out, hm nullable: the pooling weights, the collapsed mask
  int64_t chunk;          // sequences per pass (0 = default)
  void* ws;
  size_t ws_bytes;
  bool train;                // keep the activations the backward reads (ws = the saved blob)
  const xnrs_row_lists* rl;  // nullable (training): live-row / K|V-row lists
  bool live_tiles;           // inference: the row-parallel products may skip row tiles that hold only all-masked sequences
  // nullable, instead of x (inference, pooled, ids required): the table is STORED in bf16 [n_table, L, D].  An attention tower
  // with the additive pooler on the GEMM pipeline projects Q|K|V straight from the bf16 rows (launch_gemm_a16); every other
  // call widens the rows of each pass into the workspace and runs the fp32 route on them
  const uint16_t* x16;
};
int32_t seq_encode(const SeqEncode& r, hipStream_t stream);

// can every product over a device-counted row list run on the kernels that read their row count on the device?
bool device_counts_ok(const float* x, int D, int A, const xnrs_mha_params* att, const xnrs_additive_params* pool);

// ---------------------------------------------------------------- weight / input gradient products (encoder_bwd.hip)
// A product over listed rows only: rows[j] of the gradient image, j < n (its other rows are known to be zero) -- in a dW
// product contracted against rows x_rows[j] of X.  n_dev (nullable): the list's length on the device, n is then its capacity.
struct LiveRows {
  const int32_t *rows = nullptr, *x_rows = nullptr;
  int64_t n = 0;
  const int64_t* n_dev = nullptr;
};
// the bias gradient db[N] = sum_rows dY beside a dW product; csum = colsum workspace
struct DwBias {
  float *db = nullptr, *csum = nullptr;
};
// ONE product for two parameters: output rows [0, n1) are dW / db, rows [n1, N) are dW2 / db2
struct DwSecond {
  float *dW2 = nullptr, *db2 = nullptr;
  int n1 = 0;
};
hipError_t gemm_dw(const float* dY, int64_t lddy, const float* X, RowIds x_rows, int64_t ldx, float* dW, int64_t M, int N, int K,
                   float* slabs, hipStream_t stream, LiveRows live = {}, DwBias bias = {}, int accumulate = 0, DwSecond second = {});
// dX (*)= f'(aux): mode 1 tanh' = 1 - aux^2, mode 2 relu' = (aux > 0)
struct DxAct {
  const float* aux = nullptr;
  int64_t ldaux = 0;
  int mode = 0;
};
hipError_t gemm_dx(const float* dY, int64_t lddy, const float* W, float* dX, int64_t lddx, int64_t M, int N, int K,
                   hipStream_t stream, float* wt_scratch = nullptr, int accumulate = 0, LiveRows live = {}, DxAct act = {});


// autograd of fc(embedder(ids)): the one body of xnrs_embedding_linear_bwd (sparse_table == false) and
// xnrs_embedding_linear_bwd_sparse (true), which differ in the kernel that scatters dy . W into the table gradient
int32_t embedding_linear_bwd(const float* table, const int32_t* ids, const float* w, const float* dy, float* d_table, float* dw,
                             float* db, int64_t M, int N, int K, int n_rows, void* ws, size_t ws_bytes, hipStream_t stream,
                             bool sparse_table);

}  // namespace xnrs
