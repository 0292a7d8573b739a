// NPA's building block, layers.PersonalizedAttention (layers.py:72-102), and the table-scale embedding gradient of its user
// table (npa.py:12-15,60).  fp32, deterministic (no float atomics: every sum runs in a fixed order).
//   personalized_pool      : e_i = q . t_i, s_i = exp(e_i) m_i, a_i = s_i / (sum s + 1e-8), p = sum a_i x_i, where
//                            t = tanh(x_fc x) (the x_fc GEMM's tanh epilogue) and sequence s reads query row q[q_idx[s]]
//   personalized_pool_bwd  : da_i = dp.x_i, de_i = a_i (da_i - sum_j a_j da_j), dpre_i = de_i q (1 - t_i^2),
//                            dq_s = sum_i de_i t_i
//   query_reduce           : dq[r] = sum over the sequences s with q_idx[s] == r of dq_s, in sequence order
//   embedding_grad_sparse  : nn.Embedding backward as a dense table, one workgroup per id (zero fill + the rows in the batch)
// The C entry points at the bottom compose these with the library's own GEMM entry points.
#include "host.h"

namespace xnrs {

namespace {

constexpr int PA_THREADS = 256;
constexpr int PA_MAX_L = 4096;  // tokens per sequence (dynamic LDS: 2 floats per token in the backward)

__device__ __forceinline__ float pa_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

struct PersonalizedPoolArgs {
  const float* t;        // [n_seq*L, A] tanh(x_fc x)
  const float* q;        // query rows, row r at q + r * ldq
  int64_t ldq;
  const int32_t* q_idx;  // [n_seq], each in [0, n_q)
  int32_t n_q;
  int32_t* status;       // nullable: the sticky status word (XNRS_STATUS_QUERY_RANGE)
  const float* mask;     // [n_seq*L] (or the table's [n_table*L] with ids), nullable
  const int32_t* ids;    // nullable: value and mask rows of sequence s come from table row ids[s]
  const float* x;        // values (or table), row pitch D
  float* p;              // [n_seq, D]
  float* a_out;          // [n_seq*L] nullable
  float* hm_out;         // [n_seq] nullable: clamp(sum mask, 0, 1)
  int64_t n_seq;
  int32_t L, D, A;
};

__global__ __launch_bounds__(PA_THREADS) void personalized_pool_kernel(PersonalizedPoolArgs a) {
  extern __shared__ float s_w[];  // [L]
  __shared__ float s_den;
  const int64_t s = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int L = a.L, A = a.A, D = a.D;
  const int64_t src = a.ids ? (int64_t)a.ids[s] : s;
  const int32_t qi = a.q_idx[s];
  const float* mrow = a.mask ? a.mask + src * L : nullptr;
  if (qi < 0 || qi >= a.n_q) {  // no query row to read: the sequence's outputs are NaN and the status word says why
    const float nan = __builtin_nanf("");
    for (int i = threadIdx.x; i < L; i += PA_THREADS)
      if (a.a_out) a.a_out[s * L + i] = nan;
    for (int d = threadIdx.x; d < D; d += PA_THREADS) a.p[s * D + d] = nan;
    if (threadIdx.x == 0) {
      if (a.hm_out) {
        float msum = 0.f;
        for (int i = 0; i < L; ++i) msum += mrow ? mrow[i] : 1.f;
        a.hm_out[s] = fminf(fmaxf(msum, 0.f), 1.f);
      }
      if (a.status) atomicOr(a.status, XNRS_STATUS_QUERY_RANGE);
    }
    return;
  }
  const float* q = a.q + (int64_t)qi * a.ldq;
  for (int i = wave; i < L; i += PA_THREADS / 64) {
    const float* t = a.t + (s * L + i) * (int64_t)A;
    float acc = 0.f;
    for (int h = lane; h < A; h += 64) acc = fmaf(q[h], t[h], acc);
    acc = pa_wave_sum(acc);
    if (lane == 0) s_w[i] = expf(acc) * (mrow ? mrow[i] : 1.f);  // exp, then the mask (layers.py:97-99)
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float sum = 0.f, msum = 0.f;
    for (int i = 0; i < L; ++i) {
      sum += s_w[i];
      msum += mrow ? mrow[i] : 1.f;
    }
    s_den = sum + 1e-8f;
    if (a.hm_out) a.hm_out[s] = fminf(fmaxf(msum, 0.f), 1.f);
  }
  __syncthreads();
  const float den = s_den;
  for (int i = threadIdx.x; i < L; i += PA_THREADS) {
    const float ai = s_w[i] / den;
    s_w[i] = ai;
    if (a.a_out) a.a_out[s * L + i] = ai;
  }
  __syncthreads();
  const float* xs = a.x + src * L * (int64_t)D;
  for (int d = threadIdx.x; d < D; d += PA_THREADS) {
    float acc = 0.f;
    for (int i = 0; i < L; ++i) acc = fmaf(s_w[i], xs[(int64_t)i * D + d], acc);
    a.p[s * D + d] = acc;
  }
}

struct PersonalizedPoolBwdArgs {
  const float* dp;       // [n_seq, D]
  const float* x;        // values (or table)
  const int32_t* ids;
  const float* a;        // [n_seq*L] from the forward
  const float* t;        // [n_seq*L, A] from the forward
  const float* q;
  int64_t ldq;
  const int32_t* q_idx;
  int32_t n_q;
  float* dpre;           // [n_seq*L, A]
  float* dq_seq;         // [n_seq, A]
  int64_t n_seq;
  int32_t L, D, A;
};

__global__ __launch_bounds__(PA_THREADS) void personalized_pool_bwd_kernel(PersonalizedPoolBwdArgs a) {
  extern __shared__ float s_buf[];  // da [L] | de [L]
  __shared__ float s_c;
  const int64_t s = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int L = a.L, A = a.A, D = a.D;
  const int64_t src = a.ids ? (int64_t)a.ids[s] : s;
  const int32_t qi = a.q_idx[s];
  if (qi < 0 || qi >= a.n_q) {  // (the forward reported it): no gradient reaches x_fc, dq_s is NaN and no query row gets it
    for (int h = threadIdx.x; h < A; h += PA_THREADS) {
      for (int i = 0; i < L; ++i) a.dpre[(s * L + i) * (int64_t)A + h] = 0.f;
      a.dq_seq[s * A + h] = __builtin_nanf("");
    }
    return;
  }
  const float* dp = a.dp + s * D;
  const float* xs = a.x + src * L * (int64_t)D;
  float* s_da = s_buf;
  float* s_de = s_buf + L;
  for (int i = wave; i < L; i += PA_THREADS / 64) {
    // a masked token has a_i = 0 and therefore de_i = 0 whatever da_i is: its row is not read
    if (a.a[s * L + i] == 0.f) {
      if (lane == 0) s_da[i] = 0.f;
      continue;
    }
    const float* xi = xs + (int64_t)i * D;
    float acc = 0.f;
    for (int d = lane; d < D; d += 64) acc = fmaf(dp[d], xi[d], acc);
    acc = pa_wave_sum(acc);
    if (lane == 0) s_da[i] = acc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float c = 0.f;
    for (int i = 0; i < L; ++i) c = fmaf(a.a[s * L + i], s_da[i], c);
    s_c = c;
  }
  __syncthreads();
  const float c = s_c;
  for (int i = threadIdx.x; i < L; i += PA_THREADS) s_de[i] = a.a[s * L + i] * (s_da[i] - c);
  __syncthreads();
  const float* q = a.q + (int64_t)qi * a.ldq;
  for (int h = threadIdx.x; h < A; h += PA_THREADS) {
    const float qh = q[h];
    float acc = 0.f;
    for (int i = 0; i < L; ++i) {
      const int64_t r = (s * L + i) * (int64_t)A + h;
      const float t = a.t[r], de = s_de[i];
      acc = fmaf(de, t, acc);
      a.dpre[r] = de * qh * (1.f - t * t);
    }
    a.dq_seq[s * A + h] = acc;
  }
}

// dx_i += a_i dp (the pooling term of the input gradient; the x_fc term dpre . Wx is already there)
__global__ __launch_bounds__(PA_THREADS) void personalized_dx_add_kernel(const float* __restrict__ a, const float* __restrict__ dp,
                                                                        float* __restrict__ dx, int64_t rows, int L, int D) {
  const int64_t r = blockIdx.x;
  if (r >= rows) return;
  const float ai = a[r];
  const float* g = dp + (r / L) * D;
  float* o = dx + r * D;
  for (int d = threadIdx.x; d < D; d += PA_THREADS) o[d] = fmaf(ai, g[d], o[d]);
}

// dq[r * ldo + h] = sum_{s: q_idx[s] == r} dq_seq[s][h], s ascending
__global__ __launch_bounds__(128) void personalized_query_reduce_kernel(const float* __restrict__ dq_seq,
                                                                       const int32_t* __restrict__ q_idx, int64_t n_seq,
                                                                       int A, float* __restrict__ dq, int64_t ldo) {
  const int r = blockIdx.x;
  for (int h = threadIdx.x; h < A; h += 128) {
    float acc = 0.f;
    for (int64_t s = 0; s < n_seq; ++s)
      if (q_idx[s] == r) acc += dq_seq[s * A + h];
    dq[(int64_t)r * ldo + h] = acc;
  }
}

__global__ __launch_bounds__(PA_THREADS) void personalized_act_bwd_kernel(float* __restrict__ g, const float* __restrict__ y,
                                                                         int64_t n, int act) {
  const int64_t i = (int64_t)blockIdx.x * PA_THREADS + threadIdx.x;
  if (i >= n) return;
  const float v = y[i];
  if (act == XNRS_ACT_RELU) g[i] = v > 0.f ? g[i] : 0.f;
  else if (act == XNRS_ACT_TANH) g[i] *= 1.f - v * v;
}

// p[0 .. n) = 0 with 16-byte stores (p 16-byte aligned)
__global__ __launch_bounds__(PA_THREADS) void zero_fill_kernel(float* __restrict__ p, int64_t n) {
  const int64_t i = ((int64_t)blockIdx.x * PA_THREADS + threadIdx.x) * 4;
  if (i + 3 < n) {
    *reinterpret_cast<f32x4*>(p + i) = f32x4{0.f, 0.f, 0.f, 0.f};
  } else {
    for (int64_t j = i; j < n; ++j) p[j] = 0.f;
  }
}

// The workgroup of an id's FIRST occurrence writes that table row: the sum of all its occurrences' rows in batch order.
// Every other workgroup returns at once.  Ids outside [0, n_rows) are skipped.
__global__ __launch_bounds__(64) void embedding_grad_sparse_kernel(const float* __restrict__ d_rows, const int32_t* __restrict__ ids,
                                                                  int64_t M, int K, float* __restrict__ d_table, int n_rows) {
  const int64_t m = blockIdx.x;
  const int32_t id = ids[m];
  if (id < 0 || id >= n_rows) return;
  for (int64_t j = 0; j < m; ++j)
    if (ids[j] == id) return;
  for (int k = threadIdx.x; k < K; k += 64) {
    float acc = 0.f;
    for (int64_t j = m; j < M; ++j)
      if (ids[j] == id) acc += d_rows[j * K + k];
    d_table[(int64_t)id * K + k] = acc;
  }
}

struct PaLayout {  // saved blob of a (training) forward: T | a | p | h1
  size_t t, a, p, h1, total;
};
PaLayout pa_layout(int64_t n_seq, int32_t L, int32_t D, int32_t A, int32_t E, int32_t has_head) {
  PaLayout o;
  const int64_t rows = n_seq * L;
  Carver c;
  o.t = c.take((size_t)rows * A * F32);
  o.a = c.take((size_t)rows * F32);
  o.p = c.off;  // (without a head nothing is kept here: the pooled vectors are the output)
  if (has_head) c.take((size_t)n_seq * D * F32);
  o.h1 = c.off;
  if (has_head) c.take((size_t)n_seq * E * F32);
  o.total = c.total();
  return o;
}

size_t pa_linear_ws(int64_t n_seq, int32_t L, int32_t D, int32_t A, int32_t E, bool has_head) {
  size_t lin = xnrs_linear_bwd_workspace_bytes(n_seq * L, A, D);
  if (has_head) {
    const size_t l2 = xnrs_linear_bwd_workspace_bytes(n_seq, E, E), l0 = xnrs_linear_bwd_workspace_bytes(n_seq, E, D);
    lin = lin > l2 ? lin : l2;
    lin = lin > l0 ? lin : l0;
  }
  return align_up(lin);
}

struct PaBwdWs {  // backward workspace: linear-backward scratch (lin bytes) | dpre | dq per sequence | dh1 | dp  (the last two: head)
  size_t lin, dpre, dq_seq, dh1, dpb, total;
};
PaBwdWs pa_bwd_ws(int64_t n_seq, int32_t L, int32_t D, int32_t A, int32_t E, bool has_head) {
  PaBwdWs o;
  o.lin = pa_linear_ws(n_seq, L, D, A, E, has_head);
  Carver c{o.lin};
  o.dpre = c.take((size_t)n_seq * L * A * F32);
  o.dq_seq = c.take((size_t)n_seq * A * F32);
  o.dh1 = c.take_if(has_head, (size_t)n_seq * E * F32);
  o.dpb = c.take_if(has_head, (size_t)n_seq * D * F32);
  o.total = c.total();
  return o;
}

int32_t pa_check(const float* x, int64_t n_seq, int32_t L, int32_t D, const xnrs_personalized_params* p,
                 const xnrs_head_params* head) {
  if (!x || !p || !p->wx || !p->q || !p->q_idx || n_seq < 0 || L <= 0 || D <= 0 || p->hidden <= 0 || p->n_q < 0)
    return XNRS_EINVAL;
  if (p->q_ld != 0 && p->q_ld < p->hidden) return XNRS_EINVAL;
  if (head && (!head->w0 || !head->w2 || head->out_features <= 0)) return XNRS_EINVAL;
  if (head && (head->activation < 0 || head->activation > 2)) return XNRS_EINVAL;
  if (L > PA_MAX_L || n_seq * L >= ((int64_t)1 << 31)) return XNRS_EUNSUPPORTED;
  return XNRS_OK;
}

int32_t pa_forward(const float* x, const float* m, const int32_t* ids, int64_t n_seq, int32_t L, int32_t D,
                   const xnrs_personalized_params* p, const xnrs_head_params* head, float* y, float* a_out, float* hm,
                   char* buf, hipStream_t stream) {
  const int32_t A = p->hidden, E = head ? head->out_features : D;
  const PaLayout lo = pa_layout(n_seq, L, D, A, E, head != nullptr);
  float *T = at(buf, lo.t), *a = at(buf, lo.a), *pooled = head ? at(buf, lo.p) : y, *h1 = at(buf, lo.h1);
  XNRS_TRY_RC(xnrs_linear_fwd(x, ids, L, p->wx, p->bx, T, n_seq * L, A, D, XNRS_ACT_TANH, stream));  // layers.py:88
  PersonalizedPoolArgs pa;
  pa.t = T;
  pa.q = p->q;
  pa.ldq = p->q_ld ? p->q_ld : A;
  pa.q_idx = p->q_idx;
  pa.n_q = p->n_q;
  pa.status = status_word();
  pa.mask = m;
  pa.ids = ids;
  pa.x = x;
  pa.p = pooled;
  pa.a_out = a;
  pa.hm_out = hm;
  pa.n_seq = n_seq;
  pa.L = L;
  pa.D = D;
  pa.A = A;
  hipLaunchKernelGGL(personalized_pool_kernel, dim3((unsigned)n_seq), dim3(PA_THREADS), (size_t)L * sizeof(float), stream, pa);
  XNRS_TRY(hipGetLastError());
  if (a_out) XNRS_TRY(hipMemcpyAsync(a_out, a, (size_t)n_seq * L * sizeof(float), hipMemcpyDeviceToDevice, stream));
  if (head) {  // news_head (npa.py:22-26): Linear(D,E) - act - Linear(E,E)
    XNRS_TRY_RC(xnrs_linear_fwd(pooled, nullptr, 0, head->w0, head->b0, h1, n_seq, E, D, head->activation, stream));
    XNRS_TRY_RC(xnrs_linear_fwd(h1, nullptr, 0, head->w2, head->b2, y, n_seq, E, E, XNRS_ACT_NONE, stream));
  }
  return XNRS_OK;
}

}  // namespace
}  // namespace xnrs

using namespace xnrs;

extern "C" {

size_t xnrs_personalized_saved_bytes(int64_t n_seq, int32_t L, int32_t D, int32_t A, int32_t E, int32_t has_head) {
  return pa_layout(n_seq, L, D, A, E, has_head).total;
}

int32_t xnrs_personalized_fwd(const float* x, const float* m, const int32_t* ids, int64_t n_seq, int32_t L, int32_t D,
                              const xnrs_personalized_params* p, const xnrs_head_params* head, float* y, float* a_out,
                              float* hm, void* ws, size_t ws_bytes, void* stream) {
  XNRS_TRY_RC(pa_check(x, n_seq, L, D, p, head));
  if (!y) return XNRS_EINVAL;
  if (n_seq == 0) return XNRS_OK;
  const int32_t E = head ? head->out_features : D;
  if (!ws || ws_bytes < pa_layout(n_seq, L, D, p->hidden, E, head != nullptr).total) return XNRS_EWORKSPACE;
  return pa_forward(x, m, ids, n_seq, L, D, p, head, y, a_out, hm, static_cast<char*>(ws), (hipStream_t)stream);
}

int32_t xnrs_personalized_fwd_train(const float* x, const float* m, const int32_t* ids, int64_t n_seq, int32_t L, int32_t D,
                                    const xnrs_personalized_params* p, const xnrs_head_params* head, float* y, float* a_out,
                                    float* hm, void* saved, size_t saved_bytes, void* stream) {
  return xnrs_personalized_fwd(x, m, ids, n_seq, L, D, p, head, y, a_out, hm, saved, saved_bytes, stream);
}

size_t xnrs_personalized_bwd_workspace_bytes(int64_t n_seq, int32_t L, int32_t D, int32_t A, int32_t E, int32_t has_head) {
  return pa_bwd_ws(n_seq, L, D, A, E, has_head != 0).total;
}

int32_t xnrs_personalized_bwd(const float* x, const int32_t* ids, int64_t n_seq, int32_t L, int32_t D,
                              const xnrs_personalized_params* p, const xnrs_head_params* head, const void* saved,
                              size_t saved_bytes, const float* dy, float* dx, float* dwx, float* dbx, float* dq, int64_t n_q,
                              const xnrs_head_grads* g_head, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  XNRS_TRY_RC(pa_check(x, n_seq, L, D, p, head));
  if (!saved || !dy || n_q < 0 || n_q >= ((int64_t)1 << 31)) return XNRS_EINVAL;
  if (ids && dx) return XNRS_EINVAL;  // a gathered table gets no gradient
  const int32_t A = p->hidden, E = head ? head->out_features : D;
  const int64_t rows = n_seq * L;
  const PaLayout lo = pa_layout(n_seq, L, D, A, E, head != nullptr);
  if (saved_bytes < lo.total) return XNRS_EINVAL;
  const xnrs_head_grads none = {nullptr, nullptr, nullptr, nullptr};
  const xnrs_head_grads& g = (head && g_head) ? *g_head : none;
  if (n_seq == 0) {  // nothing pooled: zero weight / query gradients
    if (dwx) XNRS_TRY(hipMemsetAsync(dwx, 0, (size_t)A * D * sizeof(float), stream));
    if (dbx) XNRS_TRY(hipMemsetAsync(dbx, 0, (size_t)A * sizeof(float), stream));
    if (dq && n_q) XNRS_TRY(hipMemsetAsync(dq, 0, (size_t)n_q * A * sizeof(float), stream));
    if (g.w0) XNRS_TRY(hipMemsetAsync(g.w0, 0, (size_t)E * D * sizeof(float), stream));
    if (g.b0) XNRS_TRY(hipMemsetAsync(g.b0, 0, (size_t)E * sizeof(float), stream));
    if (g.w2) XNRS_TRY(hipMemsetAsync(g.w2, 0, (size_t)E * E * sizeof(float), stream));
    if (g.b2) XNRS_TRY(hipMemsetAsync(g.b2, 0, (size_t)E * sizeof(float), stream));
    return XNRS_OK;
  }
  if (!ws || ws_bytes < pa_bwd_ws(n_seq, L, D, A, E, head != nullptr).total) return XNRS_EWORKSPACE;
  const float *T = at(saved, lo.t), *a = at(saved, lo.a), *pooled = at(saved, lo.p), *h1 = at(saved, lo.h1);
  const PaBwdWs wl = pa_bwd_ws(n_seq, L, D, A, E, head != nullptr);
  const size_t lin = wl.lin;
  void* w = ws;
  float *dpre = at(ws, wl.dpre), *dq_seq = at(ws, wl.dq_seq), *dh1 = at(ws, wl.dh1), *dpb = at(ws, wl.dpb);
  const bool pool_grads = dx || dwx || dbx || dq;
  const float* dp = dy;
  if (head) {
    const bool below = pool_grads || g.w0 || g.b0;  // does anything need the gradient below the second head layer?
    XNRS_TRY_RC(xnrs_linear_bwd(h1, nullptr, 0, head->w2, dy, below ? dh1 : nullptr, g.w2, g.b2, n_seq, E, E, w, lin, stream));
    if (!below) return XNRS_OK;
    if (head->activation != XNRS_ACT_NONE) {
      const int64_t n = n_seq * E;
      hipLaunchKernelGGL(personalized_act_bwd_kernel, dim3((unsigned)((n + PA_THREADS - 1) / PA_THREADS)), dim3(PA_THREADS), 0,
                         stream, dh1, h1, n, head->activation);
      XNRS_TRY(hipGetLastError());
    }
    XNRS_TRY_RC(xnrs_linear_bwd(pooled, nullptr, 0, head->w0, dh1, pool_grads ? dpb : nullptr, g.w0, g.b0, n_seq, E, D, w, lin, stream));
    dp = dpb;
  }
  if (!pool_grads) return XNRS_OK;
  PersonalizedPoolBwdArgs pb;
  pb.dp = dp;
  pb.x = x;
  pb.ids = ids;
  pb.a = a;
  pb.t = T;
  pb.q = p->q;
  pb.ldq = p->q_ld ? p->q_ld : A;
  pb.q_idx = p->q_idx;
  pb.n_q = p->n_q;
  pb.dpre = dpre;
  pb.dq_seq = dq_seq;
  pb.n_seq = n_seq;
  pb.L = L;
  pb.D = D;
  pb.A = A;
  hipLaunchKernelGGL(personalized_pool_bwd_kernel, dim3((unsigned)n_seq), dim3(PA_THREADS), (size_t)2 * L * sizeof(float), stream, pb);
  XNRS_TRY(hipGetLastError());
  if (dx || dwx || dbx)  // x_fc (layers.py:88): dWx = dpre^T x, dbx = colsum dpre, dx = dpre Wx
    XNRS_TRY_RC(xnrs_linear_bwd(x, ids, L, p->wx, dpre, dx, dwx, dbx, rows, A, D, w, lin, stream));
  if (dx) {
    hipLaunchKernelGGL(personalized_dx_add_kernel, dim3((unsigned)rows), dim3(PA_THREADS), 0, stream, a, dp, dx, rows, L, D);
    XNRS_TRY(hipGetLastError());
  }
  if (dq && n_q > 0) {
    hipLaunchKernelGGL(personalized_query_reduce_kernel, dim3((unsigned)n_q), dim3(128), 0, stream, dq_seq, p->q_idx, n_seq, A, dq,
                       (int64_t)A);
    XNRS_TRY(hipGetLastError());
  }
  return XNRS_OK;
}

int32_t xnrs_embedding_grad_sparse(const float* d_rows, const int32_t* ids, int64_t M, int32_t K, float* d_table, int32_t n_rows,
                                   void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!d_table || K <= 0 || n_rows <= 0 || M < 0 || (M > 0 && (!d_rows || !ids))) return XNRS_EINVAL;
  if (M >= ((int64_t)1 << 31)) return XNRS_EUNSUPPORTED;
  const int64_t n = (int64_t)n_rows * K;
  if ((reinterpret_cast<uintptr_t>(d_table) & 15) != 0) {
    XNRS_TRY(hipMemsetAsync(d_table, 0, (size_t)n * sizeof(float), stream));
  } else {
    const int64_t blocks = (n + 4 * PA_THREADS - 1) / (4 * PA_THREADS);
    hipLaunchKernelGGL(zero_fill_kernel, dim3((unsigned)blocks), dim3(PA_THREADS), 0, stream, d_table, n);
    XNRS_TRY(hipGetLastError());
  }
  if (M == 0) return XNRS_OK;
  hipLaunchKernelGGL(embedding_grad_sparse_kernel, dim3((unsigned)M), dim3(64), 0, stream, d_rows, ids, M, K, d_table, n_rows);
  XNRS_TRY(hipGetLastError());
  return XNRS_OK;
}

size_t xnrs_embedding_linear_bwd_sparse_workspace_bytes(int64_t M, int32_t N, int32_t K) {
  return xnrs_embedding_linear_bwd_workspace_bytes(M, N, K);
}

int32_t xnrs_embedding_linear_bwd_sparse(const float* table, const int32_t* ids, const float* w, const float* dy, float* d_table,
                                         float* dw, float* db, int64_t M, int32_t N, int32_t K, int32_t n_rows, void* ws,
                                         size_t ws_bytes, void* stream) {
  return embedding_linear_bwd(table, ids, w, dy, d_table, dw, db, M, N, K, n_rows, ws, ws_bytes, (hipStream_t)stream, true);
}

}  // extern "C"
