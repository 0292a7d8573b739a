// The bilinear and MLP scorers of the reference (xnrs/models/components/scoring.py:41-102) around the existing GEMMs:
// the dense projections (v = U.W, q = U.W1u^T + b1, p = C.W1c^T and the weight-gradient products) run on
// launch_gemm_f32 (the C entry points at the bottom); these kernels are the per-pair parts no GEMM does, and the fixed-order reductions.
//   bilinear : s[b,n] = v_b . c^_bn + bias                    v_b = W[0]^T u^_b, u^ / c^ optionally L2-normalised
//   MLP      : s[b,n] = w2 . tanh(q_b + p_bn) + b2            q_b = W1u u_b + b1, p_bn = W1c c_bn
// fp32 throughout, no atomics: every sum runs in an order fixed by the launch shape alone, which does not depend on
// the data (the same bits on every run, in a hipGraph replay too).
#include "host.h"

namespace xnrs {

namespace {

__device__ __forceinline__ float sc_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// y[r, :] = x[r, :] / ||x[r, :]|| (no epsilon, as scoring.py:20-22): one wave per row
__global__ __launch_bounds__(256) void l2_normalize_rows_kernel(const float* x, float* y, int64_t rows, int E) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + r * E;
  float ss = 0.f;
  for (int e = lane; e < E; e += 64) ss = fmaf(xr[e], xr[e], ss);
  const float inv = 1.f / sqrtf(sc_wave_sum(ss));
  for (int e = lane; e < E; e += 64) y[r * E + e] = xr[e] * inv;
}

// s[b,n] = v_b . c_bn (/ ||c_bn|| when normalize) + bias: one wave per pair
__global__ __launch_bounds__(256) void bilinear_pair_fwd_kernel(const float* v, const float* c, const float* bias, float* s,
                                                                int64_t n_pairs, int N, int E, int normalize) {
  const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= n_pairs) return;
  const int lane = threadIdx.x & 63;
  const float* vb = v + (pair / N) * E;
  const float* cp = c + pair * E;
  float dot = 0.f, cc = 0.f;
  for (int e = lane; e < E; e += 64) {
    const float y = cp[e];
    dot = fmaf(vb[e], y, dot);
    cc = fmaf(y, y, cc);
  }
  dot = sc_wave_sum(dot);
  if (normalize) dot = dot * (1.f / sqrtf(sc_wave_sum(cc)));
  if (lane == 0) s[pair] = bias ? dot + bias[0] : dot;
}

// One workgroup per impression b, candidates in groups of four (one wave each for the per-candidate scalars):
//   G_b = sum_n g_bn c^_bn                              (each thread owns fixed columns: sequential in n)
//   dc_bn = g_bn v_b                                     (raw)
//   dc_bn = g_bn (v_b - c^_bn (c^_bn . v_b)) / ||c_bn||  (normalised: the chain rule through c / ||c||)
__global__ __launch_bounds__(256) void bilinear_pair_bwd_kernel(const float* v, const float* c, const float* g, float* dc,
                                                                float* G, int N, int E, int normalize) {
  __shared__ float s_inv[4], s_cv[4];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* vb = v + b * E;
  float* Gb = G + b * E;
  for (int n0 = 0; n0 < N; n0 += 4) {
    const int n = n0 + wave;
    if (normalize && n < N) {
      const float* cp = c + (b * N + n) * E;
      float cc = 0.f, cv = 0.f;
      for (int e = lane; e < E; e += 64) {
        cc = fmaf(cp[e], cp[e], cc);
        cv = fmaf(cp[e], vb[e], cv);
      }
      cc = sc_wave_sum(cc);
      cv = sc_wave_sum(cv);
      const float inv = 1.f / sqrtf(cc);
      if (lane == 0) {
        s_inv[wave] = inv;
        s_cv[wave] = cv * inv;  // c^ . v
      }
    }
    __syncthreads();
    const int nn = N - n0 < 4 ? N - n0 : 4;
    for (int e = threadIdx.x; e < E; e += 256) {
      float acc = n0 == 0 ? 0.f : Gb[e];
      const float ve = vb[e];
      for (int w = 0; w < nn; ++w) {
        const int64_t pair = b * N + n0 + w;
        const float gg = g[pair];
        const float ce = c[pair * E + e];
        if (normalize) {
          const float inv = s_inv[w];
          const float ch = ce * inv;
          acc = fmaf(gg, ch, acc);
          if (dc) dc[pair * E + e] = gg * (ve - ch * s_cv[w]) * inv;
        } else {
          acc = fmaf(gg, ce, acc);
          if (dc) dc[pair * E + e] = gg * ve;
        }
      }
      Gb[e] = acc;
    }
    __syncthreads();
  }
}

// du_b = (du^_b - u^_b (u^_b . du^_b)) / ||u_b||: one wave per row (the chain rule through u / ||u||)
__global__ __launch_bounds__(256) void l2_normalize_bwd_kernel(const float* u, const float* uh, const float* duh, float* du,
                                                               int64_t rows, int E) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* ur = u + r * E;
  const float* hr = uh + r * E;
  const float* dr = duh + r * E;
  float ss = 0.f, dot = 0.f;
  for (int e = lane; e < E; e += 64) {
    ss = fmaf(ur[e], ur[e], ss);
    dot = fmaf(hr[e], dr[e], dot);
  }
  const float inv = 1.f / sqrtf(sc_wave_sum(ss));
  dot = sc_wave_sum(dot);
  for (int e = lane; e < E; e += 64) du[r * E + e] = (dr[e] - hr[e] * dot) * inv;
}

// s[b,n] = sum_h w2[h] tanh(q[b,h] + p[bn,h]) + b2: one wave per pair
__global__ __launch_bounds__(256) void mlp_pair_fwd_kernel(const float* q, const float* p, const float* w2, const float* b2,
                                                           float* s, int64_t n_pairs, int N, int H) {
  const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= n_pairs) return;
  const int lane = threadIdx.x & 63;
  const float* qb = q + (pair / N) * H;
  const float* pp = p + pair * H;
  float acc = 0.f;
  for (int h = lane; h < H; h += 64) acc = fmaf(w2[h], tanhf(qb[h] + pp[h]), acc);
  acc = sc_wave_sum(acc);
  if (lane == 0) s[pair] = b2 ? acc + b2[0] : acc;
}

// One workgroup per impression b, one thread per hidden unit h (strided), candidates in order:
//   t = tanh(q_b + p_bn) (recomputed: the forward's expression, the forward's bits), delta_bn = g_bn w2 (1 - t^2),
//   Delta_b = sum_n delta_bn, dw2 partial_b = sum_n g_bn t_bn.
__global__ __launch_bounds__(256) void mlp_pair_bwd_kernel(const float* q, const float* p, const float* w2, const float* g,
                                                           float* delta, float* Delta, float* dw2_part, int N, int H) {
  const int64_t b = blockIdx.x;
  for (int h = threadIdx.x; h < H; h += 256) {
    const float qh = q[b * H + h], wh = w2[h];
    float sd = 0.f, sw = 0.f;
    for (int n = 0; n < N; ++n) {
      const int64_t pair = b * N + n;
      const float t = tanhf(qh + p[pair * H + h]);
      const float gg = g[pair];
      const float d = gg * wh * (1.f - t * t);
      if (delta) delta[pair * H + h] = d;
      sd += d;
      sw = fmaf(gg, t, sw);
    }
    if (Delta) Delta[b * H + h] = sd;
    if (dw2_part) dw2_part[b * H + h] = sw;
  }
}

// r[e] = relu?(v[sess[e]] . vecs[rows[e]] + bias): one wave per candidate entry
__global__ __launch_bounds__(256) void score_csr_bilinear_kernel(const float* vecs, const int32_t* rows, const int32_t* sess,
                                                                 const float* v, const float* bias, float* r, int64_t n, int E,
                                                                 int relu) {
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= n) return;
  const int lane = threadIdx.x & 63;
  const float* x = vecs + (int64_t)rows[e] * E;
  const float* vv = v + (int64_t)sess[e] * E;
  float acc = 0.f;
  for (int k = lane; k < E; k += 64) acc = fmaf(vv[k], x[k], acc);
  acc = sc_wave_sum(acc);
  if (bias) acc += bias[0];
  if (lane == 0) r[e] = relu ? fmaxf(acc, 0.f) : acc;
}

// r[e] = relu?(w2 . tanh(q[sess[e]] + P[rows[e]]) + b2): one wave per candidate entry
__global__ __launch_bounds__(256) void score_csr_mlp_kernel(const float* P, const int32_t* rows, const int32_t* sess, const float* q,
                                                            const float* w2, const float* b2, float* r, int64_t n, int H, int relu) {
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= n) return;
  const int lane = threadIdx.x & 63;
  const float* pr = P + (int64_t)rows[e] * H;
  const float* qs = q + (int64_t)sess[e] * H;
  float acc = 0.f;
  for (int h = lane; h < H; h += 64) acc = fmaf(w2[h], tanhf(qs[h] + pr[h]), acc);
  acc = sc_wave_sum(acc);
  if (b2) acc += b2[0];
  if (lane == 0) r[e] = relu ? fmaxf(acc, 0.f) : acc;
}

// Column sums of up to three row-major blocks in one launch: out_i[j] = sum_r X_i[r * ld_i + j].  A workgroup takes 64
// columns of one block (lane = column); its four waves take every fourth row, and the four partials are added in wave
// order: an order fixed by the shape alone.
__global__ __launch_bounds__(256) void colsum_segments_kernel(ColSumSeg s0, ColSumSeg s1, ColSumSeg s2) {
  __shared__ float part[4][64];
  int blk = blockIdx.x;
  const int nb0 = (s0.ncol + 63) / 64, nb1 = (s1.ncol + 63) / 64;
  ColSumSeg s = s0;
  if (blk >= nb0) {
    blk -= nb0;
    s = s1;
    if (blk >= nb1) {
      blk -= nb1;
      s = s2;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blk * 64 + lane;
  float acc = 0.f;
  if (j < s.ncol)
    for (int64_t r = wave; r < s.rows; r += 4) acc += s.X[r * s.ld + j];
  part[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && j < s.ncol) s.out[j] = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}

inline unsigned blocks4(int64_t n) { return (unsigned)((n + 3) / 4); }

}  // namespace

hipError_t launch_l2_normalize_rows(const float* x, float* y, int64_t rows, int E, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(l2_normalize_rows_kernel, dim3(blocks4(rows)), dim3(256), 0, stream, x, y, rows, E);
  return hipGetLastError();
}

hipError_t launch_l2_normalize_bwd(const float* u, const float* uh, const float* duh, float* du, int64_t rows, int E,
                                   hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(l2_normalize_bwd_kernel, dim3(blocks4(rows)), dim3(256), 0, stream, u, uh, duh, du, rows, E);
  return hipGetLastError();
}

hipError_t launch_bilinear_pair_fwd(const float* v, const float* c, const float* bias, float* s, int64_t B, int N, int E,
                                    int normalize, hipStream_t stream) {
  const int64_t n = B * N;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(bilinear_pair_fwd_kernel, dim3(blocks4(n)), dim3(256), 0, stream, v, c, bias, s, n, N, E, normalize);
  return hipGetLastError();
}

hipError_t launch_bilinear_pair_bwd(const float* v, const float* c, const float* g, float* dc, float* G, int64_t B, int N, int E,
                                    int normalize, hipStream_t stream) {
  if (B <= 0 || N <= 0) return hipSuccess;
  if (B > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bilinear_pair_bwd_kernel, dim3((unsigned)B), dim3(256), 0, stream, v, c, g, dc, G, N, E, normalize);
  return hipGetLastError();
}

hipError_t launch_mlp_pair_fwd(const float* q, const float* p, const float* w2, const float* b2, float* s, int64_t B, int N, int H,
                               hipStream_t stream) {
  const int64_t n = B * N;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(mlp_pair_fwd_kernel, dim3(blocks4(n)), dim3(256), 0, stream, q, p, w2, b2, s, n, N, H);
  return hipGetLastError();
}

hipError_t launch_mlp_pair_bwd(const float* q, const float* p, const float* w2, const float* g, float* delta, float* Delta,
                               float* dw2_part, int64_t B, int N, int H, hipStream_t stream) {
  if (B <= 0 || N <= 0) return hipSuccess;
  if (B > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mlp_pair_bwd_kernel, dim3((unsigned)B), dim3(256), 0, stream, q, p, w2, g, delta, Delta, dw2_part, N, H);
  return hipGetLastError();
}

hipError_t launch_score_csr_bilinear(const float* vecs, const int32_t* rows, const int32_t* sess, const float* v, const float* bias,
                                     float* r, int64_t n, int E, int relu, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(score_csr_bilinear_kernel, dim3(blocks4(n)), dim3(256), 0, stream, vecs, rows, sess, v, bias, r, n, E, relu);
  return hipGetLastError();
}

hipError_t launch_score_csr_mlp(const float* P, const int32_t* rows, const int32_t* sess, const float* q, const float* w2,
                                const float* b2, float* r, int64_t n, int H, int relu, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(score_csr_mlp_kernel, dim3(blocks4(n)), dim3(256), 0, stream, P, rows, sess, q, w2, b2, r, n, H, relu);
  return hipGetLastError();
}

hipError_t launch_colsum_segments(const ColSumSeg* segs, int n_segs, hipStream_t stream) {
  ColSumSeg s[3] = {};
  int64_t blocks = 0;
  int k = 0;
  for (int i = 0; i < n_segs; ++i) {
    if (!segs[i].out || segs[i].ncol <= 0) continue;  // (a gradient nobody asked for)
    if (k == 3) return hipErrorInvalidValue;
    s[k++] = segs[i];
  }
  for (int i = 0; i < k; ++i) blocks += (s[i].ncol + 63) / 64;
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(colsum_segments_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, s[0], s[1], s[2]);
  return hipGetLastError();
}

}  // namespace xnrs

// =================================================================================================
// C entry points of the bilinear / MLP scorers (scoring.py:41-102): the dense projections on the fp32 GEMM, the per-pair
// parts on the kernels above
// =================================================================================================
using namespace xnrs;

namespace {

// dW[M, N] (pitch ldc) = dY[R, M]^T . X[R, N] over R rows (dY pitch lddy, X pitch ldx); one launch, no split-K
hipError_t sc_gemm_dw(const float* dY, int64_t lddy, const float* X, int64_t ldx, float* dW, int64_t ldc, int M, int N, int64_t R,
                      hipStream_t stream) {
  if (R <= 0) return hipMemset2DAsync(dW, (size_t)ldc * sizeof(float), 0, (size_t)N * sizeof(float), (size_t)M, stream);
  return launch_gemm_f32(gemm_kmajor_ab(dY, lddy, X, ldx, dW, ldc, M, N, R), stream);
}

}  // namespace

extern "C" {

size_t xnrs_bilinear_scoring_saved_bytes(int64_t B, int32_t E, int32_t normalize) {  // v [B, E] | u^ [B, E] (normalize)
  if (B < 0 || E <= 0) return 0;
  return carve_total({(size_t)B * E * F32, normalize ? (size_t)B * E * F32 : 0});
}

int32_t xnrs_bilinear_scoring_fwd(const float* u, const float* c, const float* w, const float* bias, float* s, int64_t B, int32_t N,
                                  int32_t E, int32_t normalize, void* saved, size_t saved_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B < 0 || N < 0 || E <= 0) return XNRS_EINVAL;
  if (B == 0 || N == 0) return XNRS_OK;
  if (!u || !c || !w || !s) return XNRS_EINVAL;
  if (!saved || saved_bytes < xnrs_bilinear_scoring_saved_bytes(B, E, normalize)) return XNRS_EWORKSPACE;
  Carver sv;
  float* v = at(saved, sv.take((size_t)B * E * F32));
  const float* uh = u;
  if (normalize) {  // u^ = u / ||u|| kept beside v for the backward (dW = U^^T G)
    float* un = at(saved, sv.take((size_t)B * E * F32));
    XNRS_TRY(launch_l2_normalize_rows(u, un, B, E, stream));
    uh = un;
  }
  XNRS_TRY(sc_gemm(uh, E, w, E, 1, nullptr, v, E, B, E, E, stream));  // v_b = W[0]^T u^_b
  XNRS_TRY(launch_bilinear_pair_fwd(v, c, bias, s, B, N, E, normalize, stream));
  return XNRS_OK;
}

size_t xnrs_bilinear_scoring_bwd_workspace_bytes(int64_t B, int32_t E, int32_t normalize) {  // G [B, E] | du^ [B, E] (normalize)
  return xnrs_bilinear_scoring_saved_bytes(B, E, normalize);
}

int32_t xnrs_bilinear_scoring_bwd(const float* u, const float* c, const float* w, const void* saved, size_t saved_bytes,
                                  const float* ds, float* du, float* dc, float* dw, float* dbias, int64_t B, int32_t N, int32_t E,
                                  int32_t normalize, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B < 0 || N < 0 || E <= 0) return XNRS_EINVAL;
  if ((B == 0 || N == 0) && !dw && !dbias) return XNRS_OK;
  if (!w || (B * N > 0 && (!u || !c || !ds))) return XNRS_EINVAL;  // (an empty tensor may have no storage)
  if (B > 0x7fffffffLL || B * N >= (1ll << 31)) return XNRS_EUNSUPPORTED;  // one workgroup per impression; 32-bit contraction
  if (!saved || saved_bytes < xnrs_bilinear_scoring_saved_bytes(B, E, normalize)) return XNRS_EWORKSPACE;
  const size_t second = align_up((size_t)B * E * F32);  // the second region of the saved blob and of the workspace
  const float* v = static_cast<const float*>(saved);
  const float* uh = normalize ? at(saved, second) : u;
  const bool pairs = B > 0 && N > 0;
  if (du || dc || dw) {
    if (pairs && (!ws || ws_bytes < xnrs_bilinear_scoring_bwd_workspace_bytes(B, E, normalize))) return XNRS_EWORKSPACE;
    float* G = static_cast<float*>(ws);
    if (pairs) XNRS_TRY(launch_bilinear_pair_bwd(v, c, ds, dc, G, B, N, E, normalize, stream));
    if (dw) XNRS_TRY(sc_gemm_dw(uh, E, G, E, dw, E, E, E, pairs ? B : 0, stream));  // dW[0] = U^^T G
    if (du && B > 0) {
      if (N == 0) XNRS_TRY(hipMemsetAsync(du, 0, (size_t)B * E * sizeof(float), stream));
      else if (!normalize) XNRS_TRY(sc_gemm(G, E, w, E, 0, nullptr, du, E, B, E, E, stream));  // du_b = W[0] G_b
      else {
        float* duh = at(ws, second);
        XNRS_TRY(sc_gemm(G, E, w, E, 0, nullptr, duh, E, B, E, E, stream));
        XNRS_TRY(launch_l2_normalize_bwd(u, uh, duh, du, B, E, stream));
      }
    }
  }
  if (dbias) {
    ColSumSeg seg{ds, 1, B * N, 1, dbias};
    XNRS_TRY(launch_colsum_segments(&seg, 1, stream));
  }
  return XNRS_OK;
}

size_t xnrs_mlp_scoring_saved_bytes(int64_t B, int32_t N, int32_t H) {
  if (B < 0 || N < 0 || H <= 0) return 0;
  return carve_total({(size_t)B * H * F32, (size_t)B * N * H * F32});  // q [B, H] | p [B*N, H]
}

int32_t xnrs_mlp_scoring_news_proj(const float* c, int64_t rows, int32_t E, const float* w1, int32_t H, float* p, void* stream) {
  if (rows < 0 || E <= 0 || H <= 0) return XNRS_EINVAL;
  if (rows == 0) return XNRS_OK;
  if (!c || !w1 || !p) return XNRS_EINVAL;
  return hip_rc(sc_gemm(c, E, w1 + E, 2 * (int64_t)E, 0, nullptr, p, H, rows, H, E, (hipStream_t)stream));  // p = C W1c^T
}

int32_t xnrs_mlp_scoring_fwd(const float* u, const float* c, const float* w1, const float* b1, const float* w2, const float* b2,
                             float* s, int64_t B, int32_t N, int32_t E, int32_t H, void* saved, size_t saved_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B < 0 || N < 0 || E <= 0 || H <= 0) return XNRS_EINVAL;
  if (B == 0 || N == 0) return XNRS_OK;
  if (!u || !c || !w1 || !w2 || !s) return XNRS_EINVAL;
  if (!saved || saved_bytes < xnrs_mlp_scoring_saved_bytes(B, N, H)) return XNRS_EWORKSPACE;
  Carver sv;
  float *q = at(saved, sv.take((size_t)B * H * F32)), *p = at(saved, sv.take((size_t)B * N * H * F32));
  XNRS_TRY(sc_gemm(u, E, w1, 2 * (int64_t)E, 0, b1, q, H, B, H, E, stream));      // q_b = W1u u_b + b1, once per impression
  XNRS_TRY(sc_gemm(c, E, w1 + E, 2 * (int64_t)E, 0, nullptr, p, H, B * N, H, E, stream));  // p_bn = W1c c_bn
  XNRS_TRY(launch_mlp_pair_fwd(q, p, w2, b2, s, B, N, H, stream));
  return XNRS_OK;
}

size_t xnrs_mlp_scoring_bwd_workspace_bytes(int64_t B, int32_t N, int32_t H) {
  if (B < 0 || N < 0 || H <= 0) return 0;
  // delta [B*N, H] | Delta [B, H] | per-impression dw2 partials [B, H]
  return carve_total({(size_t)B * N * H * F32, (size_t)B * H * F32, (size_t)B * H * F32});
}

int32_t xnrs_mlp_scoring_bwd(const float* u, const float* c, const float* w1, const float* w2, const void* saved, size_t saved_bytes,
                             const float* ds, float* du, float* dc, float* dw1, float* db1, float* dw2, float* db2, int64_t B,
                             int32_t N, int32_t E, int32_t H, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B < 0 || N < 0 || E <= 0 || H <= 0) return XNRS_EINVAL;
  const int64_t BN = B * N;
  if (!w1 || !w2 || (BN > 0 && (!u || !c || !ds))) return XNRS_EINVAL;  // (an empty tensor may have no storage)
  if (!saved || saved_bytes < xnrs_mlp_scoring_saved_bytes(B, N, H)) return XNRS_EWORKSPACE;
  if (B > 0x7fffffffLL || BN >= (1ll << 31)) return XNRS_EUNSUPPORTED;  // one workgroup per impression; 32-bit contraction
  Carver sv, wl;
  const float *q = at(saved, sv.take((size_t)B * H * F32)), *p = at(saved, sv.take((size_t)BN * H * F32));
  float* delta = at(ws, wl.take((size_t)BN * H * F32));
  float *Delta = at(ws, wl.take((size_t)B * H * F32)), *dw2p = at(ws, wl.take((size_t)B * H * F32));
  const bool need_delta = dc || dw1;
  const bool need_Delta = du || dw1 || db1;
  if (BN == 0) {  // no pair: every gradient is zero
    if (du && B > 0) XNRS_TRY(hipMemsetAsync(du, 0, (size_t)B * E * sizeof(float), stream));
    if (dw1) XNRS_TRY(hipMemsetAsync(dw1, 0, (size_t)H * 2 * E * sizeof(float), stream));
    if (db1) XNRS_TRY(hipMemsetAsync(db1, 0, (size_t)H * sizeof(float), stream));
    if (dw2) XNRS_TRY(hipMemsetAsync(dw2, 0, (size_t)H * sizeof(float), stream));
    if (db2) XNRS_TRY(hipMemsetAsync(db2, 0, sizeof(float), stream));
    return XNRS_OK;
  }
  if (!ws || ws_bytes < xnrs_mlp_scoring_bwd_workspace_bytes(B, N, H)) return XNRS_EWORKSPACE;
  if (need_delta || need_Delta || dw2)
    XNRS_TRY(launch_mlp_pair_bwd(q, p, w2, ds, need_delta ? delta : nullptr, need_Delta ? Delta : nullptr, dw2 ? dw2p : nullptr, B,
                                 N, H, stream));
  if (dw1) {  // fc1.weight.grad = [dW1u | dW1c]: the two column halves of one (H, 2E) buffer
    XNRS_TRY(sc_gemm_dw(Delta, H, u, E, dw1, 2 * (int64_t)E, H, E, B, stream));       // dW1u = sum_b Delta_b (x) u_b
    XNRS_TRY(sc_gemm_dw(delta, H, c, E, dw1 + E, 2 * (int64_t)E, H, E, BN, stream));  // dW1c = sum_bn delta_bn (x) c_bn
  }
  {  // dw2 = sum_b (sum_n g t), db1 = sum_b Delta_b, db2 = sum g: one fixed-order launch
    ColSumSeg segs[3] = {{dw2p, H, B, H, dw2}, {Delta, H, B, H, db1}, {ds, 1, BN, 1, db2}};
    XNRS_TRY(launch_colsum_segments(segs, 3, stream));
  }
  if (du) XNRS_TRY(sc_gemm(Delta, H, w1, 2 * (int64_t)E, 1, nullptr, du, E, B, E, H, stream));       // du_b = W1u^T Delta_b
  if (dc) XNRS_TRY(sc_gemm(delta, H, w1 + E, 2 * (int64_t)E, 1, nullptr, dc, E, BN, E, H, stream));  // dc_bn = W1c^T delta_bn
  return XNRS_OK;
}

size_t xnrs_score_csr_scorer_workspace_bytes(int64_t n_sess, int32_t width) {
  if (n_sess < 0 || width <= 0) return 0;
  return align_up((size_t)n_sess * width * sizeof(float));
}

int32_t xnrs_score_csr_bilinear(const float* vecs, const int32_t* cand_rows, const int32_t* cand_sess, const float* u, int64_t n_sess,
                                const float* w, const float* bias, float* r, int64_t n_cand, int32_t E, int32_t relu, void* ws,
                                size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_cand < 0 || n_sess < 0 || E <= 0) return XNRS_EINVAL;
  if (n_cand == 0) return XNRS_OK;
  if (!vecs || !cand_rows || !cand_sess || !u || !w || !r) return XNRS_EINVAL;
  if (!ws || ws_bytes < xnrs_score_csr_scorer_workspace_bytes(n_sess, E)) return XNRS_EWORKSPACE;
  float* v = static_cast<float*>(ws);
  XNRS_TRY(sc_gemm(u, E, w, E, 1, nullptr, v, E, n_sess, E, E, stream));  // v_b = W[0]^T u_b, once per impression
  XNRS_TRY(launch_score_csr_bilinear(vecs, cand_rows, cand_sess, v, bias, r, n_cand, E, relu, stream));
  return XNRS_OK;
}

int32_t xnrs_score_csr_mlp(const float* P, const int32_t* cand_rows, const int32_t* cand_sess, const float* u, int64_t n_sess,
                           const float* w1, const float* b1, const float* w2, const float* b2, float* r, int64_t n_cand, int32_t E,
                           int32_t H, int32_t relu, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_cand < 0 || n_sess < 0 || E <= 0 || H <= 0) return XNRS_EINVAL;
  if (n_cand == 0) return XNRS_OK;
  if (!P || !cand_rows || !cand_sess || !u || !w1 || !w2 || !r) return XNRS_EINVAL;
  if (!ws || ws_bytes < xnrs_score_csr_scorer_workspace_bytes(n_sess, H)) return XNRS_EWORKSPACE;
  float* q = static_cast<float*>(ws);
  XNRS_TRY(sc_gemm(u, E, w1, 2 * (int64_t)E, 0, b1, q, H, n_sess, H, E, stream));  // q_b = W1u u_b + b1
  XNRS_TRY(launch_score_csr_mlp(P, cand_rows, cand_sess, q, w2, b2, r, n_cand, H, relu, stream));
  return XNRS_OK;
}

int32_t xnrs_l2_normalize_rows(const float* x, float* y, int64_t rows, int32_t E, void* stream) {
  if (rows < 0 || E <= 0) return XNRS_EINVAL;
  if (rows == 0) return XNRS_OK;
  if (!x || !y) return XNRS_EINVAL;
  return hip_rc(launch_l2_normalize_rows(x, y, rows, E, (hipStream_t)stream));
}

}  // extern "C"
