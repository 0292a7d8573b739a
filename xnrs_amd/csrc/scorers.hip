// The bilinear and MLP scorers of the reference (xnrs/models/components/scoring.py:41-102) around the existing GEMMs:
// the dense projections (v = U.W, q = U.W1u^T + b1, p = C.W1c^T and the weight-gradient products) run on
// launch_gemm_f32 (api.hip); these kernels are the per-pair parts no GEMM does, and the fixed-order reductions.
//   bilinear : s[b,n] = v_b . c^_bn + bias                    v_b = W[0]^T u^_b, u^ / c^ optionally L2-normalised
//   MLP      : s[b,n] = w2 . tanh(q_b + p_bn) + b2            q_b = W1u u_b + b1, p_bn = W1c c_bn
// fp32 throughout, no atomics: every sum runs in an order fixed by the launch shape alone, which does not depend on
// the data (the same bits on every run, in a hipGraph replay too).
#include "kernels.h"

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
