// One-layer GRU over the first T history vectors of every user (LSTUR's short-term tower, lstur.py:113-154; nn.GRU with
// batch_first, gate order r, z, n, both bias vectors), forward and backward, fp32 on v_mfma_f32_32x32x2_f32.
//
//   Gi = X . W_ih^T + b_ih for all B*T rows           one launch of the dense forward GEMM (gemm_f32.hip)
//   per step t:  Gh = h_{t-1} . W_hh^T + b_hh, the gates and h_t in the epilogue            (gru_fwd_tile)
//   backward:    per step the gate gradients and dh_{t-1} = dGh_t . W_hh + z dh_t            (gru_bwd_tile)
//                then dW_hh = dGh^T . H_prev, dW_ih = dGi^T . X, dX = dGi . W_ih: ONE product each over the stacked
//                B*T rows on the existing weight-gradient / input-gradient GEMMs, the bias gradients beside them
//
// A step is a [B, Hd] x [Hd, 3Hd] product: 32 x 32 output tiles of h_t, one workgroup of four waves per tile, each wave
// taking every fourth 8-wide k slice of all three gates (three accumulators), the partial tiles added up in LDS in wave
// order (no atomics: bit-identical run to run) and the epilogue spread over the four waves.  Operands are read straight
// from global memory as 16-byte chunks along k -- both MFMA operands take their k index from the same lane rule, so a lane
// that loads k .. k+3 of its row feeds four MFMAs without any shuffle; W_hh (888 KB at Hd = 272) stays in L2.
//
// Two layouts of the same tile code (knob XNRS_GRU_LAYOUT; DESIGN.md section 10b compares them):
//   0  one 2-D launch per step (row tiles x column tiles); the stream orders the steps
//   1  one launch; a workgroup owns 32 batch rows, walks the column tiles and all T steps alone (the recurrence is
//      independent across batch rows), a workgroup barrier + fence between steps.  No grid-wide barrier exists in either.
//
// Rows that have run out of history (t >= len) carry their state through; the training forward stores z = 1, r = n = 0 for
// them, which makes every backward formula below give dh_{t-1} = dh_t and zero gate gradients without a special case.  A
// row of length 0 therefore returns its initial state (the reference raises in pack_padded_sequence).
#include "host.h"

using namespace xnrs;

namespace {

constexpr int TILE = 32;   // rows and columns of an output tile (one MFMA block)
constexpr int WAVES = 4;   // k slices in flight per tile
constexpr int KCHUNK = 8;  // k values per wave and iteration: lanes 0-31 take k .. k+3, lanes 32-63 k+4 .. k+7

__device__ __forceinline__ float4 load_k4(const float* __restrict__ p, int64_t k, int64_t K, bool ok, bool vec) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!ok || k >= K) return v;
  if (vec) return *reinterpret_cast<const float4*>(p + k);  // K % 4 == 0 and k % 4 == 0: the chunk is inside the row
  v.x = p[k];
  if (k + 1 < K) v.y = p[k + 1];
  if (k + 2 < K) v.z = p[k + 2];
  if (k + 3 < K) v.w = p[k + 3];
  return v;
}

// acc[g] += A[row0 .., :] . B_g[col0 .., :]^T over this wave's k slices; ap / bp[g]: the lane's row of A / of B_g
template <int NB>
__device__ __forceinline__ void tile_product(const float* __restrict__ ap, bool aok, const float* __restrict__ bp, int64_t b_gate_stride,
                                             bool bok, int64_t K, bool vec, int wave, int half, f32x16 (&acc)[NB]) {
  for (int64_t k0 = (int64_t)wave * KCHUNK; k0 < K; k0 += WAVES * KCHUNK) {
    const int64_t k = k0 + half * 4;
    const float4 av = load_k4(ap, k, K, aok, vec);
    float4 bv[NB];
#pragma unroll
    for (int g = 0; g < NB; ++g) bv[g] = load_k4(bp + g * b_gate_stride, k, K, bok, vec);
#pragma unroll
    for (int g = 0; g < NB; ++g) {
      acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv[g].x, acc[g], 0, 0, 0);
      acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv[g].y, acc[g], 0, 0, 0);
      acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv[g].z, acc[g], 0, 0, 0);
      acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv[g].w, acc[g], 0, 0, 0);
    }
  }
}

// The four waves' partial tiles added in wave order; wave w leaves with accumulator registers 4w .. 4w+3 of every block:
// out[g][j] is element (row 8w + 4 half + j, column lane & 31) of block g.
template <int NB>
__device__ __forceinline__ void reduce_tiles(const f32x16 (&acc)[NB], float* red, int wave, int lane, float (&out)[NB][4]) {
  __syncthreads();  // the readers of the previous tile are done with `red`
#pragma unroll
  for (int g = 0; g < NB; ++g)
#pragma unroll
    for (int i = 0; i < 16; ++i) red[((wave * NB + g) * 16 + i) * 64 + lane] = acc[g][i];
  __syncthreads();
#pragma unroll
  for (int g = 0; g < NB; ++g)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) s += red[((w * NB + g) * 16 + 4 * wave + j) * 64 + lane];
      out[g][j] = s;
    }
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// the state after s steps: where it lives and its row pitch (s == 0: the caller's h0, possibly null = zeros)
__device__ __forceinline__ float* gru_state(const GruFwdArgs& a, int s, int64_t* ld) {
  *ld = a.Hd;
  if (s == 0) return const_cast<float*>(a.h0);
  if (s == a.T) return a.y;
  if (a.q) {  // training: hs row b*T + s is the state before step s
    *ld = (int64_t)a.T * a.Hd;
    return a.hs + (int64_t)s * a.Hd;
  }
  return a.hs + (int64_t)(s & 1) * a.B * a.Hd;
}

__device__ __forceinline__ void gru_fwd_tile(const GruFwdArgs& a, int t, int row0, int col0) {
  __shared__ float red[WAVES * 3 * 16 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
  const int Hd = a.Hd, T = a.T;
  int64_t ldin, ldout;
  const float* hin = gru_state(a, t, &ldin);
  float* hout = gru_state(a, t + 1, &ldout);
  f32x16 acc[3];
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[g][i] = 0.f;
  const int col = col0 + l31;
  if (hin) {
    const int arow = row0 + l31;
    tile_product<3>(hin + (int64_t)arow * ldin, arow < a.B, a.whh + (int64_t)col * Hd, (int64_t)Hd * Hd, col < Hd, Hd, a.vec != 0,
                    wave, half, acc);
  }
  float gh[3][4];
  reduce_tiles<3>(acc, red, wave, lane, gh);
  if (col >= Hd) return;
  const float br = a.bhh ? a.bhh[col] : 0.f, bz = a.bhh ? a.bhh[Hd + col] : 0.f, bn = a.bhh ? a.bhh[2 * Hd + col] : 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = row0 + 8 * wave + 4 * half + j;
    if (row >= a.B) continue;
    const float hp = hin ? hin[(int64_t)row * ldin + col] : 0.f;
    float* g = a.g + ((int64_t)row * T + t) * 3 * Hd + col;
    const bool active = t < a.len[row];
    const float q = gh[2][j] + bn;
    const float r = sigmoid_f(g[0] + gh[0][j] + br);
    const float z = sigmoid_f(g[Hd] + gh[1][j] + bz);
    const float n = tanhf(fmaf(r, q, g[2 * Hd]));
    hout[(int64_t)row * ldout + col] = active ? fmaf(z, hp - n, n) : hp;
    if (a.q) {
      g[0] = active ? r : 0.f;
      g[Hd] = active ? z : 1.f;
      g[2 * Hd] = active ? n : 0.f;
      a.q[((int64_t)row * T + t) * Hd + col] = active ? q : 0.f;
      if (t == 0) a.hs[(int64_t)row * T * Hd + col] = hp;
    }
  }
}

__global__ __launch_bounds__(256) void gru_fwd_step_kernel(GruFwdArgs a, int t) {
  gru_fwd_tile(a, t, blockIdx.x * TILE, blockIdx.y * TILE);
}

__global__ __launch_bounds__(256) void gru_fwd_rows_kernel(GruFwdArgs a) {
  const int row0 = blockIdx.x * TILE;
  for (int t = 0; t < a.T; ++t) {
    for (int col0 = 0; col0 < a.Hd; col0 += TILE) gru_fwd_tile(a, t, row0, col0);
    __threadfence();  // h_t of this workgroup's rows: written above, read by all its waves in the next step
    __syncthreads();
  }
}

// One tile of the backward: (tg >= 0) dh = dGh[:, tg, :] . W_hh + z_tg dh, else dh = dy; then (te >= 0) the gate
// gradients of step te from that dh.  The state gradient of an element is read and written by its own lane only.
__device__ __forceinline__ void gru_bwd_tile(const GruBwdArgs& a, int tg, int te, int row0, int col0) {
  __shared__ float red[WAVES * 16 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
  const int Hd = a.Hd, T = a.T;
  const int64_t K = 3 * (int64_t)Hd;
  const int col = col0 + l31;
  float s[1][4] = {{0.f, 0.f, 0.f, 0.f}};
  if (tg >= 0) {
    f32x16 acc[1];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[0][i] = 0.f;
    const int arow = row0 + l31;
    tile_product<1>(a.dgh + ((int64_t)arow * T + tg) * K, arow < a.B, a.whh_t + (int64_t)col * K, 0, col < Hd, K, a.vec != 0, wave,
                    half, acc);
    reduce_tiles<1>(acc, red, wave, lane, s);
  }
  if (col >= Hd) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = row0 + 8 * wave + 4 * half + j;
    if (row >= a.B) continue;
    const int64_t ih = (int64_t)row * Hd + col;
    float d = tg >= 0 ? a.dh[ih] : a.dy[ih];
    if (tg >= 0) d = fmaf(a.g[((int64_t)row * T + tg) * K + Hd + col], d, s[0][j]);
    a.dh[ih] = d;
    if (te < 0) continue;
    const int64_t rt = (int64_t)row * T + te;
    const float* g = a.g + rt * K + col;
    const float r = g[0], z = g[Hd], n = g[2 * Hd], q = a.q[rt * Hd + col], hp = a.hs[rt * Hd + col];
    const float dnp = d * (1.f - z) * (1.f - n * n);
    const float dzp = d * (hp - n) * z * (1.f - z);
    const float drp = dnp * q * r * (1.f - r);
    float* gi = a.dgi + rt * K + col;
    float* gh = a.dgh + rt * K + col;
    gi[0] = drp;
    gi[Hd] = dzp;
    gi[2 * Hd] = dnp;
    gh[0] = drp;
    gh[Hd] = dzp;
    gh[2 * Hd] = dnp * r;
  }
}

__global__ __launch_bounds__(256) void gru_bwd_step_kernel(GruBwdArgs a, int tg, int te) {
  gru_bwd_tile(a, tg, te, blockIdx.x * TILE, blockIdx.y * TILE);
}

__global__ __launch_bounds__(256) void gru_bwd_rows_kernel(GruBwdArgs a) {
  const int row0 = blockIdx.x * TILE;
  for (int t = a.T; t >= 0; --t) {  // t == T: dy and the gates of the last step; t == 0: the gradient of h0
    for (int col0 = 0; col0 < a.Hd; col0 += TILE) gru_bwd_tile(a, t < a.T ? t : -1, t - 1, row0, col0);
    __threadfence();  // dGh of step t - 1: written above, read by all waves of this workgroup in the next round
    __syncthreads();
  }
}

// len[b] = number of ones among the first T mask values of row b (lstur.py:140-141), clamped to [0, T]; no mask: T
__global__ __launch_bounds__(256) void gru_lengths_kernel(const float* __restrict__ m, int64_t ldm, int32_t* __restrict__ len,
                                                          int64_t B, int T) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float s = (float)T;
  if (m) {
    s = 0.f;
    for (int t = 0; t < T; ++t) s += m[b * ldm + t];
  }
  const int n = (int)(s + 0.5f);
  len[b] = n < 0 ? 0 : (n > T ? T : n);
}

dim3 step_grid(int B, int Hd) { return dim3((unsigned)((B + TILE - 1) / TILE), (unsigned)((Hd + TILE - 1) / TILE)); }

}  // namespace

hipError_t xnrs::launch_gru_lengths(const float* m, int64_t ldm, int32_t* len, int64_t B, int T, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(gru_lengths_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, m, ldm, len, B, T);
  return hipGetLastError();
}

hipError_t xnrs::launch_gru_fwd(const GruFwdArgs& a, hipStream_t stream) {
  if (a.B <= 0) return hipSuccess;
  if (knobs().gru_layout == 1) {
    hipLaunchKernelGGL(gru_fwd_rows_kernel, dim3((unsigned)((a.B + TILE - 1) / TILE)), dim3(256), 0, stream, a);
    return hipGetLastError();
  }
  for (int t = 0; t < a.T; ++t) {
    hipLaunchKernelGGL(gru_fwd_step_kernel, step_grid(a.B, a.Hd), dim3(256), 0, stream, a, t);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t xnrs::launch_gru_bwd(const GruBwdArgs& a, hipStream_t stream) {
  if (a.B <= 0) return hipSuccess;
  if (knobs().gru_layout == 1) {
    hipLaunchKernelGGL(gru_bwd_rows_kernel, dim3((unsigned)((a.B + TILE - 1) / TILE)), dim3(256), 0, stream, a);
    return hipGetLastError();
  }
  for (int t = a.T; t >= 0; --t) {
    hipLaunchKernelGGL(gru_bwd_step_kernel, step_grid(a.B, a.Hd), dim3(256), 0, stream, a, t < a.T ? t : -1, t - 1);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

namespace {

// inference workspace / training blob: Gi (training: r | z | n) | states | Gh_n | lengths
struct GruRegions {
  size_t g, hs, q, len, total;
};
GruRegions gru_regions(int64_t B, int T, int Hd, bool train) {
  Carver c;
  GruRegions r{};
  r.g = c.take((size_t)B * T * 3 * Hd * F32);
  r.hs = c.take((train ? (size_t)B * T : (size_t)2 * B) * Hd * F32);
  r.q = c.take_if(train, (size_t)B * T * Hd * F32);
  r.len = c.take((size_t)B * sizeof(int32_t));
  r.total = c.total();
  return r;
}

// split-K slabs | column-sum partials | W_hh^T | W_ih^T scratch of the dX product | dh | dGi | dGh
struct GruBwdRegions {
  size_t slabs, csum, whh_t, wih_t, dh, dgi, dgh, total;
};
GruBwdRegions gru_bwd_regions(int64_t B, int T, int E, int Hd) {
  Carver c;
  GruBwdRegions r{};
  const size_t s1 = gemm_splitk_workspace_bytes(3 * Hd, Hd, B * T), s2 = gemm_splitk_workspace_bytes(3 * Hd, E, B * T);
  r.slabs = c.take(s1 > s2 ? s1 : s2);
  r.csum = c.take(colsum_workspace_bytes(3 * Hd));
  r.whh_t = c.take((size_t)3 * Hd * Hd * F32);
  r.wih_t = c.take((size_t)3 * Hd * E * F32);
  r.dh = c.take((size_t)B * Hd * F32);
  r.dgi = c.take((size_t)B * T * 3 * Hd * F32);
  r.dgh = c.take((size_t)B * T * 3 * Hd * F32);
  r.total = c.total();
  return r;
}

bool gru_shape_ok(int64_t B, int32_t T, int32_t E, int32_t Hd) {
  return B >= 0 && T > 0 && E > 0 && Hd > 0 && B * T * 3 * (int64_t)Hd < (1LL << 40) && B < (1LL << 30);
}

int32_t gru_forward(const float* x, const float* m, int32_t ldm, const float* h0, const xnrs_gru_params* p, float* y, int64_t B,
                    int32_t T, int32_t E, void* buf, size_t buf_bytes, bool train, hipStream_t stream) {
  if (!p || !gru_shape_ok(B, T, E, p->hidden)) return XNRS_EINVAL;
  if (B == 0) return XNRS_OK;
  if (!x || !y || !p->w_ih || !p->w_hh || (m && ldm < T)) return XNRS_EINVAL;
  const int Hd = p->hidden;
  const GruRegions r = gru_regions(B, T, Hd, train);
  if (!buf || buf_bytes < r.total) return XNRS_EWORKSPACE;
  GruFwdArgs a{};
  a.g = at(buf, r.g);
  a.whh = p->w_hh;
  a.bhh = p->b_hh;
  a.h0 = h0;
  a.len = at<int32_t>(buf, r.len);
  a.y = y;
  a.hs = at(buf, r.hs);
  a.q = train ? at(buf, r.q) : nullptr;
  a.B = (int32_t)B;
  a.T = T;
  a.Hd = Hd;
  a.vec = (Hd % 4 == 0 && aligned16(p->w_hh) && (!h0 || aligned16(h0))) ? 1 : 0;
  XNRS_TRY(launch_gru_lengths(m, ldm, at<int32_t>(buf, r.len), B, T, stream));
  XNRS_TRY(launch_gemm_f32(gemm_linear(x, {}, E, p->w_ih, p->b_ih, a.g, 3 * (int64_t)Hd, B * T, 3 * Hd, E), stream));
  XNRS_TRY(launch_gru_fwd(a, stream));
  return XNRS_OK;
}

}  // namespace

extern "C" {

size_t xnrs_gru_workspace_bytes(int64_t B, int32_t T, int32_t E, int32_t Hd) {
  return gru_shape_ok(B, T, E, Hd) ? gru_regions(B, T, Hd, false).total : 0;
}

size_t xnrs_gru_saved_bytes(int64_t B, int32_t T, int32_t E, int32_t Hd) {
  return gru_shape_ok(B, T, E, Hd) ? gru_regions(B, T, Hd, true).total : 0;
}

int32_t xnrs_gru_fwd(const float* x, const float* m, int32_t ldm, const float* h0, const xnrs_gru_params* p, float* y, int64_t B,
                     int32_t T, int32_t E, void* ws, size_t ws_bytes, void* stream) {
  return gru_forward(x, m, ldm, h0, p, y, B, T, E, ws, ws_bytes, false, (hipStream_t)stream);
}

int32_t xnrs_gru_fwd_train(const float* x, const float* m, int32_t ldm, const float* h0, const xnrs_gru_params* p, float* y,
                           int64_t B, int32_t T, int32_t E, void* saved, size_t saved_bytes, void* stream) {
  return gru_forward(x, m, ldm, h0, p, y, B, T, E, saved, saved_bytes, true, (hipStream_t)stream);
}

size_t xnrs_gru_bwd_workspace_bytes(int64_t B, int32_t T, int32_t E, int32_t Hd) {
  return gru_shape_ok(B, T, E, Hd) ? gru_bwd_regions(B, T, E, Hd).total : 0;
}

int32_t xnrs_gru_bwd(const float* x, const xnrs_gru_params* p, const void* saved, size_t saved_bytes, const float* dy, float* dx,
                     float* dh0, const xnrs_gru_grads* g, int64_t B, int32_t T, int32_t E, void* ws, size_t ws_bytes,
                     void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!p || !gru_shape_ok(B, T, E, p->hidden)) return XNRS_EINVAL;
  const int Hd = p->hidden;
  const int64_t M = B * T;
  if (B == 0) {  // nothing was encoded: the weight gradients are zero
    if (g && g->w_ih) XNRS_TRY(hipMemsetAsync(g->w_ih, 0, (size_t)3 * Hd * E * F32, stream));
    if (g && g->w_hh) XNRS_TRY(hipMemsetAsync(g->w_hh, 0, (size_t)3 * Hd * Hd * F32, stream));
    if (g && g->b_ih) XNRS_TRY(hipMemsetAsync(g->b_ih, 0, (size_t)3 * Hd * F32, stream));
    if (g && g->b_hh) XNRS_TRY(hipMemsetAsync(g->b_hh, 0, (size_t)3 * Hd * F32, stream));
    return XNRS_OK;
  }
  if (!x || !saved || !dy || !p->w_ih || !p->w_hh) return XNRS_EINVAL;
  const GruRegions s = gru_regions(B, T, Hd, true);
  if (saved_bytes < s.total) return XNRS_EINVAL;
  const GruBwdRegions r = gru_bwd_regions(B, T, E, Hd);
  if (!ws || ws_bytes < r.total) return XNRS_EWORKSPACE;
  GruBwdArgs a{};
  a.g = at(saved, s.g);
  a.q = at(saved, s.q);
  a.hs = at(saved, s.hs);
  a.whh_t = at(ws, r.whh_t);
  a.dy = dy;
  a.dh = dh0 ? dh0 : at(ws, r.dh);
  a.dgi = at(ws, r.dgi);
  a.dgh = at(ws, r.dgh);
  a.B = (int32_t)B;
  a.T = T;
  a.Hd = Hd;
  a.vec = Hd % 4 == 0 ? 1 : 0;  // both operands of the step product live in the 256-byte aligned workspace
  XNRS_TRY(launch_transpose(p->w_hh, at(ws, r.whh_t), 3 * Hd, Hd, stream));
  XNRS_TRY(launch_gru_bwd(a, stream));
  float *slabs = at(ws, r.slabs), *csum = at(ws, r.csum);
  const int N = 3 * Hd;
  if (g && g->w_hh) XNRS_TRY(gemm_dw(a.dgh, N, a.hs, {}, Hd, g->w_hh, M, N, Hd, slabs, stream, {}, {g->b_hh, csum}));
  else if (g && g->b_hh) XNRS_TRY(launch_colsum(a.dgh, N, nullptr, M, N, g->b_hh, csum, stream));
  if (g && g->w_ih) XNRS_TRY(gemm_dw(a.dgi, N, x, {}, E, g->w_ih, M, N, E, slabs, stream, {}, {g->b_ih, csum}));
  else if (g && g->b_ih) XNRS_TRY(launch_colsum(a.dgi, N, nullptr, M, N, g->b_ih, csum, stream));
  if (dx) XNRS_TRY(gemm_dx(a.dgi, N, p->w_ih, dx, E, M, N, E, stream, at(ws, r.wih_t)));
  return XNRS_OK;
}

}  // extern "C"
