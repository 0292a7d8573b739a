// Device-side batch assembly and evaluation kernels -- the callers / data formats on either side of the
// encoders.  Integer / index work, HBM-bound, no MFMA.
//
//   assemble_train : NewsRecDataset.__getitem__ in 'train' mode (xnrs/data/dataset.py:54-57,77-85,97-109,147)
//                    + custom_collate_fn (xnrs/utils.py:190-204), producing ROW IDS into the device-resident
//                    news table instead of 4.6 MB of gathered token tensors per impression.
//   assemble_eval  : the same in 'eval' mode (dataset.py:58-61,149): all positives then all negatives,
//                    variable C -> CSR.
//   score_csr      : DotScoring over a CSR candidate list against pre-encoded news vectors
//                    (scoring.py:23 applied per impression, training.py:194-203 with batch_size 1).
//   rank_metrics   : xnrs/evaluation/metrics.py:9-64 per impression (nDCG@k, RR, CTR@k, AUC, acc/rec/prec).
//   gather_rows    : the dict look-ups + torch.cat of NewsRecDataset.__getitem__ (dataset.py:63-85,97-109) as a
//                    device copy: out[i] = table[ids[i]] for whole news blocks (S*D floats, 150 KB at the shipped
//                    shape) -- the materialised batch for consumers that need dense token tensors (input gradients
//                    of the explainer, explain.py:160-166); the encoders themselves gather inside their first load.
//   dropout_rows   : the towers' input dropout (news_encoding.py:51, user_encoding.py:69) on dense rows, or fused with
//                    gather_rows for the id path: the dropped batch is materialised in the launch that gathers it.
#include <atomic>
#include <type_traits>

#include "host.h"

namespace xnrs {

__device__ __forceinline__ uint64_t mix64(uint64_t seed, uint64_t a, uint64_t b) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (a * 0x100000001B3ull + b + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// one thread per output id
__global__ __launch_bounds__(256) void assemble_train_kernel(BatchArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int W = a.l_hist + 1 + a.n_neg;
  if (i >= a.B * W) return;
  const int64_t b = i / W;
  const int j = (int)(i - b * W);
  const int64_t s = a.sess[b];
  if (j < a.l_hist) {
    // the LAST l_hist clicked news first, zero padding behind them (dataset.py:77-85)
    const int64_t lo = a.hist_off[s], hi = a.hist_off[s + 1];
    const int64_t n = (hi - lo < a.l_hist) ? (hi - lo) : a.l_hist;
    a.hist_out[b * a.l_hist + j] = (j < n) ? a.hist_val[hi - n + j] : a.pad_row;
  } else {
    const int c = j - a.l_hist;  // 0 = the positive, 1.. = negatives
    int32_t row = a.pad_row;
    if (c == 0) {
      const int64_t lo = a.pos_off[s], n = a.pos_off[s + 1] - lo;
      if (n > 0) row = a.pos_val[lo + (int64_t)(mix64(a.seed, (uint64_t)s, 0) % (uint64_t)n)];  // random.choice
    } else {
      const int64_t lo = a.neg_off[s], n = a.neg_off[s + 1] - lo;
      if (n > 0) row = a.neg_val[lo + (int64_t)(mix64(a.seed, (uint64_t)s, (uint64_t)c) % (uint64_t)n)];  // random.choices (with replacement)
    }
    a.cand_out[b * (1 + a.n_neg) + c] = row;
  }
}

hipError_t launch_assemble_train(const BatchArgs& a, hipStream_t stream) {
  const int64_t n = a.B * (a.l_hist + 1 + a.n_neg);
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(assemble_train_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// one wave per impression: history ids + candidate CSR fill (offsets computed by the caller)
__global__ __launch_bounds__(256) void assemble_eval_kernel(BatchArgs a) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const int lane = threadIdx.x & 63;
  const int64_t s = a.sess[b];
  {
    const int64_t lo = a.hist_off[s], hi = a.hist_off[s + 1];
    const int64_t n = (hi - lo < a.l_hist) ? (hi - lo) : a.l_hist;
    for (int j = lane; j < a.l_hist; j += 64) a.hist_out[b * a.l_hist + j] = (j < n) ? a.hist_val[hi - n + j] : a.pad_row;
  }
  const int64_t plo = a.pos_off[s], np = a.pos_off[s + 1] - plo;
  const int64_t nlo = a.neg_off[s], nn = a.neg_off[s + 1] - nlo;
  const int64_t o = a.cand_off_out[b];
  for (int64_t k = lane; k < np + nn; k += 64) {
    a.cand_out[o + k] = (k < np) ? a.pos_val[plo + k] : a.neg_val[nlo + (k - np)];
    a.cand_sess_out[o + k] = (int32_t)b;
    a.targets_out[o + k] = (k < np) ? 1.f : 0.f;
  }
}

hipError_t launch_assemble_eval(const BatchArgs& a, hipStream_t stream) {
  if (a.B <= 0) return hipSuccess;
  hipLaunchKernelGGL(assemble_eval_kernel, dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// r[e] = <vecs[cand_rows[e], :], u[cand_sess[e], :]> : one wave per candidate entry
__global__ __launch_bounds__(256) void score_csr_kernel(const float* vecs, const int32_t* rows, const int32_t* sess, const float* u,
                                                         float* r, int64_t n, int E, int relu) {
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= n) return;
  const int lane = threadIdx.x & 63;
  const float* v = vecs + (int64_t)rows[e] * E;
  const float* uu = u + (int64_t)sess[e] * E;
  float acc = 0.f;
  for (int k = lane; k < E; k += 64) acc = fmaf(v[k], uu[k], acc);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if (lane == 0) r[e] = relu ? fmaxf(acc, 0.f) : acc;
}

hipError_t launch_score_csr(const float* vecs, const int32_t* rows, const int32_t* sess, const float* u, float* r, int64_t n,
                            int E, int relu, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(score_csr_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, vecs, rows, sess, u, r, n, E, relu);
  return hipGetLastError();
}

// Per-impression ranking metrics, one wave per impression, O(C^2) rank counting (C is tens to hundreds).
// Order = np.argsort(score)[::-1]; ties are broken "higher original index first" (what a stable ascending
// sort reversed gives; numpy's default sort is stable below 17 elements -- beyond that the reference's own
// tie order is unspecified).  out[b, :] = {ndcg@5, ndcg@10, rr, ctr@1, ctr@10, auc, acc, rec, prec}.
__global__ __launch_bounds__(256) void rank_metrics_kernel(const float* score, const float* target, const int64_t* off, float* out,
                                                            int64_t B) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const int64_t lo = off[b];
  const int C = (int)(off[b + 1] - lo);
  const float* s = score + lo;
  const float* t = target + lo;
  float dcg5 = 0.f, dcg10 = 0.f, rr = 0.f, top1 = 0.f, top10 = 0.f, npos = 0.f, conc = 0.f;
  float tp = 0.f, fp = 0.f, fn = 0.f, tn = 0.f;
  for (int e = lane; e < C; e += 64) {
    float se = s[e];
    if (se != se) se = 0.f;  // np.nan_to_num(nan=0, posinf=1, neginf=0) (training.py:210-211)
    else if (se == INFINITY) se = 1.f;
    else if (se == -INFINITY) se = 0.f;
    const float te = t[e];
    int rank = 1;
    float gt = 0.f, eq = 0.f;  // negatives scored below / equal (for AUC), only used when te == 1
    for (int f = 0; f < C; ++f) {
      float sf = s[f];
      if (sf != sf) sf = 0.f;
      else if (sf == INFINITY) sf = 1.f;
      else if (sf == -INFINITY) sf = 0.f;
      if (sf > se || (sf == se && f > e)) ++rank;
      if (t[f] == 0.f) {
        if (sf < se) gt += 1.f;
        else if (sf == se) eq += 1.f;
      }
    }
    const float gain = exp2f(te) - 1.f;  // 2**y - 1 (metrics.py:12)
    const float disc = log2f((float)rank + 1.f);
    if (rank <= 5) dcg5 += gain / disc;
    if (rank <= 10) dcg10 += gain / disc;
    if (te > 0.f) {
      rr = fmaxf(rr, te / (float)rank);
      conc += gt + 0.5f * eq;
      npos += 1.f;
    }
    if (rank <= 1) top1 += te;
    if (rank <= 10) top10 += te;
    const float pred = rintf(fminf(fmaxf(se, 0.f), 1.f));  // np.round(np.clip(s, 0, 1)): round-half-even
    if (pred > 0.5f) { if (te > 0.5f) tp += 1.f; else fp += 1.f; }
    else { if (te > 0.5f) fn += 1.f; else tn += 1.f; }
  }
  float v[11] = {dcg5, dcg10, top1, top10, npos, conc, tp, fp, fn, tn, 0.f};
#pragma unroll
  for (int i = 0; i < 10; ++i)
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) v[i] += __shfl_xor(v[i], o2);
#pragma unroll
  for (int o2 = 32; o2 > 0; o2 >>= 1) rr = fmaxf(rr, __shfl_xor(rr, o2));
  if (lane == 0) {
    const float np_ = v[4], nneg = (float)C - v[4];
    // ideal DCG: the positives first (metrics.py:18-19: dcg_score(y_true, y_true, k))
    float best5 = 0.f, best10 = 0.f;
    for (int i = 0; i < 10 && i < (int)np_; ++i) {
      const float d = 1.f / log2f((float)i + 2.f);
      if (i < 5) best5 += d;
      best10 += d;
    }
    float* o = out + b * 9;
    o[0] = v[0] / best5;
    o[1] = v[1] / best10;
    o[2] = rr;
    o[3] = v[2] / (float)(C < 1 ? C : 1);
    o[4] = v[3] / (float)(C < 10 ? C : 10);
    o[5] = v[5] / (np_ * nneg);
    o[6] = (v[6] + v[9]) / (float)C;
    o[7] = v[6] / (v[6] + v[8]);
    o[8] = (v[6] + v[7]) > 0.f ? v[6] / (v[6] + v[7]) : 0.f;  // zero_division=0 (metrics.py:58)
  }
}

hipError_t launch_rank_metrics(const float* score, const float* target, const int64_t* off, float* out, int64_t B,
                               hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(rank_metrics_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, stream, score, target, off, out, B);
  return hipGetLastError();
}

// ---------------------------------------------------------------- gather_rows (HBM-bound block copy)
// one workgroup per (output row, 16-KB piece): 4 independent 16-byte loads per thread, streaming (nontemporal) on both
// sides -- every byte is touched once.  Each load sits behind its own bounds branch, and the compiler waits for it inside
// that branch, so a wave has ONE of the four in flight at a time and the other waves of the CU cover the latency: a
// branch-free path for full pieces (all four in flight) was measured on dropout_rows_kernel below, which has this loop
// shape, and moved nothing
template <bool VEC>
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ table, const int32_t* __restrict__ ids,
                                                           float* __restrict__ out, int64_t row_floats, int pieces) {
  const int64_t row = blockIdx.x / pieces;
  const int piece = (int)(blockIdx.x - row * pieces);
  const int64_t src = (int64_t)ids[row] * row_floats, dst = row * row_floats;
  if (VEC) {
    const int64_t n4 = row_floats >> 2;
    const f32x4* s4 = reinterpret_cast<const f32x4*>(table + src);
    f32x4* d4 = reinterpret_cast<f32x4*>(out + dst);
    const int64_t base = (int64_t)piece * 1024 + threadIdx.x;
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (base + 256 * u < n4) v[u] = __builtin_nontemporal_load(s4 + base + 256 * u);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (base + 256 * u < n4) __builtin_nontemporal_store(v[u], d4 + base + 256 * u);
  } else {
    const int64_t base = (int64_t)piece * 4096 + threadIdx.x;
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (base + 256 * u < row_floats) out[dst + base + 256 * u] = table[src + base + 256 * u];
  }
}

hipError_t launch_gather_rows(const float* table, const int32_t* ids, float* out, int64_t n, int64_t row_floats,
                              hipStream_t stream) {
  if (n <= 0 || row_floats <= 0) return hipSuccess;
  const bool vec = row_floats % 4 == 0 && ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int64_t pieces = (row_floats + 4095) / 4096;  // 16 KB per workgroup
  if (n * pieces > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(n * pieces));
  if (vec) hipLaunchKernelGGL((gather_rows_kernel<true>), grid, dim3(256), 0, stream, table, ids, out, row_floats, (int)pieces);
  else hipLaunchKernelGGL((gather_rows_kernel<false>), grid, dim3(256), 0, stream, table, ids, out, row_floats, (int)pieces);
  return hipGetLastError();
}

// ---------------------------------------------------------------- dropout_rows (gather_rows + the towers' input dropout)
// The shape of gather_rows_kernel: one workgroup per (output row, 16-KB piece), 16-byte streaming accesses.  Element j of
// output row i draws drop_uniform(row i of the CALL, j): the 64-bit part of the draw depends on (seed, i) alone -- uniform
// over the workgroup, computed once -- and each element pays the 32-bit finaliser.  x and out are not __restrict__: a dense
// call may run in place (every thread loads its elements before it stores them, and no other thread touches them).
__device__ __forceinline__ float drop_element(const DropRowsArgs& a, int64_t row, uint32_t j, float v, float keep, float scale) {
  return drop_uniform(a, row, j) < keep ? v * scale : 0.f;
}
template <bool VEC>
__global__ __launch_bounds__(256) void dropout_rows_kernel(const float* x, const int32_t* __restrict__ ids, float* out,
                                                            int64_t row_floats, int pieces, float p, DropRowsArgs a0) {
  // the device word is read ONCE, before any store (out is not __restrict__: a later read would have to be repeated)
  const DropRowsArgs a{drop_seed(a0), nullptr, 1};
  const int64_t row = blockIdx.x / pieces;
  const int piece = (int)(blockIdx.x - row * pieces);
  const int64_t src = (ids ? (int64_t)ids[row] : row) * row_floats, dst = row * row_floats;
  const float keep = 1.f - p, scale = 1.f / (1.f - p);
  if (VEC) {
    const int64_t n4 = row_floats >> 2;
    const f32x4* s4 = reinterpret_cast<const f32x4*>(x + src);
    f32x4* d4 = reinterpret_cast<f32x4*>(out + dst);
    const int64_t base = (int64_t)piece * 1024 + threadIdx.x;
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (base + 256 * u < n4) v[u] = __builtin_nontemporal_load(s4 + base + 256 * u);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (base + 256 * u < n4) {
        const uint32_t j = (uint32_t)(base + 256 * u) * 4u;  // < row_floats < 2^32
#pragma unroll
        for (int c = 0; c < 4; ++c) v[u][c] = drop_element(a, row, j + c, v[u][c], keep, scale);
        __builtin_nontemporal_store(v[u], d4 + base + 256 * u);
      }
  } else {
    const int64_t base = (int64_t)piece * 4096 + threadIdx.x;
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (base + 256 * u < row_floats)
        out[dst + base + 256 * u] = drop_element(a, row, (uint32_t)(base + 256 * u), x[src + base + 256 * u], keep, scale);
  }
}

// 0 < p < 1
hipError_t launch_dropout_rows(const float* x, const int32_t* ids, float* out, int64_t n, int64_t row_floats, float p,
                               uint64_t seed, const uint64_t* seed_dev, hipStream_t stream) {
  if (n <= 0 || row_floats <= 0) return hipSuccess;
  const bool vec = row_floats % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int64_t pieces = (row_floats + 4095) / 4096;  // 16 KB per workgroup
  if (n * pieces > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(n * pieces));
  const DropRowsArgs a{seed, seed_dev, 1};
  if (vec) hipLaunchKernelGGL((dropout_rows_kernel<true>), grid, dim3(256), 0, stream, x, ids, out, row_floats, (int)pieces, p, a);
  else hipLaunchKernelGGL((dropout_rows_kernel<false>), grid, dim3(256), 0, stream, x, ids, out, row_floats, (int)pieces, p, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------- gather_rows / dropout_rows from a table stored in bf16
// The streaming shape of the two kernels above with the widening on the way (a bf16 value is the high half of its fp32 value:
// bits << 16, exact): one workgroup per (output row, 16 KB of output), a thread's 8 consecutive elements are ONE 16-byte
// load and two 16-byte stores.  Logical row i is table row ids[i / S] * S + i % S (ids nullable: row i).  DROP: the input
// dropout of dropout_rows_kernel on the widened value -- the same drop_element with the same (seed, row of the call, column).
typedef unsigned u32x4b __attribute__((ext_vector_type(4)));
template <bool VEC, bool DROP>
__global__ __launch_bounds__(256) void gather_rows_bf16_kernel(const unsigned short* __restrict__ table, const int32_t* __restrict__ ids,
                                                                int S, int64_t row0, float* __restrict__ out, int64_t row_elems,
                                                                int pieces, float p, DropRowsArgs a0) {
  const DropRowsArgs a{DROP ? drop_seed(a0) : 0ull, nullptr, 1};
  const int64_t row = blockIdx.x / pieces;
  const int piece = (int)(blockIdx.x - row * pieces);
  int64_t srow = row0 + row;  // (row0: the launch writes logical rows row0 .. row0 + n of a longer list to out rows 0 .. n)
  if (ids) {
    const int64_t n = srow / S;
    srow = (int64_t)ids[n] * S + (srow - n * S);
  }
  const int64_t src = srow * row_elems, dst = row * row_elems;
  const float keep = 1.f - p, scale = 1.f / (1.f - p);
  if (VEC) {
    const int64_t n8 = row_elems >> 3;
    const u32x4b* s8 = reinterpret_cast<const u32x4b*>(table + src);
    f32x4* d4 = reinterpret_cast<f32x4*>(out + dst);
    const int64_t base = (int64_t)piece * 512 + threadIdx.x;
    u32x4b v[2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (base + 256 * u < n8) v[u] = __builtin_nontemporal_load(s8 + base + 256 * u);
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (base + 256 * u < n8) {
        const int64_t c = base + 256 * u;
        f32x4 lo, hi;  // elements 0..3 and 4..7 of the chunk: the low half of a word is the earlier element
#pragma unroll
        for (int w = 0; w < 2; ++w) {
          lo[2 * w] = __uint_as_float(v[u][w] << 16);
          lo[2 * w + 1] = __uint_as_float(v[u][w] & 0xffff0000u);
          hi[2 * w] = __uint_as_float(v[u][2 + w] << 16);
          hi[2 * w + 1] = __uint_as_float(v[u][2 + w] & 0xffff0000u);
        }
        if (DROP) {
          const uint32_t j = (uint32_t)c * 8u;  // < row_elems < 2^32
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            lo[e] = drop_element(a, row, j + e, lo[e], keep, scale);
            hi[e] = drop_element(a, row, j + 4 + e, hi[e], keep, scale);
          }
        }
        __builtin_nontemporal_store(lo, d4 + 2 * c);
        __builtin_nontemporal_store(hi, d4 + 2 * c + 1);
      }
  } else {
    const int64_t base = (int64_t)piece * 4096 + threadIdx.x;
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (base + 256 * u < row_elems) {
        const float x = __uint_as_float((unsigned)table[src + base + 256 * u] << 16);
        out[dst + base + 256 * u] = DROP ? drop_element(a, row, (uint32_t)(base + 256 * u), x, keep, scale) : x;
      }
  }
}

template <bool DROP>
static hipError_t launch_rows_bf16(const unsigned short* table, const int32_t* ids, int S, int64_t row0, float* out, int64_t n,
                                   int64_t row_elems, float p, uint64_t seed, const uint64_t* seed_dev, hipStream_t stream) {
  if (n <= 0 || row_elems <= 0) return hipSuccess;
  if (ids && S <= 0) return hipErrorInvalidValue;
  const bool vec = row_elems % 8 == 0 && ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int64_t pieces = (row_elems + 4095) / 4096;  // 16 KB of output per workgroup
  if (n * pieces > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(n * pieces));
  const DropRowsArgs a{seed, seed_dev, 1};
  if (vec)
    hipLaunchKernelGGL((gather_rows_bf16_kernel<true, DROP>), grid, dim3(256), 0, stream, table, ids, S, row0, out, row_elems, (int)pieces, p, a);
  else
    hipLaunchKernelGGL((gather_rows_bf16_kernel<false, DROP>), grid, dim3(256), 0, stream, table, ids, S, row0, out, row_elems, (int)pieces, p, a);
  return hipGetLastError();
}

hipError_t launch_gather_rows_bf16(const unsigned short* table, const int32_t* ids, int S, float* out, int64_t n, int64_t row_elems,
                                   hipStream_t stream, int64_t row0) {
  return launch_rows_bf16<false>(table, ids, S, row0, out, n, row_elems, 0.f, 0, nullptr, stream);
}

// 0 < p < 1
hipError_t launch_dropout_rows_bf16(const unsigned short* table, const int32_t* ids, float* out, int64_t n, int64_t row_elems, float p,
                                    uint64_t seed, const uint64_t* seed_dev, hipStream_t stream) {
  return launch_rows_bf16<true>(table, ids, 1, 0, out, n, row_elems, p, seed, seed_dev, stream);
}

// ---- row compaction on the device (the padding-free encoder without a host round trip).
// For every pass of `chunk` news (mask [.., S] fp32 0/1, optionally gathered by news id): CSR offsets of the live token rows
// per news, the list of live token rows, and the list of ALL token rows of the non-empty news (K / V are projected for
// every token of a news that has a live query: the reference masks QUERY rows only, layers.py:142-144 -- and for none of
// an all-masked news, whose keys nobody reads).  ONE launch for the whole call, one 1024-thread workgroup per pass
// (blockIdx.x = pass p, news p*chunk .. ; its lists start at p*chunk*S, its offsets at p*(chunk+1), its counts at 3*p):
// a wave reads one news' mask row coalesced and counts / places its live tokens by ballot, the two scans over the news of
// the pass are wave scans joined through LDS.  (A first version ran per pass with one thread per news walking its mask
// row three times: 109 us per pass, 2.4 ms of a 50 ms step.)
//   row_off [chunk+1]   compact range of news j: row_off[j] .. row_off[j+1]
//   live_src [<= chunk*S]  source token row (x row space: ids[news]*S + s with a table, else news*S + s) of compact row i
//   kv_src [<= chunk*S]  source row of the i-th kept token row: the K|V image of a pass holds the non-empty news as
//                        CONSECUTIVE blocks of S rows; kv_block[j] = block of news j (the attention kernel's MhaCoreArgs::kv_block)
//   counts[0] = live rows, counts[1] = kept K|V rows      (device scalars the GEMMs read: GemmArgs::m_dev)
//   counts[2] = 1 if a mask value other than 0 / 1 was seen: the pooling kernel then writes NaN instead of a result that
//               would silently differ from the reference's exp(e) * m (there is no host read here to raise from)
__global__ __launch_bounds__(1024) void compact_rows_kernel(const float* __restrict__ mask, const int32_t* __restrict__ ids,
                                                             int64_t n_news, int64_t chunk, int S, int64_t* __restrict__ row_off_all,
                                                             int32_t* __restrict__ live_all, int32_t* __restrict__ kvs_all,
                                                             int32_t* __restrict__ kvb_all, int64_t* __restrict__ counts_all) {
  __shared__ int s_cnt[1024];
  __shared__ int s_ex[2][1024];
  __shared__ int s_wsum[2][16];
  __shared__ int s_carry[2];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t news0 = (int64_t)blockIdx.x * chunk;
  const int cn = (int)(n_news - news0 < chunk ? n_news - news0 : chunk);
  int64_t* row_off = row_off_all + (int64_t)blockIdx.x * (chunk + 1);
  int32_t* live_src = live_all + (int64_t)blockIdx.x * chunk * S;
  int32_t* kv_src = kvs_all + (int64_t)blockIdx.x * chunk * S;
  int32_t* kv_block = kvb_all + (int64_t)blockIdx.x * chunk;
  int64_t* counts = counts_all + 3 * (int64_t)blockIdx.x;
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;  // the lanes before this one
  int bad = 0;
  if (tid < 2) s_carry[tid] = 0;
  if (tid == 0) row_off[0] = 0;
  __syncthreads();
  for (int base = 0; base < cn; base += 1024) {
    // live tokens per news: wave w takes the news base + w, base + w + 16, ...
    for (int jj = wave; jj < 1024; jj += 16) {
      const int j = base + jj;
      int cnt = 0;
      if (j < cn) {
        const int64_t mrow = ids ? (int64_t)ids[news0 + j] : news0 + j;
        const float* mp = mask + mrow * S;
        for (int s0 = 0; s0 < S; s0 += 64) {
          const float mv = s0 + lane < S ? mp[s0 + lane] : 0.f;
          bad |= (mv != 0.f && mv != 1.f) ? 1 : 0;
          cnt += __popcll(__ballot(mv != 0.f));
        }
      }
      if (lane == 0) s_cnt[jj] = cnt;
    }
    __syncthreads();
    // exclusive scans of (live count) and (kept K|V rows = S for a non-empty news) over the 1024 news of this round
    const int cnt = s_cnt[tid];
    const int v[2] = {cnt, cnt > 0 ? S : 0};
    int incl[2];
    for (int which = 0; which < 2; ++which) {
      int x = v[which];
      for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(x, off);
        if (lane >= off) x += up;
      }
      incl[which] = x;
      if (lane == 63) s_wsum[which][wave] = x;
    }
    __syncthreads();
    for (int which = 0; which < 2; ++which) {
      int before = s_carry[which];
      for (int w = 0; w < wave; ++w) before += s_wsum[which][w];
      s_ex[which][tid] = before + incl[which] - v[which];
    }
    if (base + tid < cn) row_off[base + tid + 1] = s_ex[0][tid] + cnt;
    __syncthreads();
    if (tid == 1023) {
      s_carry[0] = s_ex[0][1023] + v[0];
      s_carry[1] = s_ex[1][1023] + v[1];
    }
    // the lists, a wave per news again
    for (int jj = wave; jj < 1024; jj += 16) {
      const int j = base + jj;
      if (j >= cn) break;
      const int64_t mrow = ids ? (int64_t)ids[news0 + j] : news0 + j;
      const float* mp = mask + mrow * S;
      const int64_t src0 = mrow * S;  // source token row of (news, 0)
      const bool kept = s_cnt[jj] > 0;
      int w = s_ex[0][jj];
      const int e1 = s_ex[1][jj];
      for (int s0 = 0; s0 < S; s0 += 64) {
        const int sl = s0 + lane;
        const bool on = sl < S && mp[sl] != 0.f;
        const uint64_t b = __ballot(on);
        if (on) live_src[w + __popcll(b & below)] = (int32_t)(src0 + sl);
        w += __popcll(b);
        if (kept && sl < S) kv_src[e1 + sl] = (int32_t)(src0 + sl);
      }
      if (lane == 0) kv_block[j] = e1 / S;  // (an empty news: the block the next non-empty one gets -- never read)
    }
    __syncthreads();
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) {
    counts[0] = s_carry[0];
    counts[1] = s_carry[1];
    counts[2] = bad ? 1 : 0;
  }
}

// The same lists for S <= 64 (every shape with an attention tower), throughput-shaped: the mask of a round of 1 024 news is
// read ONCE, flattened over the workgroup (element i -> news i / S, token i % S: coalesced, ~50 independent loads per
// thread instead of a wave walking 64 news one dependent load at a time), each live token sets its bit in the news' 64-bit
// word in LDS; counts are popcounts, and the lists are written by the same flattened sweep (a live token's place = the
// news' offset + the popcount of the bits below it).  378 -> 249 us per call of 25 600 news x 50 in five passes (it sits on
// the critical path of the device-compacted encoder; one workgroup per pass is what bounds it now: the passes' rounds of
// 1 024 news run one after the other).  (The dense encoder passes have a list kernel of their own: dense_row_lists_kernel.)
__global__ __launch_bounds__(1024) void compact_rows64_kernel(const float* __restrict__ mask, const int32_t* __restrict__ ids,
                                                               int64_t n_news, int64_t chunk, int S, int64_t* __restrict__ row_off_all,
                                                               int32_t* __restrict__ live_all, int32_t* __restrict__ kvs_all,
                                                               int32_t* __restrict__ kvb_all, int64_t* __restrict__ counts_all) {
  __shared__ unsigned long long s_bits[1024];
  __shared__ int64_t s_row[1024];
  __shared__ int s_ex[2][1024];
  __shared__ int s_wsum[2][16];
  __shared__ int s_carry[2];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t news0 = (int64_t)blockIdx.x * chunk;
  const int cn = (int)(n_news - news0 < chunk ? n_news - news0 : chunk);
  int64_t* row_off = row_off_all + (int64_t)blockIdx.x * (chunk + 1);
  int32_t* live_src = live_all + (int64_t)blockIdx.x * chunk * S;
  int32_t* kv_src = kvs_all + (int64_t)blockIdx.x * chunk * S;
  int32_t* kv_block = kvb_all + (int64_t)blockIdx.x * chunk;
  int64_t* counts = counts_all + 3 * (int64_t)blockIdx.x;
  int bad = 0;
  if (tid < 2) s_carry[tid] = 0;
  if (tid == 0) row_off[0] = 0;
  for (int base = 0; base < cn; base += 1024) {
    const int nn = cn - base < 1024 ? cn - base : 1024;
    s_bits[tid] = 0ull;
    s_row[tid] = tid < nn ? (ids ? (int64_t)ids[news0 + base + tid] : news0 + base + tid) : 0;
    __syncthreads();
    const int n_el = nn * S;
    // four elements per trip, their loads issued together (the sweep is latency-bound: one load, one LDS atomic per element)
    for (int i0 = tid; i0 < n_el; i0 += 4096) {
      float mv[4];
      int jj[4], sl[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + 1024 * u;
        jj[u] = (i < n_el ? i : 0) / S;
        sl[u] = (i < n_el ? i : 0) - jj[u] * S;
        mv[u] = i < n_el ? mask[s_row[jj[u]] * S + sl[u]] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        bad |= (mv[u] != 0.f && mv[u] != 1.f) ? 1 : 0;
        if (mv[u] != 0.f) atomicOr(&s_bits[jj[u]], 1ull << sl[u]);
      }
    }
    __syncthreads();
    const unsigned long long bits = s_bits[tid];
    const int cnt = __popcll(bits);
    const int v[2] = {cnt, cnt > 0 ? S : 0};
    int incl[2];
    for (int which = 0; which < 2; ++which) {
      int x = v[which];
      for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(x, off);
        if (lane >= off) x += up;
      }
      incl[which] = x;
      if (lane == 63) s_wsum[which][wave] = x;
    }
    __syncthreads();
    for (int which = 0; which < 2; ++which) {
      int before = s_carry[which];
      for (int w = 0; w < wave; ++w) before += s_wsum[which][w];
      s_ex[which][tid] = before + incl[which] - v[which];
    }
    if (tid < nn) {
      row_off[base + tid + 1] = s_ex[0][tid] + cnt;
      kv_block[base + tid] = s_ex[1][tid] / S;  // (an empty news: the block the next non-empty one gets -- never read)
    }
    __syncthreads();
    if (tid == 1023) {
      s_carry[0] = s_ex[0][1023] + v[0];
      s_carry[1] = s_ex[1][1023] + v[1];
    }
#pragma unroll 4
    for (int i = tid; i < n_el; i += 1024) {
      const int jj = i / S, sl = i - jj * S;
      const unsigned long long b = s_bits[jj];
      if (b == 0ull) continue;
      const int32_t src = (int32_t)(s_row[jj] * S + sl);
      kv_src[s_ex[1][jj] + sl] = src;
      if ((b >> sl) & 1ull) live_src[s_ex[0][jj] + __popcll(b & ((1ull << sl) - 1ull))] = src;
    }
    __syncthreads();
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) {
    counts[0] = s_carry[0];
    counts[1] = s_carry[1];
    counts[2] = bad ? 1 : 0;
  }
}

// ---- the grad step's row lists on the device (xnrs_build_row_lists): the unmasked token rows ("live") and all token rows of
// the non-empty sequences ("kv"), each in the batch's own row space [n_seq*L] and -- with a gathered table -- in the table's,
// plus both counts as device scalars the GEMMs read (GemmArgs::m_dev / k_dev).  Replaces the torch bookkeeping of
// xnrs_amd/autograd.py (a nonzero + ONE host read of the counts per encoder call).  Two short launches, both chip-wide:
//   counts: a wave per sequence -> cnt[seq] = live tokens (ballot popcounts)
//   lists : a workgroup per 64 sequences: its base offsets = sums over cnt[0 .. first) (coalesced, a few KB), a wave scan
//           over its own 64 counts, then a wave per sequence places its tokens by ballot.  Order = row order, exactly the
//           lists torch.nonzero gave.
__global__ __launch_bounds__(256) void row_counts_kernel(const float* __restrict__ mask, const int32_t* __restrict__ ids,
                                                          int64_t n_seq, int L, int32_t* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t seq = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seq >= n_seq) return;
  const float* mp = mask + (ids ? (int64_t)ids[seq] : seq) * L;
  int c = 0;
  for (int s0 = 0; s0 < L; s0 += 64) c += __popcll(__ballot(s0 + lane < L && mp[s0 + lane] != 0.f));
  if (lane == 0) cnt[seq] = c;
}

constexpr int RL_SEQ = 64;  // sequences per workgroup of row_lists_kernel
__global__ __launch_bounds__(1024) void row_lists_kernel(const float* __restrict__ mask, const int32_t* __restrict__ ids,
                                                          int64_t n_seq, int L, const int32_t* __restrict__ cnt,
                                                          int32_t* __restrict__ live, int32_t* __restrict__ live_src,
                                                          int32_t* __restrict__ kv, int32_t* __restrict__ kv_src,
                                                          int64_t* __restrict__ counts) {
  __shared__ int s_red[2][16];
  __shared__ int s_base[2];
  __shared__ int s_ex[2][RL_SEQ];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t first = (int64_t)blockIdx.x * RL_SEQ;
  // base offsets of this workgroup: live tokens / non-empty sequences before `first`
  int a0 = 0, a1 = 0;
  for (int64_t i = tid; i < first; i += 1024) {
    const int c = cnt[i];
    a0 += c;
    a1 += c > 0 ? 1 : 0;
  }
  for (int off = 32; off > 0; off >>= 1) {
    a0 += __shfl_xor(a0, off);
    a1 += __shfl_xor(a1, off);
  }
  if (lane == 0) {
    s_red[0][wave] = a0;
    s_red[1][wave] = a1;
  }
  __syncthreads();
  if (tid == 0) {
    int b0 = 0, b1 = 0;
    for (int w = 0; w < 16; ++w) {
      b0 += s_red[0][w];
      b1 += s_red[1][w];
    }
    s_base[0] = b0;
    s_base[1] = b1 * L;
  }
  if (wave == 0) {  // exclusive scan over this workgroup's 64 sequences
    const int64_t seq = first + lane;
    const int c = seq < n_seq ? cnt[seq] : 0;
    int x0 = c, x1 = c > 0 ? L : 0;
    const int v0 = x0, v1 = x1;
    for (int off = 1; off < 64; off <<= 1) {
      const int u0 = __shfl_up(x0, off), u1 = __shfl_up(x1, off);
      if (lane >= off) {
        x0 += u0;
        x1 += u1;
      }
    }
    s_ex[0][lane] = x0 - v0;
    s_ex[1][lane] = x1 - v1;
  }
  __syncthreads();
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (int j = wave; j < RL_SEQ; j += 16) {
    const int64_t seq = first + j;
    if (seq >= n_seq) break;
    const int64_t mrow = ids ? (int64_t)ids[seq] : seq;
    const float* mp = mask + mrow * L;
    const bool kept = cnt[seq] > 0;
    int w = s_base[0] + s_ex[0][j];
    const int e1 = s_base[1] + s_ex[1][j];
    for (int s0 = 0; s0 < L; s0 += 64) {
      const int sl = s0 + lane;
      const bool on = sl < L && mp[sl] != 0.f;
      const uint64_t b = __ballot(on);
      if (on) {
        const int at = w + __popcll(b & below);
        live[at] = (int32_t)(seq * L + sl);
        if (live_src) live_src[at] = (int32_t)(mrow * L + sl);
      }
      w += __popcll(b);
      if (kept && sl < L) {
        kv[e1 + sl] = (int32_t)(seq * L + sl);
        if (kv_src) kv_src[e1 + sl] = (int32_t)(mrow * L + sl);
      }
    }
  }
  if (first + RL_SEQ >= n_seq && tid == 0) {  // the last workgroup knows the totals
    const int nn = (int)(n_seq - first);
    const int lastc = cnt[n_seq - 1];
    counts[0] = s_base[0] + s_ex[0][nn - 1] + lastc;
    counts[1] = s_base[1] + s_ex[1][nn - 1] + (lastc > 0 ? L : 0);
  }
}

hipError_t launch_build_row_lists(const float* mask, const int32_t* ids, int64_t n_seq, int L, int32_t* live, int32_t* live_src,
                                  int32_t* kv, int32_t* kv_src, int64_t* counts, int32_t* cnt_scratch, hipStream_t stream) {
  if (n_seq <= 0 || L <= 0) return hipSuccess;
  if (n_seq * (int64_t)L > 0x7fffffffLL) return hipErrorInvalidValue;  // int32 row indices
  hipLaunchKernelGGL(row_counts_kernel, dim3((unsigned)((n_seq + 3) / 4)), dim3(256), 0, stream, mask, ids, n_seq, L, cnt_scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(row_lists_kernel, dim3((unsigned)((n_seq + RL_SEQ - 1) / RL_SEQ)), dim3(1024), 0, stream, mask, ids, n_seq, L,
                     cnt_scratch, live, live_src, kv, kv_src, counts);
  return hipGetLastError();
}

// NaN over a result whose precondition turned out violated on the device (the flags of every pass, OR-ed)
__global__ __launch_bounds__(256) void poison_kernel(float* y, int64_t n, const int64_t* flags, int n_flags, int flag_stride,
                                                     int32_t* status) {
  bool bad = false;
  for (int i = 0; i < n_flags; ++i) bad = bad || flags[(int64_t)i * flag_stride] != 0;
  if (!bad) return;
  if (status && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, 1 /* XNRS_STATUS_NONBINARY_MASK */);
  const float nanv = __builtin_nanf("");
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = nanv;
}

hipError_t launch_poison(float* y, int64_t n, const int64_t* flags, int n_flags, int flag_stride, hipStream_t stream) {
  if (n <= 0 || n_flags <= 0) return hipSuccess;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(poison_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, y, n, flags, n_flags, flag_stride, status_word());
  return hipGetLastError();
}

// ONE word, on the device that was current when it was registered: a launch on another device gets nullptr (its kernels must
// not be handed a pointer into this device's memory; their NaN outputs remain the signal there)
static std::atomic<int32_t*> g_status_word{nullptr};
static std::atomic<int> g_status_device{-1};
int32_t* status_word() {
  int32_t* w = g_status_word.load(std::memory_order_relaxed);
  if (!w) return nullptr;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != g_status_device.load(std::memory_order_relaxed)) return nullptr;
  return w;
}
void set_status_word(int32_t* w) {
  int dev = -1;
  (void)hipGetDevice(&dev);
  g_status_device.store(w ? dev : -1, std::memory_order_relaxed);
  g_status_word.store(w, std::memory_order_relaxed);
}

hipError_t launch_compact_rows(const float* mask, const int32_t* ids, int64_t n_news, int64_t chunk, int S, int64_t* row_off,
                               int32_t* live_src, int32_t* kv_src, int32_t* kv_block, int64_t* counts, hipStream_t stream) {
  if (n_news <= 0 || chunk <= 0) return hipSuccess;
  const int64_t passes = (n_news + chunk - 1) / chunk;
  if (passes > 0x7fffffffLL) return hipErrorInvalidValue;
  if (S <= 64)
    hipLaunchKernelGGL(compact_rows64_kernel, dim3((unsigned)passes), dim3(1024), 0, stream, mask, ids, n_news, chunk, S, row_off,
                       live_src, kv_src, kv_block, counts);
  else
    hipLaunchKernelGGL(compact_rows_kernel, dim3((unsigned)passes), dim3(1024), 0, stream, mask, ids, n_news, chunk, S, row_off,
                       live_src, kv_src, kv_block, counts);
  return hipGetLastError();
}

// ---- live row tiles of the DENSE encoder passes (GemmArgs::live_tiles).
// The rows stay where they are; what is listed is, for every pass of `chunk` sequences, the BM-row tiles of its
// [cn * L]-row image in which at least one row belongs to a sequence with any mask value != 0 (mask [.., L] fp32,
// optionally gathered by id), in ascending order, and their number.  A sequence whose mask is all zero has a result that
// needs none of its rows (encoder_fwd.hip), so a tile that holds only such rows is not computed.  ONE launch for the whole
// call, one 1024-thread workgroup per pass, like the row compaction above:
//   alive [n_seq] bytes     scratch: 1 = the sequence has an unmasked token (a thread per sequence walks its mask row)
//   n_tiles [pass]          number of live tiles of the pass (device scalar the GEMMs read)
//   tiles [pass * cap ..]   their indices; cap = tiles of a full pass
__device__ void list_live_tiles(const uint8_t* __restrict__ alive, int64_t cn, int L, int BM, int32_t* __restrict__ tiles,
                                int64_t* __restrict__ n_out, int* s_wsum, int* s_carry);

__global__ __launch_bounds__(1024) void live_tiles_kernel(const float* __restrict__ mask, const int32_t* __restrict__ ids,
                                                           int64_t n_seq, int64_t chunk, int L, int BM, int64_t cap,
                                                           uint8_t* __restrict__ alive_all, int64_t* __restrict__ n_tiles,
                                                           int32_t* __restrict__ tiles_all) {
  __shared__ int s_wsum[16];
  __shared__ int s_carry;
  const int tid = threadIdx.x;
  const int64_t seq0 = (int64_t)blockIdx.x * chunk;
  const int64_t cn = n_seq - seq0 < chunk ? n_seq - seq0 : chunk;
  uint8_t* alive = alive_all + seq0;
  int32_t* tiles = tiles_all + (int64_t)blockIdx.x * cap;
  for (int64_t j = tid; j < cn; j += 1024) {
    const float* mp = mask + (ids ? (int64_t)ids[seq0 + j] : seq0 + j) * L;
    int any = 0;
#pragma unroll 4
    for (int s = 0; s < L; ++s) any |= mp[s] != 0.f ? 1 : 0;
    alive[j] = (uint8_t)any;
  }
  if (tid == 0) s_carry = 0;
  __syncthreads();  // (the flags were written by this workgroup: visible to it behind the barrier)
  list_live_tiles(alive, cn, L, BM, tiles, n_tiles + blockIdx.x, s_wsum, &s_carry);
}

// the tile scan of a pass (one 1024-thread workgroup; *s_carry == 0 and the alive flags visible on entry, s_wsum: 16 ints):
// tiles[0 .. *n_out) = the BM-row tiles of the [cn * L]-row image that hold a row of an alive sequence, ascending
__device__ void list_live_tiles(const uint8_t* __restrict__ alive, int64_t cn, int L, int BM, int32_t* __restrict__ tiles,
                                int64_t* __restrict__ n_out, int* s_wsum, int* s_carry) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t rows = cn * L;
  const int64_t nt = (rows + BM - 1) / BM;
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (int64_t base = 0; base < nt; base += 1024) {
    const int64_t t = base + tid;
    bool live = false;
    if (t < nt) {
      const int64_t r0 = t * BM, r1 = (r0 + BM < rows ? r0 + BM : rows) - 1;
      for (int64_t n = r0 / L; n <= r1 / L; ++n) live = live || alive[n] != 0;
    }
    const uint64_t b = __ballot(live);
    if (lane == 0) s_wsum[wave] = __popcll(b);
    __syncthreads();
    int before = *s_carry;
    for (int w = 0; w < wave; ++w) before += s_wsum[w];
    if (live) tiles[before + __popcll(b & below)] = (int32_t)t;
    __syncthreads();
    if (tid == 0) {
      int tot = *s_carry;
      for (int w = 0; w < 16; ++w) tot += s_wsum[w];
      *s_carry = tot;
    }
    __syncthreads();
  }
  if (tid == 0) *n_out = *s_carry;
}

hipError_t launch_live_tiles(const float* mask, const int32_t* ids, int64_t n_seq, int64_t chunk, int L, int BM, uint8_t* alive,
                             int64_t* n_tiles, int32_t* tiles, hipStream_t stream) {
  if (n_seq <= 0 || chunk <= 0 || L <= 0 || BM <= 0) return hipSuccess;
  const int64_t passes = (n_seq + chunk - 1) / chunk;
  const int64_t cap = live_tiles_cap(chunk, L, BM);
  if (passes > 0x7fffffffLL || cap > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(live_tiles_kernel, dim3((unsigned)passes), dim3(1024), 0, stream, mask, ids, n_seq, chunk, L, BM, cap, alive,
                     n_tiles, tiles);
  return hipGetLastError();
}

// ---- live rows AND live row tiles of the DENSE encoder passes in one launch (encoder_fwd.hip "live rows"; S <= 64).
// Rows stay where they are, so what a pass needs is the ascending list of its unmasked token rows in the pass's own row space
// (live_loc: where Q and the scores are written, and where the O rows are read), the same tokens' rows in the gathered table
// when there are ids (live_src, else not written), their number (counts[0]; counts[1] = S x its non-empty news), and the
// live 128-row tile list of launch_live_tiles.  A mask value other than 0 / 1 is legal (a row is live iff mask != 0, the
// dense path's own rule).
// This used to be one 1 024-thread workgroup per pass (compact_rows64_kernel's sweep): 20 workgroups on 256 CUs, 61-69 us at
// the head of every encoder call with nothing beside it.  Now a pass is cut into slices of DL_SLICE news, a workgroup each.
// No workgroup waits for another and no atomic decides a place: a slice finds its offset in the pass's list by COUNTING the
// live tokens of the news before it in the same pass (at most chunk x S mask floats, 262 KB at the benchmark's pass, out of
// L2), a wave per news row and one ballot per row -- so the list order, and every byte written, is what the one workgroup
// wrote.  The workgroup of a pass's LAST slice has then seen every news of the pass: it alone writes the alive flags, the
// two counts and -- from those flags -- the tile list (list_live_tiles).
constexpr int DL_SLICE = 64;  // news per workgroup: 4 rows per wave of its own, and at most chunk / 16 rows per wave to count
constexpr int DL_ROWS = 16;   // mask rows a wave has in flight (8 waves per SIMD: two workgroups per CU, every slice of a call resident at once)
__global__ __launch_bounds__(1024, 8) void dense_row_lists_kernel(const float* __restrict__ mask, const int32_t* __restrict__ ids,
                                                                int64_t n_news, int64_t chunk, int S, int nsl,
                                                                int32_t* __restrict__ live_loc_all, int32_t* __restrict__ live_src_all,
                                                                int64_t* __restrict__ counts_all, uint8_t* __restrict__ alive_all,
                                                                int64_t* __restrict__ n_tiles, int32_t* __restrict__ tiles_all,
                                                                int64_t cap, int BM) {
  __shared__ unsigned long long s_bits[DL_SLICE];  // the live tokens of the slice's news
  __shared__ int32_t s_row[DL_SLICE];              // their mask rows
  __shared__ int s_ex[DL_SLICE];                   // their first places in the pass's list
  __shared__ int s_part[2][16];                    // per wave: live tokens / non-empty news BEFORE the slice
  __shared__ int s_wsum[16];
  __shared__ int s_carry;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (scalar: the rows a wave walks are addressed from SGPRs)
  const int64_t pass = blockIdx.x / nsl;
  const int slice = blockIdx.x % nsl;
  const int64_t news0 = pass * chunk;
  const int cn = (int)(n_news - news0 < chunk ? n_news - news0 : chunk);
  const int j0 = slice * DL_SLICE;
  if (j0 >= cn) return;  // (a short last pass has fewer slices; uniform)
  const int j1 = j0 + DL_SLICE < cn ? j0 + DL_SLICE : cn;
  const bool last = j1 == cn;
  if (tid < DL_SLICE) {
    s_bits[tid] = 0ull;
    s_row[tid] = 0;
  }
  __syncthreads();
  // the news [0, j1) of the pass, a wave per row, DL_ROWS rows per trip.  Every load of a trip is UNCONDITIONAL (row and token
  // clamped, the value dropped afterwards): behind a "load or constant" select the compiler branches around each load and
  // waits for it, and the sweep -- 82 rows per wave for the last slice of a 1 310-news pass -- becomes 82 dependent round
  // trips to memory (that, not the one workgroup per pass, was most of the old kernel's 61-69 us).
  int before = 0, kept = 0;  // (wave-uniform)
  const int lc = lane < S ? lane : S - 1;
  auto sweep = [&](auto gathered) {
    for (int jb = wave; jb < j1; jb += 16 * DL_ROWS) {
      int32_t row[DL_ROWS];  // (a news index or an id: 32 bits, the launcher checks n_news)
      float mv[DL_ROWS];
#pragma unroll
      for (int u = 0; u < DL_ROWS; ++u) {
        const int jc = jb + 16 * u < j1 ? jb + 16 * u : j1 - 1;
        if constexpr (decltype(gathered)::value)
          row[u] = ids[news0 + jc];
        else
          row[u] = (int32_t)(news0 + jc);
      }
#pragma unroll
      for (int u = 0; u < DL_ROWS; ++u) mv[u] = mask[(int64_t)row[u] * S + lc];
#pragma unroll
      for (int u = 0; u < DL_ROWS; ++u) {
        const int j = jb + 16 * u;
        const unsigned long long b = __ballot(lane < S && mv[u] != 0.f);
        if (j >= j1) continue;  // (uniform)
        if (j < j0) {
          before += __popcll(b);
          kept += b != 0ull ? 1 : 0;
        } else if (lane == 0) {
          s_bits[j - j0] = b;
          s_row[j - j0] = row[u];
        }
        if (last && lane == 0) alive_all[news0 + j] = b != 0ull ? 1 : 0;
      }
    }
  };
  if (ids)
    sweep(std::true_type{});
  else
    sweep(std::false_type{});
  if (lane == 0) {
    s_part[0][wave] = before;
    s_part[1][wave] = kept;
  }
  __syncthreads();
  if (wave == 0) {  // the slice's own news: lane = news, an inclusive scan of the counts behind the tokens before the slice
    const unsigned long long bits = s_bits[lane];
    const int cnt = __popcll(bits);
    int x = cnt;
    for (int off = 1; off < 64; off <<= 1) {
      const int up = __shfl_up(x, off);
      if (lane >= off) x += up;
    }
    int base = 0, kbase = 0;
    for (int w = 0; w < 16; ++w) {
      base += s_part[0][w];
      kbase += s_part[1][w];
    }
    s_ex[lane] = base + x - cnt;
    const int kown = __popcll(__ballot(bits != 0ull));
    if (last && lane == 63) {
      int64_t* counts = counts_all + 3 * pass;
      counts[0] = base + x;
      counts[1] = (int64_t)(kbase + kown) * S;
    }
  }
  __syncthreads();
  int32_t* live_loc = live_loc_all + pass * chunk * S;
  int32_t* live_src = live_src_all ? live_src_all + pass * chunk * S : nullptr;
  const int n_el = (j1 - j0) * S;
  for (int i = tid; i < n_el; i += 1024) {  // the flattened sweep: a live token's place = its news' + the live tokens below it
    const int jj = i / S, sl = i - jj * S;
    const unsigned long long b = s_bits[jj];
    if (!((b >> sl) & 1ull)) continue;
    const int at = s_ex[jj] + __popcll(b & ((1ull << sl) - 1ull));
    live_loc[at] = (int32_t)((j0 + jj) * S + sl);
    if (live_src) live_src[at] = (int32_t)((int64_t)s_row[jj] * S + sl);
  }
  if (!last) return;  // (uniform)
  if (tid == 0) s_carry = 0;
  __syncthreads();  // (the alive flags of the whole pass were written by this workgroup: visible to it behind the barrier)
  list_live_tiles(alive_all + news0, cn, S, BM, tiles_all + pass * cap, n_tiles + pass, s_wsum, &s_carry);
}

// the lists of the dense passes' live rows AND live row tiles in one launch (S <= 64; kernels.h)
hipError_t launch_dense_row_lists(const float* mask, const int32_t* ids, int64_t n_seq, int64_t chunk, int L, int BM,
                                  int32_t* live_loc, int32_t* live_src, int64_t* counts, uint8_t* alive, int64_t* n_tiles,
                                  int32_t* tiles, hipStream_t stream) {
  if (n_seq <= 0 || chunk <= 0 || L <= 0 || BM <= 0) return hipSuccess;
  const int64_t passes = (n_seq + chunk - 1) / chunk;
  const int64_t cap = live_tiles_cap(chunk, L, BM);
  if (L > 64 || passes > 0x7fffffffLL || cap > 0x7fffffffLL || chunk * L > 0x7fffffffLL || n_seq > 0x7fffffffLL) return hipErrorInvalidValue;
  // one workgroup per slice of DL_SLICE news of a pass; the grid is sized from the shapes alone (hipGraph)
  const int64_t per_pass = chunk < n_seq ? chunk : n_seq;
  const int64_t nsl = (per_pass + DL_SLICE - 1) / DL_SLICE;
  if (passes * nsl > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dense_row_lists_kernel, dim3((unsigned)(passes * nsl)), dim3(1024), 0, stream, mask, ids, n_seq, chunk, L,
                     (int)nsl, live_loc, ids ? live_src : nullptr, counts, alive, n_tiles, tiles, cap, BM);
  return hipGetLastError();
}

}  // namespace xnrs

// ---------------------------------------------------------------- C entry points (include/xnrs_hip.h)
using namespace xnrs;

extern "C" {

size_t xnrs_row_lists_workspace_bytes(int64_t n_seq) { return n_seq > 0 ? align_up((size_t)n_seq * sizeof(int32_t)) : 0; }

int32_t xnrs_build_row_lists(const float* m, const int32_t* ids, int64_t n_seq, int32_t L, int32_t* live_rows,
                             int32_t* live_src_rows, int32_t* kv_rows, int32_t* kv_src_rows, int64_t* counts, void* ws,
                             size_t ws_bytes, void* stream) {
  if (n_seq < 0 || L <= 0 || !m || !live_rows || !kv_rows || !counts) return XNRS_EINVAL;
  if (ids && (!live_src_rows || !kv_src_rows)) return XNRS_EINVAL;  // a gathered table needs the tokens' table rows
  if (n_seq * (int64_t)L > 0x7fffffffLL) return XNRS_EUNSUPPORTED;   // int32 row indices
  if (n_seq == 0) return hip_rc(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), (hipStream_t)stream));
  if (!ws || ws_bytes < xnrs_row_lists_workspace_bytes(n_seq)) return XNRS_EWORKSPACE;
  return hip_rc(launch_build_row_lists(m, ids, n_seq, L, live_rows, ids ? live_src_rows : nullptr, kv_rows,
                                       ids ? kv_src_rows : nullptr, counts, static_cast<int32_t*>(ws), (hipStream_t)stream));
}

int32_t xnrs_assemble_train_batch(const int64_t* sess, int64_t B, const int64_t* hist_off, const int32_t* hist_val,
                                  const int64_t* pos_off, const int32_t* pos_val, const int64_t* neg_off,
                                  const int32_t* neg_val, int32_t l_hist, int32_t n_neg, int32_t pad_row, uint64_t seed,
                                  int32_t* hist_rows, int32_t* cand_rows, void* stream) {
  if (B == 0) return XNRS_OK;
  if (!sess || !hist_off || !pos_off || !neg_off || !hist_rows || !cand_rows || B < 0 || l_hist <= 0 || n_neg < 0)
    return XNRS_EINVAL;
  BatchArgs a{};
  a.sess = sess; a.hist_off = hist_off; a.hist_val = hist_val; a.pos_off = pos_off; a.pos_val = pos_val;
  a.neg_off = neg_off; a.neg_val = neg_val; a.B = B; a.l_hist = l_hist; a.n_neg = n_neg; a.pad_row = pad_row;
  a.seed = seed; a.hist_out = hist_rows; a.cand_out = cand_rows;
  return hip_rc(launch_assemble_train(a, (hipStream_t)stream));
}

int32_t xnrs_assemble_eval_batch(const int64_t* sess, int64_t B, const int64_t* hist_off, const int32_t* hist_val,
                                 const int64_t* pos_off, const int32_t* pos_val, const int64_t* neg_off,
                                 const int32_t* neg_val, int32_t l_hist, int32_t pad_row, const int64_t* cand_off,
                                 int32_t* hist_rows, int32_t* cand_rows, int32_t* cand_sess, float* targets, void* stream) {
  if (B == 0) return XNRS_OK;
  if (!sess || !hist_off || !pos_off || !neg_off || !cand_off || !hist_rows || !cand_rows || !cand_sess || !targets ||
      B < 0 || l_hist <= 0)
    return XNRS_EINVAL;
  BatchArgs a{};
  a.sess = sess; a.hist_off = hist_off; a.hist_val = hist_val; a.pos_off = pos_off; a.pos_val = pos_val;
  a.neg_off = neg_off; a.neg_val = neg_val; a.B = B; a.l_hist = l_hist; a.pad_row = pad_row;
  a.hist_out = hist_rows; a.cand_out = cand_rows; a.cand_off_out = cand_off; a.cand_sess_out = cand_sess;
  a.targets_out = targets;
  return hip_rc(launch_assemble_eval(a, (hipStream_t)stream));
}

int32_t xnrs_gather_rows(const float* table, const int32_t* ids, float* out, int64_t n, int64_t row_floats, void* stream) {
  if (n == 0) return XNRS_OK;
  if (!table || !ids || !out || n < 0 || row_floats <= 0) return XNRS_EINVAL;
  return hip_rc(launch_gather_rows(table, ids, out, n, row_floats, (hipStream_t)stream));
}

int32_t xnrs_dropout_rows(const float* x, const int32_t* ids, float* out, int64_t n, int64_t row_floats, float p, uint64_t seed,
                          const uint64_t* seed_dev, void* stream) {
  if (!(p >= 0.f && p <= 1.f)) return XNRS_EINVAL;  // (NaN fails both comparisons)
  if (n == 0) return XNRS_OK;
  if (!x || !out || n < 0 || row_floats <= 0 || row_floats >= (1LL << 32)) return XNRS_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const size_t bytes = (size_t)n * (size_t)row_floats * F32;
  if (p >= 1.f) return hip_rc(hipMemsetAsync(out, 0, bytes, st));
  if (p <= 0.f) {  // no draw: the plain gather, or a copy (nothing at all in place)
    if (ids) return hip_rc(launch_gather_rows(x, ids, out, n, row_floats, st));
    return out == x ? XNRS_OK : hip_rc(hipMemcpyAsync(out, x, bytes, hipMemcpyDeviceToDevice, st));
  }
  return hip_rc(launch_dropout_rows(x, ids, out, n, row_floats, p, seed, seed_dev, st));
}

int32_t xnrs_gather_rows_bf16(const uint16_t* table, const int32_t* ids, float* out, int64_t n, int64_t row_elems, void* stream) {
  if (n == 0) return XNRS_OK;
  if (!table || !ids || !out || n < 0 || row_elems <= 0) return XNRS_EINVAL;
  return hip_rc(launch_gather_rows_bf16(table, ids, 1, out, n, row_elems, (hipStream_t)stream));
}

int32_t xnrs_dropout_rows_bf16(const uint16_t* table, const int32_t* ids, float* out, int64_t n, int64_t row_elems, float p,
                               uint64_t seed, const uint64_t* seed_dev, void* stream) {
  if (!(p >= 0.f && p <= 1.f)) return XNRS_EINVAL;  // (NaN fails both comparisons)
  if (n == 0) return XNRS_OK;
  if (!table || !ids || !out || n < 0 || row_elems <= 0 || row_elems >= (1LL << 32)) return XNRS_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (p >= 1.f) return hip_rc(hipMemsetAsync(out, 0, (size_t)n * (size_t)row_elems * F32, st));
  if (p <= 0.f) return hip_rc(launch_gather_rows_bf16(table, ids, 1, out, n, row_elems, st));  // no draw: the widening gather
  return hip_rc(launch_dropout_rows_bf16(table, ids, out, n, row_elems, p, seed, seed_dev, st));
}

int32_t xnrs_score_csr(const float* vecs, const int32_t* cand_rows, const int32_t* cand_sess, const float* u, float* r,
                       int64_t n_cand, int32_t E, int32_t relu, void* stream) {
  if (n_cand == 0) return XNRS_OK;
  if (!vecs || !cand_rows || !cand_sess || !u || !r || n_cand < 0 || E <= 0) return XNRS_EINVAL;
  return hip_rc(launch_score_csr(vecs, cand_rows, cand_sess, u, r, n_cand, E, relu, (hipStream_t)stream));
}

int32_t xnrs_rank_metrics(const float* scores, const float* targets, const int64_t* cand_off, float* out, int64_t B,
                          void* stream) {
  if (B == 0) return XNRS_OK;
  if (!scores || !targets || !cand_off || !out || B < 0) return XNRS_EINVAL;
  return hip_rc(launch_rank_metrics(scores, targets, cand_off, out, B, (hipStream_t)stream));
}

}  // extern "C"
