// Row lists from a token mask, built on the device: which token rows and which row tiles every later launch of an encoder
// call computes.  Integer work at the head of every call, forward and training; latency-bound, no MFMA.  A token is LIVE
// when its mask value is != 0; a sequence (a news) is KEPT / ALIVE / non-empty when it has a live token.  Every list is in
// ascending row order (sequence by sequence, token by token: what torch.nonzero of the mask gives), and every route builds
// its lists in ONE launch per call (two for the training lists), sized from the shapes alone, so a call can be captured.
//
//   list (launcher)            kernel(s)                 read by
//   -------------------------  ------------------------  ---------------------------------------------------------------
//   launch_compact_rows        compact_rows64_kernel     the device-compacted encoder (encoder_fwd.hip:
//                              (S <= 64), else           xnrs_text_encoder_fwd_compact): per pass of `chunk` news the CSR
//                              compact_rows_kernel       offsets row_off of the live rows per news, live_src (live token
//                                                        rows) and kv_src (all token rows of the kept news) in the SOURCE
//                                                        row space (ids[news] * S + s with a table, else news * S + s),
//                                                        kv_block[news] = its block of S rows in the pass's K|V image.
//                                                        counts[3p + 0] = live rows, [3p + 1] = kept K|V rows, [3p + 2] =
//                                                        1 if a mask value other than 0 / 1 was seen.  The mask must be
//                                                        binary here: the pooler multiplies by it.  A caller that breaks
//                                                        that gets NaN results and the status bit (launch_poison), not an
//                                                        error code -- there is no host read to raise from.
//   launch_dense_row_lists     dense_row_lists_kernel    the dense encoder passes with their live-row route on, S <= 64
//                                                        (encoder_fwd.hip: run_passes): per pass live_loc in the PASS's
//                                                        own row space (news j of the pass, token s: j * S + s), live_src
//                                                        in the gathered table's (with ids only), counts[3p + 0] = live
//                                                        rows, [3p + 1] = S x kept news ([3p + 2] is not written), and
//                                                        the tile list below.  Any mask value is legal (live iff != 0).
//   launch_live_tiles          live_tiles_kernel         the dense passes that skip dead row tiles only (run_passes, any
//                                                        S): per pass the ascending BM-row tiles of its [cn * L]-row
//                                                        image that hold a row of an alive sequence, and their number
//                                                        n_tiles[p]; alive[n_seq] bytes of scratch.  Any mask value.
//   launch_build_row_lists     row_counts_kernel +       the training forward and backward (xnrs_build_row_lists, called
//                              row_lists_kernel          by xnrs_amd/autograd.py): live and kv over the WHOLE batch in
//                                                        its own row space [n_seq * L], live_src / kv_src in the table's
//                                                        (with ids only), counts[0] = live rows, counts[1] = kv rows.
//                                                        Any mask value (as the host bookkeeping it replaced had it).
//   launch_poison              poison_kernel             the end of the device-compacted call: NaN over its outputs and
//                                                        XNRS_STATUS_NONBINARY_MASK into the caller's status word when a
//                                                        pass raised counts[3p + 2].  Its only input is that flag, which
//                                                        is why it lives here.
//
// The counts are device scalars the GEMMs read (GemmArgs::m_dev / k_dev / live_tiles): no list is ever read on the host by
// the routes above.  The wave and workgroup steps the kernels share (scans, the ballot walk of a mask row, the flattened
// placement from bit words) are in scan.h.
#include <type_traits>

#include "host.h"
#include "scan.h"

namespace xnrs {

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
  const PassLists out(blockIdx.x, chunk, S, row_off_all, live_all, kvs_all, kvb_all, counts_all);
  int bad = 0;
  if (tid < 2) s_carry[tid] = 0;
  if (tid == 0) out.row_off[0] = 0;
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
    wg_excl_scan2(cnt, cnt > 0 ? S : 0, s_ex, s_wsum, s_carry, [&](int ex0, int) {
      if (base + tid < cn) out.row_off[base + tid + 1] = ex0 + cnt;
    });
    // the lists, a wave per news again
    for (int jj = wave; jj < 1024; jj += 16) {
      const int j = base + jj;
      if (j >= cn) break;
      const int64_t mrow = ids ? (int64_t)ids[news0 + j] : news0 + j;
      const int64_t src0 = mrow * S;  // source token row of (news, 0)
      const bool kept = s_cnt[jj] > 0;
      const int e0 = s_ex[0][jj], e1 = s_ex[1][jj];
      ballot_walk_row(
          mask + mrow * S, S, e0, kept, lane, [&](unsigned at, int sl) { out.live_src[at] = (int32_t)(src0 + sl); },
          [&](int sl) { out.kv_src[e1 + sl] = (int32_t)(src0 + sl); });
      if (lane == 0) out.kv_block[j] = e1 / S;  // (an empty news: the block the next non-empty one gets -- never read)
    }
    __syncthreads();
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) {
    out.counts[0] = s_carry[0];
    out.counts[1] = s_carry[1];
    out.counts[2] = bad ? 1 : 0;
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
  const int tid = threadIdx.x;
  const int64_t news0 = (int64_t)blockIdx.x * chunk;
  const int cn = (int)(n_news - news0 < chunk ? n_news - news0 : chunk);
  const PassLists out(blockIdx.x, chunk, S, row_off_all, live_all, kvs_all, kvb_all, counts_all);
  int bad = 0;
  if (tid < 2) s_carry[tid] = 0;
  if (tid == 0) out.row_off[0] = 0;
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
    const int cnt = __popcll(s_bits[tid]);
    wg_excl_scan2(cnt, cnt > 0 ? S : 0, s_ex, s_wsum, s_carry, [&](int ex0, int ex1) {
      if (tid < nn) {
        out.row_off[base + tid + 1] = ex0 + cnt;
        out.kv_block[base + tid] = ex1 / S;  // (an empty news: the block the next non-empty one gets -- never read)
      }
    });
#pragma unroll 4
    for (int i = tid; i < n_el; i += 1024)
      place_flat(
          s_bits, s_ex[0], i, S, [&](int jj, int sl) { out.kv_src[s_ex[1][jj] + sl] = (int32_t)(s_row[jj] * S + sl); },
          [&](int jj, int sl, unsigned at) { out.live_src[at] = (int32_t)(s_row[jj] * S + sl); });
    __syncthreads();
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) {
    out.counts[0] = s_carry[0];
    out.counts[1] = s_carry[1];
    out.counts[2] = bad ? 1 : 0;
  }
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
    const int v0 = c, v1 = c > 0 ? L : 0;
    s_ex[0][lane] = wave_incl_scan(v0, lane) - v0;
    s_ex[1][lane] = wave_incl_scan(v1, lane) - v1;
  }
  __syncthreads();
  for (int j = wave; j < RL_SEQ; j += 16) {
    const int64_t seq = first + j;
    if (seq >= n_seq) break;
    const int64_t mrow = ids ? (int64_t)ids[seq] : seq;
    const int e1 = s_base[1] + s_ex[1][j];
    ballot_walk_row(
        mask + mrow * L, L, s_base[0] + s_ex[0][j], cnt[seq] > 0, lane,
        [&](unsigned at, int sl) {
          live[at] = (int32_t)(seq * L + sl);
          if (live_src) live_src[at] = (int32_t)(mrow * L + sl);
        },
        [&](int sl) {
          kv[e1 + sl] = (int32_t)(seq * L + sl);
          if (kv_src) kv_src[e1 + sl] = (int32_t)(mrow * L + sl);
        });
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

// ---- live row tiles of the DENSE encoder passes (GemmArgs::live_tiles).
// The rows stay where they are; what is listed is, for every pass of `chunk` sequences, the BM-row tiles of its
// [cn * L]-row image in which at least one row belongs to a sequence with any mask value != 0 (mask [.., L] fp32,
// optionally gathered by id), in ascending order, and their number.  A sequence whose mask is all zero has a result that
// needs none of its rows (encoder_fwd.hip), so a tile that holds only such rows is not computed.  ONE launch for the whole
// call, one 1024-thread workgroup per pass, like the row compaction above:
//   alive [n_seq] bytes     scratch: 1 = the sequence has an unmasked token (a thread per sequence walks its mask row)
//   n_tiles [pass]          number of live tiles of the pass (device scalar the GEMMs read)
//   tiles [pass * cap ..]   their indices; cap = tiles of a full pass

// the tile scan of a pass (one 1024-thread workgroup; *s_carry == 0 and the alive flags visible on entry, s_wsum: 16 ints):
// tiles[0 .. *n_out) = the BM-row tiles of the [cn * L]-row image that hold a row of an alive sequence, ascending
__device__ void list_live_tiles(const uint8_t* __restrict__ alive, int64_t cn, int L, int BM, int32_t* __restrict__ tiles,
                                int64_t* __restrict__ n_out, int* s_wsum, int* s_carry) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t rows = cn * L;
  const int64_t nt = (rows + BM - 1) / BM;
  const uint64_t below = lanes_below(lane);
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
    const int x = wave_incl_scan(cnt, lane);
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
  // the flattened sweep: a live token's place = its news' + the live tokens below it.  The empty `each` is deliberate: rows
  // stay where they are here, so there is no list of ALL tokens of a kept news to write (compact_rows64_kernel's kv_src)
  for (int i = tid; i < n_el; i += 1024)
    place_flat(
        s_bits, s_ex, i, S, [](int, int) {},
        [&](int jj, int sl, unsigned at) {
          live_loc[at] = (int32_t)((j0 + jj) * S + sl);
          if (live_src) live_src[at] = (int32_t)((int64_t)s_row[jj] * S + sl);
        });
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

}  // extern "C"
