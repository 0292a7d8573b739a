// fp32 GEMM on the CDNA4 matrix cores.
//
//   forward   C = act(A . W^T + bias)            A row-major [M,K], W = nn.Linear weight [N,K]     (ROW, WT)
//   backward  dX = (dY . W) (*) f'(aux) [+ C]    A = dY [M,N'] row-major, B = W as [K'=N'][N=K_in] (ROW, KN)
//             dW = dY^T . X                      A = dY read k-major (A^T[k=m][i]), B = X [k=m][n]  (COL, KN)
//
// Replaces nn.Linear (and its autograd) as used by the reference hot path
// (xnrs/models/components/layers.py:60,128-130,154; news_encoding.py:27-31).  Numerics:
// v_mfma_f32_32x32x2_f32 is an exact fp32 fmaf chain (no TF32/xf32 on gfx950), so results differ from
// torch-CPU only by summation order.
//
// Design (gfx950, 64-wide waves); measurements and the dropped alternatives: DESIGN.md section 4.1
//   * workgroup = 256 threads = 4 waves in a 2x2 grid; wave tile (32*TM)x(32*TN), i.e. the block tile is
//     (64*TM)x(64*TN): 128x128 by default, 128x64 / 64x128 / 64x64 picked by a padded-work estimate.
//   * k-contiguous operands (ROW / WT): a lane fetches 4 consecutive k with ONE ds_read_b128 and feeds 4 MFMA
//     steps from it: step j of an 8-wide k group uses k = 4*(lane>>5) + j for A and B alike (any bijection of k is
//     legal as long as A and B agree).
//   * shipped forward configuration (template PIPE 5, BK 16, BUF, MINW 4): K tiles of 16, 64-byte LDS rows with
//     the 16-byte chunk XOR-swizzled by (row>>2)&3 (conflict-free ds_read_b128 and ds_write_b128), two LDS buffers
//     (32 KB), ONE register set, an explicitly interleaved instruction stream (one LDS store, one tile load and the
//     next fragment reads behind each slot of TM*TN MFMAs, pinned by sched_barrier), raw buffer loads whose
//     bounds check zero-fills ragged rows / k tails, registers capped at 128 -> 4 workgroups per CU.
//     PIPE 1 (plain double buffering, BK 32, rows padded to 36 floats) serves the scalar-load fallback.
//   * k-major operands (COL / KN, the backward's dW and small-M dX): LDS image [k][i] (rows padded by 4),
//     fragments are 4 ds_read_b32 with the 32 lanes of a half-wave on 32 consecutive floats; PIPE 5, BK 32,
//     2 workgroups per CU.
//   * optional row gather on the rows of a ROW-layout A / KN-layout B (device-resident news-token table + ids:
//     SURVEY.md section 8 a0) folded into the per-thread row offsets, so gathered rows are still read as full lines.
//   * XCD-aware block order: each XCD walks a contiguous range of the tile sequence; column GROUPS of tiles
//     outermost so the weight panels an XCD touches stay in its 4 MB L2.
//   * split-K (dW: the contraction is the token-row count, the output is a small weight matrix): each k-slice
//     writes its own fp32 slab; a second kernel sums the slabs in a fixed order (bitwise reproducible, no float
//     atomics).
#include <atomic>
#include <cstdlib>
#include <type_traits>

#include "kernels.h"

namespace xnrs {

constexpr int KALIGN = 32;  // split-K slices are aligned to the largest K tile

// Out-of-range lanes of a tile load read this zero line instead of being zeroed AFTER the load: the
// select is on the ADDRESS, so no instruction depends on the loaded data until the LDS store and the
// loads of two tiles can stay in flight (a select on the data makes hipcc wait right behind the load).
__device__ __attribute__((aligned(16))) float g_zero_line[4] = {0.f, 0.f, 0.f, 0.f};

// PIPE selects the software pipeline:
//   1: plain double buffering -- loads of tile t+1 fly during the MFMAs of tile t, LDS store + barrier at the
//      end of the tile (used for the scalar-load fallback; 117 TF on the Q/K/V projection)
//   5: the same two LDS buffers and ONE register set, but an explicitly interleaved instruction stream
//      (default; 130-136 TF).  Measured alternatives that were dropped: two register sets / LDS store
//      mid-stream without interleave 121 TF; three LDS buffers with cross-barrier fragment prefetch at one
//      workgroup per CU 112 TF, at two per CU 130 TF; 128x256 / 256x128 block tiles (2 waves/SIMD) 131 TF
//      against 133 TF for the default on the same device.
// BUF: tile loads are raw buffer loads (ROW/WT layouts, no gather, operands <= 1 GB): the row offset is a
// loop-invariant 32-bit VGPR, the k offset rides in the scalar offset, and out-of-range rows / k chunks
// are handled by the hardware bounds check (offset bit 30 set -> beyond num_records -> returns 0).  The
// loop then carries ~10 VALU instructions per K tile instead of ~50 (64-bit adds + address selects).
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr unsigned BUF_OOB = 0x40000000u;

// GATH (with BUF): the rows of A are gathered (or A is too large for a buffer descriptor): A is read through per-thread
// 64-bit row pointers, UNCONDITIONALLY -- rows past M are clamped to row M-1 (their results are never stored) and the k
// tail is clamped to K-4 (it meets the zeros the bounds check returns for B) -- while B keeps the raw buffer loads (one
// VGPR offset per weight row here: the scalar-offset form of the dense kernel measured 1.5 % slower in this variant).
// Measured inside the B = 512 step (tools/bench_idpath.py, same ids, interleaved): Q/K/V projection 37.6 ms gathered vs
// 35.5 ms dense = 6 % on that GEMM, 3.7 % on the step (the first gather variant -- a select between row pointer and zero
// line per load, 139 VGPRs, 45 spills, 3 workgroups per CU -- cost 7.1 % / 4.4 %).  What the rest is and is not:
//   * not the random rows: the same kernel over a table that IS the materialised batch, ids = 0..n-1, takes the same
//     time (bench_idpath.py "seq_ids") -- the cost is the per-lane 64-bit address form of the load;
//   * a descriptor cannot replace it: the rows of one tile belong to up to four news anywhere in a 10-GB table; a raw
//     buffer / saddr offset reaches 4 GB from one wave-uniform base, and a STRUCTURED buffer load (idxen: base + row
//     index * 3072 + offset) wraps at the same 4 GB -- rows >= 2^32 / stride read as zeros (tools/probes/struct_buffer.hip);
//   * advancing the row pointers in place (no clamp, no 64-bit temporaries, 4 instead of 12 extra VALU per K tile)
//     measured SLOWER (6.3 % on the step): the add writes the address registers of the load issued just before it.
// KG (k-major operands): how the k rows are gathered -- 0: not at all; 1: both operands through one-row-per-id lists
// (the live-row backward); 2: anything else, decided at run time.  A template parameter because the run-time tests
// (`if (gather_ids) { if (S == 1) ...`) sat in front of each of the 8 tile loads of an iteration: 29 basic blocks, the
// interleaved MFMA / load schedule gone, 3.4 VALU instructions per MFMA and 65 % matrix-pipe occupancy in the dW GEMMs
// (profiles/r02_train_step_pmc.txt).
// MDEV (forward layout): the row count is a device scalar (GemmArgs::m_dev), read once into SGPRs -- its own
// instantiations (a first version wrote it into the by-value argument block: that moved the whole 400-byte struct to
// scratch in EVERY variant -- 59 spilled VGPRs in the main forward kernel, 140 -> 84 TFLOP/s).
// LIVE (forward layout): the launch computes the row tiles of a device-built list only (GemmArgs::live_n / live_tiles: the
// tiles of a dense encoder pass that hold a row of a sequence with an unmasked token) -- the same mechanism: the number of
// listed tiles is read once into an SGPR, the tile walk runs over them, the workgroups past them leave at once, and the row
// tile of a workgroup is looked up in the list (one scalar load).  Its own instantiations; the K loop is the dense one.
// The kernel's body lives in gemm_f32_body.h, as text: it is compiled twice, into the kernel itself and into a __device__
// function of (workgroup index, workgroup count, LDS tile arrays) that the one-launch Q + K|V entry below calls for each of
// its two sections (the reason for text instead of a wrapper: the note in that file).
template <int TM, int TN, bool A_COL, bool B_KN, bool VEC, int PIPE, int BK, bool BUF = false, int MINW = 2, bool GATH = false,
          int KG = 2, bool RDOT = false, bool MDEV = false, bool LIVE = false>
__global__ __launch_bounds__(256, MINW) void gemm_f32_kernel(const GemmArgs a, int m_tiles, int n_tiles_seg, int gn) {
#define XNRS_GEMM_BID blockIdx.x
#define XNRS_GEMM_NWG gridDim.x
#define XNRS_GEMM_LDS_TILES(A, B)                            \
  __shared__ __attribute__((aligned(16))) float A[NBUF][A_SZ]; \
  __shared__ __attribute__((aligned(16))) float B[NBUF][B_SZ];
#include "gemm_f32_body.h"  // LAST statement of the function: the text returns early (workgroups without work, the RDOT and
                            // row-scatter epilogues) -- code placed after it would be skipped for those workgroups
#undef XNRS_GEMM_BID
#undef XNRS_GEMM_NWG
#undef XNRS_GEMM_LDS_TILES
}

// floats of the two LDS buffers of one forward-layout operand tile of 64 T rows (gemm_f32_body.h: NBUF * A_SZ / B_SZ)
template <int T, int BK>
constexpr int gemm_f32_lds_floats() {
  return 2 * 64 * T * (BK == 16 ? BK : BK + 4);
}

template <int TM, int TN, bool A_COL, bool B_KN, bool VEC, int PIPE, int BK, bool BUF = false, int MINW = 2, bool GATH = false,
          int KG = 2, bool RDOT = false, bool MDEV = false, bool LIVE = false>
__device__ __forceinline__ void gemm_f32_body(const GemmArgs& a, int m_tiles, const int n_tiles_seg, const int gn, const int bid_in,
                                              const int nwg_in, float* As0, float* Bs0) {
  static_assert(!A_COL && !B_KN, "forward layout (the LDS tile sizes of gemm_f32_lds_floats)");
#define XNRS_GEMM_BID bid_in
#define XNRS_GEMM_NWG nwg_in
#define XNRS_GEMM_LDS_TILES(A, B)                                                                                   \
  static_assert(NBUF * A_SZ == gemm_f32_lds_floats<TM, BK>() && NBUF * B_SZ == gemm_f32_lds_floats<TN, BK>(), "LDS"); \
  float(*const A)[A_SZ] = reinterpret_cast<float(*)[A_SZ]>(As0);                                                    \
  float(*const B)[B_SZ] = reinterpret_cast<float(*)[B_SZ]>(Bs0);
#include "gemm_f32_body.h"  // LAST statement of the function: the text returns early (workgroups without work, the RDOT and
                            // row-scatter epilogues) -- code placed after it would be skipped for those workgroups
#undef XNRS_GEMM_BID
#undef XNRS_GEMM_NWG
#undef XNRS_GEMM_LDS_TILES
}

// Q and K|V of a dense live-row pass in ONE grid (kernels.h: qkv_one_launch_map; DESIGN.md section 4.1 "One launch").  Two
// launches leave two partly filled last rounds of co-resident workgroups and a launch boundary; here the Q tiles fill the
// tail of the K|V tiles.  Each section runs the body of the instantiation that its own launch would run -- K|V: LIVE with
// buffer loads for A (dense rows), Q: GATH + MDEV with the row-scattered epilogue on the 128 x 64 tile -- with its index
// inside the section as the workgroup index, so every output element comes from the same instruction sequence and both
// XCD-aware walks see the hardware's XCD (the Q section starts at a multiple of 8).  ONE pair of LDS arrays serves both
// bodies (each body's own __shared__ arrays would add up: 56 KB, two workgroups per CU instead of four).
// What is NOT built, by the compiler's verdict (profiles/qkv_one_launch_resource_usage.md): a K|V section with gathered
// rows (table + ids) -- next to the Q body the GATH + LIVE body no longer fits 128 VGPRs cleanly, a loop invariant is
// reloaded from scratch at the head of every K tile, in front of the tile loads' vmcnt queue (the pattern of the MDEV note
// above) -- and Q on the 128 x 128 tile (5 spilled VGPRs; measured 0.02-0.03 ms per step slower than 128 x 64).  Calls with
// ids keep the two launches.
// The entry reads both device counts to place the workgroup and the body it calls reads its own count again (two scalar
// loads of a cached line): the bodies stay the text the stand-alone kernels run.
__global__ __launch_bounds__(256, 4) void gemm_qkv_one_launch_kernel(const GemmArgs kv, const GemmArgs q, int kv_m_tiles,
                                                                     int kv_n_tiles_seg, int kv_gn, int q_m_tiles, int q_n_tiles,
                                                                     int q_gn) {
  // both sections have 128-row A tiles; the B tile of the Q section (64 weight rows) fits that of K|V (128)
  __shared__ __attribute__((aligned(16))) float As[gemm_f32_lds_floats<2, 16>()];
  __shared__ __attribute__((aligned(16))) float Bs[gemm_f32_lds_floats<2, 16>()];
  static_assert(sizeof(As) + sizeof(Bs) <= 32768, "four workgroups per CU");
  // the two device counts, as the bodies read them (wave-uniform)
  const int64_t ln = __builtin_amdgcn_readfirstlane((int)load_dev_scalar(kv.live_n));
  const int64_t md0 = load_dev_scalar(q.m_dev);
  const int64_t md = ((int64_t)__builtin_amdgcn_readfirstlane((int)(md0 >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)md0);
  const QkvOneLaunchWork w = qkv_one_launch_map((int64_t)blockIdx.x, ln, md, kv_m_tiles, kv_n_tiles_seg * kv.nseg, q.M, 128, q_n_tiles);
  if (w.section < 0) return;  // workgroup-uniform, before any barrier
  // (nothing may follow the calls: a body returns early for its own reasons, see gemm_f32_body)
  if (w.section == 0)
    gemm_f32_body<2, 2, false, false, true, 5, 16, true, 4, false, 2, false, false, true>(kv, kv_m_tiles, kv_n_tiles_seg, kv_gn, w.index, 0,
                                                                                        As, Bs);
  else
    gemm_f32_body<2, 1, false, false, true, 5, 16, true, 4, true, 2, false, true, false>(q, q_m_tiles, q_n_tiles, q_gn, w.index, 0, As, Bs);
}

// ... and fc1 of the PREVIOUS pass behind them (kernels.h: qkv_fc1_launch_map; DESIGN.md section 4.1 "fc1 in the tail").  The
// pooler's fc1 over a pass's live rows is 7 % of the projection's work on the smallest tile of the family: as a launch of its
// own it is mostly ramp-up and tail (4.5 tiles per CU), and the projection launch above still ends in a partly filled round.
// Here it is a third section of the next pass's projection grid: the body of the instantiation its own launch runs (GATH +
// RDOT + MDEV, row-scattered row dots) on the same LDS arrays, its index inside the section as the workgroup index, the
// section starting at a multiple of 8 -- every score comes from the same instruction sequence.  It reads the attention
// output of the previous pass and writes that pass's scores; the two projection sections touch neither.
// FTM x FTN: the third section's tile in units of 64 (every shape gives the same bits: the 32-column blocks of the row dots
// do not depend on it); which shapes compile clean next to the two other bodies: profiles/fc1_in_tail_resource_usage.md.
template <int FTM, int FTN>
__global__ __launch_bounds__(256, 4) void gemm_qkv_fc1_launch_kernel(const GemmArgs kv, const GemmArgs q, const GemmArgs f, int kv_m_tiles,
                                                                     int kv_n_tiles_seg, int kv_gn, int q_m_tiles, int q_n_tiles, int q_gn,
                                                                     int f_m_tiles, int f_n_tiles, int f_gn) {
  __shared__ __attribute__((aligned(16))) float As[gemm_f32_lds_floats<2, 16>()];
  __shared__ __attribute__((aligned(16))) float Bs[gemm_f32_lds_floats<2, 16>()];
  static_assert(sizeof(As) + sizeof(Bs) <= 32768, "four workgroups per CU");
  static_assert(FTM >= 1 && FTM <= 2 && FTN >= 1 && FTN <= 2, "the third section's tiles fit the arrays of the first");
  // the three device counts, as the bodies read them (wave-uniform); an empty third section (f.M == 0) has none
  auto dev64 = [](const int64_t* p) {
    const int64_t v = load_dev_scalar(p);
    return ((int64_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
  };
  const int64_t ln = __builtin_amdgcn_readfirstlane((int)load_dev_scalar(kv.live_n));
  const int64_t md = dev64(q.m_dev);
  const int64_t fd = f.M > 0 ? dev64(f.m_dev) : 0;
  const QkvOneLaunchWork w = qkv_fc1_launch_map((int64_t)blockIdx.x, ln, md, fd, kv_m_tiles, kv_n_tiles_seg * kv.nseg, q.M, 128, q_n_tiles,
                                                f.M, 64 * FTM, f_n_tiles);
  if (w.section < 0) return;  // workgroup-uniform, before any barrier
  // (nothing may follow the calls: a body returns early for its own reasons, see gemm_f32_body)
  if (w.section == 0)
    gemm_f32_body<2, 2, false, false, true, 5, 16, true, 4, false, 2, false, false, true>(kv, kv_m_tiles, kv_n_tiles_seg, kv_gn, w.index, 0,
                                                                                        As, Bs);
  else if (w.section == 1)
    gemm_f32_body<2, 1, false, false, true, 5, 16, true, 4, true, 2, false, true, false>(q, q_m_tiles, q_n_tiles, q_gn, w.index, 0, As, Bs);
  else
    gemm_f32_body<FTM, FTN, false, false, true, 5, 16, true, 4, true, 2, true, true, false>(f, f_m_tiles, f_n_tiles, f_gn, w.index, 0, As, Bs);
}

// Wt[c][r] = W[r][c]: 32x32 tiles through LDS (padded rows), both sides coalesced
__global__ __launch_bounds__(256) void transpose_kernel(const float* W, float* Wt, int rows, int cols) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + ty + 8 * i, c = c0 + tx;
    if (r < rows && c < cols) tile[ty + 8 * i][tx] = W[(int64_t)r * cols + c];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, r = r0 + tx;
    if (r < rows && c < cols) Wt[(int64_t)c * rows + r] = tile[tx][ty + 8 * i];
  }
}

// zero `width` floats (multiple of 4, 16-byte aligned) of each of `rows` rows of pitch `ld` floats: the column block of
// one segment inside a [rows, 3D] image.  (hipMemset2DAsync took 311 us for 80 000 x 768 floats, this runs at HBM speed.)
__global__ __launch_bounds__(256) void zero_cols_kernel(float* p, int64_t ld, int w4, int64_t n4) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int64_t r = i / w4;
  const int c = (int)(i - r * w4);
  __builtin_nontemporal_store(f32x4{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f32x4*>(p + r * ld) + c);
}

hipError_t launch_zero_cols(float* p, int64_t ld, int width, int64_t rows, hipStream_t stream) {
  if (rows <= 0 || width <= 0) return hipSuccess;
  if (width % 4 != 0 || ld % 4 != 0 || (reinterpret_cast<uintptr_t>(p) & 15) != 0)
    return hipMemset2DAsync(p, (size_t)ld * sizeof(float), 0, (size_t)width * sizeof(float), (size_t)rows, stream);
  const int64_t n4 = rows * (width / 4);
  hipLaunchKernelGGL(zero_cols_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, p, ld, width / 4, n4);
  return hipGetLastError();
}

// The rows of a [n_seq*L, 3D] Q|K|V image that the live-row / kv-row projections (encoder_fwd.hip, xnrs_row_lists) leave unwritten,
// zeroed by the mask itself (fp32 [.., L], optionally through news ids): the Q columns of every masked token row, and the
// K|V columns of every row of an all-masked sequence.  One workgroup per sequence; writes 0.37 instead of 0.74 GB at the
// grad step's 80 000 x 2304 image (zero_cols over the whole image: 0.14 ms per encode).
__global__ __launch_bounds__(256) void zero_dead_qkv_kernel(float* qkv, const float* __restrict__ mask,
                                                            const int32_t* __restrict__ ids, int L, int D4) {
  const int64_t seq = blockIdx.x;
  const float* mp = mask + (ids ? (int64_t)ids[seq] : seq) * L;
  int any = 0;
  for (int s = threadIdx.x; s < L; s += 256) any |= mp[s] != 0.f ? 1 : 0;
  const bool empty = !__syncthreads_or(any);
  const int w4 = empty ? 3 * D4 : D4;  // all-masked sequence: Q, K and V; otherwise the Q columns of its masked rows
  f32x4* base = reinterpret_cast<f32x4*>(qkv) + seq * L * (int64_t)(3 * D4);
  for (int s = 0; s < L; ++s) {
    if (!empty && mp[s] != 0.f) continue;  // (uniform)
    f32x4* row = base + (int64_t)s * (3 * D4);
    for (int c = threadIdx.x; c < w4; c += 256) __builtin_nontemporal_store(f32x4{0.f, 0.f, 0.f, 0.f}, row + c);
  }
}

hipError_t launch_zero_dead_qkv(float* qkv, const float* mask, const int32_t* ids, int64_t n_seq, int L, int D, hipStream_t stream) {
  if (n_seq <= 0) return hipSuccess;
  if (D % 4 != 0 || (reinterpret_cast<uintptr_t>(qkv) & 15) != 0 || n_seq > 0x7fffffffLL || !mask)
    return launch_zero_cols(qkv, 3 * (int64_t)D, 3 * D, n_seq * L, stream);
  hipLaunchKernelGGL(zero_dead_qkv_kernel, dim3((unsigned)n_seq), dim3(256), 0, stream, qkv, mask, ids, L, D / 4);
  return hipGetLastError();
}

hipError_t launch_transpose(const float* W, float* Wt, int rows, int cols, hipStream_t stream) {
  if (rows <= 0 || cols <= 0) return hipSuccess;
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32)), dim3(256), 0, stream, W,
                     Wt, rows, cols);
  return hipGetLastError();
}

// C (+)= sum_s slabs[s]  (fixed order -> bitwise reproducible); elements past n: the fused bias-gradient partials
// (GemmArgs::colsum, [nsplit][cs_n]) summed the same way into cs_out -- one launch instead of a reduce and a colsum_final
// (C2 / n1 / cs_out2 / cs_n1: elements from n1 on -- whole rows -- go to C2, bias gradients from cs_n1 on to cs_out2:
// GemmArgs::C2, one product for two parameters)
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* slabs, int64_t slab_stride, int nsplit, float* C,
                                                             int64_t n, int accumulate, const float* cs_partial, float* cs_out,
                                                             int cs_n, float* C2, int64_t n1, float* cs_out2, int cs_n1) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) {
    const int64_t c = i - n;
    if (c < cs_n) {
      float v = 0.f;
      for (int s = 0; s < nsplit; ++s) v += cs_partial[(int64_t)s * cs_n + c];
      if (cs_out2 && c >= cs_n1) cs_out2[c - cs_n1] = v;
      else cs_out[c] = v;
    }
    return;
  }
  float* dst = (C2 && i >= n1) ? C2 + (i - n1) : C + i;
  float v = accumulate ? *dst : 0.f;
  for (int s = 0; s < nsplit; ++s) v += slabs[(int64_t)s * slab_stride + i];
  *dst = v;
}

// column tiles per group of the tile walk (see the kernel): as many as keep the group's weight panels within
// ~2.5 MB, evened out over the groups.  The k-major (backward) layouts keep the plain M-major walk.
int gemm_group_tiles(int n_tiles, int bn, int64_t K, bool plain) {
  int64_t gn = (int64_t)(2.5 * 1024 * 1024) / ((int64_t)bn * (K > 0 ? K : 1) * 4);
  if (knobs().gemm_group >= 0) gn = knobs().gemm_group;  // development knob: tiles per group, 0 = plain walk
  if (plain || gn <= 0 || gn >= n_tiles) return n_tiles;
  const int groups = (int)((n_tiles + gn - 1) / gn);
  return (n_tiles + groups - 1) / groups;
}

template <int TM, int TN, bool A_COL, bool B_KN>
static hipError_t launch_cfg(const GemmArgs& a, bool vec, int nsplit, hipStream_t stream) {
  constexpr int BM = 64 * TM, BN = 64 * TN;
  const int64_t m_tiles = (a.M + BM - 1) / BM;
  const int n_tiles_seg = (a.Nseg + BN - 1) / BN;
  const int64_t grid = m_tiles * n_tiles_seg * a.nseg;
  if (grid <= 0 || grid > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 g((unsigned)grid, (unsigned)nsplit);
  const int gn = gemm_group_tiles(n_tiles_seg * a.nseg, BN, a.K, A_COL || B_KN);
  // development knobs for in-process A/B runs (tools/bench_gemm.py; kernels.h: Knobs).  Default (pipe 6): PIPE 5,
  // BK 16, registers capped for 4 workgroups per CU on the main tile.
  const int pipe = knobs().gemm_pipe;
  const int bk = knobs().gemm_bk;
  const bool bufB = knobs().gemm_buf && vec && (int64_t)a.Nseg * a.ldw * 4 <= (int64_t)BUF_OOB;
  const bool buf = bufB && !a.gather_ids && a.M * a.lda * 4 <= (int64_t)BUF_OOB;
  // gathered rows / an A operand beyond the 1-GB descriptor window: pointers for A, buffer loads for B (K >= 4: the
  // k-tail clamp reads K-4 .. K-1)
  const bool gath = bufB && !buf && a.K >= 4;  // (row scatter of C is an epilogue matter: any A-load variant serves it)
#define XNRS_LAUNCH(VECV, PIPEV, BKV, BUFV, MINWV)                                                                  \
  hipLaunchKernelGGL((gemm_f32_kernel<TM, TN, A_COL, B_KN, VECV, PIPEV, BKV, BUFV, MINWV>), g, dim3(256), 0, stream, a, \
                     (int)m_tiles, n_tiles_seg, gn)
#define XNRS_LAUNCH_GATH(MINWV)                                                                                       \
  hipLaunchKernelGGL((gemm_f32_kernel<TM, TN, A_COL, B_KN, true, 5, 16, true, MINWV, true>), g, dim3(256), 0, stream, a, \
                     (int)m_tiles, n_tiles_seg, gn)
  if constexpr (TM == 2 && TN == 2 && !A_COL && !B_KN) {
    if (a.live_tiles) {  // live row tiles of a dense encoder pass: its own instantiations of the main tile
      if (!vec || !(buf || gath) || a.m_dev || !a.live_n || nsplit != 1 || a.c_scatter) return hipErrorInvalidValue;
#define XNRS_LAUNCH_LIVE(GATHV, RDOTV)                                                                                            \
  hipLaunchKernelGGL((gemm_f32_kernel<2, 2, false, false, true, 5, 16, true, 4, GATHV, 2, RDOTV, false, true>), g, dim3(256), 0, \
                     stream, a, (int)m_tiles, n_tiles_seg, gn)
      if (a.rowdot_out) {
        if (buf) XNRS_LAUNCH_LIVE(false, true);
        else XNRS_LAUNCH_LIVE(true, true);
      } else if (buf) XNRS_LAUNCH_LIVE(false, false);
      else XNRS_LAUNCH_LIVE(true, false);
#undef XNRS_LAUNCH_LIVE
      return hipGetLastError();
    }
  }
  if constexpr (!A_COL && !B_KN) {
    if (a.live_tiles && !(TM == 2 && TN == 2)) return hipErrorInvalidValue;  // (the launcher forces the main tile)
    if (a.m_dev) {  // device row count (the device-compacted padding-free encoder): its own instantiations
      if (!vec || !(buf || gath)) return hipErrorInvalidValue;
      if (a.rowdot_out) {
        if (buf)
          hipLaunchKernelGGL((gemm_f32_kernel<TM, TN, false, false, true, 5, 16, true, 4, false, 2, true, true>), g, dim3(256), 0,
                             stream, a, (int)m_tiles, n_tiles_seg, gn);
        else
          hipLaunchKernelGGL((gemm_f32_kernel<TM, TN, false, false, true, 5, 16, true, 4, true, 2, true, true>), g, dim3(256), 0,
                             stream, a, (int)m_tiles, n_tiles_seg, gn);
      } else if (buf) {
        hipLaunchKernelGGL((gemm_f32_kernel<TM, TN, false, false, true, 5, 16, true, 4, false, 2, false, true>), g, dim3(256), 0,
                           stream, a, (int)m_tiles, n_tiles_seg, gn);
      } else {
        hipLaunchKernelGGL((gemm_f32_kernel<TM, TN, false, false, true, 5, 16, true, 4, true, 2, false, true>), g, dim3(256), 0,
                           stream, a, (int)m_tiles, n_tiles_seg, gn);
      }
      return hipGetLastError();
    }
    if (a.rowdot_out) {  // fused row dots: its own instantiation, so that the plain kernel's registers stay as they are
      if (!vec || !(buf || gath)) return hipErrorInvalidValue;
      if (buf)
        hipLaunchKernelGGL((gemm_f32_kernel<TM, TN, false, false, true, 5, 16, true, 4, false, 2, true>), g, dim3(256), 0, stream,
                           a, (int)m_tiles, n_tiles_seg, gn);
      else  // gathered A rows (a news table, the compact rows of the padding-free path) or an A beyond 1 GB
        hipLaunchKernelGGL((gemm_f32_kernel<TM, TN, false, false, true, 5, 16, true, 4, true, 2, true>), g, dim3(256), 0, stream,
                           a, (int)m_tiles, n_tiles_seg, gn);
      return hipGetLastError();
    }
  }
  if (!vec) XNRS_LAUNCH(false, 1, 32, false, 2);
  else if constexpr (TM == 2 && TN == 2 && !A_COL && !B_KN) {  // forward main tile: all variants are built
    if (pipe == 1 && buf) XNRS_LAUNCH(true, 1, 32, true, 2);
    else if (pipe == 1) XNRS_LAUNCH(true, 1, 32, false, 2);
    else if (pipe == 5 && bk == 16 && buf) XNRS_LAUNCH(true, 5, 16, true, 2);
    else if (pipe == 5 && buf) XNRS_LAUNCH(true, 5, 32, true, 2);
    else if (pipe == 5) XNRS_LAUNCH(true, 5, 32, false, 2);
    else if (buf) XNRS_LAUNCH(true, 5, 16, true, 4);
    else if (gath) XNRS_LAUNCH_GATH(4);
    else XNRS_LAUNCH(true, 5, 16, false, 3);  // pointers + zero-line selects on both operands (row scatter, > 1 GB
                                               // weights): 139 VGPRs -> 3 workgroups per CU
  } else if constexpr (!A_COL && !B_KN) {
    // the smaller forward tiles use the main tile's configuration too (BK 16, registers capped for 4 WG/CU):
    // +19..25 % on the Q/K/V projection at D = 300 / 320 against BK 32 at 2 WG/CU
    if (buf) XNRS_LAUNCH(true, 5, 16, true, 4);
    else if (gath) XNRS_LAUNCH_GATH(4);
    else XNRS_LAUNCH(true, 5, 16, false, 4);
  } else if constexpr (A_COL && B_KN) {
    // backward dW = dY^T . X (both operands k-major): BK 32, 2 workgroups per CU (BK 16 / 4 per CU measured no better);
    // one instantiation per k-row gather mode
    const bool g_none = !a.gather_ids && !a.b_gather_ids;
    const bool g_live = a.gather_ids && a.b_gather_ids && a.gather_S == 1 && a.b_gather_S == 1;
#define XNRS_LAUNCH_KG(KGV)                                                                                              \
  hipLaunchKernelGGL((gemm_f32_kernel<TM, TN, A_COL, B_KN, true, 5, 32, false, 2, false, KGV>), g, dim3(256), 0, stream, a, \
                     (int)m_tiles, n_tiles_seg, gn)
    if (g_none) XNRS_LAUNCH_KG(0);
    else if (g_live) XNRS_LAUNCH_KG(1);
    else XNRS_LAUNCH_KG(2);
#undef XNRS_LAUNCH_KG
  } else {
    XNRS_LAUNCH(true, 5, 32, false, 2);  // ROW x KN (small-M dX products)
  }
#undef XNRS_LAUNCH
#undef XNRS_LAUNCH_GATH
  return hipGetLastError();
}

template <bool A_COL, bool B_KN>
static hipError_t launch_layout(const GemmArgs& a, bool vec, int nsplit, hipStream_t stream) {
  // pick the tile with the least estimated time: rounds of co-resident workgroups x padded tile work
  // (forward variants: 4 workgroups/CU x 256 CUs per round, k-major variants 2/CU); bigger tiles have slightly
  // better MFMA duty.  Measured with the forced-tile knob: 30 720 x 256 x 300 -> 87 TF at 128x128 (480 of
  // 1 024 slots filled), 98 TF at 64x64.
  const int cand[4][2] = {{2, 2}, {2, 1}, {1, 2}, {1, 1}};
  const double eff[4] = {1.0, 0.94, 0.94, 0.86};
  int best = 0;
  double best_t = 1e300;
  for (int c = 0; c < 4; ++c) {
    const int64_t bm = 64 * cand[c][0], bn = 64 * cand[c][1];
    // (m_dev launches: the rows expected to exist, GemmArgs::m_fill_hint, not the capacity the grid is sized for)
    const int64_t m_exp = (a.m_dev && a.m_fill_hint > 0.f && a.m_fill_hint < 1.f) ? (int64_t)(a.M * (double)a.m_fill_hint) + 1 : a.M;
    const int64_t wgs = ((m_exp + bm - 1) / bm) * ((a.Nseg + bn - 1) / bn) * a.nseg * nsplit;
    const double slots = (A_COL || B_KN) ? 512.0 : 1024.0;
    // fractional rounds above one: workgroups are re-dispatched one by one, so 7.3 rounds of 128x128 tiles do not cost
    // 8 (whole rounds made the k-major dX GEMMs pick 128x64 tiles: 87 TF)
    const double rounds = (double)wgs / slots > 1.0 ? (double)wgs / slots : 1.0;
    const double t = rounds * (double)(bm * bn) / eff[c];
    if (t < best_t * 0.999) {
      best_t = t;
      best = c;
    }
  }
  if (knobs().gemm_tile >= 0 && knobs().gemm_tile <= 3) best = knobs().gemm_tile;  // development knob
  if (a.live_tiles) best = 0;  // the list is in tiles of LIVE_TILE_BM = 128 rows (every tile shape gives the same bits)
  switch (best) {
    case 0: return launch_cfg<2, 2, A_COL, B_KN>(a, vec, nsplit, stream);
    case 1: return launch_cfg<2, 1, A_COL, B_KN>(a, vec, nsplit, stream);
    case 2: return launch_cfg<1, 2, A_COL, B_KN>(a, vec, nsplit, stream);
    default: return launch_cfg<1, 1, A_COL, B_KN>(a, vec, nsplit, stream);
  }
}

size_t gemm_splitk_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  const int ns0 = gemm_pick_splits(M, N, K, false), ns1 = gemm_pick_splits(M, N, K, true);
  const int ns = ns0 > ns1 ? ns0 : ns1;
  return ns > 1 ? (size_t)ns * (size_t)M * (size_t)N * sizeof(float) : 0;
}

int gemm_pick_splits(int64_t M, int64_t N, int64_t K, bool dw_kernel) {
  // aim for one round of 128x128 workgroups (2 per CU x 256 CUs for the k-major variants, 3 per CU for gemm_dw.hip; one
  // 256x256 workgroup per CU for its big tile) and at least 256 contraction steps per slice
  int64_t tiles = ((M + 127) / 128) * ((N + 127) / 128);
  int64_t slots = dw_kernel ? 768 : 512;
  if (dw_kernel && knobs().gemm_dw_tile != 128 && M >= 384 && N >= 384) {
    tiles = ((M + 255) / 256) * ((N + 255) / 256);
    slots = 256;
  }
  int64_t ns = slots / tiles;
  const int64_t max_by_k = K / 256;
  if (ns > max_by_k) ns = max_by_k;
  if (ns > 64) ns = 64;
  if (ns < 1) ns = 1;
  return (int)ns;
}

// ---- process-global state of the library: the knobs (read once) and the forward-GEMM arithmetic mode
static Knobs read_knobs() {
  Knobs k;
  auto num = [](const char* name, long long dflt) {
    const char* e = getenv(name);
    return (e && *e) ? atoll(e) : dflt;
  };
  k.gemm_pipe = (int)num("XNRS_GEMM_PIPE", 6);
  k.gemm_bk = num("XNRS_GEMM_BK", 32) == 16 ? 16 : 32;
  k.gemm_buf = num("XNRS_GEMM_BUF", 1) != 0;
  k.gemm_group = num("XNRS_GEMM_GROUP", -1);
  k.gemm_tile = (int)num("XNRS_GEMM_TILE", -1);
  k.split_min_tiles = num("XNRS_GEMM_SPLIT_MIN_TILES", 512);
  k.mha_lds = (int)num("XNRS_MHA_LDS", -1);
  k.mha_headwave = num("XNRS_MHA_HEADWAVE", 1) != 0;
  k.mha_pair = num("XNRS_MHA_PAIR", 1) != 0;
  k.mha_bwd_fused = num("XNRS_MHA_BWD_FUSED", 1) != 0;
  k.gemm_dw = (int)num("XNRS_GEMM_DW", 2);
  k.gemm_dw_tile = (int)num("XNRS_GEMM_DW_TILE", 256);
  k.fold_out = (int)num("XNRS_FOLD_OUT", 1);
  k.fc1_rowdot = num("XNRS_FC1_ROWDOT", 1) != 0;
  k.fold_train = (int)num("XNRS_FOLD_TRAIN", 1);
  k.news_fused = (int)num("XNRS_NEWS_FUSED", 1);
  k.news_fused_npw = (int)num("XNRS_NEWS_FUSED_NPW", 0);
  k.fast_tanh = num("XNRS_FAST_TANH", 1) != 0;
  k.additive_fused = (int)num("XNRS_ADDITIVE_FUSED", 1);
  k.af_fbuf = num("XNRS_AF_FBUF", 1) == 2 ? 2 : 1;
  k.mha_skip_masked = num("XNRS_MHA_SKIP_MASKED", 1) != 0;
  k.mha_live_o = num("XNRS_MHA_LIVE_O", 1) != 0;
  {
    k.gemm_qkv_one_launch = num("XNRS_GEMM_QKV_ONE_LAUNCH", 1) != 0;
  }
  k.gemm_fc1_in_tail = num("XNRS_GEMM_FC1_IN_TAIL", 1) != 0;
  k.gemm_live_tiles = num("XNRS_GEMM_LIVE_TILES", 1) != 0;
  k.gemm_live_tiles_min_rows = num("XNRS_GEMM_LIVE_TILES_MIN_ROWS", 16384);
  k.gemm_live_rows = num("XNRS_GEMM_LIVE_ROWS", 1) != 0;
  k.gemm_live_rows_min_rows = num("XNRS_GEMM_LIVE_ROWS_MIN_ROWS", 16384);
  k.bwd_side_stream = num("XNRS_BWD_SIDE_STREAM", 1) != 0;
  k.bwd_side_min_rows = num("XNRS_BWD_SIDE_MIN_ROWS", 0);
  k.gru_layout = num("XNRS_GRU_LAYOUT", 0) == 1 ? 1 : 0;
  k.gemm_a16 = num("XNRS_GEMM_A16", 1) != 0;
  const long long m = num("XNRS_GEMM_MODE", 0);
  k.gemm_mode_init = (m >= 0 && m <= 2) ? (int)m : 0;
  return k;
}
static Knobs g_knobs = read_knobs();  // at library load
static std::atomic<int> g_gemm_mode{g_knobs.gemm_mode_init};
const Knobs& knobs() { return g_knobs; }
void reload_knobs() { g_knobs = read_knobs(); }
int gemm_mode() { return g_gemm_mode.load(std::memory_order_relaxed); }
void set_gemm_mode(int mode) { g_gemm_mode.store((mode >= 0 && mode <= 2) ? mode : 0, std::memory_order_relaxed); }

// what a forward launcher fills in (kernels.h: "filled in by the launcher"), for a launch without split-K
static void complete_args(GemmArgs* a) {
  if (a->act == 2 && knobs().fast_tanh) a->act = ACT_TANH_FAST;
  a->k_per_split = a->K > 0 ? a->K : 1;
  // an output of hundreds of MB (the Q/K/V image of a 65 500-row pass: 604 MB) is written once and read by the next
  // kernel from HBM anyway: non-temporal stores keep it from evicting the operand panels (-0.5 % on the Q/K/V GEMM)
  a->nt_store = (!a->accumulate && !a->c_scatter && a->M * a->ldc * 4 >= (64ll << 20)) ? 1 : 0;
}

hipError_t launch_gemm_f32(const GemmArgs& a_in, hipStream_t stream, int* nsplit_used) {
  GemmArgs a = a_in;
  if (a.M <= 0 || a.Nseg <= 0) return hipSuccess;
  complete_args(&a);
  if (a.K >= (1ll << 31)) return hipErrorInvalidValue;  // 32-bit contraction indices in the kernel
  // 16-byte vector loads need the contiguous dimension of each operand on 16-B boundaries
  bool vec = (a.lda % 4 == 0) && (a.ldw % 4 == 0) && aligned16(a.A);
  vec = vec && (a.a_col ? (a.M % 4 == 0) : (a.K % 4 == 0));
  vec = vec && (a.b_kn ? (a.Nseg % 4 == 0) : (a.K % 4 == 0));
  for (int s = 0; s < a.nseg; ++s) vec = vec && aligned16(a.W[s]);

  int nsplit = 1;
  if (a.slabs && a.nsplit > 1) {
    nsplit = a.nsplit;
    const int64_t per = ((a.K + nsplit - 1) / nsplit + KALIGN - 1) / KALIGN * KALIGN;  // tile-aligned slices
    nsplit = (int)((a.K + per - 1) / per);
    if (nsplit > 1) a.k_per_split = per;  // (one slice: the whole contraction, as complete_args left it)
    a.slab_stride = a.M * a.ldc;
    if (a.nseg != 1 || a.ldc != a.Nseg) return hipErrorInvalidValue;
  }
  if (nsplit <= 1) nsplit = 1;
  if (nsplit_used) *nsplit_used = nsplit;
  if (a.colsum && !(a.a_col && a.b_kn)) return hipErrorInvalidValue;  // fused column sums: dW layout only
  if (a.k_dev && !(a.a_col && a.b_kn)) return hipErrorInvalidValue;   // device contraction length: dW layout only
  if (a.colsum_out && !a.colsum) return hipErrorInvalidValue;
  if (a.C2 && (nsplit <= 1 || !(a.a_col && a.b_kn) || a.c2_row0 <= 0 || a.c2_row0 >= a.M)) return hipErrorInvalidValue;  // two
                                                                                                   // destinations: split-K dW only
  bool cs_copy = false;  // one slice: its partial IS the bias gradient (written in place when 16-byte aligned)
  if (a.colsum && a.colsum_out && nsplit == 1) {
    if (aligned16(a.colsum_out)) a.colsum = a.colsum_out;
    else cs_copy = true;
  }
  if (a.rowdot_out && (a.a_col || a.b_kn || a.nseg != 1 || nsplit != 1 || !a.rowdot_w || a.accumulate || a.aux_mode ||
                       (a.act != 2 && a.act != ACT_TANH_FAST)))
    return hipErrorInvalidValue;  // fused row dots: plain forward launches with a tanh epilogue only (the pooler's fc1)
  // ... scattered in place only from a one-row-per-id list with a device count (the GATH + MDEV instantiation)
  if (a.rowdot_out && a.c_scatter && !(a.gather_ids && a.gather_S == 1 && a.m_dev)) return hipErrorInvalidValue;
  hipError_t e;
  const int mode = gemm_mode();
  // the split kernel has one tile shape (128x128): below one full round of workgroups the fp32 kernel with its
  // smaller tiles is faster (measured: 4099 x 260 x 300 -> 38 TF fp32 vs 22 TF split)
  const int64_t min_tiles = knobs().split_min_tiles;  // tests force the split kernel onto tiny shapes with 0
  if (a.m_dev && (a.a_col || a.b_kn || nsplit != 1 || mode != 0)) return hipErrorInvalidValue;  // device row count: fp32 forward only
  if (a.live_tiles && (a.a_col || a.b_kn || nsplit != 1 || mode != 0 || a.m_dev)) return hipErrorInvalidValue;  // live row tiles: fp32 forward only
  if (a.rowscale && (a.a_col || a.b_kn || a.nseg != 1 || nsplit != 1 || !a.rowscale_vec || a.c_scatter || a.rowdot_out))
    return hipErrorInvalidValue;  // rank-1 epilogue term: plain forward launches only
  if (mode && !a.rowdot_out && !a.rowscale && !a.a_col && !a.b_kn && vec && nsplit == 1 &&
      ((a.M + 127) / 128) * ((a.Nseg + 127) / 128) * a.nseg >= min_tiles)
    return launch_gemm_split(a, mode == 1 ? 3 : 2, stream);
  if (!a.a_col && !a.b_kn) e = launch_layout<false, false>(a, vec, nsplit, stream);
  else if (!a.a_col && a.b_kn) e = launch_layout<false, true>(a, vec, nsplit, stream);
  else if (a.a_col && a.b_kn) {
    // weight gradients: the register-transposing kernel (gemm_dw.hip) when the shape allows, else the k-major variant
    if (knobs().gemm_dw && gemm_dw_eligible(a)) e = launch_gemm_dw(a, nsplit, stream);
    else e = launch_layout<true, true>(a, vec, nsplit, stream);
  }
  else return hipErrorInvalidValue;
  if (e != hipSuccess) return e;
  if (nsplit > 1) {
    const int64_t n = a.M * a.ldc;
    const int cs_n = (a.colsum && a.colsum_out) ? (int)a.M : 0;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((n + cs_n + 255) / 256)), dim3(256), 0, stream, a.slabs,
                       a.slab_stride, nsplit, a.C, n, a.accumulate, a.colsum, a.colsum_out, cs_n, a.C2, a.c2_row0 * a.ldc,
                       a.C2 ? a.colsum_out2 : nullptr, (int)a.c2_row0);
    e = hipGetLastError();
  } else if (cs_copy) {
    e = launch_colsum_final(a.colsum, 1, (int)a.M, a.colsum_out, stream);
  }
  return e;
}

// ---- Q + K|V of a dense live-row pass in one grid (kernels.h)
static std::atomic<int64_t> g_qkv_launches{0};
void qkv_launches_add(int n) { g_qkv_launches.fetch_add(n, std::memory_order_relaxed); }
int64_t qkv_launches_read(bool reset) {
  return reset ? g_qkv_launches.exchange(0, std::memory_order_relaxed) : g_qkv_launches.load(std::memory_order_relaxed);
}

// the conditions under which launch_gemm_f32 runs a forward launch on the 16-byte-vector, buffer-load kernels; *gath: A through
// row pointers (launch_cfg: gathered rows, or an A beyond the descriptor window)
static bool qkv_section_ok(const GemmArgs& a, bool* gath) {
  if (a.a_col || a.b_kn || a.M <= 0 || a.Nseg <= 0 || a.nseg < 1 || a.K < 4 || a.K >= (1ll << 31) || a.K % 4 != 0) return false;
  if (a.lda % 4 != 0 || a.ldw % 4 != 0 || !aligned16(a.A)) return false;
  for (int s = 0; s < a.nseg; ++s)
    if (!aligned16(a.W[s])) return false;
  if ((a.slabs && a.nsplit > 1) || a.rowdot_out || a.rowscale || a.colsum || a.k_dev || a.C2) return false;
  if (!knobs().gemm_buf || (int64_t)a.Nseg * a.ldw * 4 > (int64_t)BUF_OOB) return false;
  *gath = a.gather_ids || a.M * a.lda * 4 > (int64_t)BUF_OOB;
  return true;
}

bool gemm_qkv_one_launch_ok(const GemmArgs& kv, const GemmArgs& q) {
  if (!knobs().gemm_qkv_one_launch || gemm_mode() != 0 || knobs().gemm_tile >= 0) return false;
  bool kv_gath = false, q_gath = false;
  if (!qkv_section_ok(kv, &kv_gath) || !qkv_section_ok(q, &q_gath)) return false;
  // K|V: the LIVE instantiation with buffer loads for A (listed row tiles, host row count, plain epilogue).  Gathered rows
  // (table + ids, or an A beyond the descriptor window) keep the two launches: the entry is not built for them (see the kernel)
  if (kv_gath || !kv.live_tiles || !kv.live_n || kv.m_dev || kv.c_scatter) return false;
  // Q: the GATH + MDEV instantiation with the row-scattered epilogue, one row per id
  if (!q_gath || !q.gather_ids || q.gather_S != 1 || !q.c_scatter || !q.m_dev || q.live_tiles || q.nseg != 1) return false;
  const int64_t grid = qkv_one_launch_grid((int)((kv.M + 127) / 128), (kv.Nseg + 127) / 128 * kv.nseg, q.M, 128, (q.Nseg + 63) / 64);
  return (kv.M + 127) / 128 <= 0x7fffffffLL && grid <= 0x7fffffffLL;
}

hipError_t launch_gemm_qkv_one(const GemmArgs& kv_in, const GemmArgs& q_in, hipStream_t stream) {
  if (!gemm_qkv_one_launch_ok(kv_in, q_in)) return hipErrorInvalidValue;
  GemmArgs kv = kv_in, q = q_in;
  for (GemmArgs* a : {&kv, &q}) complete_args(a);  // (K >= 4 here, gemm_qkv_one_launch_ok: k_per_split = K)
  const int kv_m_tiles = (int)((kv.M + 127) / 128), kv_n_tiles_seg = (kv.Nseg + 127) / 128;
  const int q_m_tiles = (int)((q.M + 127) / 128), q_n_tiles = (q.Nseg + 63) / 64;
  const int kv_gn = gemm_group_tiles(kv_n_tiles_seg * kv.nseg, 128, kv.K, false);
  const int q_gn = gemm_group_tiles(q_n_tiles, 64, q.K, false);
  const dim3 g((unsigned)qkv_one_launch_grid(kv_m_tiles, kv_n_tiles_seg * kv.nseg, q.M, 128, q_n_tiles));
  hipLaunchKernelGGL(gemm_qkv_one_launch_kernel, g, dim3(256), 0, stream, kv, q, kv_m_tiles, kv_n_tiles_seg, kv_gn, q_m_tiles, q_n_tiles,
                     q_gn);
  return hipGetLastError();
}

// ---- ... with fc1 of the previous pass as a third section (kernels.h)
static std::atomic<int64_t> g_fc1_in_tail{0};
void fc1_in_tail_add(int n) { g_fc1_in_tail.fetch_add(n, std::memory_order_relaxed); }
int64_t fc1_in_tail_read(bool reset) {
  return reset ? g_fc1_in_tail.exchange(0, std::memory_order_relaxed) : g_fc1_in_tail.load(std::memory_order_relaxed);
}

// what launch_gemm_f32 asks of a launch before it takes the GATH + RDOT + MDEV instantiation with scattered row dots
bool gemm_fc1_in_tail_ok(const GemmArgs& f) {
  if (!knobs().gemm_fc1_in_tail || gemm_mode() != 0 || knobs().gemm_tile >= 0 || !knobs().gemm_buf) return false;
  if (f.a_col || f.b_kn || f.M <= 0 || f.Nseg <= 0 || f.nseg != 1 || f.K < 4 || f.K >= (1ll << 31) || f.K % 4 != 0) return false;
  if (f.lda % 4 != 0 || f.ldw % 4 != 0 || !aligned16(f.A) || !aligned16(f.W[0]) || (int64_t)f.Nseg * f.ldw * 4 > (int64_t)BUF_OOB) return false;
  if ((f.slabs && f.nsplit > 1) || f.rowscale || f.colsum || f.k_dev || f.C2 || f.live_tiles || f.accumulate || f.aux_mode) return false;
  if (!f.rowdot_out || !f.rowdot_w || (f.act != 2 && f.act != ACT_TANH_FAST)) return false;
  if (!f.gather_ids || f.gather_S != 1 || !f.c_scatter || !f.m_dev) return false;
  return (f.M + FC1_TAIL_BM - 1) / FC1_TAIL_BM * ((f.Nseg + FC1_TAIL_BN - 1) / FC1_TAIL_BN) <= 0x3fffffffLL;
}

hipError_t launch_gemm_qkv_fc1(const GemmArgs& kv_in, const GemmArgs& q_in, const GemmArgs* f_in, hipStream_t stream) {
  if (!gemm_qkv_one_launch_ok(kv_in, q_in) || (f_in && !gemm_fc1_in_tail_ok(*f_in))) return hipErrorInvalidValue;
  GemmArgs kv = kv_in, q = q_in, f{};  // f.M == 0: an empty third section, nothing of f is read
  if (f_in) f = *f_in;
  for (GemmArgs* a : {&kv, &q, &f}) complete_args(a);  // (the empty third section: K = 0, k_per_split = 1)
  constexpr int FTM = FC1_TAIL_BM / 64, FTN = FC1_TAIL_BN / 64;
  const int kv_m_tiles = (int)((kv.M + 127) / 128), kv_n_tiles_seg = (kv.Nseg + 127) / 128;
  const int q_m_tiles = (int)((q.M + 127) / 128), q_n_tiles = (q.Nseg + 63) / 64;
  const int f_m_tiles = (int)((f.M + FC1_TAIL_BM - 1) / FC1_TAIL_BM), f_n_tiles = f_in ? (f.Nseg + FC1_TAIL_BN - 1) / FC1_TAIL_BN : 1;
  const int kv_gn = gemm_group_tiles(kv_n_tiles_seg * kv.nseg, 128, kv.K, false);
  const int q_gn = gemm_group_tiles(q_n_tiles, 64, q.K, false);
  const int f_gn = gemm_group_tiles(f_n_tiles, FC1_TAIL_BN, f.K, false);
  const int64_t grid = qkv_fc1_launch_grid(kv_m_tiles, kv_n_tiles_seg * kv.nseg, q.M, 128, q_n_tiles, f.M, FC1_TAIL_BM, f_n_tiles);
  if (grid <= 0 || grid > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((gemm_qkv_fc1_launch_kernel<FTM, FTN>), dim3((unsigned)grid), dim3(256), 0, stream, kv, q, f, kv_m_tiles, kv_n_tiles_seg,
                     kv_gn, q_m_tiles, q_n_tiles, q_gn, f_m_tiles, f_n_tiles, f_gn);
  return hipGetLastError();
}

}  // namespace xnrs
