// The body of the fp32 GEMM kernel (gemm_f32.hip), as TEXT: included once into the __global__ template gemm_f32_kernel and
// once into the __device__ function gemm_f32_body, inside a template with the parameters TM, TN, A_COL, B_KN, VEC, PIPE,
// BK, BUF, MINW, GATH, KG, RDOT, MDEV, LIVE and with `a`, `m_tiles`, `n_tiles_seg`, `gn` in scope.  The including function
// says where the workgroup stands and where its LDS tiles are:
//   XNRS_GEMM_BID               the workgroup's index in the launch's tile sequence (the kernel: blockIdx.x)
//   XNRS_GEMM_NWG               the number of workgroups of that sequence (the kernel: gridDim.x)
//   XNRS_GEMM_LDS_TILES(A, B)   declares A as float[NBUF][A_SZ] and B as float[NBUF][B_SZ] in LDS (the kernel: two __shared__
//                               arrays of its own; the function: views of the caller's arrays)
// Why text and not a call: the kernel compiled as a wrapper around an always-inlined function is NOT the same kernel -- 64 of
// the 77 instantiations came out with other register counts (k-major 128x64 tiles 132 -> 150 VGPRs, the fc1 list kernel 7 -> 6
// waves per SIMD; profiles/qkv_one_launch_resource_usage.md) -- while the same text in the same place is, to the last
// register.  blockIdx.y / gridDim.y (split-K slices) are read here as before.
  static_assert(!MDEV || (!A_COL && !B_KN), "device row counts: forward layout only");
  static_assert(!LIVE || (BUF && !MDEV), "live row tiles: buffer-load forward kernels, host row count");
  static_assert(!BUF || (!A_COL && !B_KN && VEC), "buffer loads are implemented for the forward layout");
  static_assert(!RDOT || PIPE == 5, "the fused row dots ride on the interleaved pipeline (its MFMA call is the swapped one)");
  static_assert(!GATH || BUF, "the gathered-A variant keeps buffer loads for B");
  constexpr int BM = 64 * TM, BN = 64 * TN;
  // k-contiguous LDS tile rows: BK = 32 -> padded to 36 floats (conflict-free ds_read_b128, measured
  // SQ_LDS_BANK_CONFLICT = 0); BK = 16 -> 64-B rows, UNPADDED, with the 16-byte chunk index XOR-swizzled by
  // (row >> 2) & 3: reads of a 16-lane group then cover 16 distinct 16-B slots and the 8-lane groups of
  // ds_write_b128 cover two whole rows = 32 distinct banks (the padded 20-float rows measured a 2-way
  // write conflict on every store, 33 % of the LDS cycles), and the tile shrinks from 40 to 32 KB.
  constexpr bool SWZ = BK == 16;
  constexpr int LDK = SWZ ? BK : BK + 4;
  constexpr int CHK = BK / 4;  // 16-byte chunks per k-contiguous row
  constexpr int RPP = 256 / CHK;  // rows per staging pass
  constexpr int AR = BM / RPP, BR = BN / RPP;  // 16-byte chunks per thread per operand tile
  constexpr int LDA = A_COL ? (BM + 4) : LDK;
  constexpr int LDB = B_KN ? (BN + 4) : LDK;
  constexpr int A_SZ = A_COL ? BK * LDA : BM * LDA;
  constexpr int B_SZ = B_KN ? BK * LDB : BN * LDB;
  constexpr int NBUF = 2;
  XNRS_GEMM_LDS_TILES(As, Bs)

  // rows that exist: a.M, or -- MDEV -- the device scalar *a.m_dev (a.M was only the grid's worst case), kept in SGPRs.
  // The tile walk below then runs over the row tiles that exist, and the workgroups past them leave at once: mapped over
  // the launched grid instead, the live row tiles would all fall on the first XCDs (each XCD owns a contiguous range of
  // the walk) -- measured: a pass with 25 % of its rows live took as long as a full one.
  int64_t Mrun = a.M;
  int nwg = XNRS_GEMM_NWG;
  if constexpr (MDEV) {
    const int64_t md = load_dev_scalar(a.m_dev);
    Mrun = ((int64_t)__builtin_amdgcn_readfirstlane((int)(md >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)md);
    if (Mrun > a.M) Mrun = a.M;
    m_tiles = (int)((Mrun + BM - 1) / BM);
    nwg = m_tiles * n_tiles_seg * a.nseg;
    if ((int)XNRS_GEMM_BID >= nwg) return;  // workgroup-uniform, before any barrier
  }
  if constexpr (LIVE) {  // the same over the LISTED row tiles (m_tiles was the grid's worst case: every tile of the pass)
    const int nl = __builtin_amdgcn_readfirstlane((int)load_dev_scalar(a.live_n));
    m_tiles = nl < m_tiles ? (nl > 0 ? nl : 0) : m_tiles;
    nwg = m_tiles * n_tiles_seg * a.nseg;
    if ((int)XNRS_GEMM_BID >= nwg) return;  // workgroup-uniform, before any barrier
  }
  // ---- XCD-aware tile order (bijective for any grid size); blockIdx.y = k slice
  const int bid = XNRS_GEMM_BID;
  const int xcd = bid & 7;
  const int q = nwg >> 3, r = nwg & 7;
  const int wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  // tile walk: column GROUPS of gn tiles outermost, then the M tiles, then the gn tiles of the group, so the
  // weight panels an XCD touches over a long stretch (gn * BN * K * 4 <= ~2.5 MB) stay in its 4 MB L2 instead
  // of streaming through it once per handful of M tiles (Q/K/V projection: 18 column tiles = 7 MB of W).
  const int n_tiles = n_tiles_seg * a.nseg;
  const int grp = wgid / (gn * m_tiles);
  const int rem = wgid - grp * gn * m_tiles;
  const int gw = (n_tiles - grp * gn < gn) ? n_tiles - grp * gn : gn;  // the last group may be narrower
  const int mt = rem / gw;
  const int nt = grp * gn + (rem - mt * gw);
  const int seg = nt / n_tiles_seg;
  const int nts = nt - seg * n_tiles_seg;
  int64_t m0 = (int64_t)mt * BM;
  if constexpr (LIVE) m0 = (int64_t)__builtin_amdgcn_readfirstlane(a.live_tiles[mt]) * BM;  // mt-th live tile of the pass
  const int n0 = nts * BN;  // column inside the segment

  // contraction indices are 32-bit in the kernel (the launcher refuses K >= 2^31): the k-tail tests and tile offsets of
  // the inner loop are then single VALU / SALU instructions instead of 64-bit compare-and-select pairs
  int64_t kps = a.k_per_split;
  int Ktot = (int)a.K;
  if constexpr (A_COL && B_KN) {
    if (a.k_dev) {  // contraction length on the device (GemmArgs::k_dev): slices cut here, wave-uniform
      const int kd = __builtin_amdgcn_readfirstlane((int)load_dev_scalar(a.k_dev));
      Ktot = kd < Ktot ? (kd > 0 ? kd : 0) : Ktot;
      kps = (((int64_t)Ktot + gridDim.y - 1) / gridDim.y + KALIGN - 1) / KALIGN * KALIGN;
      if (kps < KALIGN) kps = KALIGN;
    }
  }
  const int kbeg = (int)((int64_t)blockIdx.y * kps);
  const int kend = (int)((kbeg + kps < Ktot) ? kbeg + kps : Ktot);

  const float* __restrict__ W = a.W[seg];
  const float* __restrict__ bias = a.bias[seg];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // ---- staging maps
  // k-contiguous tile: chunk lc (4 floats of k) of row lr + RPP*i
  const int lc = tid % CHK, lr = tid / CHK;
  // k-major tile: chunk (4 floats along i) cA of k-row kA + KROWS*i
  constexpr int CHA = BM / 4, KRA = 256 / CHA;  // chunks per k-row, k-rows per pass
  constexpr int CHB = BN / 4, KRB = 256 / CHB;
  const int cA = tid % CHA, kA = tid / CHA;
  const int cB = tid % CHB, kB = tid / CHB;

  // Every global load is unconditional (out-of-range lanes are pointed at g_zero_line), so the compiler's
  // vmcnt bookkeeping stays exact and the two-tiles-ahead pipeline below really leaves a whole tile in
  // flight across the LDS store.
  const float* pa[AR];
  const float* pb[BR];
  unsigned a_ok = 0, b_ok = 0;  // bit i: row / column i of this thread is inside the matrix
  // BUF: ONE byte offset per operand in a VGPR -- (row lr, chunk lc) of the tile; row lr + RPP * i rides in the SCALAR
  // offset (k0 * 4 + i * RPP * ld * 4), and rows / columns past the matrix need no flag: their offset is >= num_records
  // (= rows * ld * 4) and the bounds check, which includes the scalar offset (tools/probes/raw_soffset.hip), returns
  // zeros.  (With one VGPR offset per row the kernel sat at the 128-VGPR cap with 4 spilled loop invariants that were
  // re-read from scratch -- through the same vmcnt queue as the tile loads -- in every K tile.)
  unsigned offA0 = 0, offB0 = 0;
  unsigned offBv[BR];  // GATH: one VGPR offset per weight row after all (measured faster there: see the GATH note above)
  int dA = 0, dB = 0;
  __amdgpu_buffer_rsrc_t rsA, rsB;
  if constexpr (BUF) {
    if constexpr (!GATH) rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.A), 0, (int)(Mrun * a.lda * 4), 0x00020000);
    rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(W), 0, (int)((int64_t)a.Nseg * a.ldw * 4), 0x00020000);
    if constexpr (GATH) {
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        const int64_t gr = m0 + lr + RPP * i;
        int64_t src = gr < Mrun ? gr : Mrun - 1;
        if (a.gather_ids) {
          const int64_t n = src / a.gather_S;
          src = (int64_t)a.gather_ids[n] * a.gather_S + (src - n * a.gather_S);
        }
        pa[i] = a.A + src * a.lda + 4 * lc;
      }
    } else {
      const int64_t gr = m0 + lr;
      offA0 = gr < Mrun ? (unsigned)((gr * a.lda + 4 * lc) * 4) : BUF_OOB;
      dA = (int)(RPP * a.lda * 4);
    }
    const int col = n0 + lr;
    offB0 = col < a.Nseg ? (unsigned)(((int64_t)col * a.ldw + 4 * lc) * 4) : BUF_OOB;
    dB = (int)(RPP * a.ldw * 4);
    if constexpr (GATH) {
#pragma unroll
      for (int i = 0; i < BR; ++i) offBv[i] = offB0 + (unsigned)(i * dB);
    }
  } else if (!A_COL) {
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      int64_t gr = m0 + lr + RPP * i;
      if (gr < Mrun) a_ok |= 1u << i;
      else gr = Mrun - 1;
      int64_t src = gr;
      if (a.gather_ids) {
        const int64_t n = gr / a.gather_S;
        src = (int64_t)a.gather_ids[n] * a.gather_S + (gr - n * a.gather_S);
      }
      pa[i] = a.A + src * a.lda;
    }
  } else {
    if (m0 + 4 * cA < Mrun) a_ok = 1;
  }
  if (!B_KN) {
#pragma unroll
    for (int i = 0; i < BR; ++i) {
      int col = n0 + lr + RPP * i;
      if (col < a.Nseg) b_ok |= 1u << i;
      else col = a.Nseg - 1;
      pb[i] = W + (int64_t)col * a.ldw;
    }
  } else {
    if (n0 + 4 * cB < a.Nseg) b_ok = 1;
  }

  f32x4 ra[1][AR], rb[1][BR];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  // P = register set (compile-time), k0 = first k of the tile
  // `only` >= 0 restricts the call to ONE 16-byte chunk (A chunks 0..AR-1, then B chunks): the interleaved
  // pipeline issues the tile loads / LDS stores one at a time between MFMAs.
  auto gload = [&](auto P, int k0, int only = -1) {
    constexpr int p = decltype(P)::value;
    if constexpr (BUF) {
      const unsigned sel = (k0 + 4 * lc < kend) ? 0u : BUF_OOB;  // k tail of the last tile
      const int soff = (int)(k0 * 4);
      int ka = k0;  // GATH: clamp the k tail (B returns zeros there)
      if constexpr (GATH) {
        const int klim = kend - 4 - 4 * lc;
        ka = ka < klim ? ka : klim;
      }
#pragma unroll
      for (int i = 0; i < AR; ++i)
        if (only < 0 || only == i) {
          if constexpr (GATH) ra[p][i] = *reinterpret_cast<const f32x4*>(pa[i] + ka);
          else ra[p][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsA, (int)(offA0 | sel), soff + i * dA, 0));
        }
#pragma unroll
      for (int i = 0; i < BR; ++i)
        if (only < 0 || only == AR + i) {
          if constexpr (GATH) rb[p][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsB, (int)(offBv[i] | sel), soff, 0));
          else rb[p][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsB, (int)(offB0 | sel), soff + i * dB, 0));
        }
      return;
    }
    if (!A_COL) {
      const int64_t k = k0 + 4 * lc;
      const bool kok = k < kend;
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        if (only >= 0 && only != i) continue;
        if (VEC) {
          ra[p][i] = *reinterpret_cast<const f32x4*>((kok && ((a_ok >> i) & 1u)) ? pa[i] + k : g_zero_line);
        } else {
          f32x4 v = zero4;
          if ((a_ok >> i) & 1u) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (k + e < kend) v[e] = pa[i][k + e];
          }
          ra[p][i] = v;
        }
      }
    } else {
      const int64_t mi = m0 + 4 * cA;
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        if (only >= 0 && only != i) continue;
        const int k = k0 + kA + KRA * i;
        const bool kok = k < kend;
        // k-row gather in 32-bit arithmetic (the contraction is < 2^31), and with NO division for the one-row-per-id
        // lists of the live-row backward: the 64-bit `srck / gather_S` of the first version was a software division
        // per tile load -- 3.4 VALU instructions per MFMA in the dW GEMMs (profiles/r02_train_step_pmc.txt)
        int srck = kok ? k : kbeg;
        if constexpr (KG == 1) {
          srck = a.gather_ids[srck];
        } else if constexpr (KG == 2) {
          if (a.gather_ids) {
            if (a.gather_S == 1) srck = a.gather_ids[srck];
            else {
              const int n = srck / a.gather_S;
              srck = a.gather_ids[n] * a.gather_S + (srck - n * a.gather_S);
            }
          }
        }
        const float* ptr = a.A + (int64_t)srck * a.lda;
        if (VEC) {
          ra[p][i] = *reinterpret_cast<const f32x4*>((kok && a_ok) ? ptr + mi : g_zero_line);
        } else {
          f32x4 v = zero4;
          if (kok) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (mi + e < Mrun) v[e] = ptr[mi + e];
          }
          ra[p][i] = v;
        }
      }
    }
    if (!B_KN) {
      const int64_t k = k0 + 4 * lc;
      const bool kok = k < kend;
#pragma unroll
      for (int i = 0; i < BR; ++i) {
        if (only >= 0 && only != AR + i) continue;
        if (VEC) {
          rb[p][i] = *reinterpret_cast<const f32x4*>((kok && ((b_ok >> i) & 1u)) ? pb[i] + k : g_zero_line);
        } else {
          f32x4 v = zero4;
          if ((b_ok >> i) & 1u) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (k + e < kend) v[e] = pb[i][k + e];
          }
          rb[p][i] = v;
        }
      }
    } else {
      const int ni = n0 + 4 * cB;
#pragma unroll
      for (int i = 0; i < BR; ++i) {
        if (only >= 0 && only != AR + i) continue;
        const int k = k0 + kB + KRB * i;
        const bool kok = k < kend;
        int src = kok ? k : kbeg;
        if constexpr (KG == 1) {
          src = a.b_gather_ids[src];
        } else if constexpr (KG == 2) {
          if (a.b_gather_ids) {
            if (a.b_gather_S == 1) src = a.b_gather_ids[src];
            else {
              const int n = src / a.b_gather_S;
              src = a.b_gather_ids[n] * a.b_gather_S + (src - n * a.b_gather_S);
            }
          }
        }
        const float* ptr = W + (int64_t)src * a.ldw;
        if (VEC) {
          rb[p][i] = *reinterpret_cast<const f32x4*>((kok && b_ok) ? ptr + ni : g_zero_line);
        } else {
          f32x4 v = zero4;
          if (kok) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (ni + e < a.Nseg) v[e] = ptr[ni + e];
          }
          rb[p][i] = v;
        }
      }
    }
  };
  // physical 16-byte chunk of logical chunk c in row `row` of a k-contiguous LDS tile
  auto kswz = [](int row, int c) { return SWZ ? (c ^ ((row >> 2) & 3)) : c; };
  // fused column sums of a k-major A (bias gradients, GemmArgs::colsum): the first column tile of every row tile adds
  // up the A chunks it stages -- each staged exactly once per K tile (`fresh`: the pipeline's redundant re-store of the
  // last tile at the tail must not count twice)
  const bool do_cs = A_COL && a.colsum != nullptr && nt == 0;
  f32x4 cs = {0.f, 0.f, 0.f, 0.f};
  auto sstore = [&](auto P, int buf, int only = -1, bool fresh = true) {
    constexpr int p = decltype(P)::value;
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      if (only >= 0 && only != i) continue;
      if (!A_COL) *reinterpret_cast<f32x4*>(&As[buf][(lr + RPP * i) * LDA + 4 * kswz(lr + RPP * i, lc)]) = ra[p][i];
      else {
        *reinterpret_cast<f32x4*>(&As[buf][(kA + KRA * i) * LDA + 4 * cA]) = ra[p][i];
        if (do_cs && fresh) cs += ra[p][i];
      }
    }
#pragma unroll
    for (int i = 0; i < BR; ++i) {
      if (only >= 0 && only != AR + i) continue;
      if (!B_KN) *reinterpret_cast<f32x4*>(&Bs[buf][(lr + RPP * i) * LDB + 4 * kswz(lr + RPP * i, lc)]) = rb[p][i];
      else *reinterpret_cast<f32x4*>(&Bs[buf][(kB + KRB * i) * LDB + 4 * cB]) = rb[p][i];
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int frow = lane & 31;      // row of the 32x32 operand tile this lane feeds
  const int fk = (lane >> 5) * 4;  // k offset inside an 8-wide k group
  const int a_row0 = wm * 32 * TM + frow;
  const int b_row0 = wn * 32 * TN + frow;

  // MFMAs of the 8-wide k groups [KQ0, KQ1) of the tile in LDS buffer `buf`
  auto compute = [&](int buf, auto KQ0, auto KQ1) {
#pragma unroll
    for (int kq = decltype(KQ0)::value; kq < decltype(KQ1)::value; ++kq) {
      f32x4 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        if (!A_COL) {
          fa[i] = *reinterpret_cast<const f32x4*>(&As[buf][(a_row0 + 32 * i) * LDA + 4 * kswz(a_row0 + 32 * i, kq * 2 + (fk >> 2))]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) fa[i][e] = As[buf][(kq * 8 + fk + e) * LDA + a_row0 + 32 * i];
        }
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        if (!B_KN) {
          fb[j] = *reinterpret_cast<const f32x4*>(&Bs[buf][(b_row0 + 32 * j) * LDB + 4 * kswz(b_row0 + 32 * j, kq * 2 + (fk >> 2))]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) fb[j][e] = Bs[buf][(kq * 8 + fk + e) * LDB + b_row0 + 32 * j];
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fb[j][e], acc[i][j], 0, 0, 0);
    }
  };
  using I0 = std::integral_constant<int, 0>;
  using I4 = std::integral_constant<int, BK / 8>;

  const int nk = (kend - kbeg + BK - 1) / BK;
  auto ktile = [&](int t) { return kbeg + t * BK; };
  if constexpr (PIPE == 1) {
    // one tile ahead: loads of tile t+1 fly during the MFMAs of tile t, LDS store at the end
    if (nk > 0) {
      gload(I0{}, ktile(0));
      sstore(I0{}, 0);
    }
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
      const int buf = t & 1;
      if (t + 1 < nk) gload(I0{}, ktile(t + 1));
      compute(buf, I0{}, I4{});
      if (t + 1 < nk) sstore(I0{}, buf ^ 1);
      __syncthreads();
    }
  } else if constexpr (PIPE == 5) {
    // Two LDS buffers, ONE register set, ONE loop body, explicitly interleaved instruction stream.
    // Why: in-kernel cycle stamps (profiles/r01_gemm_stamps.txt) showed that issuing the 8 loads / 8
    // ds_write_b128 of a tile back to back -- all 4 waves at once, right after the barrier -- blocks an
    // in-order wave for ~1100 of every ~5400 cycles while the shared TA / LDS-write paths drain, and no
    // MFMA of that wave can issue meanwhile.  Here a K tile is cut into "slots" of TM*TN MFMAs (one k
    // step, 256 matrix cycles); behind each slot at most ONE LDS store, ONE tile load and the fragment
    // reads of the next k group are issued, and a sched_barrier pins that order.
    // During iteration t the registers hold tile t+1 (loaded during iteration t-1); chunk j is stored to
    // the other LDS buffer behind slot j+1 and reloaded with tile t+2 behind slot j+2 (~a full iteration
    // of latency hiding).  Fragments are double-buffered so their LDS latency hides behind a k group.  The
    // barrier at the end of the iteration publishes tile t+1 and frees the buffer of tile t.
    constexpr int NKQ = BK / 8;
    constexpr int NSLOT = NKQ * 4;
    constexpr int NCH = AR + BR;
    static_assert(NCH + 2 <= NSLOT, "not enough slots for the tile stores/loads");
    f32x4 fa[2][TM], fb[2][TN];
    auto ldfrag = [&](int st, int buf, int kq) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        if (!A_COL) {
          fa[st][i] = *reinterpret_cast<const f32x4*>(&As[buf][(a_row0 + 32 * i) * LDA + 4 * kswz(a_row0 + 32 * i, kq * 2 + (fk >> 2))]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) fa[st][i][e] = As[buf][(kq * 8 + fk + e) * LDA + a_row0 + 32 * i];
        }
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        if (!B_KN) {
          fb[st][j] = *reinterpret_cast<const f32x4*>(&Bs[buf][(b_row0 + 32 * j) * LDB + 4 * kswz(b_row0 + 32 * j, kq * 2 + (fk >> 2))]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) fb[st][j][e] = Bs[buf][(kq * 8 + fk + e) * LDB + b_row0 + 32 * j];
        }
      }
    };
    const int last = nk - 1;
    if (nk > 0) {
      gload(I0{}, ktile(0));
      sstore(I0{}, 0);
      gload(I0{}, ktile(1 < last ? 1 : last));
    }
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
      const int buf = t & 1;
      const int kn = ktile(t + 2 < last ? t + 2 : last);
      ldfrag(0, buf, 0);
#pragma unroll
      for (int kq = 0; kq < NKQ; ++kq) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int slot = kq * 4 + e;
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              if constexpr (RDOT)  // W . X^T: the block comes out transposed (tokens on the lanes), same fmaf chains
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[kq & 1][j][e], fa[kq & 1][i][e], acc[i][j], 0, 0, 0);
              else
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kq & 1][i][e], fb[kq & 1][j][e], acc[i][j], 0, 0, 0);
          if (e == 1 && kq + 1 < NKQ) ldfrag((kq + 1) & 1, buf, kq + 1);
          if (slot >= 1 && slot < 1 + NCH) sstore(I0{}, buf ^ 1, slot - 1, t < last);  // tile t+1 -> LDS (redundant at the tail)
          if (slot >= 2 && slot < 2 + NCH) gload(I0{}, kn, slot - 2);        // tile t+2 -> the register just stored
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      __syncthreads();
    }
  }

  if constexpr (A_COL) {
    if (a.colsum != nullptr && nt == 0) {  // workgroup-uniform
      // the KRA threads that staged the same 4 columns (same cA, k rows kA + KRA i) add up through LDS (the K loop's
      // last barrier has passed: the tile buffers are free)
      f32x4* red = reinterpret_cast<f32x4*>(&As[0][0]);
      red[kA * CHA + cA] = cs;
      __syncthreads();
      if (kA == 0) {
        f32x4 v = red[cA];
#pragma unroll
        for (int r = 1; r < KRA; ++r) v += red[r * CHA + cA];
        float* dst = a.colsum + (int64_t)blockIdx.y * Mrun + m0 + 4 * cA;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (m0 + 4 * cA + e < Mrun) dst[e] = v[e];
      }
    }
  }

  // ---- epilogue: C/D layout of the 32x32 tile: col = lane&31, row = (e&3) + 8*(e>>2) + 4*(lane>>5)
  const int ccol = lane & 31;
  const int crow = 4 * (lane >> 5);
  const bool split = gridDim.y > 1;
  float* Cout = split ? a.slabs + (int64_t)blockIdx.y * a.slab_stride : a.C;
  if constexpr (RDOT) {
    // fused row dots (GemmArgs::rowdot_w): the accumulators are TRANSPOSED blocks (see the MFMA call) -- lane l holds
    // token row l & 31 and 16 of the block's 32 hidden units -- so the score of a block is an in-lane fmaf chain and one
    // exchange with lane l ^ 32 (rowdot_block_t, kernels.h).  {bias, w} of this workgroup's columns are staged in LDS
    // first (the K loop's last barrier has passed: the tile buffers are free).
    float2* s_bw = reinterpret_cast<float2*>(&As[0][0]);
    static_assert(sizeof(float2) * BN <= sizeof(float) * A_SZ * NBUF, "bias / weight staging fits the A tile buffers");
    for (int c = tid; c < BN; c += 256) {
      const int col = n0 + c;
      const bool cok = col < a.Nseg;
      s_bw[c] = make_float2((bias && cok) ? bias[col] : 0.f, cok ? a.rowdot_w[col] : 0.f);
    }
    __syncthreads();
    const int half = lane >> 5;
    auto dots = [&](auto FAST) {
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int cb = wn * 32 * TN + 32 * j;  // first column of the block inside the tile
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const float sc = rowdot_block_t_lds<decltype(FAST)::value>(acc[i][j], s_bw + cb, half);
          int64_t row = m0 + wm * 32 * TM + 32 * i + (lane & 31);
          if (lane < 32 && row < Mrun && n0 + cb < a.Nseg) {
            if constexpr (GATH && MDEV) {  // scores scattered in place: the row the list names (one row per id; launcher)
              if (a.c_scatter) row = (a.c_scatter_ids ? a.c_scatter_ids : a.gather_ids)[row];
            }
            a.rowdot_out[row * a.ldrd + ((n0 + cb) >> 5)] = sc;
          }
        }
      }
    };
    if (a.act == ACT_TANH_FAST) dots(std::true_type{});
    else dots(std::false_type{});
    return;
  }
  if constexpr (!A_COL) {
    if (a.c_scatter) {
      // Row subset in place: the C (and aux) rows follow A's gather list (the live-row / kv-row products of the grad step).
      // The destination row is looked up ONCE per accumulator row -- (i, e) outermost, the TN column blocks inside -- and
      // without the 64-bit division of the general rule when the list holds one row per id (every list of the grad
      // step): the first version divided per ELEMENT, 64 software divisions per thread, a quarter of these launches.
      const int32_t* __restrict__ sids = a.c_scatter_ids ? a.c_scatter_ids : a.gather_ids;
      const bool one = a.gather_S == 1;
      float bvj[TN];
      int colj[TN];
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        colj[j] = n0 + wn * 32 * TN + 32 * j + ccol;
        bvj[j] = (bias && !split && colj[j] < a.Nseg) ? bias[colj[j]] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          int64_t row = m0 + wm * 32 * TM + 32 * i + (e & 3) + 8 * (e >> 2) + crow;
          if (row >= Mrun) continue;
          if (one) row = sids[row];
          else {
            const int64_t n = row / a.gather_S;
            row = (int64_t)sids[n] * a.gather_S + (row - n * a.gather_S);
          }
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            if (colj[j] >= a.Nseg) continue;
            const int64_t coff = (int64_t)seg * a.Nseg + colj[j];
            float v = acc[i][j][e];
            if (!split) {
              if (a.rowscale) v = fmaf(a.rowscale[row], a.rowscale_vec[colj[j]], v);
              v = apply_act(v + bvj[j], a.act);
              if (a.aux_mode) {
                const float x = a.aux[row * a.ldaux + coff];
                v *= (a.aux_mode == 1) ? (1.f - x * x) : (x > 0.f ? 1.f : 0.f);
              }
              if (a.accumulate) v += Cout[row * a.ldc + coff];
            }
            Cout[row * a.ldc + coff] = v;
          }
        }
      }
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + wn * 32 * TN + 32 * j + ccol;
    if (col >= a.Nseg) continue;
    const float bv = (bias && !split) ? bias[col] : 0.f;
    const int64_t coff = (int64_t)seg * a.Nseg + col;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        int64_t row = m0 + wm * 32 * TM + 32 * i + (e & 3) + 8 * (e >> 2) + crow;
        if (row < Mrun) {
          float v = acc[i][j][e];
          if (!split) {
            if (a.rowscale) v = fmaf(a.rowscale[row], a.rowscale_vec[col], v);
            v = apply_act(v + bv, a.act);
            if (a.aux_mode) {
              const float x = a.aux[row * a.ldaux + coff];
              v *= (a.aux_mode == 1) ? (1.f - x * x) : (x > 0.f ? 1.f : 0.f);
            }
            if (a.accumulate) v += Cout[row * a.ldc + coff];
          }
          if (BUF && a.nt_store) __builtin_nontemporal_store(v, &Cout[row * a.ldc + coff]);
          else Cout[row * a.ldc + coff] = v;
        }
      }
    }
  }
