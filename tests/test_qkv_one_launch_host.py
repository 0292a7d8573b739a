"""CPU: the block -> work rule of the one-launch Q + K|V projection (kernels.h qkv_one_launch_map, through the host entry
point xnrs_qkv_one_launch_map; DESIGN.md section 4.1 "One launch").

The grid is sized for every K|V tile and every Q tile of a pass; the workgroups find their work from two device counts
(live row tiles, live rows).  Enumerated here over every block of the worst-case grid: each tile of each section that
exists is produced exactly once and nothing else is, the Q section starts at a multiple of 8 blocks (both sections take
their XCD from the low three bits of the index inside the section), and with both counts 0 no block has work.

The index inside a section is turned into (row tile, column tile) by the GEMM body's own XCD-aware, column-grouped walk;
`walk` below restates it (gemm_f32.hip), so the check covers the composition: rule + walk = a bijection onto the tiles."""
import ctypes

import numpy as np
import pytest

from xnrs_amd import hip

KV_ROW_TILES = 40   # the grid's worst case: row tiles of the pass
Q_ROWS = 5000       # ... and its token rows
Q_BM = 128
ROWS = sorted({0, 1, 63, 64, 65, 127, 128, 129, 192, 255, 256, 257, 1000, 1024, 2496, 2500, 4096, 4864, 4999, 5000})


def grid_of(kv_cols, q_cols):
    n = hip.lib().xnrs_qkv_one_launch_map(0, 0, 0, KV_ROW_TILES, kv_cols, Q_ROWS, Q_BM, q_cols, None, None)
    assert n == (KV_ROW_TILES * kv_cols + 7) // 8 * 8 + (Q_ROWS + Q_BM - 1) // Q_BM * q_cols
    return n


def enumerate_grid(live_tiles, live_rows, kv_cols, q_cols):
    """(section, index) of every block of the worst-case grid."""
    l = hip.lib()
    sec, idx = ctypes.c_int32(), ctypes.c_int32()
    out = np.empty((grid_of(kv_cols, q_cols), 2), dtype=np.int64)
    for b in range(out.shape[0]):
        n = l.xnrs_qkv_one_launch_map(b, live_tiles, live_rows, KV_ROW_TILES, kv_cols, Q_ROWS, Q_BM, q_cols,
                                      ctypes.byref(sec), ctypes.byref(idx))
        assert n == out.shape[0]
        out[b] = sec.value, idx.value
    return out


def walk(bid, m_tiles, n_tiles, gn):
    """gemm_f32.hip: workgroup index -> (row tile, column tile); each XCD owns a contiguous range of the tile sequence,
    column groups of gn tiles outermost."""
    nwg = m_tiles * n_tiles
    xcd, q, r = bid & 7, nwg >> 3, nwg & 7
    wgid = np.where(xcd < r, xcd * (q + 1), r * (q + 1) + (xcd - r) * q) + (bid >> 3)
    grp = wgid // (gn * m_tiles)
    rem = wgid - grp * gn * m_tiles
    gw = np.minimum(n_tiles - grp * gn, gn)
    mt = rem // gw
    return mt, grp * gn + (rem - mt * gw)


def group_tiles(n_tiles):
    """gemm_group_tiles at D = 768: 12 column tiles of 128 go in two groups of 6, 12 of 64 (or 6 of 128) in one."""
    return 6 if n_tiles == 12 else n_tiles


@pytest.mark.parametrize("kv_cols,q_cols", [(12, 12), (12, 6), (6, 12), (6, 6)])
def test_every_tile_once_and_nothing_else(kv_cols, q_cols):
    l = hip.lib()
    total = grid_of(kv_cols, q_cols)
    sec, idx = ctypes.c_int32(), ctypes.c_int32()
    # the rule is a function of the two section sizes only: enumerate the whole grid for every live-tile count at a few
    # row counts, and for every row count at a few tile counts
    combos = {(t, r) for t in range(0, KV_ROW_TILES + 1) for r in (0, 129, 5000)}
    combos |= {(t, r) for t in (0, 1, 17, 40) for r in ROWS}
    combos |= {(t, r) for t in (3, 39) for r in range(0, Q_ROWS + 1, 32 * 7)}   # 224: hits multiples of 64 / 128 and none
    for lt, rows in sorted(combos):
        w = enumerate_grid(lt, rows, kv_cols, q_cols)
        kv = w[w[:, 0] == 0, 1]
        qq = w[w[:, 0] == 1, 1]
        q_m_tiles = (rows + Q_BM - 1) // Q_BM
        # each section: the indices 0 .. n-1 of its tile sequence, each once (blocks in ascending order)
        assert np.array_equal(kv, np.arange(lt * kv_cols)), (lt, rows)
        assert np.array_equal(qq, np.arange(q_m_tiles * q_cols)), (lt, rows)
        assert ((w[:, 0] == -1) | (w[:, 0] == 0) | (w[:, 0] == 1)).all()
        assert (w[:, 0] == -1).sum() == total - kv.size - qq.size
        # K|V first, then at most 7 idle blocks, then Q from a multiple of 8 on, then idle blocks only
        if qq.size:
            first_q = int(np.flatnonzero(w[:, 0] == 1)[0])
            assert first_q % 8 == 0 and first_q == (lt * kv_cols + 7) // 8 * 8
            assert (w[first_q:first_q + qq.size, 0] == 1).all()
            assert ((first_q + np.arange(qq.size)) & 7 == qq & 7).all()   # the XCD of the hardware's round-robin
        assert (w[:kv.size, 0] == 0).all()
        # ... and through the body's walk: every (row tile, column tile) of each section exactly once
        for ind, m_tiles, cols in ((kv, lt, kv_cols), (qq, q_m_tiles, q_cols)):
            if ind.size:
                mt, nt = walk(ind, m_tiles, cols, group_tiles(cols))
                assert sorted(zip(mt.tolist(), nt.tolist())) == [(a, b) for a in range(m_tiles) for b in range(cols)]
    # blocks outside the grid have no work either
    for b in (-1, total, total + 8):
        l.xnrs_qkv_one_launch_map(b, 40, 5000, KV_ROW_TILES, kv_cols, Q_ROWS, Q_BM, q_cols, ctypes.byref(sec), ctypes.byref(idx))
        assert sec.value == -1


def test_both_counts_zero_and_counts_past_the_capacity():
    w = enumerate_grid(0, 0, 12, 12)
    assert (w[:, 0] == -1).all()
    # counts are clamped to what the grid was sized for, negative counts to 0 (the bodies clamp the same way)
    assert np.array_equal(enumerate_grid(45, 6000, 12, 6), enumerate_grid(KV_ROW_TILES, Q_ROWS, 12, 6))
    assert (enumerate_grid(-3, -1, 12, 6)[:, 0] == -1).all()


def test_bad_shapes_are_refused():
    l = hip.lib()
    einval = hip.parse_header(open(hip.HEADER_PATH).read())[0]["EINVAL"]
    assert l.xnrs_qkv_one_launch_map(0, 0, 0, 4, 0, 100, 128, 6, None, None) == einval
    assert l.xnrs_qkv_one_launch_map(0, 0, 0, 4, 6, 100, 0, 6, None, None) == einval
    assert l.xnrs_qkv_one_launch_map(0, 0, 0, -1, 6, 100, 128, 6, None, None) == einval
    assert l.xnrs_qkv_one_launch_map(0, 0, 0, 0, 6, 0, 128, 6, None, None) == 0   # an empty pass: an empty grid


def test_launch_counter_reads_and_resets():
    l = hip.lib()
    l.xnrs_qkv_launch_count(1)
    assert l.xnrs_qkv_launch_count(0) == 0
