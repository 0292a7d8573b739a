"""CPU: the block -> work rule of the projection launch with fc1 of the previous pass in its tail (kernels.h
qkv_fc1_launch_map, through the host entry point xnrs_qkv_fc1_launch_map; DESIGN.md section 4.1 "fc1 in the tail").

The grid is sized for every K|V tile, every Q tile and every fc1 tile; the workgroups find their work from three device
counts (live row tiles and live rows of this pass, live rows of the previous one).  Enumerated here over every block of
the worst-case grid: every block is in exactly one section or none, each section's indices are a bijection onto
[0, wgs), the Q and fc1 sections start at multiples of 8 blocks (each section's XCD-aware walk takes the XCD from the
low three bits of the index inside the section), and the K|V and Q parts are those of xnrs_qkv_one_launch_map for the
same arguments."""
import ctypes
import itertools

import numpy as np
import pytest

from xnrs_amd import hip

Q_ROWS = 700     # the grid's worst case: token rows of the pass ...
F_ROWS = 650     # ... and of the previous one (the pass before a short last pass is the longer one)
Q_BM = 128
ROWS = (0, 1, 63, 64, 65, 127, 128, 129)


def enumerate_grid(kv_m_tiles, kv_cols, q_cols, f_bm, f_cols, live_tiles, live_rows, f_live):
    """(section, index) of every block of the worst-case grid, and the same from xnrs_qkv_one_launch_map."""
    l = hip.lib()
    sec, idx = ctypes.c_int32(), ctypes.c_int32()
    total = l.xnrs_qkv_fc1_launch_map(0, 0, 0, 0, kv_m_tiles, kv_cols, Q_ROWS, Q_BM, q_cols, F_ROWS, f_bm, f_cols, None, None)
    kv_pad = (kv_m_tiles * kv_cols + 7) // 8 * 8
    q_max = (Q_ROWS + Q_BM - 1) // Q_BM * q_cols
    assert total == (kv_pad + q_max + 7) // 8 * 8 + (F_ROWS + f_bm - 1) // f_bm * f_cols
    new = np.empty((total, 2), dtype=np.int64)
    old = np.empty((total, 2), dtype=np.int64)
    for b in range(total):
        assert l.xnrs_qkv_fc1_launch_map(b, live_tiles, live_rows, f_live, kv_m_tiles, kv_cols, Q_ROWS, Q_BM, q_cols, F_ROWS, f_bm,
                                         f_cols, ctypes.byref(sec), ctypes.byref(idx)) == total
        new[b] = sec.value, idx.value
        assert l.xnrs_qkv_one_launch_map(b, live_tiles, live_rows, kv_m_tiles, kv_cols, Q_ROWS, Q_BM, q_cols, ctypes.byref(sec),
                                         ctypes.byref(idx)) >= 0
        old[b] = sec.value, idx.value
    return new, old


@pytest.mark.parametrize("f_bm,f_cols", [(64, 4), (128, 4), (64, 2)])   # the three tile shapes of the third section at A = 256
@pytest.mark.parametrize("kv_cols,q_cols", [(12, 12), (18, 12)])
@pytest.mark.parametrize("kv_m_tiles", [0, 1, 5, 17])
def test_every_block_in_one_section_or_none(kv_m_tiles, kv_cols, q_cols, f_bm, f_cols):
    tiles = sorted({0, 1, kv_m_tiles, kv_m_tiles + 3})            # 0, 1, max, above max (clamped)
    rows = lambda cap: sorted(set(ROWS) | {cap, cap + 77})        # ... and the same for the two row counts
    combos = set(itertools.product(tiles, (0, 1, Q_ROWS, Q_ROWS + 77), rows(F_ROWS)))
    combos |= set(itertools.product(tiles, rows(Q_ROWS), (0, 1, F_ROWS, F_ROWS + 77)))
    for lt, lr, fl in sorted(combos):
        w, old = enumerate_grid(kv_m_tiles, kv_cols, q_cols, f_bm, f_cols, lt, lr, fl)
        what = (lt, lr, fl)
        assert np.isin(w[:, 0], (-1, 0, 1, 2)).all(), what          # one section or none (the rule is a function)
        kv, qq, ff = (w[w[:, 0] == s, 1] for s in (0, 1, 2))
        kv_wgs = min(lt, kv_m_tiles) * kv_cols
        q_wgs = (min(lr, Q_ROWS) + Q_BM - 1) // Q_BM * q_cols
        f_wgs = (min(fl, F_ROWS) + f_bm - 1) // f_bm * f_cols
        # each section: the indices 0 .. wgs-1 of its tile sequence, each once (blocks in ascending order)
        assert np.array_equal(kv, np.arange(kv_wgs)), what
        assert np.array_equal(qq, np.arange(q_wgs)), what
        assert np.array_equal(ff, np.arange(f_wgs)), what
        assert (w[:, 0] == -1).sum() == w.shape[0] - kv_wgs - q_wgs - f_wgs
        # the K|V and Q parts: xnrs_qkv_one_launch_map for the same arguments, block by block
        two = w[:, 0] != 2
        assert np.array_equal(w[two], old[two]), what
        assert (old[~two, 0] == -1).all(), what                     # ... which has nothing where the third section lies
        # the sections start at multiples of 8 and keep the XCD of the hardware's round-robin in their own index
        for ind, sec in ((qq, 1), (ff, 2)):
            if ind.size:
                first = int(np.flatnonzero(w[:, 0] == sec)[0])
                assert first % 8 == 0, what
                assert (w[first:first + ind.size, 0] == sec).all(), what
                assert ((first + np.arange(ind.size)) & 7 == ind & 7).all(), what
        if ff.size:
            first = int(np.flatnonzero(w[:, 0] == 2)[0])
            assert first == ((kv_wgs + 7) // 8 * 8 + q_wgs + 7) // 8 * 8, what


def test_counts_zero_negative_and_outside_blocks():
    l = hip.lib()
    w, _ = enumerate_grid(5, 12, 12, 64, 4, 0, 0, 0)
    assert (w[:, 0] == -1).all()
    w, _ = enumerate_grid(5, 12, 12, 64, 4, -3, -1, -9)
    assert (w[:, 0] == -1).all()
    a, _ = enumerate_grid(5, 12, 12, 64, 4, 9, Q_ROWS + 1000, F_ROWS + 1000)
    b, _ = enumerate_grid(5, 12, 12, 64, 4, 5, Q_ROWS, F_ROWS)
    assert np.array_equal(a, b)
    sec, idx = ctypes.c_int32(), ctypes.c_int32()
    total = a.shape[0]
    for blk in (-1, total, total + 8):
        l.xnrs_qkv_fc1_launch_map(blk, 5, Q_ROWS, F_ROWS, 5, 12, Q_ROWS, Q_BM, 12, F_ROWS, 64, 4, ctypes.byref(sec), ctypes.byref(idx))
        assert sec.value == -1
    # an empty third section (the first pass of a call): the grid and the rule of the two-section launch, rounded up to 8
    n = l.xnrs_qkv_fc1_launch_map(0, 0, 0, 0, 5, 12, Q_ROWS, Q_BM, 12, 0, 64, 4, None, None)
    assert n == (l.xnrs_qkv_one_launch_map(0, 0, 0, 5, 12, Q_ROWS, Q_BM, 12, None, None) + 7) // 8 * 8


def test_bad_shapes_are_refused():
    l = hip.lib()
    einval = hip.parse_header(open(hip.HEADER_PATH).read())[0]["EINVAL"]
    assert l.xnrs_qkv_fc1_launch_map(0, 0, 0, 0, 4, 6, 100, 128, 6, 100, 0, 4, None, None) == einval
    assert l.xnrs_qkv_fc1_launch_map(0, 0, 0, 0, 4, 6, 100, 128, 6, 100, 64, 0, None, None) == einval
    assert l.xnrs_qkv_fc1_launch_map(0, 0, 0, 0, 4, 6, 100, 128, 6, -1, 64, 4, None, None) == einval
    assert l.xnrs_qkv_fc1_launch_map(0, 0, 0, 0, 4, 0, 100, 128, 6, 100, 64, 4, None, None) == einval
    assert l.xnrs_qkv_fc1_launch_map(0, 0, 0, 0, 0, 6, 0, 128, 6, 0, 64, 4, None, None) == 0


def test_counter_reads_and_resets():
    l = hip.lib()
    l.xnrs_fc1_in_tail_count(1)
    assert l.xnrs_fc1_in_tail_count(0) == 0
    assert l.xnrs_fc1_in_tail_count(1) == 0
