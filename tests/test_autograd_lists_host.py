"""CPU: the row-list record of the training path (autograd._Rows) -- what autograd._host_lists puts into it, against a plain
double loop over the mask, and the hip.RowLists struct the record makes of itself for a call."""
import types

import pytest
import torch

from xnrs_amd import autograd as AG
from xnrs_amd import hip

N, L, N_TAB = 5, 7, 9
IDS = [3, 0, 8, 3, 1]
FIELDS = ("live", "live_src", "n_live", "kv", "kv_src", "n_kv", "counts")


def _table_mask():
    """(9, 7) mask: row 3 all zero, every other row with 1 to 3 live tokens at places that vary with the row."""
    m = torch.zeros(N_TAB, L)
    for r in range(N_TAB):
        if r != 3:
            for t in range(L):
                m[r, t] = float((r * 5 + t * 3) % 7 < 1 + r % 3)
    assert m[3].sum() == 0 and all(m[r].sum() > 0 for r in range(N_TAB) if r != 3)
    return m


def _cfg(n_heads):
    return types.SimpleNamespace(n_seq=N, L=L, n_heads=n_heads)


def _loops(m, ids):
    """-> (live, live_src, kv, kv_src) as Python lists: token rows of the call in order, and where each lies in the table."""
    src = ids if ids is not None else list(range(N))
    live, live_src, kv, kv_src = [], [], [], []
    for i in range(N):
        for t in range(L):
            if m[src[i], t] != 0:
                live.append(i * L + t)
                live_src.append(src[i] * L + t)
        if any(m[src[i], t] != 0 for t in range(L)):
            for t in range(L):
                kv.append(i * L + t)
                kv_src.append(src[i] * L + t)
    return live, live_src, kv, kv_src


def _as_list(t):
    assert t.dtype == torch.int32
    return t.tolist()


def test_host_lists_with_ids_equal_a_double_loop():
    m = _table_mask()
    before = dict(AG.STATS)
    r = AG._host_lists(_cfg(2), m, torch.tensor(IDS, dtype=torch.int32), torch.device("cpu"))
    live, live_src, kv, kv_src = _loops(m, IDS)
    assert len(kv) == 3 * L  # the two slots of the empty row 3 are left out
    assert _as_list(r.live) == live and _as_list(r.live_src) == live_src
    assert _as_list(r.kv) == kv and _as_list(r.kv_src) == kv_src
    assert (r.n_live, r.n_kv) == (len(live), len(kv))
    assert r.counts is None
    assert AG.STATS["live_row_forwards"] == before["live_row_forwards"] + 1
    assert AG.STATS["kv_row_forwards"] == before["kv_row_forwards"] + 1


def test_host_lists_without_ids_have_no_source_lists():
    m = _table_mask()[[3, 0, 8, 3, 1]].contiguous()
    r = AG._host_lists(_cfg(2), m, None, torch.device("cpu"))
    live, _, kv, _ = _loops(m, None)
    assert _as_list(r.live) == live and _as_list(r.kv) == kv
    assert (r.n_live, r.n_kv) == (len(live), len(kv))
    assert r.live_src is None and r.kv_src is None


def test_host_lists_without_attention_have_no_kv_list():
    m = _table_mask()
    before = AG.STATS["kv_row_forwards"]
    r = AG._host_lists(_cfg(0), m, torch.tensor(IDS, dtype=torch.int32), torch.device("cpu"))
    live, live_src, _, _ = _loops(m, IDS)
    assert _as_list(r.live) == live and _as_list(r.live_src) == live_src and r.n_live == len(live)
    assert r.kv is None and r.kv_src is None and r.n_kv == 0
    assert AG.STATS["kv_row_forwards"] == before


def test_host_lists_above_the_live_fraction_are_an_empty_record():
    m = torch.ones(N, L)
    m[1, 2] = 0  # 34 of 35 rows live
    assert m.sum().item() > AG.LIVE_ROWS_MAX_FRACTION * N * L
    before = AG.STATS["live_row_forwards"]
    r = AG._host_lists(_cfg(2), m, None, torch.device("cpu"))
    assert [getattr(r, f) for f in FIELDS] == [None, None, 0, None, None, 0, None]
    assert AG.STATS["live_row_forwards"] == before


def test_empty_record_with_nothing_to_say_makes_no_struct():
    assert AG._Rows().struct(None, None, hip.DQKV_OWN) is None


@pytest.mark.parametrize("empty", [False, True])
def test_record_struct_carries_its_fields(empty):
    t = [torch.arange(4, dtype=torch.int32) + 10 * i for i in range(4)]
    counts = torch.zeros(2, dtype=torch.int64)
    image = torch.zeros(3, 6)
    r = AG._Rows() if empty else AG._Rows(t[0], t[1], 3, t[2], t[3], 4, counts)
    s = r.struct(0x1000, image, hip.DQKV_MERGE)
    assert isinstance(s, hip.RowLists)
    want = [None, None, 0, None, None, 0] if empty else [t[0].data_ptr(), t[1].data_ptr(), 3, t[2].data_ptr(), t[3].data_ptr(), 4]
    want += [0x1000, None if empty else counts.data_ptr(), image.data_ptr(), hip.DQKV_MERGE]
    assert [getattr(s, name) for name, _ in hip.RowLists._fields_] == want
    if not empty:  # lists alone are something to pass
        assert isinstance(r.struct(None, None, hip.DQKV_OWN), hip.RowLists)
    assert isinstance(AG._Rows().struct(None, image, hip.DQKV_DEFER), hip.RowLists)
