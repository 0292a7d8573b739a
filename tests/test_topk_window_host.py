"""CPU: the host side of the row windows (include/xnrs_hip.h: xnrs_topk_deep*_win / xnrs_rank*_win): evaluation.row_windows
against a NumPy searchsorted restatement, Behaviors.time, the six prototypes as hip.parse_header reads them, their refusals
before any launch, and how recommend / rank_clicked hand the windows of a batch's sessions to a scorer (stand-ins: no
device is touched)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from xnrs_amd import evaluation as EV
from xnrs_amd import hip, synth
from xnrs_amd.data import Behaviors

EINVAL = -1
PARENTS = {"xnrs_topk_deep_win": "xnrs_topk_deep", "xnrs_topk_deep_bilinear_win": "xnrs_topk_deep_bilinear",
           "xnrs_topk_deep_mlp_win": "xnrs_topk_deep_mlp", "xnrs_rank_win": "xnrs_rank",
           "xnrs_rank_bilinear_win": "xnrs_rank_bilinear", "xnrs_rank_mlp_win": "xnrs_rank_mlp"}


# ------------------------------------------------------------------------------------------- row_windows
def np_windows(row_time, t, horizon):
    hi = np.searchsorted(row_time, t, side="right")
    lo = np.zeros_like(hi) if horizon is None else np.searchsorted(row_time, t - horizon, side="left")
    return lo.astype(np.int32), hi.astype(np.int32)


@pytest.mark.parametrize("horizon", [None, 0, 3, 100])
def test_row_windows_against_numpy_searchsorted(horizon):
    row_time = np.array([5, 5, 5, 7, 8, 8, 12, 12, 12, 12, 20], dtype=np.int64)  # ties
    t = np.array([4, 5, 6, 7, 8, 11, 12, 19, 20, 21, -50, 1000, 8, 8], dtype=np.int64)  # before the first, after the last row
    lo, hi = EV.row_windows(torch.from_numpy(row_time), torch.from_numpy(t), horizon)
    want = np_windows(row_time, t, horizon)
    assert lo.dtype == torch.int32 and hi.dtype == torch.int32 and lo.device == hi.device == torch.device("cpu")
    assert lo.numpy().tolist() == want[0].tolist() and hi.numpy().tolist() == want[1].tolist()
    # what the two bounds mean, said directly
    for i, ti in enumerate(t.tolist()):
        seen = [n for n, rt in enumerate(row_time.tolist()) if rt <= ti and (horizon is None or rt >= ti - horizon)]
        assert list(range(int(lo[i]), int(hi[i]))) == seen
    if horizon is None:
        assert (lo == 0).all()
    assert int(hi[0]) == 0 and int(hi[11]) == row_time.size  # before the first row: nothing; after the last: everything


def test_row_windows_on_random_times_and_the_refusals():
    rng = synth.rng_for(31)
    row_time = np.sort(rng.integers(0, 50, size=300)).astype(np.int64)
    t = rng.integers(-5, 60, size=64).astype(np.int64)
    for horizon in (None, 7):
        lo, hi = EV.row_windows(torch.from_numpy(row_time), torch.from_numpy(t), horizon)
        want = np_windows(row_time, t, horizon)
        assert np.array_equal(lo.numpy(), want[0]) and np.array_equal(hi.numpy(), want[1])
    bad = row_time.copy()
    bad[100], bad[101] = 40, 3
    with pytest.raises(ValueError, match="decreases"):
        EV.row_windows(torch.from_numpy(bad), torch.from_numpy(t))
    with pytest.raises(ValueError, match="1-D"):
        EV.row_windows(torch.from_numpy(row_time).reshape(2, -1), torch.from_numpy(t))
    lo, hi = EV.row_windows(torch.zeros(0, dtype=torch.int64), torch.from_numpy(t))  # an empty table
    assert (lo == 0).all() and (hi == 0).all()


# ------------------------------------------------------------------------------------------- Behaviors.time
def test_behaviors_keep_the_time_when_every_session_has_one():
    store, _ = synth.click_world(n_news=20, n_sess=5)  # (its ids are the rows 1 .. 20)
    sessions = [{"history": [i + 1, i + 2, i + 3], "positives": [i + 4], "negatives": [i + 5, i + 6]} for i in range(4)]
    b = Behaviors.from_sessions([dict(s, time=100 + 3 * i) for i, s in enumerate(sessions)], store)
    assert b.time.dtype == torch.int64 and b.time.tolist() == [100, 103, 106, 109]
    assert b.to("cpu").time.tolist() == b.time.tolist()
    assert not hasattr(Behaviors.from_sessions(sessions, store), "time")
    assert not hasattr(Behaviors.from_sessions([dict(s, time=7) for s in sessions[:-1]] + [sessions[-1]], store), "time")
    assert not hasattr(Behaviors.from_sessions([dict(s, time="11/15/2019") for s in sessions], store), "time")  # not an integer
    assert not hasattr(Behaviors.from_sessions(sessions, store).to("cpu"), "time")


# ------------------------------------------------------------------------------------------- the header and the C ABI
def test_the_six_entry_points_parse_out_of_the_header():
    with open(hip.HEADER_PATH) as f:
        consts, _, protos = hip.parse_header(f.read())
    assert consts["ABI_VERSION"] == 6
    counts = {"xnrs_topk_deep_win": 16, "xnrs_topk_deep_bilinear_win": 18, "xnrs_topk_deep_mlp_win": 21,
              "xnrs_rank_win": 17, "xnrs_rank_bilinear_win": 19, "xnrs_rank_mlp_win": 22}
    for name, n in counts.items():
        restype, args = protos[name]
        p_res, p_args = protos[PARENTS[name]]
        assert restype is ctypes.c_int32 and len(args) == n == len(p_args) + 2, name
        # the parent's list with two pointers behind excl_rows (the last pointer pair before pad_row)
        at = len(p_args) - (6 if "topk" in name else 5) - 1  # ..., excl_rows | pad_row, [k,] out, out, ws, ws_bytes, stream
        assert args[:at] == p_args[:at] and args[at + 2:] == p_args[at:], name
        assert args[at] is ctypes.c_void_p and args[at + 1] is ctypes.c_void_p and p_args[at] is ctypes.c_int32, name
        assert name in hip.SYMBOLS and hasattr(hip.lib(), name)
    assert hip.lib().xnrs_abi_version() == 6


def test_one_null_window_pointer_is_refused_on_the_host():
    l = hip.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 30
    for lo, hi in ((p, None), (None, p)):
        assert l.xnrs_topk_deep_win(p, 1000, 8, p, 3, None, None, lo, hi, -1, 10, p, p, p, big, None) == EINVAL
        assert l.xnrs_topk_deep_bilinear_win(p, 1000, 8, p, 3, p, p, None, None, lo, hi, -1, 300, p, p, p, big, None) == EINVAL
        assert l.xnrs_topk_deep_mlp_win(p, 1000, 8, 8, p, 3, p, p, p, p, None, None, lo, hi, -1, 10, p, p, p, big, None) == EINVAL
        assert l.xnrs_rank_win(p, 1000, 8, p, 3, p, p, None, None, lo, hi, -1, p, p, None, 0, None) == EINVAL
        assert l.xnrs_rank_bilinear_win(p, 1000, 8, p, 3, p, p, p, p, None, None, lo, hi, -1, p, p, p, big, None) == EINVAL
        assert l.xnrs_rank_mlp_win(p, 1000, 8, 8, p, 3, p, p, p, p, p, p, None, None, lo, hi, -1, p, p, p, big, None) == EINVAL
        # ... also for an empty batch: the pair is wrong whatever B is
        assert l.xnrs_topk_deep_win(None, 1000, 8, None, 0, None, None, lo, hi, -1, 10, None, None, None, 0, None) == EINVAL
    # the parents' refusals hold (k, the table size), and B == 0 with both or neither pointer is nothing to do
    assert l.xnrs_topk_deep_win(p, 1000, 8, p, 3, None, None, p, p, -1, 1025, p, p, p, big, None) == EINVAL
    assert l.xnrs_rank_win(p, 2 ** 31, 8, p, 3, p, p, None, None, p, p, -1, p, p, None, 0, None) == EINVAL
    assert l.xnrs_topk_deep_win(None, 1000, 8, None, 0, None, None, p, p, -1, 10, None, None, None, 0, None) == 0
    assert l.xnrs_rank_win(None, 1000, 8, None, 0, None, None, None, None, None, None, -1, None, None, None, 0, None) == 0
    assert buf.raw == bytes(64)


# ------------------------------------------------------------------------------------------- recommend / rank_clicked
class _Batcher:
    def __init__(self, behaviors, l_hist, pad_row):
        self.l_hist = l_hist

    def eval_batch(self, sess):
        return (torch.zeros((sess.numel(), self.l_hist), dtype=torch.int32),)


class _Model(torch.nn.Module):
    def __init__(self, scorer):
        super().__init__()
        self.rec_model = scorer

    def encode_user(self, h, m):
        return h.sum(1)


class OldScorer(torch.nn.Module):
    """The scorer surface as it stood before the windows: positional arguments only, no new keyword accepted."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def prepare_csr(self, vecs):
        return vecs

    def topk(self, table, u, k, excl_off=None, excl_rows=None, pad_row=-1):
        self.calls.append(("topk", u.shape[0], {}))
        return torch.zeros((u.shape[0], k), dtype=torch.int32), torch.zeros((u.shape[0], k))

    def topk_deep(self, table, u, k, excl_off=None, excl_rows=None, pad_row=-1):
        self.calls.append(("topk_deep", u.shape[0], {}))
        return torch.zeros((u.shape[0], k), dtype=torch.int32), torch.zeros((u.shape[0], k))

    def rank(self, table, u, tgt_off, tgt_rows, excl_off=None, excl_rows=None, pad_row=-1, out=None):
        self.calls.append(("rank", u.shape[0], {}))
        n = tgt_rows.numel()
        return torch.zeros(n, dtype=torch.int32), torch.zeros(n)


class NewScorer(OldScorer):
    def topk_deep(self, table, u, k, excl_off=None, excl_rows=None, pad_row=-1, win_lo=None, win_hi=None):
        self.calls.append(("topk_deep", u.shape[0], {"win_lo": win_lo, "win_hi": win_hi}))
        return torch.zeros((u.shape[0], k), dtype=torch.int32), torch.zeros((u.shape[0], k))

    def rank(self, table, u, tgt_off, tgt_rows, excl_off=None, excl_rows=None, pad_row=-1, out=None, win_lo=None, win_hi=None):
        self.calls.append(("rank", u.shape[0], {"win_lo": win_lo, "win_hi": win_hi}))
        n = tgt_rows.numel()
        return torch.zeros(n, dtype=torch.int32), torch.zeros(n)


@pytest.fixture
def world(monkeypatch):
    store, beh = synth.click_world(n_news=20, n_sess=11)
    monkeypatch.setattr(EV, "DeviceBatcher", _Batcher)
    monkeypatch.setattr(EV, "encode_news_table", lambda model, store: (torch.ones((store.n_rows, 4)), torch.ones((store.n_rows, 1))))
    return store, beh


def test_without_windows_the_scorer_is_called_as_before(world):
    store, beh = world
    old = OldScorer()
    rows, _ = EV.recommend(_Model(old), store, beh, l_hist=3, k=5, batch=4)
    assert rows.shape == (11, 5) and [c[:2] for c in old.calls] == [("topk", 4), ("topk", 4), ("topk", 3)]
    old.calls.clear()
    EV.recommend(_Model(old), store, beh, l_hist=3, k=200, batch=8)
    assert [c[:2] for c in old.calls] == [("topk_deep", 8), ("topk_deep", 3)]
    old.calls.clear()
    EV.rank_clicked(_Model(old), store, beh, l_hist=3, batch=4)
    EV.rank_clicked(_Model(old), store, beh, l_hist=3, sessions=[3, 1, 7], batch=2)
    EV.evaluate_full_ranking(_Model(old), store, beh, l_hist=3, batch=11)
    assert [c[:2] for c in old.calls] == [("rank", 4), ("rank", 4), ("rank", 3), ("rank", 2), ("rank", 1), ("rank", 11)]


def test_with_windows_the_scorer_gets_the_batch_slices(world):
    store, beh = world
    n = len(beh)
    lo, hi = torch.arange(n, dtype=torch.int64), torch.arange(n, dtype=torch.int64) + 5
    new = NewScorer()

    def windows_of(calls, name):
        got = [c[2] for c in calls if c[0] == name]
        for w in got:
            assert w["win_lo"].dtype == torch.int32 and w["win_hi"].dtype == torch.int32 and w["win_lo"].is_contiguous()
        return [w["win_lo"].tolist() for w in got], [w["win_hi"].tolist() for w in got]

    # every k goes through topk_deep; the windows follow the sessions of the batch
    EV.recommend(_Model(new), store, beh, l_hist=3, k=5, batch=4, windows=(lo, hi))
    assert not [c for c in new.calls if c[0] == "topk"]
    assert windows_of(new.calls, "topk_deep") == ([[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]], [[5, 6, 7, 8], [9, 10, 11, 12], [13, 14, 15]])
    new.calls.clear()
    EV.recommend(_Model(new), store, beh, l_hist=3, k=5, sessions=[9, 2, 4], batch=2, windows=(lo, hi))
    assert windows_of(new.calls, "topk_deep") == ([[9, 2], [4]], [[14, 7], [9]])
    new.calls.clear()
    # rank_clicked: the contiguous fast path (sessions None / a range) and the gathering one
    EV.rank_clicked(_Model(new), store, beh, l_hist=3, batch=4, windows=(lo, hi))
    EV.rank_clicked(_Model(new), store, beh, l_hist=3, sessions=range(2, 9), batch=5, windows=(lo, hi))
    EV.rank_clicked(_Model(new), store, beh, l_hist=3, sessions=[10, 0, 6], batch=2, windows=(lo, hi))
    assert windows_of(new.calls, "rank")[0] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10], [2, 3, 4, 5, 6], [7, 8], [10, 0], [6]]
    assert windows_of(new.calls, "rank")[1][-2:] == [[15, 5], [11]]
    new.calls.clear()
    EV.evaluate_full_ranking(_Model(new), store, beh, l_hist=3, batch=6, windows=(lo.int(), hi.int()))
    assert windows_of(new.calls, "rank")[0] == [[0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10]]


def test_windows_are_refused_by_a_scorer_without_the_keywords_before_anything_is_encoded(world, monkeypatch):
    store, beh = world

    def no_encoding(model, store):
        raise AssertionError("refused before anything is encoded")
    monkeypatch.setattr(EV, "encode_news_table", no_encoding)
    n = len(beh)
    w = (torch.zeros(n, dtype=torch.int64), torch.full((n,), 9, dtype=torch.int64))
    old = _Model(OldScorer())
    for k in (5, 200):
        with pytest.raises(NotImplementedError, match="OldScorer.*windows"):
            EV.recommend(old, store, beh, l_hist=3, k=k, windows=w)
    with pytest.raises(NotImplementedError, match="OldScorer.*windows"):
        EV.rank_clicked(old, store, beh, l_hist=3, windows=w)
    with pytest.raises(NotImplementedError, match="OldScorer.*windows"):
        EV.evaluate_full_ranking(old, store, beh, l_hist=3, windows=w)
    assert not old.rec_model.calls
    # the windows themselves: a pair of integer tensors, one entry per session
    new = _Model(NewScorer())
    for bad in ((w[0],), (w[0][:-1], w[1][:-1]), (w[0].float(), w[1].float()), 5):
        with pytest.raises(ValueError, match="windows"):
            EV.recommend(new, store, beh, l_hist=3, k=5, windows=bad)
        with pytest.raises(ValueError, match="windows"):
            EV.rank_clicked(new, store, beh, l_hist=3, windows=bad)


def test_the_scorers_take_the_windows_as_keywords():
    from xnrs_amd import ops
    from xnrs_amd.models.blocks import BilinScoring, DotScoring, FCScoring
    for cls in (DotScoring, BilinScoring, FCScoring):
        for name in ("topk", "topk_deep", "rank"):
            params = inspect.signature(getattr(cls, name)).parameters
            assert params["win_lo"].default is None and params["win_hi"].default is None, (cls, name)
    for fn in (ops.topk_deep_dot, ops.topk_deep_bilinear, ops.topk_deep_mlp, ops.rank_dot, ops.rank_bilinear, ops.rank_mlp):
        params = inspect.signature(fn).parameters
        assert params["win_lo"].default is None and params["win_hi"].default is None, fn
    # one bound without the other, a wrong dtype, a wrong length: refused before the call (no device is reached)
    t = torch.zeros((10, 4))
    u = torch.zeros((3, 4))
    ok = torch.zeros(3, dtype=torch.int32)
    for lo, hi in ((ok, None), (None, ok), (ok.long(), ok.long()), (ok[:2], ok[:2]), (ok.float(), ok)):
        with pytest.raises(ValueError, match="windows"):
            ops._windows(lo, hi, 3, t.device)
    assert ops._windows(None, None, 3, t.device) == ()
    del u
