"""CPU: the rank reference on a hand-written case, the pure host calls of the rank C ABI (workspace size, refusals before any
launch), the Python surface that needs no device, and the arithmetic of the full-ranking metrics."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.rank_ref import rank_reference
from xnrs_amd import hip

EINVAL, EWORKSPACE = -1, -3


def test_reference_on_a_hand_written_case():
    nan, inf = float("nan"), float("inf")
    #                 0    1    2     3    4     5     6
    s = np.array([[1.0, 3.0, 3.0, nan, -inf, -0.0, 0.0],
                  [2.0, 2.0, nan, nan, 2.0, -inf, 5.0]], dtype=np.float32)
    # the top-k order of this matrix is [1, 2, 0, 5, 6, 4] / [6, 0, 1, 4, 5] (tests/test_topk_host.py)
    r, sc = rank_reference(s, [[1, 2, 0, 5, 6, 4, 3], [6, 0, 1, 4, 5, 2]])
    assert r.tolist() == [0, 1, 2, 3, 4, 5, -1, 0, 1, 2, 3, 4, -1]  # ties by row; -0 == +0; -inf last; NaN: no answer
    assert sc.dtype == np.float32 and sc[:6].tolist() == [3.0, 3.0, 1.0, -0.0, 0.0, -inf] and np.isnan(sc[6]) and np.isnan(sc[-1])
    # outside the table, a duplicate, a user without a target
    r, sc = rank_reference(s, [[7, -1, 2, 2], []])
    assert r.tolist() == [-1, -1, 1, 1] and np.isnan(sc[:2]).all()
    # the pad row and the exclusions (duplicates, foreign ids) leave the count; the pad row as a target has no answer
    r, _ = rank_reference(s, [[0, 5, 6, 2], [1, 4, 5]], excl=[[1, 1, 99, -4], [6, 0]], pad_row=2)
    assert r.tolist() == [0, 1, 2, -1, 0, 1, 2]
    # a target on its own list is ranked among the others; a list of everything leaves rank 0
    r, sc = rank_reference(s, [[0, 1], [4]], excl=[[0, 1], range(7)])
    assert r.tolist() == [1, 0, 0] and sc.tolist() == [1.0, 3.0, 2.0]


def test_workspace_is_a_pure_host_call():
    l = hip.lib()
    w = l.xnrs_rank_workspace_bytes
    assert w(4096, 0) == 0 and w(0, 256) == 0 and w(-1, 8) == 0  # the dot form needs none
    for B, width in ((1, 8), (3, 70), (4096, 256), (64, 128)):
        assert B * width * 4 <= w(B, width) < B * width * 4 + 256  # the projected user side, nothing else
    assert w(4096, 256) == 4096 * 256 * 4


def _buf():
    b = ctypes.create_string_buffer(64)
    return b, ctypes.cast(b, ctypes.c_void_p)


@pytest.mark.parametrize("n_rows,E,B,outputs", [(1000, 8, 3, False), (-1, 8, 3, True), (2 ** 31, 8, 3, True), (1000, 0, 3, True),
                                                (1000, -2, 3, True), (1000, 8, -1, True)])
def test_refusals_need_no_device(n_rows, E, B, outputs):
    """Argument errors are found on the host before any launch: null device pointers never reach a kernel."""
    l = hip.lib()
    buf, p = _buf()
    out = p if outputs else None
    assert l.xnrs_rank(p, n_rows, E, p, B, p, p, None, None, -1, out, out, None, 0, None) == EINVAL
    assert l.xnrs_rank_bilinear(p, n_rows, E, p, B, p, p, p, p, None, None, -1, out, out, p, 1 << 30, None) == EINVAL
    assert l.xnrs_rank_mlp(p, n_rows, E, max(E, 1), p, B, p, p, p, p, p, p, None, None, -1, out, out, p, 1 << 30, None) == EINVAL
    assert buf.raw == bytes(64)


def test_more_refusals_and_the_empty_batch():
    l = hip.lib()
    buf, p = _buf()
    assert l.xnrs_rank(p, 1000, 8, p, 3, None, p, None, None, -1, p, p, None, 0, None) == EINVAL  # no target offsets
    assert l.xnrs_rank(p, 1000, 8, p, 3, p, None, None, None, -1, p, p, None, 0, None) == EINVAL  # no target rows
    assert l.xnrs_rank(p, 1000, 8, None, 3, p, p, None, None, -1, p, p, None, 0, None) == EINVAL  # no users
    assert l.xnrs_rank(None, 1000, 8, p, 3, p, p, None, None, -1, p, p, None, 0, None) == EINVAL  # no table
    assert l.xnrs_rank(p, 1000, 8, p, 3, p, p, p, None, -1, p, p, None, 0, None) == EINVAL  # excl_off without excl_rows
    assert l.xnrs_rank_mlp(p, 1000, 8, 0, p, 3, p, p, p, p, p, p, None, None, -1, p, p, p, 1 << 30, None) == EINVAL  # H == 0
    # B == 0: nothing to do, whatever else is missing
    assert l.xnrs_rank(None, 1000, 8, None, 0, None, None, None, None, -1, None, None, None, 0, None) == 0
    assert l.xnrs_rank_bilinear(None, 1000, 8, None, 0, None, None, None, None, None, None, -1, None, None, None, 0, None) == 0
    assert l.xnrs_rank_mlp(None, 1000, 8, 4, None, 0, None, None, None, None, None, None, None, None, -1, None, None, None, 0,
                           None) == 0
    # valid arguments, a short or missing workspace: refused on the host as well (the pointers are never dereferenced there)
    need = l.xnrs_rank_workspace_bytes(3, 8)
    assert l.xnrs_rank_bilinear(p, 1000, 8, p, 3, p, p, p, p, None, None, -1, p, p, None, 0, None) == EWORKSPACE
    assert l.xnrs_rank_bilinear(p, 1000, 8, p, 3, p, p, p, p, None, None, -1, p, p, p, need - 1, None) == EWORKSPACE
    assert l.xnrs_rank_mlp(p, 1000, 8, 8, p, 3, p, p, p, p, p, p, None, None, -1, p, p, p, need - 1, None) == EWORKSPACE
    assert buf.raw == bytes(64)


class _Model(torch.nn.Module):
    def __init__(self, scorer):
        super().__init__()
        self.rec_model = scorer

    def encode_news_ids(self, store, ids):
        raise AssertionError("refused before anything is encoded")


def test_scorers_have_rank_and_the_evaluation_refuses_what_it_cannot_rank():
    from xnrs_amd import evaluation as EV
    from xnrs_amd import synth
    from xnrs_amd.models.blocks import BilinScoring, DotScoring, FCScoring
    from xnrs_amd.models.caum import CAUMScoring
    for cls in (DotScoring, BilinScoring, FCScoring):
        assert callable(getattr(cls, "rank"))
    assert CAUMScoring.rank is None

    class Cosine(torch.nn.Module):
        pass

    class TopkOnly(DotScoring):
        rank = None
    store, beh = synth.click_world(n_news=20, n_sess=5)
    npa_like = _Model(DotScoring())
    npa_like.user_dependent_news = True
    lstur_like = _Model(DotScoring())
    lstur_like.uses_user_index = True
    assert not hasattr(beh, "user_index")
    for fn in (lambda m: EV.evaluate_full_ranking(m, store, beh, l_hist=8), lambda m: EV.rank_clicked(m, store, beh, l_hist=8)):
        with pytest.raises(NotImplementedError, match="Cosine"):
            fn(_Model(Cosine()))
        with pytest.raises(NotImplementedError, match="TopkOnly"):
            fn(_Model(TopkOnly()))
        with pytest.raises(NotImplementedError, match="CAUMScoring"):
            fn(_Model(CAUMScoring()))
        with pytest.raises(NotImplementedError, match="depend on the user"):
            fn(npa_like)
        with pytest.raises(ValueError, match="user index"):
            fn(lstur_like)
    with pytest.raises(RuntimeError, match="process group"):
        EV.evaluate_full_ranking(_Model(DotScoring()), store, beh, l_hist=8, distributed=True)


def test_metric_arithmetic_on_a_hand_made_rank_vector():
    from xnrs_amd import evaluation as EV
    ranks = torch.tensor([0, 4, -1, 5, 9, 10, 99, -1, 100, 2], dtype=torch.int32)
    ks = (5, 10, 100)
    sums = EV.full_ranking_sums(ranks, ks)
    assert sums.dtype == torch.float64
    got = EV.full_ranking_metrics(sums, ks)
    valid = [0, 4, 5, 9, 10, 99, 100, 2]
    want = {"n_queries": 8, "mrr": sum(1 / (1 + r) for r in valid) / 8, "mean_rank": sum(valid) / 8}
    for k in ks:
        want[f"hit@{k}"] = sum(r < k for r in valid) / 8
        want[f"ndcg@{k}"] = sum(1 / math.log2(2 + r) for r in valid if r < k) / 8
    assert set(got) == set(want) and got["n_queries"] == 8 and isinstance(got["n_queries"], int)
    for key, v in want.items():
        assert got[key] == pytest.approx(v, rel=1e-14, abs=0), key
    assert got["hit@5"] == 3 / 8 and got["hit@10"] == 5 / 8 and got["hit@100"] == 7 / 8
    # sums of shards add up to the sums of the whole; no query at all: zeros, not a division by zero
    both = EV.full_ranking_sums(ranks[:4], ks) + EV.full_ranking_sums(ranks[4:], ks)
    assert torch.allclose(both, sums, rtol=1e-15, atol=0)
    empty = EV.full_ranking_metrics(EV.full_ranking_sums(torch.tensor([-1, -1], dtype=torch.int32), ks), ks)
    assert empty["n_queries"] == 0 and empty["mrr"] == 0.0 and empty["hit@5"] == 0.0
