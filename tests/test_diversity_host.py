"""CPU: the host side of the diversity path (include/xnrs_hip.h: xnrs_row_inv_norms, xnrs_mmr_rerank, xnrs_list_diversity) --
the fp64 reference (tests/diversity_ref.py) against hand-worked cases, the refusals of the entry points before any launch, and
the refusals of evaluation.recommend_diverse / evaluate_diversity before anything is encoded."""
import ctypes

import numpy as np
import pytest
import torch

from tests import diversity_ref as R
from xnrs_amd import hip

EINVAL = -1


def test_the_constants_and_the_version():
    c = hip._CONSTANTS
    assert (c["MMR_REL_RAW"], c["MMR_REL_MINMAX"]) == (0, 1)
    assert c["DIVERSITY_MAX_E"] == 4096 and c["DIVERSITY_MAX_CATEGORIES"] == 4096
    assert c["ABI_VERSION"] == 6
    for name in ("xnrs_row_inv_norms", "xnrs_mmr_rerank", "xnrs_list_diversity"):
        assert name in hip.SYMBOLS and hasattr(hip.lib(), name)


# ------------------------------------------------------------------------------------------------ the reference, by hand
# four news in the plane: a and b point the same way, c is orthogonal to them, d is opposite to a
TABLE = np.array([[1, 0], [2, 0], [0, 3], [-1, 0], [0, 0]], dtype=np.float32)


def test_reference_cosines_and_norms():
    assert R.inv_norms(TABLE).tolist() == [1.0, 0.5, 1.0 / 3.0, 1.0, 0.0]
    cos = R._cosines(TABLE, np.arange(5), np.ones(5, dtype=bool))
    assert cos[0, 1] == 1.0 and cos[0, 2] == 0.0 and cos[0, 3] == -1.0 and cos[4].tolist() == [0.0] * 5  # a zero row: 0, no NaN


def test_reference_mmr_on_a_four_news_pool():
    rows = np.array([[0, 1, 2, 3]], dtype=np.int32)
    scores = np.array([[4.0, 3.0, 2.0, 0.0]], dtype=np.float32)
    # raw, lam = 1/2.  step 0: objectives 2, 1.5, 1, 0 -> place 0.  step 1: m = cos(., a) = (-, 1, 0, -1): 1.5 - 0.5 = 1,
    # 1 - 0 = 1, 0 + 0.5 = 0.5 -> the tie of places 1 and 2 goes to place 1.  step 2: m = max(cos a, cos b) = (-, -, 0, -1):
    # 1 and 0.5 -> place 2.  step 3: place 3.
    r, s, p = R.mmr(TABLE, rows, scores, 4, 0.5, "raw")
    assert p.tolist() == [[0, 1, 2, 3]] and r.tolist() == [[0, 1, 2, 3]] and s.tolist() == [[4.0, 3.0, 2.0, 0.0]]
    # lam = 1/4: step 1: 0.75 - 0.75 = 0, 0.5 - 0 = 0.5, 0 + 0.75 = 0.75 -> place 3 (the opposite news); step 2: m = (-, 1, 0, -):
    # 0 and 0.5 -> place 2; then place 1
    assert R.mmr(TABLE, rows, scores, 4, 0.25, "raw")[2].tolist() == [[0, 3, 2, 1]]
    # minmax: r = (1, 3/4, 1/2, 0); lam = 1/2: step 1: 3/8 - 1/2, 1/4 - 0, 0 + 1/2 -> place 3; step 2: -1/8, 1/4 -> 2; then 1
    assert R.mmr(TABLE, rows, scores, 4, 0.5, "minmax")[2].tolist() == [[0, 3, 2, 1]]
    # lam = 0: variety alone; step 0 is a tie of four zeros -> place 0; then the most distant: 3, then 2, then 1
    assert R.mmr(TABLE, rows, scores, 4, 0.0, "raw")[2].tolist() == [[0, 3, 2, 1]]


def test_reference_mmr_ignores_what_is_no_place():
    rows = np.array([[-1, 7, 2, 0, 1, 3], [-1, -1, 9, 9, 9, 9]], dtype=np.int32)
    scores = np.array([[9.0, 9.0, np.nan, np.inf, 1.0, 2.0], [1.0] * 6], dtype=np.float32)
    r, s, p = R.mmr(TABLE, rows, scores, 4, 1.0, "raw")
    assert p.tolist() == [[5, 4, -1, -1], [-1] * 4] and r.tolist() == [[3, 1, -1, -1], [-1] * 4]
    assert s[0, :2].tolist() == [2.0, 1.0] and np.isneginf(s[0, 2:]).all() and np.isneginf(s[1]).all()


@pytest.mark.parametrize("rel", ["raw", "minmax"])
def test_reference_identity_and_prefix(rel):
    rng = np.random.default_rng(5)
    table = rng.standard_normal((50, 9)).astype(np.float32)
    rows = np.stack([rng.permutation(50)[:20] for _ in range(6)]).astype(np.int32)
    scores = -np.sort(-rng.standard_normal((6, 20)).astype(np.float32), axis=1)  # a pool in top-k order
    r, s, p = R.mmr(table, rows, scores, 12, 1.0, rel)
    assert (p == np.arange(12)).all() and (r == rows[:, :12]).all() and (s.view(np.int32) == scores[:, :12].view(np.int32)).all()
    full = R.mmr(table, rows, scores, 20, 0.4, rel)
    for j in (1, 7, 19):
        for a, b in zip(full, R.mmr(table, rows, scores, j, 0.4, rel)):
            assert (a[:, :j] == b).all()
    gaps, _, legal = R.mmr_step_gaps(table, rows, scores, full[2], 0.4, rel)
    assert legal.all() and (gaps == 0).all()


def test_reference_ild_and_categories():
    rows = np.array([[0, 1, 2, 3], [0, -1, 2, 99], [4, 4, -1, -1], [3, -1, -1, -1]], dtype=np.int32)
    cat = np.array([0, 0, 1, 7, 1], dtype=np.int32)  # news 3: category 7 is outside [0, 2)
    ps, n, ncat, diff = R.list_diversity(TABLE, rows, cat, 2)
    # list 0: pairs ab 0, ac 1, ad 2, bc 1, bd 2, cd 1 = 7 over 6 pairs; categories (0, 0, 1, -): 2 distinct, ac and bc differ
    assert ps.tolist() == [7.0, 1.0, 1.0, 0.0] and n.tolist() == [4, 2, 2, 1]  # (two zero rows: cos 0, distance 1)
    assert ncat.tolist() == [2, 2, 1, 0] and diff.tolist() == [2, 1, 0, 0]
    assert R.ild(ps, n).tolist() == [7.0 / 6.0, 1.0, 1.0, 0.0]
    m = R.diversity_metrics(TABLE, rows, 5, -1, cat, 2)
    assert m["ild@4"] == pytest.approx((7.0 / 6.0 + 1.0 + 1.0) / 3) and m["cat_ild@4"] == pytest.approx((2.0 / 6.0 + 1.0 + 0.0) / 3)
    assert m["n_categories@4"] == pytest.approx((2 + 2 + 1 + 0) / 4) and m["n_lists"] == 4 and m["n_listed"] == 9


def test_reference_exposure():
    n = 8
    even = np.arange(1, n + 1, dtype=np.int32).reshape(4, 2)  # every non-pad row once (row 0 is the pad row)
    cov, gini, listed = R.exposure(even, n + 1, 0)
    assert cov == 1.0 and gini == pytest.approx(0.0, abs=1e-15) and listed == n
    one = np.full((5, 2), 3, dtype=np.int32)
    cov, gini, listed = R.exposure(one, n + 1, 0)
    assert cov == 1.0 / n and gini == pytest.approx((n - 1) / n) and listed == 10
    assert R.exposure(np.full((3, 2), -1, dtype=np.int32), n + 1, 0) == (0.0, 0.0, 0)
    assert R.exposure(np.array([[0, 0, 5, 99]], dtype=np.int32), n + 1, 0) == (1.0 / n, pytest.approx((n - 1) / n), 1)  # pad, foreign ids
    cov, _, _ = R.exposure(np.array([[1, 2], [2, 3]], dtype=np.int32), n + 1, 0)
    assert cov == 3.0 / n


# ------------------------------------------------------------------------------------------ refusals of the entry points
def _buf():
    b = ctypes.create_string_buffer(64)
    return b, ctypes.cast(b, ctypes.c_void_p)


@pytest.mark.parametrize("P,k,lam,rel,E", [(10, 11, 0.5, 1, 8), (1025, 10, 0.5, 1, 8), (10, 0, 0.5, 1, 8), (10, 5, -0.1, 1, 8),
                                           (10, 5, 1.1, 1, 8), (10, 5, float("nan"), 1, 8), (10, 5, 0.5, 2, 8), (10, 5, 0.5, 1, 0),
                                           (10, 5, 0.5, 0, 4097)])
def test_mmr_refusals_need_no_device(P, k, lam, rel, E):
    b, out = _buf()
    assert hip.lib().xnrs_mmr_rerank(out, out, 100, E, out, out, 3, P, k, lam, rel, out, out, out, None) == EINVAL
    assert b.raw == bytes(64)


@pytest.mark.parametrize("k,n_cat,E", [(129, 0, 8), (0, 0, 8), (10, 4097, 8), (10, -1, 8), (10, 0, 4097), (10, 0, 0)])
def test_list_diversity_refusals_need_no_device(k, n_cat, E):
    b, out = _buf()
    assert hip.lib().xnrs_list_diversity(out, out, 100, E, out, 3, k, out, n_cat, out, out, out, out, None) == EINVAL
    assert b.raw == bytes(64)


def test_empty_calls_and_null_operands():
    l = hip.lib()
    _, out = _buf()
    assert l.xnrs_mmr_rerank(None, None, 100, 8, None, None, 0, 10, 5, 0.5, 1, None, None, None, None) == 0  # B == 0
    assert l.xnrs_list_diversity(None, None, 100, 8, None, 0, 10, None, 0, None, None, None, None, None) == 0
    assert l.xnrs_row_inv_norms(None, 0, 8, None, None) == 0
    assert l.xnrs_row_inv_norms(out, 10, 0, out, None) == EINVAL and l.xnrs_row_inv_norms(None, 10, 8, out, None) == EINVAL
    assert l.xnrs_mmr_rerank(out, out, 100, 8, None, out, 3, 10, 5, 0.5, 1, out, out, out, None) == EINVAL
    assert l.xnrs_list_diversity(out, out, 100, 8, out, 3, 10, out, 4, out, out, None, out, None) == EINVAL  # categories, no out_ncat


def test_ops_refuse_host_tensors_and_bad_shapes():
    from xnrs_amd import ops
    t = torch.zeros(4, 8)
    with pytest.raises(hip.XnrsHipError):
        ops.row_inv_norms(t)
    with pytest.raises(hip.XnrsHipError):
        ops.mmr_rerank(t, torch.zeros(4), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3), 2, 0.5)
    with pytest.raises(hip.XnrsHipError):
        ops.list_diversity(t, torch.zeros(4), torch.zeros(2, 3, dtype=torch.int32))


# ---------------------------------------------------------------------------- refusals before anything is encoded
def _stubs():
    from xnrs_amd import synth
    from xnrs_amd.models.blocks import DotScoring
    from xnrs_amd.models.caum import CAUMScoring

    class Model(torch.nn.Module):  # (no news encoder: encoding it would raise AttributeError, not the refusal)
        def __init__(self, scorer):
            super().__init__()
            self.rec_model = scorer

    class NPALike(Model):
        user_dependent_news = True

        def score_impressions(self, *a, **k):
            raise AssertionError("nothing is scored before the refusals")

    store, beh = synth.click_world(n_news=20, n_sess=5)
    return store, beh, Model(DotScoring()), NPALike(DotScoring()), Model(CAUMScoring())


def test_recommend_diverse_refuses_before_anything_is_encoded():
    from xnrs_amd import evaluation as EV
    store, beh, gen, npa, caum = _stubs()
    for pool in (19, 1025):
        with pytest.raises(ValueError, match="pool"):
            EV.recommend_diverse(gen, store, beh, l_hist=8, k=20, lam=0.5, pool=pool)
    for lam in (-0.1, 1.1, float("nan"), None):
        with pytest.raises(ValueError, match="lam"):
            EV.recommend_diverse(gen, store, beh, l_hist=8, k=5, lam=lam)
    with pytest.raises(ValueError, match="rel"):
        EV.recommend_diverse(gen, store, beh, l_hist=8, k=5, lam=0.5, rel="softmax")
    with pytest.raises(ValueError, match="1024"):
        EV.recommend_diverse(gen, store, beh, l_hist=8, k=2000, lam=0.5)
    with pytest.raises(NotImplementedError, match="depend on the user"):
        EV.recommend_diverse(npa, store, beh, l_hist=8, k=5, lam=0.5)
    with pytest.raises(NotImplementedError, match="CAUMScoring"):
        EV.recommend_diverse(caum, store, beh, l_hist=8, k=5, lam=0.5)


def test_evaluate_diversity_refuses_before_anything_is_encoded():
    from xnrs_amd import evaluation as EV
    store, beh, gen, npa, caum = _stubs()
    with pytest.raises(ValueError, match="128"):
        EV.evaluate_diversity(gen, store, beh, l_hist=8, k=129)
    with pytest.raises(ValueError, match="128"):
        EV.evaluate_diversity(gen, store, beh, l_hist=8, k=129, lam=0.5)
    with pytest.raises(ValueError, match="pool"):
        EV.evaluate_diversity(gen, store, beh, l_hist=8, k=20, lam=0.5, pool=10)
    with pytest.raises(ValueError, match="pool"):
        EV.evaluate_diversity(gen, store, beh, l_hist=8, k=20, pool=100)  # a pool and nothing to re-rank
    with pytest.raises(ValueError, match="lam"):
        EV.evaluate_diversity(gen, store, beh, l_hist=8, k=5, lam=1.5)
    with pytest.raises(ValueError, match="rel"):
        EV.evaluate_diversity(gen, store, beh, l_hist=8, k=5, lam=0.5, rel="rank")
    for lam in (None, 0.5):
        with pytest.raises(NotImplementedError, match="depend on the user"):
            EV.evaluate_diversity(npa, store, beh, l_hist=8, k=5, lam=lam)
        with pytest.raises(NotImplementedError, match="CAUMScoring"):
            EV.evaluate_diversity(caum, store, beh, l_hist=8, k=5, lam=lam)
    with pytest.raises(ValueError, match="128"):
        EV.diversity_metrics(torch.zeros(4, 8), torch.zeros((2, 129), dtype=torch.int32), 4, 0)


def test_recommend_keeps_its_pool_refusal():
    from xnrs_amd import evaluation as EV
    store, beh, gen, _, _ = _stubs()
    with pytest.raises(ValueError, match="pool"):
        EV.recommend(gen, store, beh, l_hist=8, k=20, pool=100)
