"""CPU: the host side of the calibration path (include/xnrs_hip.h: xnrs_csr_category_counts, xnrs_calibrated_rerank,
xnrs_list_calibration) -- the fp64 reference (tests/calibration_ref.py) against its own definition and properties, the refusals
of the entry points before any launch, and the refusals of evaluation.recommend_calibrated / evaluate_calibration /
calibration_metrics before anything is encoded."""
import ctypes

import numpy as np
import pytest
import torch

from tests import calibration_ref as R
from xnrs_amd import hip

EINVAL = -1


def test_the_three_entry_points_parse_out_of_the_header():
    funcs = hip.parse_header(open(hip.HEADER_PATH).read())[2]
    for name, n_args in (("xnrs_csr_category_counts", 9), ("xnrs_calibrated_rerank", 17), ("xnrs_list_calibration", 12)):
        assert name in hip.SYMBOLS and hasattr(hip.lib(), name)
        assert len(funcs[name][1]) == n_args, name
    assert hip._CONSTANTS["ABI_VERSION"] == 6  # new entry points only


# ------------------------------------------------------------------------------------------------ the reference, by hand
def test_reference_kl_by_hand():
    p = R.target_mix(np.array([3, 1, 0, np.nan, -2, np.inf], dtype=np.float32))
    assert p.tolist() == [0.75, 0.25, 0, 0, 0, 0]
    assert R.target_mix(np.array([0, -1, np.nan], dtype=np.float32)) is None
    a = 0.25
    # counts (1, 1): q~ = 0.75 * (1/2, 1/2) + 0.25 * (3/4, 1/4) = (9/16, 7/16)
    want = 0.75 * np.log(0.75 / (9 / 16)) + 0.25 * np.log(0.25 / (7 / 16))
    assert R.kl(p, [1, 1, 5, 0, 0, 0], a) > want  # (picks of a category outside the target count in N)
    assert R.kl(p, [1, 1, 0, 0, 0, 0], a) == pytest.approx(want, rel=1e-15)
    assert R.kl(p, [0] * 6, a) == pytest.approx(-np.log(a), rel=1e-15)  # nothing categorised: -ln alpha
    assert R.kl(p, [3, 1, 0, 0, 0, 0], a) == pytest.approx(0.0, abs=1e-15)  # the target's own proportion
    assert R.kl(None, [1, 2, 3], a) == 0.0


def test_reference_penalties_are_the_definition():
    rng = np.random.default_rng(0)
    for C in (1, 4, 33):
        p = R.target_mix(rng.integers(0, 4, size=C).astype(np.float32) + (np.arange(C) == 0))
        counts = rng.integers(0, 5, size=C)
        pen, none = R.penalties(p, counts, 0.01)
        assert none == R.kl(p, counts, 0.01)
        for c in range(C):
            assert pen[c] == pytest.approx(R.kl(p, counts + (np.arange(C) == c), 0.01), rel=1e-12, abs=1e-14)
        assert (pen >= -1e-15).all() and (pen <= -np.log(0.01) + 1e-12).all()


def _pool(B, P, n_rows, rng, sort=True):
    rows = np.stack([rng.permutation(n_rows)[:P] for _ in range(B)]).astype(np.int32)
    scores = rng.standard_normal((B, P)).astype(np.float32)
    return rows, -np.sort(-scores, axis=1) if sort else scores  # (sorted: a pool in top-k order)


@pytest.mark.parametrize("rel", ["raw", "minmax"])
def test_reference_identity_and_prefix(rel):
    rng = np.random.default_rng(5)
    n_rows, C, B, P = 60, 5, 6, 20
    cat = rng.integers(-1, C + 1, size=n_rows).astype(np.int32)
    rows, scores = _pool(B, P, n_rows, rng)
    rows[0, 3], scores[1, 0], rows[2, 5] = -1, np.nan, n_rows + 7
    target = rng.integers(0, 5, size=(B, C)).astype(np.float32)
    target[4] = 0  # no target
    ok = (rows >= 0) & (rows < n_rows) & np.isfinite(scores)
    first = [np.flatnonzero(ok[b])[:12] for b in range(B)]
    r, s, p, _ = R.calibrated(rows, scores, 12, 1.0, cat, C, target, 0.01, rel)  # lam = 1: the first k valid places
    assert all((p[b] == first[b]).all() for b in range(B))
    assert all((r[b] == rows[b, first[b]]).all() and (s[b].view(np.int32) == scores[b, first[b]].view(np.int32)).all() for b in range(B))
    for lam in (0.0, 0.5):  # no target at any lam: the same
        p0 = R.calibrated(rows[4:5], scores[4:5], 12, lam, cat, C, target[4:5], 0.01, rel)[2]
        assert (p0[0] == first[4]).all()
    full = R.calibrated(rows, scores, P, 0.4, cat, C, target, 0.01, rel)
    for j in (1, 7, 19):
        for a, b in zip(full[:3], R.calibrated(rows, scores, j, 0.4, cat, C, target, 0.01, rel)[:3]):
            assert (a[:, :j] == b).all()
    assert (full[2][:, -1] == -1).sum() == 3  # the three sessions with an invalid place run out
    gaps, legal, margin, _, cplus = R.calibrated_step_gaps(rows, scores, full[2], 0.4, cat, C, target, 0.01, rel)
    assert legal.all() and (gaps[~np.isnan(gaps)] == 0).all() and (margin[~np.isnan(margin)] >= 0).all() and cplus[4] == 0
    want_kl, _, _ = R.list_calibration(full[0], cat, C, target, 0.01)
    assert np.allclose(full[3], want_kl, rtol=0, atol=1e-15)
    bad = full[2].copy()
    bad[0, 1] = bad[0, 0]  # a place picked twice is not legal
    assert not R.calibrated_step_gaps(rows, scores, bad, 0.4, cat, C, target, 0.01, rel)[1][0, 1]


def test_reference_one_hot_target_takes_that_category_in_pool_order():
    rng = np.random.default_rng(6)
    n_rows, C, P, k = 40, 4, 30, 12
    cat = (np.arange(n_rows) % C).astype(np.int32)
    rows, scores = _pool(1, P, n_rows, rng)
    target = np.zeros((1, C), dtype=np.float32)
    target[0, 2] = 5
    _, _, p, _ = R.calibrated(rows, scores, k, 0.0, cat, C, target)
    of_two = np.flatnonzero(cat[rows[0]] == 2)
    assert 0 < len(of_two) < k
    assert (p[0, :len(of_two)] == of_two).all()  # that category's places in pool order while they last
    rest = np.flatnonzero(cat[rows[0]] != 2)
    assert (p[0, len(of_two):] == rest[:k - len(of_two)]).all()  # then every penalty is equal: pool order


def test_reference_uniform_target_fills_the_categories_evenly():
    rng = np.random.default_rng(7)
    C, k, P = 5, 13, 40
    n_rows = 200
    cat = (np.arange(n_rows) % C).astype(np.int32)
    rows, scores = _pool(4, P, n_rows, rng)
    assert all((np.bincount(cat[rows[b]], minlength=C) >= -(-k // C)).all() for b in range(4))  # k / C places of each at least
    r, _, _, v = R.calibrated(rows, scores, k, 0.0, cat, C, np.ones((4, C), dtype=np.float32))
    for b in range(4):
        counts = np.bincount(cat[r[b]], minlength=C)
        assert counts.sum() == k and counts.max() - counts.min() <= 1
    assert (v < 0.05).all()  # (3, 3, 3, 2, 2) of 13 against a fifth each: 0.019


def test_reference_counts_and_metrics():
    cat = np.array([0, 1, 1, 7, -1, 2], dtype=np.int32)
    off = np.array([0, 4, 4, 9], dtype=np.int64)
    rows = np.array([0, 1, 2, 3, 5, 5, 9, -1, 0], dtype=np.int32)
    assert R.category_counts(off, rows, cat, 3).tolist() == [[1, 2, 0], [0, 0, 0], [1, 0, 2]]
    assert R.category_counts(off, rows, cat, 3, pad_row=0).tolist() == [[0, 2, 0], [0, 0, 0], [0, 0, 2]]
    lists = np.array([[1, 2, 5], [0, 0, -1], [3, 4, 9]], dtype=np.int32)
    target = np.array([[0, 2, 1], [0, 0, 0], [1, 1, 1]], dtype=np.float32)
    v, n, counts = R.list_calibration(lists, cat, 3, target, 0.01)
    assert n.tolist() == [3, 2, 0] and counts.tolist() == [[0, 2, 1], [2, 0, 0], [0, 0, 0]]
    a = float(np.float32(0.01))
    assert v[0] == pytest.approx(0.0, abs=1e-15) and v[1] == 0.0 and v[2] == pytest.approx(-np.log(a), rel=1e-14)
    m = R.calibration_metrics(lists, cat, 3, target, -1, 0.01)
    assert m == {"calibration_kl@3": pytest.approx(-np.log(a) / 2), "n_lists": 3, "n_calibrated": 2}
    m = R.calibration_metrics(lists, cat, 3, target[0], 5, 0.01)  # one mix for everybody; row 5 is the pad row
    assert m["n_calibrated"] == 3 and m["calibration_kl@3"] == pytest.approx(
        (R.kl(R.target_mix(target[0]), [0, 2, 0], a) + R.kl(R.target_mix(target[0]), [2, 0, 0], a) - np.log(a)) / 3)


# ------------------------------------------------------------------------------------------ refusals of the entry points
def _buf():
    b = ctypes.create_string_buffer(64)
    return b, ctypes.cast(b, ctypes.c_void_p)


@pytest.mark.parametrize("P,k,n_cat,lam,alpha,rel", [
    (10, 11, 4, 0.5, 0.01, 1), (1025, 10, 4, 0.5, 0.01, 1), (10, 0, 4, 0.5, 0.01, 1), (10, 5, 0, 0.5, 0.01, 1),
    (10, 5, 4097, 0.5, 0.01, 1), (10, 5, 4, -0.1, 0.01, 1), (10, 5, 4, 1.1, 0.01, 1), (10, 5, 4, float("nan"), 0.01, 1),
    (10, 5, 4, 0.5, 0.0, 1), (10, 5, 4, 0.5, 1.0, 1), (10, 5, 4, 0.5, float("nan"), 1), (10, 5, 4, 0.5, 0.01, 2)])
def test_calibrated_rerank_refusals_need_no_device(P, k, n_cat, lam, alpha, rel):
    b, out = _buf()
    assert hip.lib().xnrs_calibrated_rerank(out, out, 3, P, k, out, 100, n_cat, out, lam, alpha, rel, out, out, out, out, None) == EINVAL
    assert b.raw == bytes(64)


@pytest.mark.parametrize("k,n_cat,alpha", [(1025, 4, 0.01), (0, 4, 0.01), (10, 0, 0.01), (10, 4097, 0.01), (10, 4, 0.0), (10, 4, 1.0),
                                           (10, 4, float("nan"))])
def test_list_calibration_refusals_need_no_device(k, n_cat, alpha):
    b, out = _buf()
    assert hip.lib().xnrs_list_calibration(out, 3, k, out, 100, n_cat, out, alpha, out, out, out, None) == EINVAL
    assert b.raw == bytes(64)


def test_counts_refusals_empty_calls_and_null_operands():
    l = hip.lib()
    b, out = _buf()
    for n_cat in (0, 4097, -1):
        assert l.xnrs_csr_category_counts(out, out, 3, out, 100, n_cat, -1, out, None) == EINVAL
    assert l.xnrs_csr_category_counts(out, out, 3, out, 2 ** 31, 4, -1, out, None) == EINVAL  # n_rows above 2^31 - 1
    assert l.xnrs_calibrated_rerank(out, out, 3, 10, 5, out, 2 ** 31, 4, out, 0.5, 0.01, 1, out, out, out, out, None) == EINVAL
    assert l.xnrs_csr_category_counts(None, None, 0, None, 100, 4, -1, None, None) == 0  # B == 0
    assert l.xnrs_calibrated_rerank(None, None, 0, 10, 5, None, 100, 4, None, 0.5, 0.01, 1, None, None, None, None, None) == 0
    assert l.xnrs_list_calibration(None, 0, 10, None, 100, 4, None, 0.01, None, None, None, None) == 0
    assert l.xnrs_csr_category_counts(out, out, 3, out, 100, 4, -1, None, None) == EINVAL
    assert l.xnrs_calibrated_rerank(out, out, 3, 10, 5, out, 100, 4, None, 0.5, 0.01, 1, out, out, out, out, None) == EINVAL  # no target
    assert l.xnrs_calibrated_rerank(out, out, 3, 10, 5, out, 100, 4, out, 0.5, 0.01, 1, out, out, out, None, None) == EINVAL  # no out_kl
    assert l.xnrs_list_calibration(out, 3, 10, None, 100, 4, out, 0.01, out, out, None, None) == EINVAL  # no row_cat
    assert b.raw == bytes(64)


def test_ops_refuse_host_tensors_and_bad_shapes():
    from xnrs_amd import ops
    rows, scores = torch.zeros((2, 3), dtype=torch.int32), torch.zeros(2, 3)
    cat, target = torch.zeros(5, dtype=torch.int32), torch.ones(2, 4)
    with pytest.raises(hip.XnrsHipError):
        ops.calibrated_rerank(rows, scores, 2, 0.5, cat, 4, target)
    with pytest.raises(hip.XnrsHipError):
        ops.list_calibration(rows, cat, 4, target)
    with pytest.raises(hip.XnrsHipError):
        ops.csr_category_counts(torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), cat, 4)
    with pytest.raises(RuntimeError, match="int32"):
        ops.calibrated_rerank(rows.long(), scores, 2, 0.5, cat, 4, target)
    with pytest.raises(RuntimeError, match="int64"):
        ops.csr_category_counts(torch.zeros(3, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), cat, 4)


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
    cat = torch.zeros(store.n_rows, dtype=torch.int32)
    return store, beh, cat, Model(DotScoring()), NPALike(DotScoring()), Model(CAUMScoring())


@pytest.mark.parametrize("fn", ["recommend_calibrated", "evaluate_calibration"])
def test_the_api_refuses_before_anything_is_encoded(fn):
    from xnrs_amd import evaluation as EV
    call = getattr(EV, fn)
    store, beh, cat, gen, npa, caum = _stubs()
    kw = dict(l_hist=8, row_category=cat, n_categories=3)
    for pool in (19, 1025):
        with pytest.raises(ValueError, match="pool"):
            call(gen, store, beh, k=20, lam=0.5, pool=pool, **kw)
    for lam in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="lam"):
            call(gen, store, beh, k=5, lam=lam, **kw)
    for alpha in (0.0, 1.0, float("nan"), -1.0):
        with pytest.raises(ValueError, match="alpha"):
            call(gen, store, beh, k=5, lam=0.5, alpha=alpha, **kw)
    with pytest.raises(ValueError, match="rel"):
        call(gen, store, beh, k=5, lam=0.5, rel="softmax", **kw)
    with pytest.raises(ValueError, match="1024"):
        call(gen, store, beh, k=2000, lam=0.5, **kw)
    for n_cat in (0, 4097):
        with pytest.raises(ValueError, match="n_categories"):
            call(gen, store, beh, k=5, lam=0.5, l_hist=8, row_category=cat, n_categories=n_cat)
    for bad in (cat.long(), cat[:, None], None, cat[:5]):
        with pytest.raises(ValueError, match="row_category"):
            call(gen, store, beh, k=5, lam=0.5, l_hist=8, row_category=bad, n_categories=3)
    for target in ("catalogue", torch.ones(4), torch.ones(len(beh) + 1, 3), torch.ones(3, dtype=torch.int64), [1.0, 1.0, 1.0]):
        with pytest.raises(ValueError, match="target"):
            call(gen, store, beh, k=5, lam=0.5, target=target, **kw)
    with pytest.raises(NotImplementedError, match="depend on the user"):  # NPA without a generator
        call(npa, store, beh, k=5, lam=0.5, **kw)
    with pytest.raises(NotImplementedError, match="CAUMScoring"):
        call(caum, store, beh, k=5, lam=0.5, **kw)
    with pytest.raises(NotImplementedError, match="score_impressions"):  # a generator for a model that ranks the table itself
        call(gen, store, beh, k=5, lam=0.5, generator=gen, **kw)
    with pytest.raises(ValueError, match="user index"):  # NPA and sessions without a user index
        call(npa, store, beh, k=5, lam=0.5, generator=gen, **kw)


def test_lam_none_is_for_the_evaluation_alone():
    from xnrs_amd import evaluation as EV
    store, beh, cat, gen, _, _ = _stubs()
    with pytest.raises(ValueError, match="lam"):
        EV.recommend_calibrated(gen, store, beh, l_hist=8, k=5, lam=None, row_category=cat, n_categories=3)
    with pytest.raises(ValueError, match="pool"):  # a pool and nothing to re-rank
        EV.evaluate_calibration(gen, store, beh, l_hist=8, k=5, pool=100, row_category=cat, n_categories=3)


def test_calibration_metrics_refusals():
    from xnrs_amd import evaluation as EV
    cat = torch.zeros(9, dtype=torch.int32)
    rows = torch.zeros((2, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="int32"):
        EV.calibration_metrics(rows.long(), cat, 3, torch.ones(3), 0)
    with pytest.raises(ValueError, match="1024"):
        EV.calibration_metrics(torch.zeros((2, 1025), dtype=torch.int32), cat, 3, torch.ones(3), 0)
    with pytest.raises(ValueError, match="target"):
        EV.calibration_metrics(rows, cat, 3, "history", 0)
    with pytest.raises(ValueError, match="target"):
        EV.calibration_metrics(rows, cat, 3, torch.ones(3, 3), 0)
    with pytest.raises(ValueError, match="alpha"):
        EV.calibration_metrics(rows, cat, 3, torch.ones(3), 0, alpha=1.5)
    with pytest.raises(hip.XnrsHipError):  # checked operands on the host: no CPU path
        EV.calibration_metrics(rows, cat, 3, torch.ones(3), 0)
