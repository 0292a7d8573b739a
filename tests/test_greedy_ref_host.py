"""The two fp64 references of the greedy re-rankers (tests/diversity_ref.mmr, tests/calibration_ref.calibrated) share no code
beyond the validity rule and the relevance, yet they are the same greedy with another penalty.  Where the penalty cannot
matter they must pick the same places: at lam = 1 (with and without a target) and at the first step of a session without a
target.  Exact agreement in rows, score bits and places; tests/test_hip_greedy_skeleton.py makes the same claims of the kernels."""
import numpy as np
import pytest

from tests import calibration_ref as CR
from tests import diversity_ref as DR
from tests import greedy_cases as G

E = 20


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


@pytest.mark.parametrize("rel", G.RELS)
@pytest.mark.parametrize("P", G.POOLS)
def test_at_lam_one_both_references_list_by_relevance(P, rel):
    rows, scores, k, cat, target, _ = G.operands(P)
    assert target[0].any() and not target[1].any()  # sessions with a target and without
    m = DR.mmr(G.table(E), rows, scores, k, 1.0, rel)
    c = CR.calibrated(rows, scores, k, 1.0, cat, G.N_CAT, target, rel=rel)
    assert same(m, c)
    ok = (rows >= 0) & (rows < G.N_ROWS) & np.isfinite(scores)
    assert ((m[2] >= 0).sum(1) == np.minimum(ok.sum(1), k)).all()  # the operands hold what they promise: fillers and full lists
    if P >= 5:
        assert ok[1].sum() < P and not ok[2].any() and ok[4].sum() < k and (m[2][2] == -1).all()


@pytest.mark.parametrize("lam", G.LAMS_FIRST_STEP)
@pytest.mark.parametrize("rel", G.RELS)
@pytest.mark.parametrize("P", G.POOLS)
def test_the_first_pick_without_a_target_is_the_same(P, rel, lam):
    rows, scores, _, cat, _, none = G.operands(P)
    m = DR.mmr(G.table(E), rows, scores, 1, lam, rel)
    c = CR.calibrated(rows, scores, 1, lam, cat, G.N_CAT, none, rel=rel)
    assert same(m, c)
