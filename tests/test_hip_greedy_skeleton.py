"""mmr_kernel and cal_kernel are one greedy loop (csrc/greedy.h) under two penalties.  Where the penalty cannot matter the two
kernels must return the same rows, score BITS and places: at lam = 1 both penalties are multiplied by 1 - lam = 0, and at the
first step MMR's largest cosine is 0 and so is the penalty of a session without a target.  Exact by construction, so there is
no tolerance.  The operands are those of tests/test_greedy_ref_host.py, which makes the same claims of the fp64 references;
both table routes of MMR run (E = 20: 16-byte loads; E = 21: scalar loads)."""
import pytest
import torch

from tests import greedy_cases as G
from xnrs_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(a.copy()).to(DEV)


def same(m, c):
    return torch.equal(m[0], c[0]) and torch.equal(m[2], c[2]) and torch.equal(m[1].view(torch.int32), c[1].view(torch.int32))


@pytest.mark.parametrize("E", [20, 21])
@pytest.mark.parametrize("rel", G.RELS)
@pytest.mark.parametrize("P", G.POOLS)
def test_the_two_kernels_agree_where_the_penalty_cannot_matter(P, rel, E):
    rows, scores, k, cat, target, none = (dev(a) if hasattr(a, "shape") else a for a in G.operands(P))
    vecs = dev(G.table(E))
    inv = ops.row_inv_norms(vecs)
    m = ops.mmr_rerank(vecs, inv, rows, scores, k, 1.0, rel)
    c = ops.calibrated_rerank(rows, scores, k, 1.0, cat, G.N_CAT, target, rel=rel)
    assert same(m, c)  # lam = 1, sessions with a target and without
    assert bool((m[2][2] == -1).all()) and bool(((m[2] >= 0) == (m[0] >= 0)).all())  # (the session without a valid place)
    for lam in G.LAMS_FIRST_STEP:
        m = ops.mmr_rerank(vecs, inv, rows, scores, 1, lam, rel)
        c = ops.calibrated_rerank(rows, scores, 1, lam, cat, G.N_CAT, none, rel=rel)
        assert same(m, c)  # k = 1 without a target
