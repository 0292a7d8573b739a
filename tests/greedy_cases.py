"""The operands on which the two greedy re-rankers must agree EXACTLY (tests/test_greedy_ref_host.py between the fp64
references, tests/test_hip_greedy_skeleton.py between the kernels): at lam = 1 both penalties are multiplied by 1 - lam = 0,
and at the first step MMR's largest cosine is 0 and so is the penalty of a session without a target.  Nothing here is a test."""
import numpy as np

N_ROWS, N_CAT, B = 300, 5, 6
POOLS = (1, 5, 257, 1024)
RELS = ("raw", "minmax")
LAMS_FIRST_STEP = (0.0, 0.3, 0.7)

_made = {}


def table(E):
    """(300, E) small integers as fp32."""
    return np.random.default_rng(E).integers(-3, 4, size=(N_ROWS, E)).astype(np.float32)


def operands(P):
    """(rows:(6,P) int32, scores:(6,P) fp32, k, row_cat:(300,) int32, target:(6,5) fp32, no_target:(6,5) zeros).  Scores are
    multiples of 1/4 in [-2, 2] (many ties); categories -1, 5 and 6 are none.  Where P allows, session 1 holds places of row
    -1, row = n_rows and score NaN, +inf, -inf (one valid place stays), session 2 has no valid place, session 3 one score
    everywhere (span 0), session 4 fewer valid places than k; the targets of the odd sessions are all zero (no target), the
    others carry a zero entry.  Built once per P and never changed."""
    if P in _made:
        return _made[P]
    rng = np.random.default_rng(1000 + P)
    k = min(P, 33)
    row_cat = rng.integers(-1, N_CAT + 2, size=N_ROWS).astype(np.int32)
    rows = rng.integers(0, N_ROWS, size=(B, P)).astype(np.int32)
    scores = (rng.integers(-8, 9, size=(B, P)) / 4).astype(np.float32)
    bad = [("row", -1), ("row", N_ROWS), ("score", np.nan), ("score", np.inf), ("score", -np.inf)][:max(P - 1, 0)]
    for i, (what, v) in enumerate(bad):
        (rows if what == "row" else scores)[1, P - 1 - i] = v
    rows[2] = -1
    scores[3] = 0.75
    if P >= 2:
        rows[4, max(k // 2, 1):] = -1
    target = rng.integers(1, 6, size=(B, N_CAT)).astype(np.float32)
    target[:, 2] = 0
    target[1::2] = 0
    for a in (rows, scores, row_cat, target):
        a.setflags(write=False)
    _made[P] = rows, scores, k, row_cat, target, np.zeros_like(target)
    return _made[P]
