"""NumPy reference of the rank contract (include/xnrs_hip.h: xnrs_rank) over a (B, N) score matrix: for every query
(user b, row t) the number of eligible rows n != t that come before t in the top-k order -- a higher score, or an equal score
(==, so +0 and -0 tie) in a lower row.  A NaN-scored row is never counted, -inf is a legal score; eligible rows are all rows
minus `pad_row` (when >= 0) minus the user's exclusion list; the target itself is ranked even when it is on that list.
Rank -1 / score NaN: a target outside the table, the pad row, a NaN score.  fp32 scores are compared as fp32."""
import numpy as np


def eligible(scores_b, excl_b=None, pad_row=-1):
    """The rows of one user that may be counted."""
    N = scores_b.shape[0]
    ok = ~np.isnan(scores_b)
    if 0 <= pad_row < N:
        ok[pad_row] = False
    if excl_b is not None:
        e = np.asarray(list(excl_b), dtype=np.int64)
        ok[e[(e >= 0) & (e < N)]] = False
    return ok


def rank_reference(scores, targets, excl=None, pad_row=-1):
    """scores:(B, N); targets: per user a sequence of row ids -> (ranks int32, scores of scores' dtype), flat, in the order of
    the CSR of `targets`.  excl: per user an iterable of row ids (ids outside the table are ignored), or None."""
    scores = np.asarray(scores)
    B, N = scores.shape
    rows = np.arange(N)
    out_r, out_s = [], []
    for b in range(B):
        s = scores[b]
        ok = eligible(s, None if excl is None else excl[b], pad_row)
        for t in targets[b]:
            t = int(t)
            if not 0 <= t < N or t == pad_row or np.isnan(s[t]):
                out_r.append(-1)
                out_s.append(np.nan)
                continue
            before = ok & ((s > s[t]) | ((s == s[t]) & (rows < t)))
            before[t] = False
            out_r.append(int(before.sum()))
            out_s.append(s[t])
    return np.asarray(out_r, dtype=np.int32), np.asarray(out_s, dtype=scores.dtype if scores.dtype.kind == "f" else np.float64)
