"""NumPy reference of the top-k order contract (include/xnrs_hip.h: xnrs_topk): higher score first, equal scores (==, so
+0 and -0 tie) lower row first, a NaN score never selected, -inf a legal score; eligible rows are all rows minus `pad_row`
(when >= 0) minus the user's exclusion list; with fewer than k eligible rows the tail is row -1 / score -inf."""
import numpy as np


def topk_reference(scores, k, excl=None, pad_row=-1):
    """scores:(B, N) -> (rows:(B, k) int32, scores:(B, k) of scores' dtype).  excl: per user an iterable of row ids (ids
    outside the table are ignored), or None."""
    scores = np.asarray(scores)
    B, N = scores.shape
    out_rows = np.full((B, k), -1, dtype=np.int32)
    out_scores = np.full((B, k), -np.inf, dtype=scores.dtype if scores.dtype.kind == "f" else np.float64)
    for b in range(B):
        ok = np.ones(N, dtype=bool)
        if 0 <= pad_row < N:
            ok[pad_row] = False
        if excl is not None:
            e = np.asarray(list(excl[b]), dtype=np.int64)
            ok[e[(e >= 0) & (e < N)]] = False
        s = scores[b].astype(np.float64)
        ok &= ~np.isnan(s)
        rows = np.nonzero(ok)[0]
        s = s[rows]
        order = np.lexsort((rows, -s))[:k]
        out_rows[b, :order.size] = rows[order]
        out_scores[b, :order.size] = scores[b, rows[order]]
    return out_rows, out_scores
