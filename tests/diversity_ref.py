"""fp64 NumPy reference of xnrs_row_inv_norms, xnrs_mmr_rerank, xnrs_list_diversity (include/xnrs_hip.h) and of the exposure
metrics of evaluation.diversity_metrics.  Every function takes the fp32 operands and widens them; nothing here is a test."""
import numpy as np


def inv_norms(table):
    """1 / ||row||, 0 for a zero row."""
    t = np.asarray(table, dtype=np.float64)
    ss = (t * t).sum(axis=1)
    return np.where(ss > 0, 1.0 / np.sqrt(np.where(ss > 0, ss, 1.0)), 0.0)


def _valid(rows, scores, n_rows):
    return (rows >= 0) & (rows < n_rows) & np.isfinite(scores)


def _cosines(table, rows, ok):
    """(n, n) cosines of the listed rows (anything for a place that is not ok)."""
    t = np.asarray(table, dtype=np.float64)
    x = t[np.where(ok, rows, 0)]
    inv = inv_norms(x)
    return (x @ x.T) * inv[:, None] * inv[None, :]


def relevance(scores, ok, rel):
    """r_i of the valid places of one session (0 elsewhere)."""
    s = np.where(ok, np.asarray(scores, dtype=np.float64), 0.0)
    if rel == "raw" or not ok.any():
        return s
    assert rel == "minmax", rel
    lo, hi = s[ok].min(), s[ok].max()
    return np.where(ok, (s - lo) / (hi - lo), 0.0) if hi > lo else np.zeros_like(s)


def mmr(table, pool_rows, pool_scores, k, lam, rel="minmax"):
    """Greedy MMR per session -> (rows:(B,k) int32, scores:(B,k) fp32 -- the pool's own values --, pos:(B,k) int32)."""
    pool_rows, pool_scores = np.asarray(pool_rows), np.asarray(pool_scores, dtype=np.float32)
    B, P = pool_rows.shape
    lam = float(np.float32(lam))
    out_r = np.full((B, k), -1, dtype=np.int32)
    out_s = np.full((B, k), -np.inf, dtype=np.float32)
    out_p = np.full((B, k), -1, dtype=np.int32)
    for b in range(B):
        ok = _valid(pool_rows[b], pool_scores[b], len(table))
        cos = _cosines(table, pool_rows[b], ok)
        r = relevance(pool_scores[b], ok, rel)
        alive, m = ok.copy(), np.zeros(P)
        for t in range(k):
            if not alive.any():
                break
            obj = np.where(alive, lam * r - (1.0 - lam) * m, -np.inf)
            i = int(np.argmax(obj))  # (the first of equal maxima: the lower place)
            out_r[b, t], out_s[b, t], out_p[b, t] = pool_rows[b, i], pool_scores[b, i], i
            alive[i] = False
            m = cos[:, i].copy() if t == 0 else np.maximum(m, cos[:, i])
    return out_r, out_s, out_p


def mmr_step_gaps(table, pool_rows, pool_scores, pos, lam, rel="minmax"):
    """For picks `pos`:(B,k) made by anyone: per step, the fp64 maximum of the objective over the valid places not picked
    before, minus the fp64 objective of the pick, GIVEN the earlier picks -> (gaps:(B,k), NaN where pos is -1; max |r|;
    (B,k) bool: the pick was a valid place not picked before, or -1 exactly when no valid place was left)."""
    pool_rows, pool_scores, pos = np.asarray(pool_rows), np.asarray(pool_scores, dtype=np.float32), np.asarray(pos)
    B, P = pool_rows.shape
    k = pos.shape[1]
    lam = float(np.float32(lam))
    gaps = np.full((B, k), np.nan)
    legal = np.zeros((B, k), dtype=bool)
    rmax = 0.0
    for b in range(B):
        ok = _valid(pool_rows[b], pool_scores[b], len(table))
        cos = _cosines(table, pool_rows[b], ok)
        r = relevance(pool_scores[b], ok, rel)
        rmax = max(rmax, float(np.abs(r).max()) if P else 0.0)
        alive, m = ok.copy(), np.zeros(P)
        for t in range(k):
            i = int(pos[b, t])
            if i < 0:
                legal[b, t] = not alive.any()
                continue
            legal[b, t] = 0 <= i < P and bool(alive[i])
            if not legal[b, t]:
                continue
            obj = np.where(alive, lam * r - (1.0 - lam) * m, -np.inf)
            gaps[b, t] = obj.max() - obj[i]
            alive[i] = False
            m = cos[:, i].copy() if t == 0 else np.maximum(m, cos[:, i])
    return gaps, rmax, legal


def list_diversity(table, rows, row_cat=None, n_cat=0):
    """-> (pair_sum:(B,) fp64, n:(B,), n_cat:(B,), diff_cat:(B,)): the sum of 1 - cos over the valid pairs i < j, the valid
    places, the distinct categories and the pairs of differing category (categories outside [0, n_cat): no category)."""
    rows = np.asarray(rows)
    B, k = rows.shape
    pair_sum, n = np.zeros(B), np.zeros(B, dtype=np.int64)
    ncat, diff = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for b in range(B):
        ok = (rows[b] >= 0) & (rows[b] < len(table))
        n[b] = ok.sum()
        d = 1.0 - _cosines(table, rows[b], ok)
        pair = np.triu(ok[:, None] & ok[None, :], 1)
        pair_sum[b] = d[pair].sum()
        if row_cat is not None:
            c = np.asarray(row_cat)[np.where(ok, rows[b], 0)]
            has = ok & (c >= 0) & (c < n_cat)
            ncat[b] = len(set(c[has].tolist()))
            diff[b] = (np.triu(has[:, None] & has[None, :], 1) & (c[:, None] != c[None, :])).sum()
    return pair_sum, n, ncat, diff


def ild(pair_sum, n):
    """pair_sum / n_pairs in fp64, 0 below two places."""
    pairs = n * (n - 1) // 2
    return np.where(n >= 2, pair_sum / np.maximum(pairs, 1), 0.0)


def exposure(rows, n_rows, pad_row):
    """-> (coverage, gini, n_listed) of the lists' rows over the non-pad rows of the table."""
    rows = np.asarray(rows).reshape(-1)
    ok = (rows >= 0) & (rows < n_rows) & (rows != pad_row)
    counts = np.bincount(rows[ok], minlength=n_rows).astype(np.float64)
    if 0 <= pad_row < n_rows:
        counts = np.delete(counts, pad_row)
    n, total = len(counts), counts.sum()
    coverage = float((counts > 0).sum()) / max(n, 1)
    if total == 0:
        return coverage, 0.0, 0
    asc = np.sort(counts)
    gini = 2.0 * float((np.arange(1, n + 1) * asc).sum()) / (n * total) - (n + 1) / n
    return coverage, gini, int(total)


def diversity_metrics(table, rows, n_rows, pad_row, row_cat=None, n_cat=0):
    """The dict of evaluation.diversity_metrics."""
    rows = np.asarray(rows)
    k = rows.shape[1]
    table = np.asarray(table)[:n_rows]
    listed = np.where(rows == pad_row, -1, rows) if pad_row >= 0 else rows
    pair_sum, n, ncat, diff = list_diversity(table, listed, None if row_cat is None else np.asarray(row_cat)[:n_rows], n_cat)
    two, one = n >= 2, n >= 1
    coverage, gini, n_listed = exposure(rows, n_rows, pad_row)
    out = {f"ild@{k}": float(ild(pair_sum, n)[two].sum()) / max(int(two.sum()), 1), f"catalog_coverage@{k}": coverage,
           f"gini@{k}": gini, "n_lists": int(rows.shape[0]), "n_listed": n_listed}
    if row_cat is not None:
        pairs = np.maximum(n * (n - 1) // 2, 1)
        out[f"cat_ild@{k}"] = float((diff / pairs)[two].sum()) / max(int(two.sum()), 1)
        out[f"n_categories@{k}"] = float(ncat[one].sum()) / max(int(one.sum()), 1)
    return out
