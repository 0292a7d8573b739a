"""fp64 NumPy reference of xnrs_csr_category_counts, xnrs_calibrated_rerank, xnrs_list_calibration (include/xnrs_hip.h) and of
evaluation.calibration_metrics.  Every function takes the fp32 operands and widens them; nothing here is a test."""
import numpy as np

from tests.diversity_ref import _valid, relevance


def category_counts(off, rows, row_cat, n_cat, pad_row=-1):
    """(B, n_cat) int64: the category histogram of every list of the CSR; rows outside the table, the pad row and rows without
    a category count nowhere."""
    off, rows, row_cat = np.asarray(off), np.asarray(rows), np.asarray(row_cat)
    out = np.zeros((len(off) - 1, n_cat), dtype=np.int64)
    for b in range(len(off) - 1):
        r = rows[off[b]:off[b + 1]]
        r = r[(r >= 0) & (r < len(row_cat)) & (r != pad_row)]
        c = row_cat[r]
        out[b] = np.bincount(c[(c >= 0) & (c < n_cat)], minlength=n_cat)
    return out


def target_mix(target):
    """p:(n_cat,) fp64 of one session's fp32 weights (finite and > 0 count), or None without a target."""
    w = np.asarray(target, dtype=np.float32).astype(np.float64)
    w = np.where(np.isfinite(w) & (w > 0), w, 0.0)
    return w / w.sum() if w.sum() > 0 else None


def kl(p, counts, alpha):
    """sum over p_c > 0 of p_c log(p_c / ((1 - alpha) n_c / N + alpha p_c)), n / N = 0 at N == 0; 0 without a target."""
    if p is None:
        return 0.0
    counts = np.asarray(counts, dtype=np.float64)
    N = counts.sum()
    on = p > 0
    q = (1.0 - alpha) * (counts[on] / N if N > 0 else 0.0) + alpha * p[on]
    return float((p[on] * np.log(p[on] / q)).sum())


def penalties(p, counts, alpha):
    """(pen:(n_cat,), pen_none): the penalty of a candidate of every category -- kl(p, counts + e_c), of which only the term
    of c differs from kl at N + 1 (test_calibration_host.py holds it against the definition) -- and of one without a
    category."""
    if p is None:
        return np.zeros(len(counts)), 0.0
    pen = np.empty(len(counts))
    on = np.flatnonzero(p > 0)
    base = np.asarray(counts, dtype=np.float64)
    N1 = base.sum() + 1.0
    terms = lambda n: p[on] * np.log(p[on] / ((1.0 - alpha) * n / N1 + alpha * p[on]))
    now, then = terms(base[on]), terms(base[on] + 1.0)
    pen[:] = now.sum()  # (a category outside the target: the counts grow, no term changes)
    pen[on] = (now.sum() - now) + then
    return pen, kl(p, counts, alpha)


def _session(pool_rows, pool_scores, row_cat, n_cat, target, rel):
    row_cat = np.asarray(row_cat)
    ok = _valid(pool_rows, pool_scores, len(row_cat))
    cat = np.where(ok, row_cat[np.where(ok, pool_rows, 0)], -1) if len(row_cat) else np.full(len(pool_rows), -1)
    cat = np.where((cat >= 0) & (cat < n_cat), cat, -1)
    return ok, cat, relevance(pool_scores, ok, rel), target_mix(target)


def _objective(alive, cat, r, p, counts, lam, alpha):
    pen, pen_none = penalties(p, counts, alpha)
    return np.where(alive, lam * r - (1.0 - lam) * np.where(cat >= 0, pen[np.maximum(cat, 0)], pen_none), -np.inf)


def calibrated(pool_rows, pool_scores, k, lam, row_cat, n_cat, target, alpha=0.01, rel="minmax"):
    """The greedy per session -> (rows:(B,k) int32, scores:(B,k) fp32 -- the pool's own values --, pos:(B,k) int32, kl:(B,))."""
    pool_rows, pool_scores = np.asarray(pool_rows), np.asarray(pool_scores, dtype=np.float32)
    B, P = pool_rows.shape
    lam, alpha = float(np.float32(lam)), float(np.float32(alpha))
    out_r = np.full((B, k), -1, dtype=np.int32)
    out_s = np.full((B, k), -np.inf, dtype=np.float32)
    out_p = np.full((B, k), -1, dtype=np.int32)
    out_kl = np.zeros(B)
    for b in range(B):
        alive, cat, r, p = _session(pool_rows[b], pool_scores[b], row_cat, n_cat, target[b], rel)
        counts = np.zeros(n_cat, dtype=np.int64)
        for t in range(k):
            if not alive.any():
                break
            i = int(np.argmax(_objective(alive, cat, r, p, counts, lam, alpha)))  # (the first of equal maxima: the lower place)
            out_r[b, t], out_s[b, t], out_p[b, t] = pool_rows[b, i], pool_scores[b, i], i
            alive[i] = False
            if cat[i] >= 0:
                counts[cat[i]] += 1
        out_kl[b] = kl(p, counts, alpha)
    return out_r, out_s, out_p, out_kl


def calibrated_step_gaps(pool_rows, pool_scores, pos, lam, row_cat, n_cat, target, alpha=0.01, rel="minmax"):
    """For picks `pos`:(B,k) made by anyone: per step, GIVEN the earlier picks, the fp64 maximum of the objective over the
    valid places not picked before minus the fp64 objective of the pick -> (gaps:(B,k), NaN where pos is -1; legal:(B,k)
    bool: the pick was a valid place not picked before, or -1 exactly when no valid place was left; margin:(B,k): the fp64
    maximum minus the fp64 runner-up's objective, inf with one candidate left, NaN where pos is -1; max |r|; C+:(B,) the
    categories with p > 0)."""
    pool_rows, pool_scores, pos = np.asarray(pool_rows), np.asarray(pool_scores, dtype=np.float32), np.asarray(pos)
    B, P = pool_rows.shape
    k = pos.shape[1]
    lam, alpha = float(np.float32(lam)), float(np.float32(alpha))
    gaps, margin = np.full((B, k), np.nan), np.full((B, k), np.nan)
    legal = np.zeros((B, k), dtype=bool)
    cplus = np.zeros(B, dtype=np.int64)
    rmax = 0.0
    for b in range(B):
        alive, cat, r, p = _session(pool_rows[b], pool_scores[b], row_cat, n_cat, target[b], rel)
        cplus[b] = 0 if p is None else int((p > 0).sum())
        rmax = max(rmax, float(np.abs(r).max()) if P else 0.0)
        counts = np.zeros(n_cat, dtype=np.int64)
        for t in range(k):
            i = int(pos[b, t])
            if i < 0:
                legal[b, t] = not alive.any()
                continue
            legal[b, t] = 0 <= i < P and bool(alive[i])
            if not legal[b, t]:
                continue
            obj = _objective(alive, cat, r, p, counts, lam, alpha)
            top = np.sort(obj)[::-1][:2]
            gaps[b, t] = top[0] - obj[i]
            margin[b, t] = top[0] - top[1] if len(top) > 1 else np.inf  # (-inf for what is not alive: inf with one left)
            alive[i] = False
            if cat[i] >= 0:
                counts[cat[i]] += 1
    return gaps, legal, margin, rmax, cplus


def list_calibration(rows, row_cat, n_cat, target, alpha=0.01):
    """-> (kl:(B,) fp64, n:(B,), counts:(B,n_cat)) of the lists rows:(B,k): a place is valid when its row is inside the table."""
    rows, row_cat = np.asarray(rows), np.asarray(row_cat)
    alpha = float(np.float32(alpha))
    B = rows.shape[0]
    counts = np.zeros((B, n_cat), dtype=np.int64)
    out = np.zeros(B)
    for b in range(B):
        r = rows[b][(rows[b] >= 0) & (rows[b] < len(row_cat))]
        c = row_cat[r]
        counts[b] = np.bincount(c[(c >= 0) & (c < n_cat)], minlength=n_cat)
        out[b] = kl(target_mix(target[b]), counts[b], alpha)
    return out, counts.sum(axis=1), counts


def calibration_metrics(rows, row_cat, n_cat, target, pad_row, alpha=0.01):
    """The dict of evaluation.calibration_metrics; target:(n_cat,) or (B, n_cat)."""
    rows = np.asarray(rows)
    target = np.asarray(target, dtype=np.float32)
    if target.ndim == 1:
        target = np.broadcast_to(target, (rows.shape[0], n_cat))
    listed = np.where(rows == pad_row, -1, rows) if pad_row >= 0 else rows
    v, _, _ = list_calibration(listed, row_cat, n_cat, target, alpha)
    has = np.array([target_mix(t) is not None for t in target], dtype=bool)
    return {f"calibration_kl@{rows.shape[1]}": float(v[has].sum()) / max(int(has.sum()), 1), "n_lists": int(rows.shape[0]),
            "n_calibrated": int(has.sum())}
