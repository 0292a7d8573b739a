"""GPU: sampled top-k (include/xnrs_hip.h: xnrs_topk_sample_win / _bilinear_win / _mlp_win; csrc/topk.hip, the SAMPLE
instantiations of topk_partial_kernel), evaluation.recommend_sampled and losses.mined_negatives_loss(temperature=).

The draw is restated in tests/sample_ref.py; the reference of a case is its fp64 keys s64 / temperature + g64(w), w the exact
fp32 uniform, and the validator "top-k within tol" (sample_ref.check_sampled_topk) with
tol = 32 * 2^-23 * max(1, max |key64|) of the case.

1. validity over B, n_rows, E, k, exclusions, pad row, windows, user keys, the bilinear and the MLP form;
2. determinism and independence of batch, position and the other users; 3. prefix; 4. the cold limit equals topk_deep;
5. the distribution is Plackett-Luce within 5 sigma; 6. NaN / -inf scores and short lists; 7. recommend_sampled and the
sampled mined-negatives loss.

Largest |device key - fp64 key| observed on an MI355X: 4.587e-06 over the validity cases (the MLP form at (130, 127, 64, 129),
0.047 of its tol 9.770e-05), and at most 0.052 of tol in any case (dot (5, 2100, 64, 300): 2.184e-06 of 4.241e-05) -- nowhere
near a quarter of tol.  Every case prints its MARGIN line (error, error / tol).  The Plackett-Luce cases sat at 0.81 / 2.04
(temperature 0.5) and 1.08 / 3.30 (temperature 2) standard deviations for first places / ordered pairs, the figures of the fp64
reference in tests/test_sample_host.py: the device drew the reference's lists."""
import functools

import numpy as np
import pytest
import torch

from tests import sample_ref as SR
from tests.test_hip_topk import SWITCH_TOL, dev, excl_csr, histories, make_scorer
from xnrs_amd import evaluation as EV
from xnrs_amd import hip, losses, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAU, SEED = 0.5, 20240917


# ------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def operands(B, N, E, seed):
    """table:(N,E), u:(B,E) fp32: scores ~ N(0, 1); computed once, shared, never changed"""
    rng = synth.rng_for(31000 + seed)
    t = rng.standard_normal((N, E)).astype(np.float32)
    u = (rng.standard_normal((B, E)) / np.sqrt(E)).astype(np.float32)
    return t, u


def extras(B, N, what, seed):
    """The optional arguments of a case, from the letters of `what`: x exclusion lists (unsorted, duplicates, foreign ids,
    one empty, one long), p a pad row, w windows (user 1's empty, user 0's the whole table, some past the table's end),
    k explicit user keys (large, negative, not in order)."""
    rng = synth.rng_for(32000 + seed)
    excl = pad_row = win = keys = None
    if "x" in what:
        excl = [rng.integers(-2, N + 3, size=int(rng.integers(0, 12))).tolist() for _ in range(B)]
        excl[0] = []
        excl[-1] = rng.integers(0, max(N, 1), size=150).tolist()
    if "p" in what:
        pad_row = min(2, N - 1)
    if "w" in what:
        lo = rng.integers(-5, max(N // 2, 1), size=B)
        hi = lo + rng.integers(1, N + 10, size=B)
        lo[0], hi[0] = 0, N
        if B > 1:
            lo[1], hi[1] = 7, 7
        win = (lo.astype(np.int32), hi.astype(np.int32))
    if "k" in what:
        keys = (rng.permutation(B).astype(np.int64) * 7919 - 1000) + (np.arange(B) % 3 == 0) * 2 ** 40
    return excl, -1 if pad_row is None else pad_row, win, keys


def device_args(excl, win, keys):
    eo, er = (dev(a) for a in excl_csr(excl)) if excl is not None else (None, None)
    wl, wh = (dev(win[0]), dev(win[1])) if win is not None else (None, None)
    return eo, er, wl, wh, None if keys is None else dev(keys)


def reference(s64, B, N, k, tau, seed, excl, pad_row, win, keys):
    """(fp64 keys, eligibility, tol) of a case, with the condition on the reference alone: in at most 1 % of the users are
    the k-th and (k+1)-th fp64 keys closer than 2 tol."""
    key64 = SR.keys64(s64, tau, seed, np.arange(B) if keys is None else keys)
    ok = SR.eligible_mask(B, N, excl, pad_row, win)
    tol = SR.tolerance(key64, ok)
    assert SR.close_calls(key64, ok, k, tol) <= 0.01
    return key64, ok, tol


# B in {1, 5, 130} x n_rows in {1, 127, 300, 2100} x E in {7, 64} x k in {1, 10, 128, 129, 300}: one and several user tiles,
# one chunk / a ragged chunk / several chunks and slices, unaligned rows and vector loads, the shallow form, its limit, the
# deep form behind the floor sweep (k = 129, 300 over 17 slices) and without it (one slice)
DOT_CASES = [(1, 1, 7, 1, ""), (1, 1, 7, 10, "k"), (5, 127, 7, 10, "xp"), (130, 300, 64, 128, "xpwk"), (130, 300, 7, 129, "x"),
             (5, 2100, 64, 300, "w"), (130, 2100, 64, 10, "xk"), (130, 2100, 7, 129, "pw"), (1, 2100, 64, 128, ""),
             (5, 300, 7, 1, "wk"), (5, 300, 64, 300, "xp")]


@pytest.mark.parametrize("B,N,E,k,what", DOT_CASES)
def test_validity_dot(B, N, E, k, what):
    case = DOT_CASES.index((B, N, E, k, what))
    t, u = operands(B, N, E, case)
    excl, pad_row, win, keys = extras(B, N, what, case)
    key64, ok, tol = reference(u.astype(np.float64) @ t.astype(np.float64).T, B, N, k, TAU, SEED, excl, pad_row, win, keys)
    eo, er, wl, wh, kd = device_args(excl, win, keys)
    rows, got = ops.topk_sample_dot(dev(t), dev(u), k, TAU, SEED, kd, eo, er, pad_row, wl, wh)
    assert rows.dtype == torch.int32 and got.dtype == torch.float32
    worst = SR.check_sampled_topk(rows.cpu().numpy(), got.cpu().numpy(), key64, ok, k, tol)
    print(f"MARGIN topk_sample dot {(B, N, E, k, what)}: |key - fp64 key| {worst:.3e} = {worst / tol:.3f} of tol {tol:.3e}")
    if "w" in what and B > 1:
        assert (rows[1] == -1).all()  # the empty window


@pytest.mark.parametrize("kind,B,N,E,k,what", [("bilin", 5, 300, 64, 10, "xp"), ("bilin", 130, 300, 7, 129, "w"),
                                               ("fc", 5, 300, 14, 10, "xpk"), ("fc", 130, 127, 64, 129, "w"),
                                               ("dot_norm", 5, 300, 7, 10, "")])
def test_validity_bilinear_and_mlp(kind, B, N, E, k, what):
    case = 100 + ["bilin", "fc", "dot_norm"].index(kind) * 10 + (B > 5)
    t, u = operands(B, N, E, case)
    scorer, ref64 = make_scorer(kind, E, synth.rng_for(33000 + case))
    excl, pad_row, win, keys = extras(B, N, what, case)
    tau = 0.05 if kind == "dot_norm" else TAU  # (cosines: a temperature in their range)
    key64, ok, tol = reference(ref64(t, u), B, N, k, tau, SEED, excl, pad_row, win, keys)
    eo, er, wl, wh, kd = device_args(excl, win, keys)
    with torch.no_grad():
        rows, got = scorer.topk_sample(scorer.prepare_csr(dev(t)), dev(u), k, tau, SEED, kd, eo, er, pad_row, win_lo=wl, win_hi=wh)
    worst = SR.check_sampled_topk(rows.cpu().numpy(), got.cpu().numpy(), key64, ok, k, tol)
    print(f"MARGIN topk_sample {kind} {(B, N, E, k, what)}: |key - fp64 key| {worst:.3e} = {worst / tol:.3f} of tol {tol:.3e}")


# ------------------------------------------------------------------------------------------- 2. determinism, independence
@pytest.mark.parametrize("k", [10, 129])
def test_determinism_and_independence_of_the_batch(k):
    B, N, E = 130, 2100, 64
    t, u = operands(B, N, E, 6)
    td, ud = dev(t), dev(u)
    keys = dev(np.arange(B, dtype=np.int64) * 3 + 11)
    eo, er = (dev(a) for a in excl_csr([[b, 2 * b, 5] for b in range(B)]))
    first = ops.topk_sample_dot(td, ud, k, TAU, SEED, keys, eo, er)
    again = ops.topk_sample_dot(td, ud, k, TAU, SEED, keys, eo, er)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    other = ops.topk_sample_dot(td, ud, k, TAU, SEED + 1, keys, eo, er)
    assert not torch.equal(first[0], other[0]) and (first[0][:, 0] != other[0][:, 0]).float().mean() > 0.5
    colder = ops.topk_sample_dot(td, ud, k, TAU / 2, SEED, keys, eo, er)
    assert not torch.equal(first[0], colder[0])
    # users moved to other batch positions, in a batch of another size, keep their lists when they keep their keys
    perm = torch.from_numpy(synth.rng_for(5).permutation(B)[:77].copy()).to(DEV)
    excl_p = [[int(b), 2 * int(b), 5] for b in perm.tolist()]
    eo_p, er_p = (dev(a) for a in excl_csr(excl_p))
    moved = ops.topk_sample_dot(td, ud[perm].contiguous(), k, TAU, SEED, keys[perm].contiguous(), eo_p, er_p)
    assert torch.equal(moved[0], first[0][perm]) and torch.equal(moved[1], first[1][perm])
    for b in (0, 64, 129):  # ... and called alone
        one = ops.topk_sample_dot(td, ud[b:b + 1], k, TAU, SEED, keys[b:b + 1].contiguous(), eo[b:b + 2], er)
        assert torch.equal(one[0], first[0][b:b + 1]) and torch.equal(one[1], first[1][b:b + 1]), b
    # another key: another list; no keys: the user's index in the call
    assert not torch.equal(ops.topk_sample_dot(td, ud, k, TAU, SEED, keys + 1, eo, er)[0], first[0])
    none = ops.topk_sample_dot(td, ud, k, TAU, SEED, None, eo, er)
    arange = ops.topk_sample_dot(td, ud, k, TAU, SEED, torch.arange(B, device=DEV), eo, er)
    assert torch.equal(none[0], arange[0]) and torch.equal(none[1], arange[1]) and not torch.equal(none[0], first[0])
    # a window changes which keys are looked at, never a key: the users whose window is the whole table keep their lists
    lo = torch.zeros(B, dtype=torch.int32, device=DEV)
    hi = torch.full((B,), N, dtype=torch.int32, device=DEV)
    hi[1::2] = N // 2
    win = ops.topk_sample_dot(td, ud, k, TAU, SEED, keys, eo, er, win_lo=lo, win_hi=hi)
    assert torch.equal(win[0][::2], first[0][::2]) and torch.equal(win[1][::2], first[1][::2]) and (win[0][1::2] < N // 2).all()


# ------------------------------------------------------------------------------------------- 3. prefix
@pytest.mark.parametrize("kind", ["dot", "fc"])
def test_prefix_across_the_shallow_and_the_deep_form(kind):
    B, N, E = (130, 2100, 64) if kind == "dot" else (5, 300, 14)
    t, u = operands(B, N, E, 7)
    scorer, _ = make_scorer(kind, E, synth.rng_for(7))
    with torch.no_grad():
        table, ud = scorer.prepare_csr(dev(t)), dev(u)
        rows, keys = scorer.topk_sample(table, ud, 300, TAU, SEED)
        for j in (1, 10, 128, 129):  # the keys do not depend on k: neither on the instantiation nor on the floor sweep
            r, s = scorer.topk_sample(table, ud, j, TAU, SEED)
            assert torch.equal(r, rows[:, :j]) and torch.equal(s, keys[:, :j]), (kind, j)
    assert (rows >= 0).all() and (keys[:, :-1] >= keys[:, 1:]).all()


# ------------------------------------------------------------------------------------------- 4. the cold limit
@pytest.mark.parametrize("k", [10, 129])
def test_cold_limit_is_topk_deep(k):
    """Integer scores whose gaps are >= 1 at temperature 1/64: the gaps of score / temperature are 64, above the range of the
    draw (< 26), so the noise cannot change the order: the rows are topk_deep's exactly, the keys the scores * 64 + g."""
    B, N, E = 130, 300, 7
    rng = synth.rng_for(44)
    t = np.zeros((N, E), dtype=np.float32)
    for e in range(E):
        t[:, e] = rng.permutation(N) - N // 2  # every column holds distinct integers
    u = np.zeros((B, E), dtype=np.float32)
    u[np.arange(B), np.arange(B) % E] = np.where(np.arange(B) % 2 == 0, 1.0, -1.0)  # +- one column: distinct integer scores
    td, ud = dev(t), dev(u)
    eo, er = (dev(a) for a in excl_csr([[b % N, (b * 7) % N] for b in range(B)]))
    want = ops.topk_deep_dot(td, ud, k, eo, er, 3)
    rows, keys = ops.topk_sample_dot(td, ud, k, 1.0 / 64, SEED, None, eo, er, 3)
    assert torch.equal(rows, want[0])
    g = (keys - want[1] * 64).cpu().numpy()
    assert (g > SR.GUMBEL_MIN - 1e-2).all() and (g < SR.GUMBEL_MAX + 1e-2).all()  # (fp32 at |key| ~ 1e4: ulp 1e-3)
    x = SR.draw_words(SEED, np.arange(B), N)
    g64 = np.take_along_axis(SR.gumbel64(x), rows.cpu().numpy().astype(np.int64), axis=1)
    assert np.abs(g - g64).max() <= 32 * 2.0 ** -23 * float(keys.abs().max())


# ------------------------------------------------------------------------------------------- 5. the distribution
@pytest.mark.parametrize("tau", [0.5, 2.0])
def test_the_lists_are_plackett_luce_draws(tau):
    """8 rows, 8192 identical users with the keys 0 .. 8191: first-place frequencies and ordered first-two pairs within 5
    binomial standard deviations of Plackett-Luce (the fp64 reference of the same draws sits inside 4:
    tests/test_sample_host.py)."""
    n, E = 8192, 7
    t = np.zeros((8, E), dtype=np.float32)
    t[:, 0] = SR.PL_SCORES
    u = np.zeros((n, E), dtype=np.float32)
    u[:, 0] = 1.0
    rows, _ = ops.topk_sample_dot(dev(t), dev(u), 2, tau, 1234)
    rows = rows.cpu().numpy()
    assert (rows >= 0).all() and (rows < 8).all() and (rows[:, 0] != rows[:, 1]).all()
    z1, z2 = SR.worst_sigma(rows, t[:, 0].astype(np.float64), tau)
    print(f"MARGIN Plackett-Luce tau {tau}: first places within {z1:.2f} sigma, ordered pairs within {z2:.2f} sigma (bar 5)")
    assert z1 <= 5 and z2 <= 5
    # the device draws what the reference draws: the same lists but for keys that differ in the last bits
    key64 = SR.keys64(np.tile(t[:, 0].astype(np.float64), (n, 1)), tau, 1234, np.arange(n))
    assert np.mean(rows == SR.reference_lists(key64, np.ones((n, 8), dtype=bool), 2)) > 0.999


# ------------------------------------------------------------------------------------------- 6. edge scores
def test_nan_never_wins_minus_inf_comes_last_and_short_lists_end_in_fillers():
    B, N, E, k = 5, 40, 7, 200  # (the deep form)
    t, u = (a.copy() for a in operands(B, N, E, 8))
    u[:, 0] = 1.0
    t[[3, 17], 2] = np.nan
    t[[5, 6], 0] = -np.inf
    s64 = u.astype(np.float64) @ t.astype(np.float64).T
    assert np.isnan(s64[:, [3, 17]]).all() and np.isneginf(s64[:, [5, 6]]).all()
    key64 = SR.keys64(s64, TAU, SEED, np.arange(B))
    ok = SR.eligible_mask(B, N)
    tol = SR.tolerance(key64, ok)
    rows, keys = ops.topk_sample_dot(dev(t), dev(u), k, TAU, SEED)
    SR.check_sampled_topk(rows.cpu().numpy(), keys.cpu().numpy(), key64, ok, k, tol)
    r, s = rows.cpu().numpy(), keys.cpu().numpy()
    assert not np.isin(r, [3, 17]).any() and np.isfinite(s[:, :36]).all()
    assert (r[:, 36:38] == [5, 6]).all() and np.isneginf(s[:, 36:]).all() and (r[:, 38:] == -1).all()
    # the same through the shallow form, and with every row gone
    r10, s10 = ops.topk_sample_dot(dev(t), dev(u), 10, TAU, SEED)
    assert torch.equal(r10, rows[:, :10]) and torch.equal(s10, keys[:, :10])
    none = ops.topk_sample_dot(dev(t), dev(u), 3, TAU, SEED, win_lo=torch.zeros(B, dtype=torch.int32, device=DEV),
                               win_hi=torch.zeros(B, dtype=torch.int32, device=DEV))
    assert (none[0] == -1).all() and torch.isneginf(none[1]).all()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            ops.topk_sample_dot(dev(t), dev(u), 3, bad, SEED)
    with pytest.raises(hip.XnrsHipError, match="invalid argument"):
        ops.topk_sample_dot(dev(t), dev(u), 1025, TAU, SEED)


# ------------------------------------------------------------------------------------------- 7. the API
@pytest.mark.parametrize("kind", ["dot", "bilin", "fc"])
def test_recommend_sampled(kind):
    from tests.test_hip_scorers import _eval_model
    n_news, n_sess, k, tau, seed = 90, 40, 10, 0.3, 77
    store, beh = synth.click_world(n_news=n_news, n_sess=n_sess)
    store, beh = store.to(DEV), beh.to(DEV)
    model = _eval_model(kind)
    rows, scores, keys = EV.recommend_sampled(model, store, beh, 8, k, tau, seed, return_keys=True)
    assert rows.shape == scores.shape == keys.shape == (n_sess, k) and rows.dtype == torch.int32 and (rows >= 0).all()
    small = EV.recommend_sampled(model, store, beh, 8, k, tau, seed, batch=3, return_keys=True)
    assert all(torch.equal(a, b) for a, b in zip(small, (rows, scores, keys)))  # the bits of batch=4096
    pick = [5, 31, 3, 39, 32, 0]
    sub = EV.recommend_sampled(model, store, beh, 8, k, tau, seed, sessions=pick, batch=4)
    assert len(sub) == 2 and torch.equal(sub[0], rows[pick]) and torch.equal(sub[1], scores[pick])  # keyed by the session ids
    assert not torch.equal(EV.recommend_sampled(model, store, beh, 8, k, tau, seed + 1)[0], rows)
    hists = histories(beh)
    r = rows.cpu().numpy()
    assert all(not (set(r[i].tolist()) & set(hists[i])) and len(set(r[i].tolist())) == k for i in range(n_sess))
    assert store.pad_row not in r
    # the raw scores are recommend()'s for the same rows, at the bar of two GPU paths in another summation order
    all_rows, all_scores = EV.recommend(model, store, beh, 8, k=n_news + 1)
    dense = torch.full((n_sess, store.n_rows + 1), float("nan"), device=DEV)
    dense.scatter_(1, torch.where(all_rows >= 0, all_rows, torch.full_like(all_rows, store.n_rows)).long(), all_scores)
    want = dense.gather(1, rows.long())
    tol = SWITCH_TOL * float(all_scores[all_rows >= 0].abs().max())
    err = float((scores - want).abs().max())
    assert err <= tol, (err, tol)
    # the keys are score / temperature + the draw of (seed, SESSION ID, row)
    g = np.take_along_axis(SR.gumbel64(SR.draw_words(seed, np.arange(n_sess), store.n_rows)), r.astype(np.int64), axis=1)
    key64 = want.double().cpu().numpy() / tau + g
    ktol = 32 * 2.0 ** -23 * max(1.0, float(np.abs(key64).max()))
    kerr = float(np.abs(keys.double().cpu().numpy() - key64).max())
    assert kerr <= ktol and (keys[:, :-1] >= keys[:, 1:]).all()
    print(f"MARGIN recommend_sampled {kind}: raw scores vs recommend {err / tol:.3f}, keys vs fp64 {kerr / ktol:.3f} (error / bar)")
    # windows and short lists: -1 places carry -inf scores
    lo = torch.zeros(n_sess, dtype=torch.int32, device=DEV)
    hi = torch.full((n_sess,), 6, dtype=torch.int32, device=DEV)
    wr, ws = EV.recommend_sampled(model, store, beh, 8, k, tau, seed, windows=(lo, hi), exclude_history=False)
    assert (wr[:, :5] >= 0).all() and (wr[:, :5] < 6).all() and (wr[:, 5:] == -1).all()  # (rows 0 .. 5 less the pad row)
    assert torch.isfinite(ws[:, :5]).all() and torch.isneginf(ws[:, 5:]).all()


@pytest.mark.parametrize("kind,scoring", [("NRMS", "dot"), ("standard", "bilin")])
def test_mined_negatives_loss_with_a_temperature(kind, scoring):
    from tests import test_hip_list_loss_model as LM
    from tests import test_hip_table_loss_model as TLM
    model, store, beh = LM.build(kind, scoring)
    sess, tau, seed = LM.SESS, 0.5, 5
    model.zero_grad(set_to_none=True)
    got, rows = losses.mined_negatives_loss(model, store, beh, sess, LM.L_HIST, n_negatives=8, temperature=tau, seed=seed,
                                            return_negatives=True)
    got.backward()
    g_got = TLM.grads_of(model)
    assert rows.shape == (len(sess), 8) and rows.dtype == torch.int32
    vecs, u, hist, tgt, _, pad_row = LM.operands(model, store, beh)
    # never the pad row, a click or a history row
    ho, hr, to, tr = hist[0].tolist(), hist[1].tolist(), tgt[0].tolist(), tgt[1].tolist()
    for b, l in enumerate(rows.tolist()):
        banned = set(hr[ho[b]:ho[b + 1]]) | set(tr[to[b]:to[b + 1]]) | {pad_row}
        assert len(set(l)) == 8 and not set(l) & banned and all(0 <= x < store.n_rows for x in l), b
    # the lists are the scorer's topk_sample under the merged exclusions, keyed by the session ids
    excl = losses.merged_exclusions(hist, tgt)
    with torch.no_grad():
        want_rows = model.rec_model.topk_sample(vecs, u, 8, tau, seed, torch.tensor(sess, device=DEV), excl[0], excl[1], pad_row)[0]
        hardest = model.rec_model.topk_deep(vecs, u, 8, excl[0], excl[1], pad_row)[0]
    assert torch.equal(rows, want_rows) and not torch.equal(rows, hardest)
    # the loss behind the lists is untouched: listed_ranking_loss on the returned rows, loss and gradients bit for bit
    want = losses.listed_ranking_loss(model.rec_model, vecs, u, tgt[0], tgt[1], rows, pad_row)
    want.backward()
    g_want = TLM.grads_of(model)
    assert torch.equal(got.detach(), want.detach()) and set(g_got) == set(g_want) and g_got
    for name in g_got:
        assert torch.equal(g_got[name], g_want[name]), name
    # another seed draws other lists; the same seed the same; windows hold
    with torch.no_grad():
        again = losses.mined_negatives_loss(model, store, beh, sess, LM.L_HIST, n_negatives=8, temperature=tau, seed=seed,
                                            return_negatives=True)
        other = losses.mined_negatives_loss(model, store, beh, sess, LM.L_HIST, n_negatives=8, temperature=tau, seed=seed + 1,
                                            return_negatives=True)
        lo = torch.arange(LM.N_SESS, dtype=torch.int32, device=DEV) % 20
        _, wrows = losses.mined_negatives_loss(model, store, beh, sess, LM.L_HIST, n_negatives=8, temperature=tau, seed=seed,
                                               windows=(lo, lo + 30), return_negatives=True)
        # temperature=None is the existing call
        plain = losses.mined_negatives_loss(model, store, beh, sess, LM.L_HIST, n_negatives=8, return_negatives=True)
        none = losses.mined_negatives_loss(model, store, beh, sess, LM.L_HIST, n_negatives=8, temperature=None, seed=None,
                                           return_negatives=True)
    assert torch.equal(again[1], rows) and torch.equal(again[0], got.detach()) and not torch.equal(other[1], rows)
    s = torch.tensor(sess, device=DEV)
    listed = wrows >= 0
    assert listed.any() and ((wrows >= lo[s][:, None]) & (wrows < (lo + 30)[s][:, None]))[listed].all()
    assert torch.equal(plain[1], hardest) and torch.equal(none[1], plain[1]) and torch.equal(none[0], plain[0])
