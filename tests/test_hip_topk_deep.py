"""GPU: deep top-k (include/xnrs_hip.h: xnrs_topk_deep / _bilinear / _mlp, 1 <= k <= 1024; csrc/topk.hip) and the deep and
two-stage forms of evaluation.recommend.

1. exact-integer operands against the NumPy reference of the order contract, bit for bit;
2. same bits as xnrs_topk* for k <= 128, and deep(k)[:, :j] == deep(j);
3. xnrs_rank* over the same arguments: rank == position with the same score bits, rank >= k for what was not returned;
4. real-valued operands against the CSR scorers over all pairs and the fp64 product (the method and bars of
   tests/test_hip_topk.py); 5. exclusions, 6. NaN / +-inf / +-0, 7. batch invariance, 8. limits, 9. hipGraph,
10. recommend(k = 200), 11. recommend(NPA, generator=NRMS)."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_hip_topk import (SCORERS, SWITCH_TOL, assert_exact, check_topk, dev, excl_csr, histories, int_case, real_case,
                                 recommend_reference)
from tests.topk_ref import topk_reference
from xnrs_amd import evaluation as EV
from xnrs_amd import hip, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# k = N one past the old limit | fillers | fillers, k far above N | several user tiles | k = N - 1, two chunks | several
# slices, k larger than a slice | several chunks per slice, a ragged last slice | a long table
INT_SHAPES = [(3, 129, 8, 129), (3, 127, 8, 200), (5, 40, 12, 1024), (130, 1000, 8, 129), (66, 1025, 256, 1024),
              (3, 2100, 300, 1024), (1100, 8000, 8, 300), (130, 40000, 8, 1024)]
REAL = (130, 2100, 70)


def int_topk_deep(form, t, u, W, bias, k, excl=None, pad_row=-1, excl_dev=None):
    """(device result, reference) of one exact-integer call (tests/test_hip_topk.py: int_topk, through the deep entry)"""
    if excl_dev is None and excl is not None:
        excl_dev = tuple(dev(a) for a in excl_csr(excl))
    eo, er = excl_dev if excl_dev is not None else (None, None)
    td, ud = dev(t, torch.float32), dev(u, torch.float32)
    if form == "dot":
        got = ops.topk_deep_dot(td, ud, k, eo, er, pad_row)
        ref = u @ t.T
    else:
        got = ops.topk_deep_bilinear(td, ud, dev(W[None], torch.float32), dev(np.array([bias]), torch.float32), k, eo, er, pad_row)
        ref = (u @ W) @ t.T + bias
    assert np.abs(ref).max() < 2 ** 24
    return got, topk_reference(ref.astype(np.float32), k, excl, pad_row)


# ------------------------------------------------------------------------------------------- 1. exact integers
@pytest.mark.parametrize("form", ["dot", "bilinear"])
@pytest.mark.parametrize("B,N,E,k", INT_SHAPES)
def test_exact_integer_operands(B, N, E, k, form):
    l = hip.lib()
    if (B, N) == (1100, 8000):  # several chunks per slice and a last slice of fewer chunks than the others
        slices, chunks = l.xnrs_topk_slices(B, N), -(-N // 128)
        per = -(-chunks // slices)
        assert 1 < slices < chunks and per > 1 and 0 < chunks - (slices - 1) * per < per and N % 128 != 0
    if (B, N) == (3, 2100):
        assert l.xnrs_topk_slices(B, N) > 1 and k > 128 * -(-(-(-N // 128)) // l.xnrs_topk_slices(B, N))  # k above a slice's rows
    got, ref = int_topk_deep(form, *int_case(B, N, E), k)
    assert_exact(got, ref, f"{form} {(B, N, E, k)}")
    if k > N:
        assert (ref[0][:, N:] == -1).all() and np.isneginf(ref[1][:, N:]).all()


# ------------------------------------------------------------------------------------------- 2. same bits, prefix
@functools.lru_cache(maxsize=None)
def deep_1024(kind):
    """topk_deep(1024) of the shared real-valued case: computed once, never changed"""
    scorer, table, u, _, _ = real_case(kind, *REAL)
    with torch.no_grad():
        return scorer.topk_deep(table, u, 1024)


@pytest.mark.parametrize("kind", SCORERS)
def test_same_bits_as_topk_and_prefix(kind):
    scorer, table, u, _, _ = real_case(kind, *REAL)
    rows, scores = deep_1024(kind)
    with torch.no_grad():
        for k in (1, 10, 128):
            a, b = scorer.topk_deep(table, u, k), scorer.topk(table, u, k)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (kind, k)
        assert torch.equal(rows[:, :128], b[0]) and torch.equal(scores[:, :128], b[1]), kind
        r300, s300 = scorer.topk_deep(table, u, 300)
    assert torch.equal(rows[:, :300], r300) and torch.equal(scores[:, :300], s300), kind
    assert (rows >= 0).all()


# ------------------------------------------------------------------------------------------- 3. rank
@pytest.mark.parametrize("kind", SCORERS)
def test_rank_is_the_position(kind):
    B, N, _ = REAL
    k = 1024
    scorer, table, u, _, _ = real_case(kind, *REAL)
    rows, scores = deep_1024(kind)
    listed = torch.zeros((B, N), dtype=torch.bool, device=DEV)
    listed.scatter_(1, rows.long(), True)
    others = torch.nonzero(~listed)[:, 1].reshape(B, N - k)[:, ::5][:, :200].to(torch.int32)  # 200 rows per user not returned
    assert others.shape == (B, 200)
    tgt = torch.cat([rows, others], dim=1).contiguous()
    off = torch.arange(B + 1, device=DEV, dtype=torch.int64) * tgt.shape[1]
    with torch.no_grad():
        ranks, rscores = scorer.rank(table, u, off, tgt.reshape(-1))
    ranks, rscores = ranks.reshape(B, -1), rscores.reshape(B, -1)
    assert torch.equal(ranks[:, :k], torch.arange(k, device=DEV, dtype=torch.int32).expand(B, k)), kind
    assert torch.equal(rscores[:, :k], scores), kind  # bit for bit
    assert (ranks[:, k:] >= k).all(), kind


# ------------------------------------------------------------------------------------------- 4. real-valued operands
@pytest.mark.parametrize("kind", SCORERS)
@pytest.mark.parametrize("k", [1024, 300])
def test_real_valued_operands(k, kind):
    B, N, E = REAL
    scorer, table, u, ref, ref64 = real_case(kind, B, N, E)
    tol = SWITCH_TOL * float(np.abs(ref).max())
    # on the reference alone: criterion (e) must decide at least 95 % of the users of the case
    order = -np.sort(-ref.astype(np.float64), axis=1)
    assert np.mean(order[:, k - 1] - order[:, k] > 2 * tol) >= 0.95
    if k == 1024:
        rows, scores = deep_1024(kind)
    else:
        with torch.no_grad():
            rows, scores = scorer.topk_deep(table, u, k)
    share, worst = check_topk(rows, scores, ref, k, tol)
    got64 = np.take_along_axis(ref64, rows.cpu().numpy().astype(np.int64), axis=1)
    e64 = H.rel_err(scores, got64)
    print(f"MARGIN topk_deep {kind} {(B, N, E, k)}: vs CSR scorer {worst / tol:.3f}  vs fp64 {e64 / H.RTOL:.3f}  (error / bar); "
          f"set decided for {100 * share:.1f} % of the users")
    assert share >= 0.95
    H.assert_close(scores, got64, H.RTOL, f"{kind} {(B, N, E, k)} scores vs fp64")


# ------------------------------------------------------------------------------------------- 5. exclusions
@pytest.mark.parametrize("form", ["dot", "bilinear"])
def test_exclusions(form):
    B, N, E, k = 5, 2300, 8, 1024
    t, u, W, bias = int_case(B, N, E)
    full = (u @ t.T) if form == "dot" else ((u @ W) @ t.T + bias)
    best = np.lexsort((np.arange(N)[None, :].repeat(B, 0), -full), axis=1)  # every user's rows, best first
    pad_row = int(best[4, 0])  # the pad row is the last user's best row
    keep3 = [int(r) for r in best[1] if r != pad_row][5:8]
    excl = [
        [int(best[0, 3]), N + 7, int(best[0, 0]), int(best[0, 3]), int(best[0, 1]), -5, int(best[0, 0])],  # unsorted, duplicates,
        [r for r in range(N - 1, -1, -1) if r not in keep3],                # ids outside the table; longer than k: all but 3
        [int(r) for r in best[2, :1100]][::-1],                             # longer than k: the user's 1100 best, 1200 remain
        [int(r) for r in best[3, 100:1400]] * 2,                            # fewer than k remain (1000): fillers
        [int(best[4, 2])],
    ]
    assert len(excl[2]) > k and N - 1300 < k
    got, ref = int_topk_deep(form, t, u, W, bias, k, excl, pad_row)
    assert_exact(got, ref, f"{form} exclusions")
    rows = got[0].cpu().numpy()
    assert best[0, 0] not in rows[0] and best[0, 1] not in rows[0] and (rows[0] >= 0).all()
    assert sorted(rows[1, :3].tolist()) == sorted(keep3) and (rows[1, 3:] == -1).all()
    assert not set(rows[2].tolist()) & set(excl[2]) and (rows[2] >= 0).all()
    n3 = N - 1300 - (pad_row not in excl[3])
    assert (rows[3, :n3] >= 0).all() and (rows[3, n3:] == -1).all()
    assert pad_row not in rows and rows[4, 0] == best[4, 1] and best[4, 2] not in rows[4]
    # the offsets are absolute: a slice of a longer offset array over the whole value array
    off, val = excl_csr([[1, 2, 3, 4, 5, 6, 7]] + excl + [[9, 9]])
    off_d, val_d = dev(off), dev(val)
    got2, _ = int_topk_deep(form, t, u, W, bias, k, excl, pad_row, excl_dev=(off_d[1:B + 2], val_d))
    assert_exact(got2, ref, f"{form} exclusions through a slice of a longer offset array")


# ------------------------------------------------------------------------------------------- 6. NaN, +-inf, +-0
def test_nan_rows_infinite_scores_and_zero_ties():
    """The `infinite scores` case of tests/test_hip_topk.py at N = 400, k = 300, with NaN rows and rows of +0 and of -0
    products: -inf rows behind every finite score in row order and before any filler, +inf first, a NaN never, zeros tie."""
    B, N, E = 3, 400, 12
    t, u, _, _ = int_case(B, N, E)
    t, u = t.astype(np.float32), u.astype(np.float32)
    u[:, 0] = 2
    t[[3, 17, 30, 333], 0] = -np.inf
    t[22, 0] = np.inf
    t[[5, 77, 140, 399]] = np.nan
    t[[8, 9, 150, 151, 250, 251]] = 0.0  # score 0 ...
    t[[9, 151, 250], 0] = -0.0           # ... through a product -0 as well
    with np.errstate(invalid="ignore"):
        ref = u @ t.T
    assert np.isneginf(ref[:, [3, 17, 30, 333]]).all() and np.isposinf(ref[:, 22]).all() and np.isnan(ref[:, [5, 77, 140, 399]]).all()
    for k in (300, 396, 400):
        got = ops.topk_deep_dot(dev(t), dev(u), k)
        assert_exact(got, topk_reference(ref, k), f"k = {k}")  # (torch.equal: -0 == +0)
        rows = got[0].cpu().numpy()
        assert (rows[:, 0] == 22).all() and not set(rows.reshape(-1).tolist()) & {5, 77, 140, 399}
    assert (rows[:, 392:396] == [3, 17, 30, 333]).all() and (rows[:, 396:] == -1).all()
    # the zero rows tie: among themselves they come in row order
    for b in range(B):
        z = [r for r in rows[b].tolist() if r in (8, 9, 150, 151, 250, 251)]
        assert z == [8, 9, 150, 151, 250, 251], (b, z)


# ------------------------------------------------------------------------------------------- 7. batch invariance
@pytest.mark.parametrize("kind", ["dot", "fc"])
def test_a_users_result_does_not_depend_on_the_batch(kind):
    k = 1024
    scorer, table, u, _, _ = real_case(kind, *REAL)
    rows, scores = deep_1024(kind)
    with torch.no_grad():
        again = scorer.topk_deep(table, u, k)
        assert torch.equal(rows, again[0]) and torch.equal(scores, again[1])  # run to run
        for b in (0, 63, 64, 127, 129):
            r1, s1 = scorer.topk_deep(table, u[b:b + 1], k)
            assert torch.equal(r1[0], rows[b]) and torch.equal(s1[0], scores[b]), (kind, b)


# ------------------------------------------------------------------------------------------- 8. limits
def test_limits_and_refusals_write_nothing():
    B, N, E = 3, 200, 8
    t, u, _, _ = int_case(B, N, E)
    td, ud = dev(t, torch.float32), dev(u, torch.float32)
    for k in (0, 1025):
        with pytest.raises(hip.XnrsHipError, match=r"invalid argument.*code -1"):  # XNRS_EINVAL
            ops.topk_deep_dot(td, ud, k)
    l = hip.lib()
    k = 300
    rows = torch.full((B, 1030), -7, dtype=torch.int32, device=DEV)
    scores = torch.full((B, 1030), 123.0, dtype=torch.float32, device=DEV)
    nbytes = l.xnrs_topk_deep_workspace_bytes(B, N, 0, k)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    st = hip.stream_ptr(DEV)

    def call(k, ws_bytes, rows_t=rows):
        return l.xnrs_topk_deep(hip.ptr(td), N, E, hip.ptr(ud), B, None, None, -1, k, hip.ptr(rows_t), hip.ptr(scores), hip.ptr(ws),
                                ws_bytes, st)
    assert call(1025, nbytes) == -1 and call(0, nbytes) == -1 and call(k, nbytes, None) == -1  # XNRS_EINVAL
    assert call(k, nbytes - 1) == -3  # XNRS_EWORKSPACE
    torch.cuda.synchronize()
    assert (rows == -7).all() and (scores == 123.0).all() and not ws.any()
    assert call(k, nbytes) == 0
    torch.cuda.synchronize()
    want = topk_reference((u @ t.T).astype(np.float32), k)
    assert torch.equal(rows.reshape(-1)[:B * k].reshape(B, k).cpu(), torch.from_numpy(want[0]))
    assert (rows.reshape(-1)[B * k:] == -7).all()
    # n_rows == 0: fillers; B == 0: nothing
    r0, s0 = ops.topk_deep_dot(td[:0], ud, k)
    assert r0.shape == (B, k) and (r0 == -1).all() and torch.isneginf(s0).all()
    r0, s0 = ops.topk_deep_dot(td, ud[:0], k)
    assert r0.shape == (0, k) and s0.shape == (0, k)


# ------------------------------------------------------------------------------------------- 9. hipGraph
def test_one_call_captured_in_a_hip_graph():
    k = 300
    scorer, table, u, _, _ = real_case("bilin", *REAL)
    u_static = u.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad():
        with torch.cuda.stream(side):
            first = scorer.topk_deep(table, u_static, k)  # warm-up on the capture stream (workspace growth)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rows_g, scores_g = scorer.topk_deep(table, u_static, k)
        u_static.copy_(torch.flip(u, dims=[0]))
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
        eager = scorer.topk_deep(table, torch.flip(u, dims=[0]), k)
    assert torch.equal(rows_g, eager[0]) and torch.equal(scores_g, eager[1])
    assert torch.equal(rows_g, torch.flip(first[0], dims=[0])) and not torch.equal(rows_g, first[0])


# ------------------------------------------------------------------------------------------- 10. recommend(k = 200)
@pytest.mark.parametrize("kind", SCORERS)
def test_recommend_deep_end_to_end(kind):
    from tests.test_hip_scorers import _eval_model
    store, beh = synth.click_world(n_news=150, n_sess=120)
    store, beh = store.to(DEV), beh.to(DEV)
    model = _eval_model(kind)
    k = 200  # above the table: every eligible news of a session, then fillers
    ref = recommend_reference(model, store, beh, 8)
    tol = SWITCH_TOL * float(np.abs(ref).max())
    rows, scores = EV.recommend(model, store, beh, l_hist=8, k=k, batch=32)
    assert rows.is_cuda and rows.dtype == torch.int32 and scores.dtype == torch.float32 and rows.shape == (120, k)
    hists = histories(beh)
    share, worst = check_topk(rows, scores, ref, k, tol, excl=hists, pad_row=store.pad_row)
    r = rows.cpu().numpy()
    assert all(not (set(r[i].tolist()) & set(hists[i])) for i in range(120)) and store.pad_row not in r
    rows_h, scores_h = EV.recommend(model, store, beh, l_hist=8, k=k, batch=32, exclude_history=False)
    share_h, worst_h = check_topk(rows_h, scores_h, ref, k, tol, pad_row=store.pad_row)
    assert store.pad_row not in rows_h.cpu().numpy() and not torch.equal(rows_h, rows)
    assert (rows_h[:, :150] >= 0).all() and (rows_h[:, 150:] == -1).all()
    assert share >= 0.95 and share_h >= 0.95
    # the first 10 places are recommend(k = 10), bit for bit
    rows_10, scores_10 = EV.recommend(model, store, beh, l_hist=8, k=10, batch=32)
    assert torch.equal(rows[:, :10], rows_10) and torch.equal(scores[:, :10], scores_10)
    # a subset of the sessions: those rows of the full call, bit for bit
    pick = [5, 77, 3, 119, 31, 32, 0]
    rows_s, scores_s = EV.recommend(model, store, beh, l_hist=8, k=k, sessions=pick, batch=4)
    assert torch.equal(rows_s, rows[pick]) and torch.equal(scores_s, scores[pick])
    print(f"MARGIN recommend deep {kind}: vs CSR scorer {max(worst, worst_h) / tol:.3f}  (error / bar); set decided for "
          f"{100 * share:.1f} % / {100 * share_h:.1f} % of the sessions")


# ------------------------------------------------------------------------------------------- 11. two stages
def _npa_and_nrms():
    from tests.helpers import npa_and_nrms
    return npa_and_nrms(DEV)


def _npa_scores(npa, store, beh, l_hist, cand):
    """NPA's raw scores of the candidate rows cand[i] of every session i -> (n_sess, n_rows), NaN where not scored"""
    from xnrs_amd.data import DeviceBatcher
    n = len(beh)
    sess = torch.arange(n, device=DEV)
    hist = DeviceBatcher(beh, l_hist, store.pad_row).eval_batch(sess)[0]
    crows = torch.tensor([r for c in cand for r in c], dtype=torch.int32, device=DEV)
    csess = torch.tensor([i for i, c in enumerate(cand) for _ in c], dtype=torch.int32, device=DEV)
    with torch.no_grad():
        r = npa.score_impressions(store, hist, crows, csess, beh.user_index[sess], relu=False)
    out = np.full((n, store.n_rows), np.nan, dtype=np.float32)
    out[csess.cpu().numpy(), crows.cpu().numpy()] = r.cpu().numpy()
    return out


def test_recommend_two_stages():
    store, beh = synth.click_world(n_news=40, n_sess=10)
    store, beh = store.to(DEV), beh.to(DEV)
    npa, nrms = _npa_and_nrms()
    k, l_hist, n, N = 5, 5, len(beh), store.n_rows
    # (c) refusals
    with pytest.raises(ValueError, match="user index"):
        EV.recommend(npa, store, beh, l_hist=l_hist, k=k, generator=nrms)
    beh.user_index = torch.arange(n, device=DEV) % 7
    with pytest.raises(NotImplementedError, match="depend on the user"):
        EV.recommend(npa, store, beh, l_hist=l_hist, k=k)
    hists = histories(beh)
    # (a) a pool that holds the whole table: NPA's own top k over every eligible news
    ref = _npa_scores(npa, store, beh, l_hist, [list(range(N))] * n)
    tol = SWITCH_TOL * float(np.abs(ref).max())
    for excl_hist in (True, False):
        rows, scores = EV.recommend(npa, store, beh, l_hist=l_hist, k=k, generator=nrms, pool=128, batch=4, exclude_history=excl_hist)
        assert rows.shape == (n, k) and rows.dtype == torch.int32 and scores.dtype == torch.float32
        share, worst = check_topk(rows, scores, ref, k, tol, excl=hists if excl_hist else None, pad_row=store.pad_row)
        print(f"MARGIN recommend NPA over NRMS, whole table, exclude_history={excl_hist}: vs score_impressions {worst / tol:.3f} "
              f"(error / bar); set decided for {100 * share:.1f} % of the sessions")
    # (b) a pool of 16: only the generator's 16, in the order of NPA's scores over exactly those
    gen_rows, _ = EV.recommend(nrms, store, beh, l_hist=l_hist, k=16)
    gen = [[r for r in g if r >= 0] for g in gen_rows.cpu().numpy().tolist()]
    assert all(len(g) == 16 for g in gen)
    rows, scores = EV.recommend(npa, store, beh, l_hist=l_hist, k=k, generator=nrms, pool=16)
    r = rows.cpu().numpy()
    assert all(set(r[i].tolist()) <= set(gen[i]) for i in range(n))
    ref16 = _npa_scores(npa, store, beh, l_hist, gen)
    check_topk(rows, scores, ref16, k, SWITCH_TOL * float(np.nanmax(np.abs(ref16))))
    # the default pool (128 here) holds the table again; a subset of the sessions is those rows of the full call
    full = EV.recommend(npa, store, beh, l_hist=l_hist, k=k, generator=nrms)
    check_topk(full[0], full[1], ref, k, tol, excl=hists, pad_row=store.pad_row)
    pick = [7, 2, 9]
    sub = EV.recommend(npa, store, beh, l_hist=l_hist, k=k, generator=nrms, sessions=pick)
    check_topk(sub[0], sub[1], ref[pick], k, tol, excl=[hists[i] for i in pick], pad_row=store.pad_row)


def test_recommend_two_stages_refuses_caum():
    from tests.golden import caum_cases as CC
    from tests.test_hip_caum import _model as caum_model
    store, beh = synth.click_world(n_news=40, n_sess=10)
    store, beh = store.to(DEV), beh.to(DEV)
    beh.user_index = torch.arange(len(beh), device=DEV) % 7
    npa, nrms = _npa_and_nrms()
    caum = caum_model(CC.CASES["tiny"]).eval()
    with pytest.raises(NotImplementedError, match="CAUM"):
        EV.recommend(caum, store, beh, l_hist=5, k=5)
    with pytest.raises(NotImplementedError, match="CAUM"):
        EV.recommend(caum, store, beh, l_hist=5, k=5, generator=nrms)
    with pytest.raises(NotImplementedError, match="CAUM"):
        EV.recommend(npa, store, beh, l_hist=5, k=5, generator=caum)
