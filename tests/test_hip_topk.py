"""GPU: top-k rows of a news table per user (include/xnrs_hip.h: xnrs_topk / _bilinear / _mlp, csrc/topk.hip) and
evaluation.recommend on top of it.

1. exact-integer operands: every fp32 product and sum is exact in any order, so rows AND scores must equal the NumPy
   reference of the order contract (tests/topk_ref.py) bit for bit -- ties, fillers, ragged tiles, one and several slices;
2. real-valued operands against the project's own CSR scorers over all (user, row) pairs at the bar of two GPU paths of the
   same arithmetic in another summation order (2e-6 of the scale), and against the fp64 product at the forward bar;
3. exclusions, 4. NaN rows, 5. batch invariance, 6. limits, 7. hipGraph, 8. evaluation.recommend end to end.
Every real-valued case prints MARGIN = observed error / bar."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.topk_ref import topk_reference
from xnrs_amd import evaluation as EV
from xnrs_amd import hip, ops, synth
from xnrs_amd.models.blocks import BilinScoring, DotScoring, FCScoring

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWITCH_TOL = 2e-6  # two GPU paths of the same arithmetic in another summation order (tests/test_hip_random_shapes.py)

INT_SHAPES = [(1, 1, 8, 1), (3, 127, 8, 10), (3, 128, 70, 10), (3, 129, 70, 128), (130, 1000, 8, 10), (3, 2100, 300, 128),
              (66, 129, 256, 128), (5, 40, 12, 128)]
# several chunks per slice (the production geometry: thresholds, buffers and lists carried from chunk to chunk) and a last slice
# of fewer chunks than the others: chunks per slice 2 / 2 / 3, last slice 1 / 1 / 2 chunks
DEEP_SHAPES = [(1100, 8000, 8, 10), (130, 40000, 8, 128), (1100, 15900, 8, 10)]
REAL_SHAPES = [(130, 1000, 70, 10), (130, 1000, 70, 128), (3, 2100, 300, 128)]
SCORERS = ["dot", "dot_norm", "bilin", "bilin_norm", "fc"]


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def excl_csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(l) for l in lists])
    return off, np.array([v for l in lists for v in l], dtype=np.int32)


# ------------------------------------------------------------------------------------------- 1. exact integers
@functools.lru_cache(maxsize=None)
def int_case(B, N, E):
    rng = synth.rng_for(7000 + B + 3 * N + 11 * E)
    t = rng.integers(-3, 4, size=(N, E))
    u = rng.integers(-3, 4, size=(B, E))
    W = rng.integers(-2, 3, size=(E, E))
    bias = int(rng.integers(-5, 6))
    return t, u, W, bias


def int_topk(form, t, u, W, bias, k, excl=None, pad_row=-1, excl_dev=None):
    """(device result, reference) of one exact-integer call; excl_dev: the CSR as handed to the device, when it is not simply
    the CSR of `excl`."""
    if excl_dev is None and excl is not None:
        excl_dev = tuple(dev(a) for a in excl_csr(excl))
    eo, er = excl_dev if excl_dev is not None else (None, None)
    td, ud = dev(t, torch.float32), dev(u, torch.float32)
    if form == "dot":
        got = ops.topk_dot(td, ud, k, eo, er, pad_row)
        ref = u @ t.T
    else:
        got = ops.topk_bilinear(td, ud, dev(W[None], torch.float32), dev(np.array([bias]), torch.float32), k, eo, er, pad_row)
        ref = (u @ W) @ t.T + bias
    assert np.abs(ref).max() < 2 ** 24
    return got, topk_reference(ref.astype(np.float32), k, excl, pad_row)


def assert_exact(got, ref, what):
    rows, scores = got
    assert rows.dtype == torch.int32 and scores.dtype == torch.float32
    assert torch.equal(rows.cpu(), torch.from_numpy(ref[0])), f"{what}: rows"
    assert torch.equal(scores.cpu(), torch.from_numpy(ref[1])), f"{what}: scores"


@pytest.mark.parametrize("form", ["dot", "bilinear"])
@pytest.mark.parametrize("B,N,E,k", INT_SHAPES)
def test_exact_integer_operands(B, N, E, k, form):
    got, ref = int_topk(form, *int_case(B, N, E), k)
    assert_exact(got, ref, f"{form} {(B, N, E, k)}")
    if k > N:
        assert (ref[0][:, N:] == -1).all() and np.isneginf(ref[1][:, N:]).all()


@pytest.mark.parametrize("B,N,E,k,form", [s + ("dot",) for s in DEEP_SHAPES] + [DEEP_SHAPES[0] + ("bilinear",)])
def test_exact_integer_operands_over_several_chunks_per_slice(B, N, E, k, form):
    l = hip.lib()
    slices, chunks = l.xnrs_topk_slices(B, N), -(-N // 128)
    per = -(-chunks // slices)
    assert 1 < slices < chunks and per > 1 and 0 < chunks - (slices - 1) * per < per and N % 128 != 0
    got, ref = int_topk(form, *int_case(B, N, E), k)
    assert_exact(got, ref, f"{form} {(B, N, E, k)}")


def test_the_shapes_cover_one_slice_and_a_ragged_last_slice():
    l = hip.lib()
    slices = {s: l.xnrs_topk_slices(s[0], s[1]) for s in INT_SHAPES + REAL_SHAPES}
    assert any(v == 1 for v in slices.values())
    def last_slice_is_ragged(N, v):
        per = -(-(-(-N // 128)) // v)  # chunks per slice
        return N % (128 * per) != 0
    ragged = [s for s, v in slices.items() if v > 1 and last_slice_is_ragged(s[1], v)]
    assert ragged, slices
    assert slices[(130, 1000, 8, 10)] > 1 and slices[(3, 2100, 300, 128)] > 1 and slices[(130, 1000, 70, 128)] > 1


# ------------------------------------------------------------------------------------------- 2. real-valued operands
def make_scorer(kind, E, rng):
    """The scorer module of one kind with N(0,1)-drawn weights (scaled by 1/sqrt(fan-in)), and its fp64 score function."""
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)  # noqa: E731
    if kind in ("dot", "dot_norm"):
        norm = kind == "dot_norm"
        return DotScoring(normalize=norm).to(DEV), lambda t, u: (unit(f64(u)) @ unit(f64(t)).T if norm else f64(u) @ f64(t).T)
    if kind in ("bilin", "bilin_norm"):
        norm = kind == "bilin_norm"
        m = BilinScoring(E, normalize=norm)
        W = (rng.standard_normal((E, E)) / np.sqrt(E)).astype(np.float32)
        b = rng.standard_normal(1).astype(np.float32)
        with torch.no_grad():
            m.bilin.weight.copy_(torch.from_numpy(W[None]))
            m.bilin.bias.copy_(torch.from_numpy(b))

        def ref(t, u):
            t, u = (unit(f64(t)), unit(f64(u))) if norm else (f64(t), f64(u))
            return (u @ f64(W)) @ t.T + float(b[0])
        return m.to(DEV), ref
    Hd = E // 2
    m = FCScoring(E, Hd)
    w1 = (rng.standard_normal((Hd, 2 * E)) / np.sqrt(2 * E)).astype(np.float32)
    b1, w2, b2 = (rng.standard_normal(s).astype(np.float32) for s in ((Hd,), (1, Hd), (1,)))
    with torch.no_grad():
        for p, v in ((m.fc1.weight, w1), (m.fc1.bias, b1), (m.fc2.weight, w2), (m.fc2.bias, b2)):
            p.copy_(torch.from_numpy(v))

    def ref(t, u):
        q = f64(u) @ f64(w1[:, :E]).T + f64(b1)
        p = f64(t) @ f64(w1[:, E:]).T
        return np.tanh(q[:, None, :] + p[None, :, :]) @ f64(w2[0]) + float(b2[0])
    return m.to(DEV), ref


def all_pairs(scorer, table, u):
    """The scorer's own CSR path over ALL (user, row) pairs, no ReLU -> (B, N) fp32 on the host."""
    B, N = u.shape[0], table.shape[0]
    rows = torch.arange(N, dtype=torch.int32, device=DEV).repeat(B)
    sess = torch.arange(B, dtype=torch.int32, device=DEV).repeat_interleave(N)
    return scorer.score_csr(table, rows, sess, u, relu=False).reshape(B, N).cpu().numpy()


@functools.lru_cache(maxsize=None)
def real_case(kind, B, N, E):
    """-> (scorer, table as prepared, u, the all-pairs CSR scores, the fp64 scores): computed once, shared, never changed"""
    rng = synth.rng_for(9000 + SCORERS.index(kind) + 7 * B + 3 * N + 11 * E)
    t = rng.standard_normal((N, E)).astype(np.float32)
    u = rng.standard_normal((B, E)).astype(np.float32)
    scorer, ref64 = make_scorer(kind, E, rng)
    with torch.no_grad():
        table = scorer.prepare_csr(dev(t))
        ud = dev(u)
        ref = all_pairs(scorer, table, ud)
    return scorer, table, ud, ref, ref64(t, u)


def check_topk(rows, scores, ref, k, tol, excl=None, pad_row=-1):
    """Criteria (a)-(e) of every user against the all-pairs reference scores `ref`:(B, N); -> (share of the users whose
    returned SET had to equal the reference's, the worst |score - ref| of a returned entry)."""
    rows, scores = rows.cpu().numpy(), scores.cpu().numpy()
    B, N = ref.shape
    assert rows.shape == scores.shape == (B, k)
    decided, worst = 0, 0.0
    for b in range(B):
        ok = ~np.isnan(ref[b])
        if 0 <= pad_row < N:
            ok[pad_row] = False
        if excl is not None:
            e = np.asarray(list(excl[b]), dtype=np.int64)
            ok[e[(e >= 0) & (e < N)]] = False
        n_real = min(k, int(ok.sum()))
        r, s = rows[b, :n_real], scores[b, :n_real]
        # (a) distinct, eligible, no filler while eligible rows remain; fillers behind
        assert (r >= 0).all() and (r < N).all() and len(set(r.tolist())) == n_real and ok[r].all(), (b, r)
        assert (rows[b, n_real:] == -1).all() and np.isneginf(scores[b, n_real:]).all(), b
        if n_real == 0:
            decided += 1
            continue
        # (b) the scores are the reference's
        fin = np.isfinite(ref[b, r])
        assert (s[~fin] == ref[b, r][~fin]).all(), b  # an infinite score is returned as it is
        err = float(np.abs(s[fin].astype(np.float64) - ref[b, r][fin]).max()) if fin.any() else 0.0
        worst = max(worst, err)
        assert err <= tol, (b, err, tol)
        # (c) non-increasing; equal neighbours in ascending row order
        assert (s[:-1] >= s[1:]).all(), b
        eq = s[:-1] == s[1:]
        assert (r[:-1][eq] < r[1:][eq]).all(), b
        # (d) nothing clearly better was left out
        left = ok.copy()
        left[r] = False
        if left.any():
            assert ref[b][left].max() <= ref[b, r].min() + 2 * tol, b
        # (e) a clear gap behind the reference's k-th score: the same set
        order = np.sort(ref[b][ok].astype(np.float64))[::-1]
        if order.size <= k or order[k - 1] - order[k] > 2 * tol:
            want = topk_reference(ref[b:b + 1], k, None if excl is None else [excl[b]], pad_row)[0][0, :n_real]
            assert set(r.tolist()) == set(want.tolist()), b
            decided += 1
    return decided / B, worst


@pytest.mark.parametrize("kind", SCORERS)
@pytest.mark.parametrize("B,N,E,k", REAL_SHAPES)
def test_real_valued_operands(B, N, E, k, kind):
    scorer, table, u, ref, ref64 = real_case(kind, B, N, E)
    tol = SWITCH_TOL * float(np.abs(ref).max())
    # on the reference alone: criterion (e) must decide at least 95 % of the users of the case
    order = -np.sort(-ref.astype(np.float64), axis=1)
    assert np.mean(order[:, k - 1] - order[:, k] > 2 * tol) >= 0.95
    with torch.no_grad():
        rows, scores = scorer.topk(table, u, k)
    share, worst = check_topk(rows, scores, ref, k, tol)
    assert share >= 0.95
    got64 = np.take_along_axis(ref64, rows.cpu().numpy().astype(np.int64), axis=1)
    e64 = H.assert_close(scores, got64, H.RTOL, f"{kind} {(B, N, E, k)} scores vs fp64")
    print(f"MARGIN topk {kind} {(B, N, E, k)}: vs CSR scorer {worst / tol:.3f}  vs fp64 {e64 / H.RTOL:.3f}  (error / bar); "
          f"set decided for {100 * share:.1f} % of the users")


# ------------------------------------------------------------------------------------------- 3. exclusions
@pytest.mark.parametrize("form", ["dot", "bilinear"])
def test_exclusions(form):
    B, N, E, k = 5, 300, 8, 10
    t, u, W, bias = int_case(B, N, E)
    full = (u @ t.T) if form == "dot" else ((u @ W) @ t.T + bias)
    best = np.lexsort((np.arange(N)[None, :].repeat(B, 0), -full), axis=1)  # every user's rows, best first
    pad_row = int(best[4, 0])  # the pad row is the last user's best row
    keep3 = [int(r) for r in best[1] if r != pad_row][5:8]
    excl = [
        [int(best[0, 3]), N + 7, int(best[0, 0]), int(best[0, 3]), int(best[0, 1]), int(best[0, 0])],  # unsorted, duplicates, an id
        [r for r in range(N - 1, -1, -1) if r not in keep3],                                           # outside the table; all but 3
        list(range(N)),                                                                                # everything
        [],
        [int(best[4, 2])],
    ]
    got, ref = int_topk(form, t, u, W, bias, k, excl, pad_row)
    assert_exact(got, ref, f"{form} exclusions")
    rows = got[0].cpu().numpy()
    assert best[0, 0] not in rows[0] and best[0, 1] not in rows[0] and rows[0, 0] == [r for r in best[0] if r not in excl[0] and r != pad_row][0]
    assert sorted(rows[1, :3].tolist()) == sorted(keep3) and (rows[1, 3:] == -1).all()
    assert (rows[2] == -1).all() and np.isneginf(got[1].cpu().numpy()[2]).all()
    assert pad_row not in rows and rows[4, 0] == best[4, 1] and best[4, 2] not in rows[4]
    # the offsets are absolute: a slice of a longer offset array over the whole value array
    off, val = excl_csr([[1, 2, 3, 4, 5, 6, 7]] + excl + [[9, 9]])
    off_d, val_d = dev(off), dev(val)
    got2, _ = int_topk(form, t, u, W, bias, k, excl, pad_row, excl_dev=(off_d[1:B + 2], val_d))
    assert_exact(got2, ref, f"{form} exclusions through a slice of a longer offset array")


# ------------------------------------------------------------------------------------------- 4. NaN
def test_a_nan_row_is_never_returned():
    B, N, E, k = 3, 130, 12, 128
    t, u, _, _ = int_case(B, N, E)
    t = t.astype(np.float32)
    t[5] = np.nan
    t[77, 3] = np.nan
    ref = u.astype(np.float32) @ np.where(np.isnan(t), 0, t).T
    ref[:, [5, 77]] = np.nan
    got = ops.topk_dot(dev(t), dev(u, torch.float32), k)
    assert_exact(got, topk_reference(ref, k), "NaN rows")
    rows = got[0].cpu().numpy()
    assert 5 not in rows and 77 not in rows and (rows >= 0).all()  # 128 of the 128 finite rows
    # a normalising scorer: a zero vector has no direction (0 / 0), as a table row and as a user
    t[5] = 0
    t[77] = 1
    uu = u.astype(np.float32)
    uu[1] = 0
    scorer = DotScoring(normalize=True)
    with torch.no_grad():
        rows, scores = scorer.topk(scorer.prepare_csr(dev(t)), dev(uu), k)
    rows, scores = rows.cpu().numpy(), scores.cpu().numpy()
    assert 5 not in rows and (rows[[0, 2]] >= 0).all()  # 129 rows with a direction
    assert (rows[1] == -1).all() and np.isneginf(scores[1]).all()


def test_infinite_scores_are_legal():
    """-inf is a score like any other: its rows come behind every finite score, in row order, and before any filler (a
    filler never takes the place of an eligible row); +inf ranks first."""
    B, N, E, k = 3, 40, 12, 128
    t, u, _, _ = int_case(B, N, E)
    t, u = t.astype(np.float32), u.astype(np.float32)
    u[:, 0] = 2
    t[[3, 17, 30], 0] = -np.inf
    t[22, 0] = np.inf
    with np.errstate(invalid="ignore"):
        ref = u @ t.T
    assert np.isneginf(ref[:, [3, 17, 30]]).all() and np.isposinf(ref[:, 22]).all() and not np.isnan(ref).any()
    got = ops.topk_dot(dev(t), dev(u), k)
    assert_exact(got, topk_reference(ref, k), "infinite scores")
    rows = got[0].cpu().numpy()
    assert (rows[:, 0] == 22).all() and (rows[:, N - 3:N] == [3, 17, 30]).all() and (rows[:, N:] == -1).all()
    got = ops.topk_dot(dev(t), dev(u), 39)  # k inside the table: 37 rows above -inf, then the first two -inf rows
    assert_exact(got, topk_reference(ref, 39), "infinite scores, k = 39")
    assert (got[0].cpu().numpy()[:, -2:] == [3, 17]).all()


# ------------------------------------------------------------------------------------------- 5. batch invariance
@pytest.mark.parametrize("kind", ["dot", "fc"])
def test_a_users_result_does_not_depend_on_the_batch(kind):
    B, N, E, k = 130, 1000, 70, 128
    scorer, table, u, _, _ = real_case(kind, B, N, E)
    with torch.no_grad():
        rows, scores = scorer.topk(table, u, k)
        again = scorer.topk(table, u, k)
        assert torch.equal(rows, again[0]) and torch.equal(scores, again[1])  # run to run
        for b in (0, 63, 64, 127, 129):
            r1, s1 = scorer.topk(table, u[b:b + 1], k)
            assert torch.equal(r1[0], rows[b]) and torch.equal(s1[0], scores[b]), (kind, b)


# ------------------------------------------------------------------------------------------- 6. limits
def test_limits_and_refusals_write_nothing():
    B, N, E = 3, 200, 8
    t, u, _, _ = int_case(B, N, E)
    td, ud = dev(t, torch.float32), dev(u, torch.float32)
    for k in (0, 129):
        with pytest.raises(hip.XnrsHipError, match=r"invalid argument.*code -1"):  # XNRS_EINVAL
            ops.topk_dot(td, ud, k)
    with pytest.raises(RuntimeError, match="given together"):
        ops.topk_dot(td, ud, 10, excl_off=torch.zeros(B + 1, dtype=torch.int64, device=DEV))
    l = hip.lib()
    k = 10
    rows = torch.full((B, 130), -7, dtype=torch.int32, device=DEV)
    scores = torch.full((B, 130), 123.0, dtype=torch.float32, device=DEV)
    nbytes = l.xnrs_topk_workspace_bytes(B, N, 0, k)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    st = hip.stream_ptr(DEV)

    def call(k, ws_bytes, rows_t=rows):
        return l.xnrs_topk(hip.ptr(td), N, E, hip.ptr(ud), B, None, None, -1, k, hip.ptr(rows_t), hip.ptr(scores), hip.ptr(ws),
                           ws_bytes, st)
    assert call(129, nbytes) == -1 and call(0, nbytes) == -1 and call(k, nbytes, None) == -1  # XNRS_EINVAL
    assert call(k, nbytes - 1) == -3  # XNRS_EWORKSPACE
    torch.cuda.synchronize()
    assert (rows == -7).all() and (scores == 123.0).all() and not ws.any()
    assert call(k, nbytes) == 0
    torch.cuda.synchronize()
    want = topk_reference((u @ t.T).astype(np.float32), k)
    assert torch.equal(rows.reshape(-1)[:B * k].reshape(B, k).cpu(), torch.from_numpy(want[0]))
    assert (rows.reshape(-1)[B * k:] == -7).all()
    # n_rows == 0: fillers; B == 0: nothing
    r0, s0 = ops.topk_dot(td[:0], ud, k)
    assert (r0 == -1).all() and torch.isneginf(s0).all()
    r0, s0 = ops.topk_dot(td, ud[:0], k)
    assert r0.shape == (0, k) and s0.shape == (0, k)


# ------------------------------------------------------------------------------------------- 7. hipGraph
def test_one_call_captured_in_a_hip_graph():
    B, N, E, k = 130, 1000, 70, 10
    scorer, table, u, _, _ = real_case("bilin", B, N, E)
    u_static = u.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad():
        with torch.cuda.stream(side):
            first = scorer.topk(table, u_static, k)  # warm-up on the capture stream (workspace growth)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rows_g, scores_g = scorer.topk(table, u_static, k)
        u_static.copy_(torch.flip(u, dims=[0]))
        graph.replay()
        torch.cuda.synchronize()
        eager = scorer.topk(table, torch.flip(u, dims=[0]), k)
    assert torch.equal(rows_g, eager[0]) and torch.equal(scores_g, eager[1])
    assert torch.equal(rows_g, torch.flip(first[0], dims=[0])) and not torch.equal(rows_g, first[0])


# ------------------------------------------------------------------------------------------- 8. evaluation.recommend
def histories(beh):
    off, val = beh.hist_off.cpu().numpy(), beh.hist_val.cpu().numpy()
    return [val[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


def recommend_reference(model, store, beh, l_hist):
    """encode_news_table -> prepare_csr -> encode_user -> the scorer's all-pairs CSR scores, no ReLU"""
    from xnrs_amd.data import DeviceBatcher
    with torch.no_grad():
        vecs, hm = EV.encode_news_table(model, store)
        table = model.rec_model.prepare_csr(vecs)
        sess = torch.arange(len(beh), device=DEV)
        hist = DeviceBatcher(beh, l_hist, store.pad_row).eval_batch(sess)[0]
        h, m = vecs[hist.long()], hm[hist.long()]
        uidx = getattr(beh, "user_index", None) if getattr(model, "uses_user_index", False) else None
        u = model.encode_user(h, m) if uidx is None else model.encode_user(h, m, uidx[sess])
        return all_pairs(model.rec_model, table, u.reshape(len(beh), -1))


@pytest.mark.parametrize("kind", ["dot", "dot_norm", "bilin", "bilin_norm", "fc"])
def test_recommend_end_to_end(kind):
    from tests.test_hip_scorers import _eval_model
    store, beh = synth.click_world(n_news=150, n_sess=120)
    store, beh = store.to(DEV), beh.to(DEV)
    model = _eval_model(kind)
    k = 10
    ref = recommend_reference(model, store, beh, 8)
    tol = SWITCH_TOL * float(np.abs(ref).max())
    rows, scores = EV.recommend(model, store, beh, l_hist=8, k=k, batch=32)
    assert rows.is_cuda and rows.dtype == torch.int32 and scores.dtype == torch.float32 and rows.shape == (120, k)
    hists = histories(beh)
    share, worst = check_topk(rows, scores, ref, k, tol, excl=hists, pad_row=store.pad_row)
    r = rows.cpu().numpy()
    assert all(not (set(r[i].tolist()) & set(hists[i])) for i in range(120)) and store.pad_row not in r
    # without the history exclusion only the pad row is missing
    rows_h, scores_h = EV.recommend(model, store, beh, l_hist=8, k=k, batch=32, exclude_history=False)
    share_h, worst_h = check_topk(rows_h, scores_h, ref, k, tol, pad_row=store.pad_row)
    assert store.pad_row not in rows_h.cpu().numpy() and not torch.equal(rows_h, rows)
    assert share >= 0.95 and share_h >= 0.95
    # a subset of the sessions: those rows of the full call, bit for bit
    pick = [5, 77, 3, 119, 31, 32, 0]
    rows_s, scores_s = EV.recommend(model, store, beh, l_hist=8, k=k, sessions=pick, batch=4)
    assert torch.equal(rows_s, rows[pick]) and torch.equal(scores_s, scores[pick])
    print(f"MARGIN recommend {kind}: vs CSR scorer {max(worst, worst_h) / tol:.3f}  (error / bar); set decided for "
          f"{100 * share:.1f} % / {100 * share_h:.1f} % of the sessions")


def test_recommend_refuses_npa():
    from tests.golden import npa_cases as NC
    from tests.test_hip_npa import Cfg
    from xnrs_amd.models.npa import make_npa
    store, beh = synth.click_world(n_news=40, n_sess=10)
    model = make_npa(Cfg(NC.model_cfg(dict(NC.CASES["tiny"], D=32, n_users=50), "dot"))).to(DEV).eval()
    with pytest.raises(NotImplementedError, match="depend on the user"):
        EV.recommend(model, store.to(DEV), beh.to(DEV), l_hist=5, k=5)


def test_recommend_lstur():
    from tests.golden import lstur_cases as LC
    from tests.test_hip_lstur import Cfg
    from xnrs_amd.models.lstur import make_lstur
    store, beh = synth.click_world(n_news=60, n_sess=40)
    store, beh = store.to(DEV), beh.to(DEV)
    store.columns["category_index"] = (torch.arange(store.n_rows, device=DEV, dtype=torch.int32) % 19 + 1) * (
        torch.arange(store.n_rows, device=DEV) > 0).to(torch.int32)
    c = dict(LC.SHAPES["tiny"], D=32, n_users=50, H=5, st=3, ltm="embedding", lstm="con", scoring="dot", hole=False)
    torch.manual_seed(4)
    model = make_lstur(Cfg(LC.model_cfg(c))).to(DEV).eval()
    with pytest.raises(ValueError, match="user index"):
        EV.recommend(model, store, beh, l_hist=5, k=5)
    beh.user_index = torch.arange(len(beh), device=DEV) % 7
    ref = recommend_reference(model, store, beh, 5)
    tol = SWITCH_TOL * float(np.abs(ref).max())
    rows, scores = EV.recommend(model, store, beh, l_hist=5, k=5, batch=16)
    share, worst = check_topk(rows, scores, ref, 5, tol, excl=histories(beh), pad_row=store.pad_row)
    assert share >= 0.95
    print(f"MARGIN recommend LSTUR: vs CSR scorer {worst / tol:.3f}  (error / bar); set decided for {100 * share:.1f} % of the sessions")
