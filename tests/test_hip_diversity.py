"""GPU: xnrs_row_inv_norms, xnrs_mmr_rerank, xnrs_list_diversity (include/xnrs_hip.h; csrc/diversity.hip) against the fp64
reference tests/diversity_ref.py, their contracts, and evaluation.recommend_diverse / diversity_metrics / evaluate_diversity
end to end.

Exact operands: table rows with exactly four non-zero entries of +-1/2 (every norm exactly 1, every cosine a multiple of 1/4),
scores multiples of 1/8 in [-4, 4] whose valid values span a power of two per session, lam in {0, 1/4, 1/2, 1}: every objective
is exact in fp32, ties are frequent, and rows, score bits and positions must EQUAL the reference's.
Real operands: every pick of the kernel, evaluated in fp64 given the kernel's own earlier picks, is within
  tau = 2 * ((E + 8) + 2 * max|r|) * 2^-24
of the fp64 maximum over the remaining valid places (the dot-product error bound for unit-norm operands, plus the roundings of
the normalisation and of lam * r, times two because two objectives are compared); ild is within
  ((E + 8) + 2 * (n_pairs - 1)) * 2^-24
of the fp64 value (one term's worst case plus any-order fp32 summation of terms in [0, 2]).

The exact shapes are the issue's plus E = 21: 20 is a multiple of 4, so without it no exact case would take the scalar loads.

Value-only mutations, each made in a scratch build and never committed:
  m_i starts as max(0, cos) instead of cos at the first pick: 7 cases failed (every exact MMR shape with P > 1 and the three
      real-operand MMR cases; run before the E = 21 cases existed)
  equal objectives go to the HIGHER place, and in the same build the scalar form of load4 drops its fourth element: 12 of 29
      failed (every exact MMR shape with P > 1; MMR and ILD at E = 21; the E = 70 real-operand MMR and ILD cases; the
      unaligned table / all cases, which compare two GPU runs and so see the load alone)."""
import numpy as np
import pytest
import torch

from tests import align_ref as A
from tests import diversity_ref as R
from xnrs_amd import evaluation as EV
from xnrs_amd import hip, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
N_ROWS = 300
LAMS = (0.0, 0.25, 0.5, 1.0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.view(torch.int32)


def exact_table(E, seed=1):
    """(N_ROWS, E): four entries of +-1/2 per row; row 0 is a zero row."""
    rng = np.random.default_rng(seed)
    t = np.zeros((N_ROWS, E), dtype=np.float32)
    for r in range(1, N_ROWS):
        t[r, rng.choice(E, size=4, replace=False)] = rng.choice([-0.5, 0.5], size=4)
    return t


def exact_pool(B, P, seed):
    """Pools with everything a pool may hold: empty places, NaN and +-inf scores, rows beyond the table, the zero row, rows
    listed twice, a session without a valid place, a session with few valid places.  The valid scores of a session span a
    power of two (its minimum and maximum are planted)."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, N_ROWS, size=(B, P)).astype(np.int32)  # (with replacement: duplicates, the zero row)
    scores = np.zeros((B, P), dtype=np.float32)
    for b in range(B):
        span = float(rng.choice([1, 2, 4]))
        lo = rng.integers(-32, int(8 * (4 - span)) + 1) / 8.0
        scores[b] = lo + rng.integers(0, int(8 * span) + 1, size=P) / 8.0
        if P >= 8:
            junk = rng.choice(P, size=P // 4, replace=False)
            kinds = rng.integers(0, 6, size=junk.size)
            rows[b, junk[kinds == 0]] = -1
            rows[b, junk[kinds == 1]] = N_ROWS + rng.integers(0, 5)
            scores[b, junk[kinds == 2]] = np.nan
            scores[b, junk[kinds == 3]] = np.inf
            scores[b, junk[kinds == 4]] = -np.inf
            rows[b, junk[kinds == 5]] = 0  # the zero row
            rows[b, P - 1] = rows[b, P // 2]  # a row listed twice
            if b == 1:  # few valid places
                rows[b, rng.choice(P, size=P - 3, replace=False)] = -1
            ok = (rows[b] >= 0) & (rows[b] < N_ROWS) & np.isfinite(scores[b])
            first = np.flatnonzero(ok)
            if first.size >= 2:
                scores[b, first[0]], scores[b, first[-1]] = lo, lo + span
    if B >= 3:
        rows[B - 1] = -1  # no valid place
    return rows, scores


def gpu_mmr(table_d, rows, scores, k, lam, rel):
    inv = ops.row_inv_norms(table_d)
    return ops.mmr_rerank(table_d, inv, dev(rows), dev(scores), k, lam, rel)


def assert_mmr_equal(got, want):
    r, s, p = (t.cpu().numpy() for t in got)
    assert (p == want[2]).all(), np.argwhere(p != want[2])[:5]
    assert (r == want[0]).all()
    assert (s.view(np.int32) == want[1].view(np.int32)).all()


# ------------------------------------------------------------------------------------------------ 1. exact arithmetic
# (E = 21: the scalar loads behind a width that is no multiple of 4; the other widths take the 16-byte loads)
@pytest.mark.parametrize("B,P,E,k", [(5, 37, 20, 7), (5, 37, 21, 7), (3, 64, 64, 64), (2, 1, 8, 1), (130, 129, 36, 33),
                                     (3, 1024, 16, 1024)])
def test_mmr_exact(B, P, E, k):
    table = exact_table(E)
    table_d = dev(table)
    inv = ops.row_inv_norms(table_d)
    want_inv = R.inv_norms(table).astype(np.float32)
    assert (inv.cpu().numpy() == want_inv).all() and want_inv[0] == 0 and (want_inv[1:] == 1).all()
    rows, scores = exact_pool(B, P, seed=B * 1000 + P)
    if P >= 8:
        ok = (rows >= 0) & (rows < N_ROWS) & np.isfinite(scores)
        assert (ok.sum(1) == 0).any() and ((ok.sum(1) > 0) & (ok.sum(1) < k)).any() or B < 3
    for rel in ("raw", "minmax"):
        for lam in LAMS:
            got = gpu_mmr(table_d, rows, scores, k, lam, rel)
            assert_mmr_equal(got, R.mmr(table, rows, scores, k, lam, rel))
            # the scores pass through: the pool's bits at the picked places, fillers behind
            pos = got[2].long()
            took = torch.where(pos >= 0, bits(dev(scores)).gather(1, pos.clamp(min=0)), bits(torch.full_like(got[1], float("-inf"))))
            assert torch.equal(bits(got[1]), took)


@pytest.mark.parametrize("k,E", [(2, 20), (37, 20), (37, 21), (128, 20)])
def test_list_diversity_exact(k, E):
    B = 130
    table = exact_table(E)
    rng = np.random.default_rng(k)
    rows = rng.integers(-1, N_ROWS + 3, size=(B, k)).astype(np.int32)  # -1 and rows beyond the table among them
    rows[0] = -1
    rows[1, 1:] = N_ROWS
    rows[2] = 7  # one row at every place
    cat = rng.integers(0, 7, size=N_ROWS).astype(np.int32)  # seven values, 6 is outside [0, 6)
    table_d = dev(table)
    inv = ops.row_inv_norms(table_d)
    ild, n, ncat, diff = ops.list_diversity(table_d, inv, dev(rows), dev(cat), 6)
    ps, wn, wncat, wdiff = R.list_diversity(table, rows, cat, 6)
    assert (n.cpu().numpy() == wn).all() and (ncat.cpu().numpy() == wncat).all() and (diff.cpu().numpy() == wdiff).all()
    want = np.where(wn >= 2, ps / np.maximum(wn * (wn - 1) // 2, 1), 0.0).astype(np.float32)  # fl32(sum / n_pairs): the sum is exact
    assert (ild.cpu().numpy().view(np.int32) == want.view(np.int32)).all()
    assert wn[0] == 0 and wn[1] == 1 and want[2] == 0.0
    ild2, n2, none1, none2 = ops.list_diversity(table_d, inv, dev(rows))  # without categories
    assert none1 is None and none2 is None and torch.equal(bits(ild2), bits(ild)) and torch.equal(n2, n)


# --------------------------------------------------------------------------------------------------- 2. real operands
def real_case(B=130, P=200, E=70, n_rows=900, seed=3):
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((n_rows, E)).astype(np.float32)
    rows = np.stack([rng.permutation(n_rows)[:P] for _ in range(B)]).astype(np.int32)
    scores = (rng.standard_normal((B, P)) * 3).astype(np.float32)
    rows[:, 5] = -1
    scores[:, 9] = np.nan
    return table, rows, scores


@pytest.mark.parametrize("rel,lam", [("minmax", 0.7), ("raw", 0.3), ("minmax", 0.0)])
def test_mmr_real_operands_every_step(rel, lam):
    table, rows, scores = real_case()
    E, k = table.shape[1], 40
    _, s, pos = gpu_mmr(dev(table), rows, scores, k, lam, rel)
    gaps, rmax, legal = R.mmr_step_gaps(table, rows, scores, pos.cpu().numpy(), lam, rel)
    assert legal.all() and not np.isnan(gaps).any()
    tau = 2 * ((E + 8) + 2 * rmax) * EPS
    print(f"MARGIN mmr {rel} lam={lam}: max gap {gaps.max():.3e} tau {tau:.3e}")
    assert gaps.max() <= tau


def test_ild_real_operands():
    table, rows, _ = real_case()
    E, k = table.shape[1], 40
    lists = rows[:, :k]
    table_d = dev(table)
    ild, n, _, _ = ops.list_diversity(table_d, ops.row_inv_norms(table_d), dev(lists))
    ps, wn, _, _ = R.list_diversity(table, lists)
    assert (n.cpu().numpy() == wn).all() and (wn == k - 1).all()
    err = np.abs(ild.cpu().numpy().astype(np.float64) - R.ild(ps, wn))
    bound = ((E + 8) + 2 * (wn * (wn - 1) // 2 - 1)) * EPS
    print(f"MARGIN ild: max err / bound {(err / bound).max():.3e}")
    assert (err <= bound).all()
    inv = ops.row_inv_norms(table_d).cpu().numpy().astype(np.float64)
    assert np.abs(inv / R.inv_norms(table) - 1).max() <= (E + 8) * EPS


# ---------------------------------------------------------------------------------------------------- 3. the contracts
def test_identity_at_lam_one_for_a_pool_in_topk_order():
    rng = np.random.default_rng(8)
    table = dev(rng.standard_normal((500, 32)).astype(np.float32))
    u = dev(rng.standard_normal((7, 32)).astype(np.float32))
    P, k = 200, 50
    pool_rows, pool_scores = ops.topk_deep_dot(table, u, P)
    inv = ops.row_inv_norms(table)
    for rel in ("raw", "minmax"):
        r, s, p = ops.mmr_rerank(table, inv, pool_rows, pool_scores, k, 1.0, rel)
        assert torch.equal(p, torch.arange(k, dtype=torch.int32, device=DEV).expand(7, k))
        assert torch.equal(r, pool_rows[:, :k]) and torch.equal(bits(s), bits(pool_scores[:, :k].contiguous()))


@pytest.mark.parametrize("rel", ["raw", "minmax"])
def test_prefix(rel):
    table, rows, scores = real_case(B=9, P=150, E=36)
    table_d = dev(table)
    full = gpu_mmr(table_d, rows, scores, 150, 0.6, rel)
    for j in (1, 2, 63, 149):
        for a, b in zip(full, gpu_mmr(table_d, rows, scores, j, 0.6, rel)):
            assert torch.equal(bits(a[:, :j].contiguous()), bits(b))


def test_batch_invariance():
    table, rows, scores = real_case(B=130, P=129, E=36)
    table_d = dev(table)
    k = 33
    whole = gpu_mmr(table_d, rows, scores, k, 0.5, "minmax")
    inv = ops.row_inv_norms(table_d)
    lists = dev(rows[:, :100])
    cat = dev(np.random.default_rng(0).integers(0, 9, size=table.shape[0]).astype(np.int32))
    whole_div = ops.list_diversity(table_d, inv, lists, cat, 9)
    perm = np.roll(np.arange(130), 57)  # session b of the rolled batch is session perm[b]
    moved = gpu_mmr(table_d, rows[perm], scores[perm], k, 0.5, "minmax")
    moved_div = ops.list_diversity(table_d, inv, lists[torch.from_numpy(perm).to(DEV)].contiguous(), cat, 9)
    for a, b in zip(whole + whole_div, moved + moved_div):
        assert torch.equal(bits(a[torch.from_numpy(perm).to(DEV)].contiguous()), bits(b))
    for b in (0, 64, 129):
        alone = gpu_mmr(table_d, rows[b:b + 1], scores[b:b + 1], k, 0.5, "minmax")
        alone_div = ops.list_diversity(table_d, inv, lists[b:b + 1].contiguous(), cat, 9)
        for a, c in zip(whole + whole_div, alone + alone_div):
            assert torch.equal(bits(a[b:b + 1].contiguous()), bits(c))


def test_scores_pass_through_bit_for_bit():
    """Scores whose bits no arithmetic would reproduce: -0.0, denormals, values one ulp apart."""
    table = exact_table(16)
    rng = np.random.default_rng(2)
    P = 40
    rows = rng.permutation(N_ROWS - 1)[:P].astype(np.int32)[None] + 1
    s = np.linspace(-1, 1, P).astype(np.float32)
    s[3], s[4], s[5], s[6] = -0.0, 1e-41, np.nextafter(np.float32(0.5), np.float32(1)), 0.5
    scores = s[None]
    for rel, lam in (("raw", 0.5), ("minmax", 0.25), ("minmax", 1.0)):
        r, sc, pos = gpu_mmr(dev(table), rows, scores, P, lam, rel)
        assert sorted(pos[0].tolist()) == list(range(P))
        assert torch.equal(bits(sc), bits(dev(scores)).gather(1, pos.long()))
        assert torch.equal(r, dev(rows).gather(1, pos.long()))


@pytest.mark.parametrize("which", ["table", "pool_rows", "pool_scores", "inv", "all"])
def test_unaligned_operands_take_the_fallback_with_the_same_bits(which):
    table, rows, scores = real_case(B=6, P=80, E=36)  # E % 4 == 0: the aligned call takes the 16-byte loads
    cat = np.random.default_rng(1).integers(0, 5, size=table.shape[0]).astype(np.int32)
    t0, r0, s0, c0 = dev(table), dev(rows), dev(scores), dev(cat)
    assert all(t.data_ptr() % 16 == 0 for t in (t0, r0, s0))
    inv0 = ops.row_inv_norms(t0)
    want = ops.mmr_rerank(t0, inv0, r0, s0, 20, 0.5, "minmax") + ops.list_diversity(t0, inv0, r0, c0, 5)
    shift = lambda t, name: A.shifted(t, 4) if which in (name, "all") else t
    t1, r1, s1 = shift(t0, "table"), shift(r0, "pool_rows"), shift(s0, "pool_scores")
    inv1 = ops.row_inv_norms(t1)
    assert torch.equal(bits(inv1), bits(inv0))
    inv1 = shift(inv1, "inv")
    c1 = A.shifted(c0, 4) if which == "all" else c0
    got = ops.mmr_rerank(t1, inv1, r1, s1, 20, 0.5, "minmax") + ops.list_diversity(t1, inv1, r1, c1, 5)
    if which in ("table", "all"):
        assert t1.data_ptr() % 16 == 4
    for a, b in zip(want, got):
        assert torch.equal(bits(a), bits(b))
    for t in (t1, r1, s1, inv1, c1):
        assert not hasattr(t, "_align_guard") or A.guards_intact(t)
    hip.check_status(DEV)


def test_graph_capture_replays_bit_for_bit():
    table, rows, scores = real_case(B=20, P=100, E=36)
    table_d, rows_s, scores_s = dev(table), dev(rows), dev(scores)
    cat = dev(np.random.default_rng(4).integers(0, 5, size=table.shape[0]).astype(np.int32))

    def run():
        inv = ops.row_inv_norms(table_d)
        r, s, p = ops.mmr_rerank(table_d, inv, rows_s, scores_s, 25, 0.4, "minmax")
        return (r, s, p) + ops.list_diversity(table_d, inv, r, cat, 5)

    first = [t.clone() for t in run()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = run()
    other_rows, other_scores = dev(rows[::-1].copy()), dev(scores[::-1].copy())
    rows_s.copy_(other_rows)  # other pools in the same buffers: the replay reads them on the device
    scores_s.copy_(other_scores)
    graph.replay()
    torch.cuda.synchronize()
    flipped = [t.clone() for t in out]
    assert not torch.equal(flipped[0], first[0])
    for a, b in zip(flipped, run()):
        assert torch.equal(bits(a), bits(b))
    rows_s.copy_(dev(rows))
    scores_s.copy_(dev(scores))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, first):
        assert torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ 4. limits and refusals
def test_refusals_come_from_the_host_with_the_invalid_argument_code():
    table = dev(exact_table(8))
    inv = ops.row_inv_norms(table)
    rows = torch.zeros((3, 10), dtype=torch.int32, device=DEV)
    scores = torch.zeros((3, 10), device=DEV)
    code = r"\(code -1\)"
    with pytest.raises(hip.XnrsHipError, match=code):  # k > P
        ops.mmr_rerank(table, inv, rows, scores, 11, 0.5)
    with pytest.raises(hip.XnrsHipError, match=code):  # P = 1025
        ops.mmr_rerank(table, inv, torch.zeros((3, 1025), dtype=torch.int32, device=DEV), torch.zeros((3, 1025), device=DEV), 10, 0.5)
    for lam in (-0.1, 1.1, float("nan")):
        with pytest.raises(hip.XnrsHipError, match=code):
            ops.mmr_rerank(table, inv, rows, scores, 5, lam)
    with pytest.raises(hip.XnrsHipError, match=code):  # k = 129
        ops.list_diversity(table, inv, torch.zeros((3, 129), dtype=torch.int32, device=DEV))
    cat = torch.zeros((N_ROWS,), dtype=torch.int32, device=DEV)
    with pytest.raises(hip.XnrsHipError, match=code):  # one past the category limit
        ops.list_diversity(table, inv, rows, cat, hip._CONSTANTS["DIVERSITY_MAX_CATEGORIES"] + 1)
    wide = torch.zeros((4, hip._CONSTANTS["DIVERSITY_MAX_E"] + 1), device=DEV)  # one past the E limit
    with pytest.raises(hip.XnrsHipError, match=code):
        ops.mmr_rerank(wide, torch.zeros(4, device=DEV), rows, scores, 5, 0.5)
    with pytest.raises(hip.XnrsHipError, match=code):
        ops.list_diversity(wide, torch.zeros(4, device=DEV), rows)
    with pytest.raises(ValueError, match="rel"):
        ops.mmr_rerank(table, inv, rows, scores, 5, 0.5, rel="zscore")
    # B == 0: fine, nothing to write
    r, s, p = ops.mmr_rerank(table, inv, rows[:0], scores[:0], 5, 0.5)
    assert r.shape == (0, 5) and ops.list_diversity(table, inv, rows[:0])[0].shape == (0,)
    # the limits themselves run: the widest row, the most categories, the longest pool and list
    big = torch.zeros((4, hip._CONSTANTS["DIVERSITY_MAX_E"]), device=DEV)
    big[:, :4] = torch.tensor([[1., 0, 0, 0], [0, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0]])
    binv = ops.row_inv_norms(big)
    small = torch.tensor([[0, 1, 2, 3]], dtype=torch.int32, device=DEV)
    ild, n, ncat, diff = ops.list_diversity(big, binv, small, torch.tensor([0, 4095, 4095, 4096], dtype=torch.int32, device=DEV),
                                            hip._CONSTANTS["DIVERSITY_MAX_CATEGORIES"])
    assert n.tolist() == [4] and ncat.tolist() == [2] and diff.tolist() == [2]
    _, _, p = ops.mmr_rerank(big, binv, small, torch.tensor([[3., 2, 1, 0]], device=DEV), 4, 0.5, "raw")
    assert sorted(p[0].tolist()) == [0, 1, 2, 3]
    hip.check_status(DEV)


# ------------------------------------------------------------------------------------------------------- 5. end to end
class Cfg(dict):
    __getattr__ = dict.__getitem__


@pytest.fixture(scope="module")
def world():
    from xnrs_amd.models import make_model
    store, beh = synth.click_world(n_news=300, n_sess=40, seed=2)
    store, beh = store.to(DEV), beh.to(DEV)
    torch.manual_seed(11)
    model = make_model(Cfg(synth.model_cfg(dict(model="NRMS", E=32, bias=True, h=4, D=32, H=8, S=6)))).to(DEV).eval()
    cat = torch.from_numpy(np.random.default_rng(6).integers(0, 6, size=store.n_rows).astype(np.int32)).to(DEV)  # 5: outside [0, 5)
    with torch.no_grad():
        vecs = EV.encode_news_table(model, store)[0]
    return store, beh, model, cat, vecs


def test_evaluate_diversity_is_the_metrics_of_recommends_lists(world):
    store, beh, model, cat, vecs = world
    k = 10
    rows, _ = EV.recommend(model, store, beh, l_hist=8, k=k)
    got = EV.evaluate_diversity(model, store, beh, l_hist=8, k=k, row_category=cat, n_categories=5, batch=16)
    same = EV.diversity_metrics(vecs, rows, store.n_rows, store.pad_row, cat, 5)
    want = R.diversity_metrics(vecs.cpu().numpy(), rows.cpu().numpy(), store.n_rows, store.pad_row, cat.cpu().numpy(), 5)
    E = vecs.shape[1]
    ild_bound = ((E + 8) + 2 * (k * (k - 1) // 2 - 1)) * EPS
    for name, w in want.items():
        tol = ild_bound if name.startswith("ild@") else 1e-12
        assert abs(got[name] - w) <= tol and abs(same[name] - w) <= tol, (name, got[name], same[name], w)
    assert want["n_lists"] == len(beh) and 0 < want[f"catalog_coverage@{k}"] < 1 and 0 < want[f"gini@{k}"] < 1
    assert set(got) == set(want) | {f"hit@{k}", f"ndcg@{k}", "n_queries"}
    without = EV.evaluate_diversity(model, store, beh, l_hist=8, k=k, batch=16)
    assert f"cat_ild@{k}" not in without and without[f"ild@{k}"] == got[f"ild@{k}"]


def test_accuracy_within_the_list_is_that_of_full_ranking(world):
    store, beh, model, _, _ = world
    k = 10
    full = EV.evaluate_full_ranking(model, store, beh, l_hist=8, ks=(k,), exclude_history=False)
    for lam in (None, 1.0):
        got = EV.evaluate_diversity(model, store, beh, l_hist=8, k=k, lam=lam, exclude_history=False, batch=16)
        assert got["n_queries"] == full["n_queries"] > 0
        assert abs(got[f"hit@{k}"] - full[f"hit@{k}"]) <= 1e-12 and abs(got[f"ndcg@{k}"] - full[f"ndcg@{k}"]) <= 1e-12
    assert 0 < full[f"hit@{k}"]


def test_recommend_diverse(world):
    store, beh, model, _, vecs = world
    k, pool = 10, 40
    rows, scores = EV.recommend(model, store, beh, l_hist=8, k=k)
    for rel in ("raw", "minmax"):  # lam = 1: recommend(k), rows and score bits
        r1, s1 = EV.recommend_diverse(model, store, beh, l_hist=8, k=k, lam=1.0, pool=pool, rel=rel, batch=16)
        assert torch.equal(r1, rows) and torch.equal(bits(s1), bits(scores))
    r, s = EV.recommend_diverse(model, store, beh, l_hist=8, k=k, lam=0.3, pool=pool, batch=16)
    prow, pscore = EV.recommend(model, store, beh, l_hist=8, k=pool)
    rn, pn = r.cpu().numpy(), prow.cpu().numpy()
    for b in range(len(beh)):
        assert (rn[b] >= 0).all() and len(set(rn[b].tolist())) == k and set(rn[b].tolist()) <= set(pn[b].tolist())
        assert store.pad_row not in rn[b]
    at = (r[:, :, None] == prow[:, None, :]).int().argmax(dim=2)  # the scores are the pool's
    assert torch.equal(bits(s), bits(pscore.gather(1, at)))
    assert not torch.equal(r, rows)  # variety changed something
    gaps, rmax, legal = R.mmr_step_gaps(vecs.cpu().numpy(), pn, pscore.cpu().numpy(), at.cpu().numpy(), 0.3, "minmax")
    assert legal.all() and gaps.max() <= 2 * ((vecs.shape[1] + 8) + 2 * rmax) * EPS  # every pick, as in the real-operand test
    div = EV.evaluate_diversity(model, store, beh, l_hist=8, k=k, lam=0.3, pool=pool)
    base = EV.evaluate_diversity(model, store, beh, l_hist=8, k=k)
    assert div[f"ild@{k}"] > base[f"ild@{k}"]
    # sessions: a selection, row i of the result is session sessions[i]
    sel = [7, 3, 30]
    rs, _ = EV.recommend_diverse(model, store, beh, l_hist=8, k=k, lam=0.3, pool=pool, sessions=sel)
    assert torch.equal(rs, r[torch.tensor(sel, device=DEV)])
