"""GPU: LSTUR (xnrs/models/full_models/lstur.py:9-159) on the HIP path -- the model against the real reference
(tests/golden/lstur_model.npz: the five working (long_term_method, long_short_term_method) pairs, a history mask with a hole,
the shipped shape, the bilin / fc scorers) in eval mode and in the MSE grad step, the GRU kernels alone against an fp64
restatement over random shapes, the id path, determinism, hipGraph capture, the evaluation epoch and the ('mean', 'con') error.

Bars: the project's for a model against the reference, 1e-4 on scores and 2e-4 on gradients (tests/test_hip_npa.py).  The
reference in fp32 sits within 2.3e-7 (scores) and 2.0e-5 (gradients) of itself in fp64 on the recorded cases
(lstur_model.json "fp32_vs_fp64"), so the 25 chained fp32 steps need no wider bar."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import helpers as H
from tests.golden import lstur_cases as LC
from xnrs_amd import hip, ops, synth
from xnrs_amd.models.lstur import make_lstur

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = H.golden("lstur_model")
META = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lstur_model.json")))
TOL_S, TOL_G = 1e-4, 2e-4


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _model(c):
    model = make_lstur(Cfg(LC.model_cfg(c)))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(synth.fill_state_dict(shapes, LC.weight_seed(c)))
    return model.to(DEV)


# ------------------------------------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("name", list(LC.CASES))
def test_scores_equal_the_reference(name):
    c = LC.CASES[name]
    model = _model(c).eval()
    batch = synth.batch_to(LC.batch(c), DEV)
    with torch.no_grad():
        r, u, cv = model(batch, return_embeddings=True)
        u2 = model.get_user_embeddings(batch)
    assert u.shape == (c["B"], 1, c["Et"] + c["Ec"]) and u2.shape == (c["B"], c["Et"] + c["Ec"])
    assert torch.equal(u2, u[:, 0])
    H.assert_close(r, GOLD[f"{name}/eval/r"], TOL_S, f"{name} r")
    H.assert_close(u.reshape(c["B"], -1), GOLD[f"{name}/eval/u"], TOL_S, f"{name} u")
    H.assert_close(cv, GOLD[f"{name}/eval/c"], TOL_S, f"{name} c")


def _grad_step(model, batch, input_grads=True):
    h, _ = batch["user_features"]["history"]["title_emb"]
    cx, _ = batch["candidate_features"]["title_emb"]
    if input_grads:
        h.requires_grad_(True)
        cx.requires_grad_(True)
    preds = torch.relu(model(batch))
    loss = F.mse_loss(preds, batch["targets"])
    loss.backward()
    return loss, preds, h.grad, cx.grad


@pytest.mark.parametrize("name", list(LC.CASES))
def test_grad_step_equals_the_reference(name):
    c = LC.CASES[name]
    model = _model(c).train()
    batch = synth.batch_to(LC.batch(c), DEV)
    loss, preds, dh, dc = _grad_step(model, batch)
    pre = f"{name}/grad"
    H.assert_close(loss.reshape(1), GOLD[f"{pre}/loss"].reshape(1), TOL_S, f"{pre} loss")
    H.assert_close(preds, GOLD[f"{pre}/preds"], TOL_S, f"{pre} preds")
    no_grad = META["no_grad"][name]
    gmax = max(float(v) for k, v in GOLD.items() if k.startswith(f"{pre}/max/dW/"))
    grads = {"in/hist": dh, "in/cand": dc}
    grads.update({f"dW/{k}": p.grad for k, p in model.named_parameters()})
    checked = 0
    for k, g in grads.items():
        if k in no_grad:  # the reference leaves .grad at None there (lt_only: the GRU; with the user table the history too)
            assert g is None or float(g.abs().max()) == 0.0, f"{pre} {k} must get no gradient"
            continue
        # every tensor against max(its own scale, 1e-3 of the largest parameter gradient), as helpers.assert_grads_close does
        own = float(GOLD[f"{pre}/max/{k}"])
        scale = max(own, 1e-3 * gmax)
        err = np.abs(LC.sample(g).astype(np.float64) - GOLD[f"{pre}/{k}"]).max()
        assert err <= TOL_G * scale, f"{pre} {k}: {err:.3e} vs scale {scale:.3e}"
        assert abs(float(g.abs().max()) - own) <= TOL_G * scale, f"{pre} max {k}"
        checked += 1
    assert checked >= 8
    if c["ltm"] == "embedding":
        dt = model.user_encoder.long_term_encoder.weight.grad
        assert float(dt[0].abs().max()) == 0.0, "the padding row of the user table gets exactly zero"
        used = set(c["uids"]) - {0}  # (a used row may still get zero: a user whose scores the relu cut off)
        rest = [i for i in range(dt.shape[0]) if i not in used]
        assert float(dt[rest].abs().max()) == 0.0, "rows of users outside the batch get exactly zero"
        assert float(dt.abs().max()) > 0
    if c["lstm"] == "lt_only":
        assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in model.user_encoder.gru.parameters())
    else:
        assert all(float(p.grad.abs().max()) > 0 for p in model.user_encoder.gru.parameters())


# ------------------------------------------------------------------------------------------- 2. the recurrence vs fp64
def _ref_gru(x, lens, h0, w_ih, w_hh, b_ih, b_hh):
    """fp64 restatement of nn.GRU (gate order r, z, n) over the first lens[b] steps of row b."""
    B, T, _ = x.shape
    Hd = w_hh.shape[1]
    h = h0 if h0 is not None else x.new_zeros(B, Hd)
    for t in range(T):
        gi = x[:, t] @ w_ih.T + b_ih
        gh = h @ w_hh.T + b_hh
        r = torch.sigmoid(gi[:, :Hd] + gh[:, :Hd])
        z = torch.sigmoid(gi[:, Hd:2 * Hd] + gh[:, Hd:2 * Hd])
        n = torch.tanh(gi[:, 2 * Hd:] + r * gh[:, 2 * Hd:])
        new = (1 - z) * n + z * h
        h = torch.where((t < lens)[:, None], new, h)
    return h


@pytest.mark.parametrize("layout", ["0", "1"])
@pytest.mark.parametrize("seed,B,T,N,E,Hd,with_h0,full", [
    (1, 5, 7, 9, 12, 20, True, False),     # Hd not a multiple of the 32-wide tile
    (2, 37, 6, 6, 24, 72, False, False),   # two row tiles, three column tiles, zero initial state
    (3, 4, 1, 3, 8, 18, True, False),      # T = 1; Hd not a multiple of 4 (the scalar load path)
    (4, 33, 5, 5, 16, 40, True, True),     # all rows full
    (5, 3, 25, 50, 272, 136, True, False),  # the shipped widths ('con': Hd = 136)
])
def test_gru_kernels_match_fp64(layout, seed, B, T, N, E, Hd, with_h0, full):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    x = torch.randn(B, T, E, generator=g)
    m = (torch.rand(B, N, generator=g) > 0.4).float()  # ones anywhere: the length is their count among the first T slots
    if full:
        m[:] = 1
    else:
        m[0, :T] = 0  # a row of length 0
        m[B - 1, :T] = 1
    lens = m[:, :T].sum(1).long()
    h0 = torch.randn(B, Hd, generator=g) * 0.5 if with_h0 else None
    gru = nn.GRU(E, Hd, batch_first=True)
    dy = torch.randn(B, Hd, generator=g)
    xd = x.double().requires_grad_(True)
    hd = h0.double().requires_grad_(True) if with_h0 else None
    pd = [p.detach().double().requires_grad_(True) for p in (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)]
    yr = _ref_gru(xd, lens, hd, *pd)
    yr.backward(dy.double())
    gru = gru.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    hg = h0.to(DEV).requires_grad_(True) if with_h0 else None
    with hip.knobs(XNRS_GRU_LAYOUT=layout):
        with torch.no_grad():
            y_inf = ops.gru(xg.detach(), m.to(DEV)[..., None], None if hg is None else hg.detach(), gru)
        y = ops.gru(xg, m.to(DEV)[..., None], hg, gru)
        y.backward(dy.to(DEV))
        torch.cuda.synchronize()
    assert torch.equal(y_inf, y.detach()), "inference and training forwards are the same arithmetic"
    assert torch.isfinite(y).all()
    H.assert_close(y, yr.detach(), TOL_S, "y")
    if not full:  # a row of length 0 keeps its initial state, exactly
        assert torch.equal(y[0].cpu(), h0[0] if with_h0 else torch.zeros(Hd))
        assert float(xg.grad[0].abs().max()) == 0.0
        if with_h0:
            assert torch.equal(hg.grad[0].cpu(), dy[0])
    H.assert_close(xg.grad, xd.grad, TOL_G, "dx")
    if with_h0:
        H.assert_close(hg.grad, hd.grad, TOL_G, "dh0")
    for got, ref, k in zip((gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0), pd, ("dW_ih", "dW_hh", "db_ih", "db_hh")):
        H.assert_close(got.grad, ref.grad, TOL_G, k)


def test_both_recurrence_layouts_give_the_same_bits():
    torch.manual_seed(7)
    gru = nn.GRU(24, 40, batch_first=True).to(DEV)
    x = torch.randn(35, 6, 24, device=DEV)
    m = (torch.rand(35, 6, 1, device=DEV) > 0.3).float()
    outs = []
    for layout in ("0", "1"):
        with hip.knobs(XNRS_GRU_LAYOUT=layout):
            xg = x.clone().requires_grad_(True)
            gru.zero_grad(set_to_none=True)
            y = ops.gru(xg, m, None, gru)
            y.square().sum().backward()
            torch.cuda.synchronize()
            outs.append([y.detach().clone(), xg.grad.clone()] + [p.grad.clone() for p in gru.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ------------------------------------------------------------------------------------------- 3. id path, determinism
class _Store:
    def __init__(self, x, m, cat):
        self.x, self.m, self.cat, self.pad_row = x, m, cat, 0

    def text(self, feature):
        return self.x, self.m

    def column(self, name):
        assert name == "category_index"
        return self.cat


def _store_case(name):
    c = dict(LC.CASES[name], n_users=30)
    rng = np.random.default_rng(12)
    n_news, S, D = 20, c["S"], c["D"]
    x = torch.from_numpy(rng.standard_normal((n_news, S, D)).astype(np.float32))
    lens = torch.from_numpy(rng.integers(1, S + 1, size=n_news))
    lens[0] = 0
    x[0] = 0
    m = (torch.arange(S)[None, :] < lens[:, None]).float()
    cat = torch.from_numpy(rng.integers(1, 20, size=n_news).astype(np.int32))
    cat[0] = 0
    hist = torch.from_numpy(rng.integers(1, n_news, size=(4, c["H"])).astype(np.int32))
    hist[1, 2:] = 0   # ragged: empty trailing slots
    hist[3, 1] = 0    # a hole
    cand = torch.from_numpy(rng.integers(1, n_news, size=(4, c["C"])).astype(np.int32))
    uid = torch.tensor([3, 0, 3, 29], dtype=torch.int32)
    return c, _Store(x.to(DEV), m.to(DEV), cat.to(DEV)), hist.to(DEV), cand.to(DEV), uid.to(DEV)


@pytest.mark.parametrize("name", ["tiny/embedding_con", "tiny/mean_ini"])
def test_id_path_is_bitwise_equal_to_forward_on_gathered_rows(name):
    c, store, hist, cand, uid = _store_case(name)
    model = _model(c).eval()
    hl, cl = hist.long(), cand.long()
    batch = {"user_features": {"history": {"title_emb": (store.x[hl], store.m[hl][..., None]), "category_index": store.cat[hl]},
                               "other": {"user_index": uid[:, None]}},
             "candidate_features": {"title_emb": (store.x[cl], store.m[cl][..., None]), "category_index": store.cat[cl]}}
    with torch.no_grad():
        r_ids = model.forward_store(store, hist, cand, uid)
        r = model(batch)
        r_again = model.forward_store(store, hist, cand, uid)
    assert torch.isfinite(r).all()
    assert torch.equal(r_ids, r)
    assert torch.equal(r_ids, r_again)


def test_grad_step_twice_is_bitwise_equal():
    c = LC.CASES["shipped/embedding_con"]
    model = _model(c).train()
    outs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        batch = synth.batch_to(LC.batch(c), DEV)
        loss, preds, _, _ = _grad_step(model, batch, input_grads=False)
        outs.append((loss.detach().clone(), preds.detach().clone(), [p.grad.clone() for p in model.parameters() if p.grad is not None]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert len(outs[0][2]) == len(outs[1][2]) and all(torch.equal(a, b) for a, b in zip(outs[0][2], outs[1][2]))


@pytest.mark.parametrize("name", ["tiny/embedding_ini", "tiny/embedding_con", "tiny/hole_mean_ini"])
def test_grad_step_is_captured_in_a_hipgraph_and_replays_bitwise(name):
    c = LC.CASES[name]
    model = _model(c).train()
    batch = synth.batch_to(LC.batch(c), DEV)
    params = [p for k, p in model.named_parameters() if not k.endswith("dummy_param")]
    for p in params:
        p.grad = torch.zeros_like(p)

    def step():
        for p in params:
            p.grad.zero_()
        preds = torch.relu(model(batch))
        loss = F.mse_loss(preds, batch["targets"])
        loss.backward()
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        l0 = step().detach().clone()
        g0 = [p.grad.clone() for p in params]
        l1 = step().detach().clone()
        assert torch.equal(l0, l1) and all(torch.equal(p.grad, r) for p, r in zip(params, g0))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        loss_g = step()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss_g, l0)
        for p, ref in zip(params, g0):
            assert torch.equal(p.grad, ref)
    assert model.user_encoder.gru.weight_hh_l0.grad.abs().max() > 0


# ------------------------------------------------------------------------------------------- 4. evaluation, errors
@pytest.mark.parametrize("ltm,lstm", [("embedding", "con"), ("mean", "ini")])
def test_evaluate_matches_dense_forwards(ltm, lstm):
    from xnrs_amd import evaluation as EV
    from xnrs_amd.data import DeviceBatcher
    store, beh = synth.click_world(n_news=60, n_sess=40)
    store, beh = store.to(DEV), beh.to(DEV)
    store.columns["category_index"] = (torch.arange(store.n_rows, device=DEV, dtype=torch.int32) % 19 + 1) * (
        torch.arange(store.n_rows, device=DEV) > 0).to(torch.int32)
    c = dict(LC.SHAPES["tiny"], D=32, n_users=50, H=5, st=3, ltm=ltm, lstm=lstm, scoring="dot", hole=False)
    torch.manual_seed(4)
    model = make_lstur(Cfg(LC.model_cfg(c))).to(DEV).eval()
    if ltm == "embedding":
        with pytest.raises(ValueError, match="user index"):
            EV.evaluate(model, store, beh, l_hist=5)
    beh.user_index = torch.arange(len(beh), device=DEV) % 7
    res = EV.evaluate(model, store, beh, l_hist=5, batch=16)
    bat = DeviceBatcher(beh, 5, store.pad_row)
    cat = store.column("category_index")
    sums = torch.zeros(len(EV.METRIC_NAMES), dtype=torch.float64)
    for s in range(len(beh)):
        sess = torch.tensor([s], device=DEV)
        hist, off, rows, csess, targets = bat.eval_batch(sess)
        hl, cl = hist.long(), rows.long()[None, :]
        batch = {"user_features": {"history": {"title_emb": (store.x[hl], store.m[hl][..., None]), "category_index": cat[hl]},
                                   "other": {"user_index": beh.user_index[sess][:, None]}},
                 "candidate_features": {"title_emb": (store.x[cl], store.m[cl][..., None]), "category_index": cat[cl]}}
        with torch.no_grad():
            r = torch.relu(model(batch)).reshape(-1)
        sums += EV.rank_metrics(r, targets, off).double().sum(0).cpu()
    for k, v in zip(EV.METRIC_NAMES, (sums / len(beh)).tolist()):
        assert abs(res[k] - v) <= 1e-5, (k, res[k], v)


def test_mean_con_constructs_and_its_forward_names_the_mismatch():
    c = dict(LC.SHAPES["tiny"], ltm="mean", lstm="con", scoring="dot", hole=False)
    model = _model(c).eval()
    e = c["Et"] + c["Ec"]
    with pytest.raises(hip.XnrsHipError, match=rf"{e // 2 + e} columns.*{e}.*lstur\.py:99-109,151-154"):
        model(synth.batch_to(LC.batch(c), DEV))
    shipped = dict(LC.SHAPES["shipped"], B=1, ltm="mean", lstm="con", scoring="dot", hole=False)
    with pytest.raises(hip.XnrsHipError, match="408 columns.*272"):
        _model(shipped).eval()(synth.batch_to(LC.batch(shipped), DEV))


def test_user_ids_outside_the_table_are_clamped_and_reported():
    c = LC.CASES["tiny/embedding_ini"]
    model = _model(c).eval()
    hip.check_status(DEV)
    h = torch.randn(3, c["H"], c["Et"] + c["Ec"], device=DEV)
    hm = torch.ones(3, c["H"], 1, device=DEV)
    with torch.no_grad():
        u = model.user_encoder((h, hm), torch.tensor([[c["n_users"] + 5], [0], [-3]], dtype=torch.int32, device=DEV))
        ref = model.user_encoder((h, hm), torch.tensor([[c["n_users"]], [0], [0]], dtype=torch.int32, device=DEV))
    assert torch.equal(u, ref)
    with pytest.raises(hip.XnrsHipError, match="user id"):
        hip.check_status(DEV)


def test_users_without_a_short_term_history_keep_the_long_term_state():
    """Beyond the reference (it raises in pack_padded_sequence): a row of length 0 returns the initial state, nothing is NaN."""
    c = LC.CASES["tiny/embedding_ini"]
    model = _model(c).eval()
    h = torch.randn(2, c["H"], c["Et"] + c["Ec"], device=DEV)
    hm = torch.ones(2, c["H"], 1, device=DEV)
    hm[0] = 0
    uid = torch.tensor([[4], [6]], dtype=torch.int32, device=DEV)
    with torch.no_grad():
        u = model.user_encoder((h, hm), uid)
    assert torch.isfinite(u).all()
    assert torch.equal(u[0, 0], model.user_encoder.long_term_encoder.weight[4])
    assert not torch.equal(u[1, 0], model.user_encoder.long_term_encoder.weight[6])
