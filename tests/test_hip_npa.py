"""GPU: NPA (xnrs/models/full_models/npa.py:8-95) on the HIP path -- layers.PersonalizedAttention's kernels (forward,
backward, per-query reduction), the table-scale user-table gradient, the model against the real reference
(tests/golden/npa.npz) in eval mode and in the MSE grad step for the dot / bilin / fc scorers, an fp64 restatement over
random shapes, the id path, determinism, hipGraph capture and the per-batch evaluation epoch."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import helpers as H
from tests.golden import npa_cases as NC
from xnrs_amd import hip, ops, synth
from xnrs_amd.models import PersonalizedAttention
from xnrs_amd.models.npa import make_npa

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = H.golden("npa")
TOL_S, TOL_G = 1e-4, 2e-4


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _model(c, scoring):
    model = make_npa(Cfg(NC.model_cfg(c, scoring)))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(synth.fill_state_dict(shapes, NC.weight_seed(c)))
    return model.to(DEV)


def _pieces(model, batch):
    """(r, u, c) of forward(batch), u and c as the scorer saw them."""
    seen = {}
    real = model.rec_model.forward
    model.rec_model.forward = lambda u, c: seen.update(u=u, c=c) or real(u, c)
    try:
        r = model(batch)
    finally:
        del model.rec_model.forward
    return r, seen["u"], seen["c"]


# ------------------------------------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("scoring", NC.SCORERS)
@pytest.mark.parametrize("name", list(NC.CASES))
def test_scores_equal_the_reference(name, scoring):
    c = NC.CASES[name]
    model = _model(c, scoring).eval()
    batch = synth.batch_to(NC.batch(c), DEV)
    with torch.no_grad():
        r, u, cv = _pieces(model, batch)
    pre = f"{name}/{scoring}/eval"
    H.assert_close(r, GOLD[f"{pre}/r"], TOL_S, f"{pre} r")
    H.assert_close(u.reshape(c["B"], -1), GOLD[f"{pre}/u"], TOL_S, f"{pre} u")
    H.assert_close(cv, GOLD[f"{pre}/c"], TOL_S, f"{pre} c")


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


@pytest.mark.parametrize("scoring", NC.SCORERS)
@pytest.mark.parametrize("name", list(NC.CASES))
def test_grad_step_equals_the_reference(name, scoring):
    c = NC.CASES[name]
    model = _model(c, scoring).train()
    batch = synth.batch_to(NC.batch(c), DEV)
    loss, preds, dh, dc = _grad_step(model, batch)
    pre = f"{name}/{scoring}/grad"
    H.assert_close(loss.reshape(1), GOLD[f"{pre}/loss"].reshape(1), TOL_S, f"{pre} loss")
    H.assert_close(preds, GOLD[f"{pre}/preds"], TOL_S, f"{pre} preds")
    for what, g in (("hist", dh), ("cand", dc)):
        scale = float(GOLD[f"{pre}/max/in/{what}"])
        err = np.abs(NC.sample(g).astype(np.float64) - GOLD[f"{pre}/in/{what}"]).max()
        assert err <= TOL_G * scale, f"{pre} d{what}: {err:.3e} vs max {scale:.3e}"
    for k, p in model.named_parameters():
        scale = float(GOLD[f"{pre}/max/{k}"])
        err = np.abs(NC.sample(p.grad).astype(np.float64) - GOLD[f"{pre}/dW/{k}"]).max()
        assert err <= TOL_G * scale, f"{pre} d{k}: {err:.3e} vs max {scale:.3e}"
        assert abs(float(p.grad.abs().max()) - scale) <= TOL_G * scale, f"{pre} max d{k}"


# ------------------------------------------------------------------------------------------- 2. random shapes vs fp64
def _ref_pa(x, m, q, q_idx, wx, bx, head=None):
    """fp64 restatement of layers.py:88-102 (+ npa.py:22-26)."""
    t = torch.tanh(x @ wx.T + bx)
    e = (t * q[q_idx.long()][:, None, :]).sum(-1)
    s = torch.exp(e) * m
    a = s / (s.sum(1, keepdim=True) + 1e-8)
    p = (a[..., None] * x).sum(1)
    if head is not None:
        w0, b0, w2, b2 = head
        p = torch.relu(p @ w0.T + b0) @ w2.T + b2
    return p


@pytest.mark.parametrize("seed,n_q,per,L,D,A,E", [(1, 3, 4, 7, 24, 40, 12), (2, 5, 3, 13, 64, 128, 0), (3, 2, 6, 5, 20, 96, 16)])
def test_personalized_encoder_matches_fp64(seed, n_q, per, L, D, A, E):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    n = n_q * per
    x = torch.randn(n, L, D, generator=g)
    lens = torch.randint(0, L + 1, (n,), generator=g)
    lens[1] = 0  # an all-masked sequence
    m = (torch.arange(L)[None, :] < lens[:, None]).float()
    q = torch.randn(n_q, A, generator=g) * 0.3
    q_idx = torch.div(torch.arange(n), per, rounding_mode="floor").to(torch.int32)
    x_fc = nn.Linear(D, A)
    head = nn.Sequential(nn.Linear(D, E), nn.ReLU(), nn.Linear(E, E)) if E else None
    dy = torch.randn(n, E or D, generator=g)
    xd, qd = x.double().requires_grad_(True), q.double().requires_grad_(True)
    pd = [p.detach().double().requires_grad_(True) for p in x_fc.parameters()]
    hd = [p.detach().double().requires_grad_(True) for p in head.parameters()] if head is not None else []
    yr = _ref_pa(xd, m.double(), qd, q_idx, pd[0], pd[1], hd if hd else None)
    yr.backward(dy.double())
    x_fc = x_fc.to(DEV)
    head = head.to(DEV) if head is not None else None
    xg, qg = x.to(DEV).requires_grad_(True), q.to(DEV).requires_grad_(True)
    y, hm = ops.personalized(xg, m.to(DEV), None, qg, q_idx.to(DEV), x_fc, head)
    y.backward(dy.to(DEV))
    H.assert_close(y, yr.detach(), TOL_S, "y")
    assert torch.equal(hm.cpu(), (lens > 0).float())
    if head is None:
        assert torch.all(y[1] == 0), "an all-masked sequence pools to 0"
    H.assert_close(xg.grad, xd.grad, TOL_G, "dx")
    H.assert_close(qg.grad, qd.grad, TOL_G, "dq")
    for got, ref, k in zip(x_fc.parameters(), pd, ("dWx", "dbx")):
        H.assert_close(got.grad, ref.grad, TOL_G, k)
    if head is not None:
        for got, ref in zip(head.parameters(), hd):
            H.assert_close(got.grad, ref.grad, TOL_G, "head")


def test_user_table_gradient_at_table_scale_equals_index_add():
    n_rows, du, N = 703789 + 1, 64, 256
    g = torch.Generator().manual_seed(5)
    uid = torch.tensor([5, 703789, 0, 5, 123456, 5, 0, 42], dtype=torch.int32)
    table = torch.zeros(n_rows, du)
    table[uid.long()] = torch.randn(uid.numel(), du, generator=g)
    w = torch.randn(N, du, generator=g) * 0.1
    b = torch.randn(N, generator=g)
    dy = torch.randn(uid.numel(), N, generator=g)
    tg = table.to(DEV).requires_grad_(True)
    wg, bg = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = ops.embedding_linear_table(uid.to(DEV), tg, wg, bg)
    y.backward(dy.to(DEV))
    H.assert_close(y, table[uid.long()].double() @ w.double().T + b.double(), TOL_S, "y")
    ref = torch.zeros(n_rows, du, dtype=torch.float64).index_add_(0, uid.long(), dy.double() @ w.double())
    rows = torch.unique(uid.long())
    H.assert_close(tg.grad[rows.to(DEV)], ref[rows], TOL_G, "table rows")
    keep = torch.ones(n_rows, dtype=torch.bool, device=DEV)
    keep[rows.to(DEV)] = False
    assert int(torch.count_nonzero(tg.grad[keep]).item()) == 0, "rows not in the batch must be exactly 0"
    H.assert_close(wg.grad, dy.double().T @ table[uid.long()].double(), TOL_G, "dw")
    H.assert_close(bg.grad, dy.double().sum(0), TOL_G, "db")


def test_personalized_attention_module_matches_fp64():
    torch.manual_seed(3)
    mod = PersonalizedAttention(24, 40, 8)
    x, m, q = torch.randn(4, 9, 24), (torch.rand(4, 9, 1) > 0.3).float(), torch.randn(4, 1, 8)
    with torch.no_grad():
        qp = q[:, 0].double() @ mod.q_fc.weight.double().T + mod.q_fc.bias.double()
        ref = _ref_pa(x.double(), m[..., 0].double(), qp, torch.arange(4), mod.x_fc.weight.double(), mod.x_fc.bias.double())
        y = mod.to(DEV)(q.to(DEV), x.to(DEV), m.to(DEV))
    assert y.shape == (4, 1, 24)
    H.assert_close(y[:, 0], ref, TOL_S, "PersonalizedAttention")


# ------------------------------------------------------------------------------------------- 3. id path, determinism
class _Store:
    def __init__(self, x, m):
        self.x, self.m, self.pad_row = x, m, 0

    def text(self, feature):
        return self.x, self.m


def _store_case():
    c = dict(NC.CASES["tiny"], n_users=30)
    rng = np.random.default_rng(12)
    n_news, S, D = 20, c["S"], c["D"]
    x = torch.from_numpy(rng.standard_normal((n_news, S, D)).astype(np.float32))
    lens = torch.from_numpy(rng.integers(0, S + 1, size=n_news))
    lens[0] = 0
    x[0] = 0
    m = (torch.arange(S)[None, :] < lens[:, None]).float()
    hist = torch.from_numpy(rng.integers(0, n_news, size=(4, c["H"])).astype(np.int32))
    cand = torch.from_numpy(rng.integers(1, n_news, size=(4, c["C"])).astype(np.int32))
    uid = torch.tensor([3, 0, 3, 29], dtype=torch.int32)
    return c, _Store(x.to(DEV), m.to(DEV)), hist.to(DEV), cand.to(DEV), uid.to(DEV)


def test_id_path_is_bitwise_equal_to_forward_on_gathered_rows():
    c, store, hist, cand, uid = _store_case()
    model = _model(c, "dot").eval()
    hl, cl = hist.long(), cand.long()
    batch = {"user_features": {"history": {"title_emb": (store.x[hl], store.m[hl][..., None])},
                               "other": {"user_index": uid[:, None]}},
             "candidate_features": {"title_emb": (store.x[cl], store.m[cl][..., None])}}
    with torch.no_grad():
        r_ids = model.forward_store(store, hist, cand, uid)
        r = model(batch)
        r_again = model.forward_store(store, hist, cand, uid)
    assert torch.equal(r_ids, r)
    assert torch.equal(r_ids, r_again)


def test_grad_step_twice_is_bitwise_equal():
    c = NC.CASES["shipped"]
    model = _model(c, "bilin").train()
    outs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        batch = synth.batch_to(NC.batch(c), DEV)
        loss, preds, _, _ = _grad_step(model, batch, input_grads=False)
        outs.append((loss.detach().clone(), preds.detach().clone(), [p.grad.clone() for p in model.parameters()]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(outs[0][2], outs[1][2]))


@pytest.mark.parametrize("scoring", NC.SCORERS)
def test_grad_step_is_captured_in_a_hipgraph_and_replays_bitwise(scoring):
    c = NC.CASES["tiny"]
    model = _model(c, scoring).train()
    with torch.no_grad():  # scorer biases that lift the scores above the relu
        for p in model.rec_model.parameters():
            if p.dim() == 1:
                p.fill_(0.5)
    batch = synth.batch_to(NC.batch(c), DEV)
    params = list(model.parameters())
    for p in params:
        p.grad = torch.zeros_like(p)

    def step():
        for p in params:
            p.grad.zero_()
        preds = torch.relu(model(batch))
        loss = F.mse_loss(preds, batch["targets"])
        loss.backward()
        return loss

    # (one side stream for the eager steps and the capture, as tests/test_hip_scorers.py does)
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
    assert model.user_embedder.weight.grad.abs().max() > 0


# ------------------------------------------------------------------------------------------- 4. evaluation
def test_evaluate_matches_a_batch_of_one_loop():
    from xnrs_amd import evaluation as EV
    from xnrs_amd.data import DeviceBatcher
    store, beh = synth.click_world(n_news=60, n_sess=40)
    store, beh = store.to(DEV), beh.to(DEV)
    c = dict(NC.CASES["tiny"], D=32, n_users=50)
    torch.manual_seed(4)
    model = make_npa(Cfg(NC.model_cfg(c, "dot"))).to(DEV).eval()
    with pytest.raises(ValueError, match="user index"):
        EV.evaluate(model, store, beh, l_hist=5)
    beh.user_index = torch.arange(len(beh), device=DEV) % 7
    res = EV.evaluate(model, store, beh, l_hist=5, batch=16)
    bat = DeviceBatcher(beh, 5, store.pad_row)
    sums = torch.zeros(len(EV.METRIC_NAMES), dtype=torch.float64)
    for s in range(len(beh)):
        sess = torch.tensor([s], device=DEV)
        hist, off, rows, csess, targets = bat.eval_batch(sess)
        hl, cl = hist.long(), rows.long()[None, :]
        batch = {"user_features": {"history": {"title_emb": (store.x[hl], store.m[hl][..., None])},
                                   "other": {"user_index": beh.user_index[sess][:, None]}},
                 "candidate_features": {"title_emb": (store.x[cl], store.m[cl][..., None])}}
        with torch.no_grad():
            r = torch.relu(model(batch)).reshape(-1)
        sums += EV.rank_metrics(r, targets, off).double().sum(0).cpu()
    for k, v in zip(EV.METRIC_NAMES, (sums / len(beh)).tolist()):
        assert abs(res[k] - v) <= 1e-5, (k, res[k], v)


def test_cpu_tensors_raise():
    x_fc = nn.Linear(8, 4)
    with pytest.raises(hip.XnrsHipError):
        ops.personalized(torch.randn(2, 3, 8), None, None, torch.randn(2, 4), torch.zeros(2, dtype=torch.int32), x_fc)
    with pytest.raises(hip.XnrsHipError):
        ops.embedding_linear_table(torch.zeros(2, dtype=torch.int32), torch.randn(5, 3), torch.randn(4, 3), None)


def test_evaluate_runs_without_autograd(monkeypatch):
    """evaluate() runs under torch.no_grad() for the per-batch path and for the table path of the other models."""
    from xnrs_amd import evaluation as EV
    from xnrs_amd.models import make_model
    store, beh = synth.click_world(n_news=40, n_sess=20)
    store, beh = store.to(DEV), beh.to(DEV)
    seen = []
    c = dict(NC.CASES["tiny"], D=32, n_users=50)
    torch.manual_seed(5)
    npa = make_npa(Cfg(NC.model_cfg(c, "dot"))).to(DEV).eval()
    beh.user_index = torch.arange(len(beh), device=DEV) % 5
    real = npa.score_impressions
    monkeypatch.setattr(npa, "score_impressions", lambda *a, **k: seen.append(torch.is_grad_enabled()) or real(*a, **k))
    EV.evaluate(npa, store, beh, l_hist=5, batch=8)
    std = make_model(Cfg(synth.model_cfg(dict(model="standard", E=32, bias=True, h=4, D=32, H=8, S=6)))).to(DEV).eval()
    real_u = std.encode_user
    monkeypatch.setattr(std, "encode_user", lambda *a, **k: seen.append(torch.is_grad_enabled()) or real_u(*a, **k))
    EV.evaluate(std, store, beh, l_hist=5, batch=8)
    assert len(seen) == 3 + 3 and not any(seen), seen


def test_query_index_out_of_range_is_reported_not_read():
    hip.check_status(DEV)
    x_fc = nn.Linear(16, 8).to(DEV)
    x = torch.randn(4, 5, 16, device=DEV)
    q = torch.randn(2, 8, device=DEV)
    q_idx = torch.tensor([0, 1, 2, -1], dtype=torch.int32, device=DEV)  # rows 2 and -1 do not exist
    hip.status_word(DEV)
    with torch.no_grad():
        y, hm = ops.personalized(x, None, None, q, q_idx, x_fc)
    assert torch.isfinite(y[:2]).all() and torch.isnan(y[2:]).all()
    assert torch.equal(hm.cpu(), torch.ones(4))
    with pytest.raises(hip.XnrsHipError, match="query row"):
        hip.check_status(DEV)
    # the same through autograd: the bad sequences pass no gradient into dq of the real rows
    qg = q.clone().requires_grad_(True)
    ok = torch.tensor([0, 1, 1, 0], dtype=torch.int32, device=DEV)
    y_ok, _ = ops.personalized(x, None, None, qg, ok, x_fc)
    y_ok.sum().backward()
    assert torch.isfinite(qg.grad).all()
    hip.check_status(DEV)


def test_user_ids_outside_the_table_are_clamped_and_reported():
    c = NC.CASES["tiny"]
    model = _model(c, "dot").eval()
    hip.check_status(DEV)
    uid = torch.tensor([c["n_users"] + 5, 0, -3], dtype=torch.int32, device=DEV)
    with torch.no_grad():
        q = model.queries(uid)
        ref = model.queries(torch.tensor([c["n_users"], 0, 0], dtype=torch.int32, device=DEV))
    assert torch.equal(q, ref)
    with pytest.raises(hip.XnrsHipError, match="user id"):
        hip.check_status(DEV)
