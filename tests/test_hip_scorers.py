"""GPU: the bilinear and MLP scorers (cfg.scoring 'bilin' / 'fc', xnrs/models/components/scoring.py:41-102) on the HIP
path -- forward and backward against the real reference (tests/golden/scorers.npz) and an fp64 restatement over random
shapes, the whole-model grad step in the reference's call order, hipGraph capture, integrated gradients without weight
gradients, and the device-side evaluation epoch scoring with the model's own scorer."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helpers as H
from tests.golden import cases, scorer_cases as SC
from tests.test_hip_grads import Cfg, load
from xnrs_amd import autograd as AG, hip, ops, synth
from xnrs_amd.losses import contrastive_loss
from xnrs_amd.models import make_model
from xnrs_amd.models.blocks import BilinScoring, DotScoring, FCScoring

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = H.golden("scorers")
TOL_S, TOL_G = 1e-4, 2e-4


def _scorer(c):
    mod = BilinScoring(c["E"], normalize=c["normalize"], bias=c["bias"]) if c["kind"] == "bilin" else \
        FCScoring(c["E"], hidden_dim=c["H"], bias=c["bias"])
    mod, _ = load(mod, c["seed"] + 1)
    return mod


def _run(mod, u, c, g):
    u = u.to(DEV).requires_grad_(True)
    c = c.to(DEV).requires_grad_(True)
    s = mod(u, c)
    s.backward(g.to(DEV))
    return s, u.grad, c.grad, {k: p.grad for k, p in mod.named_parameters()}


# ------------------------------------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("name", list(SC.SCORER))
def test_scorer_forward_backward_equal_the_reference(name):
    c = SC.SCORER[name]
    mod = _scorer(c)
    u, cv, g = SC.scorer_inputs(c)
    s, du, dc, dp = _run(mod, u, cv, g)
    H.assert_close(s, GOLD[f"{name}/s"], TOL_S, f"{name} s")
    H.assert_close(du, GOLD[f"{name}/du"], TOL_G, f"{name} du")
    H.assert_close(dc, GOLD[f"{name}/dc"], TOL_G, f"{name} dc")
    for k, grad in dp.items():
        H.assert_close(grad, GOLD[f"{name}/d/{k}"], TOL_G, f"{name} d{k}")
    # no gradient: the inference path, the same scores bit for bit
    with torch.no_grad():
        assert torch.equal(mod(u.to(DEV), cv.to(DEV)), s.detach())


# ------------------------------------------------------------------------------------------- 2. random shapes vs fp64
def _fp64(kind, sd, u, c, normalize, g):
    u = u.double().requires_grad_(True)
    c = c.double().requires_grad_(True)
    p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    uu, cc = u, c
    if kind == "bilin":
        if normalize:
            uu = u / u.norm(p=2, dim=2, keepdim=True)
            cc = c / c.norm(p=2, dim=2, keepdim=True)
        s = F.bilinear(uu.expand(-1, c.shape[1], -1), cc, p["bilin.weight"], p.get("bilin.bias"))
    else:
        x = torch.cat([u.repeat((1, c.shape[1], 1)), c], dim=2)
        s = F.linear(torch.tanh(F.linear(x, p["fc1.weight"], p.get("fc1.bias"))), p["fc2.weight"], p.get("fc2.bias"))
    s.backward(g.double())
    return s, u.grad, c.grad, {k: v.grad for k, v in p.items()}


SHAPES = [  # (B, N, E, H)
    (1, 1, 64, 32), (5, 3, 70, 35), (1, 7, 33, 17), (3, 1, 130, 65), (16, 5, 256, 128), (17000, 4, 16, 7), (2, 9, 5, 3),
]


@pytest.mark.parametrize("kind,normalize", [("bilin", False), ("bilin", True), ("fc", False)])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("bias", [True, False])
def test_random_shapes_against_fp64(kind, normalize, shape, bias):
    B, N, E, Hd = shape
    rng = synth.rng_for(9000 + B + 7 * N + 13 * E + Hd)
    mod = BilinScoring(E, normalize=normalize, bias=bias) if kind == "bilin" else FCScoring(E, hidden_dim=Hd, bias=bias)
    sd = {k: v.clone() for k, v in synth.fill_state_dict({k: tuple(v.shape) for k, v in mod.state_dict().items()},
                                                          int(rng.integers(1 << 30))).items()}
    mod.load_state_dict(sd)
    mod.to(DEV)
    u = torch.from_numpy(rng.standard_normal((B, 1, E)).astype(np.float32))
    c = torch.from_numpy(rng.standard_normal((B, N, E)).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal((B, N, 1)).astype(np.float32))
    got = _run(mod, u, c, g)
    ref = _fp64(kind, sd, u, c, normalize, g)
    H.assert_close(got[0], ref[0], TOL_S, "s")
    H.assert_close(got[1], ref[1], TOL_G, "du")
    H.assert_close(got[2], ref[2], TOL_G, "dc")
    for k in ref[3]:
        H.assert_close(got[3][k], ref[3][k], TOL_G, f"d{k}")


@pytest.mark.parametrize("mod", [BilinScoring(8), BilinScoring(8, normalize=True, bias=False), FCScoring(8, 4)],
                         ids=["bilin", "bilin_norm", "fc"])
def test_empty_batches_and_errors(mod):
    mod = mod.to(DEV)
    for B, N in ((0, 3), (2, 0)):
        u = torch.randn(B, 1, 8, device=DEV, requires_grad=True)
        c = torch.randn(B, N, 8, device=DEV, requires_grad=True)
        s = mod(u, c)
        assert s.shape == (B, N, 1)
        s.sum().backward()
        assert u.grad.shape == u.shape and (u.grad == 0).all()
        for p in mod.parameters():
            assert (p.grad == 0).all()
        mod.zero_grad(set_to_none=True)
    with pytest.raises(RuntimeError):
        mod(torch.randn(2, 1, 8, device=DEV), torch.randn(3, 4, 8, device=DEV))
    with pytest.raises(RuntimeError):
        mod(torch.randn(2, 1, 6, device=DEV), torch.randn(2, 4, 6, device=DEV))
    with pytest.raises(hip.XnrsHipError):
        mod(torch.randn(2, 1, 8), torch.randn(2, 4, 8))


def test_a_weight_gradient_only_pass_and_an_input_gradient_only_pass():
    """The nullable gradient outputs: a pass asked for the weights alone computes no du / dc, a pass asked for the inputs
    alone no weight gradient -- and what each computes equals the full pass bit for bit."""
    for mod in (BilinScoring(24, normalize=True).to(DEV), FCScoring(24, 12).to(DEV)):
        u = torch.randn(6, 1, 24, device=DEV, requires_grad=True)
        c = torch.randn(6, 5, 24, device=DEV, requires_grad=True)
        s = mod(u, c)
        params = list(mod.parameters())
        full = torch.autograd.grad(s.sum(), [u, c] + params, retain_graph=True)
        wonly = torch.autograd.grad(s.sum(), params, retain_graph=True)
        ionly = torch.autograd.grad(s.sum(), [u, c])
        for a, b in zip(full[2:], wonly):
            assert torch.equal(a, b)
        for a, b in zip(full[:2], ionly):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------- 3. the whole-model grad step
def _step_model(c, scoring):
    model, _ = load(make_model(Cfg(SC.step_cfg(c, scoring))), c["seed"] + 1)
    return model


def _step(model, batch, labels, c):
    model.zero_grad(set_to_none=True)
    preds = torch.relu(model(batch))
    loss_rec = F.mse_loss(preds, batch["targets"])
    ue = model.get_user_embeddings(batch).reshape(labels.numel(), -1)
    loss = loss_rec + c["lambda_cl"] * contrastive_loss(ue, labels, c["temperature"])
    loss.backward()
    return loss.detach().clone(), preds.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()
                                                            if p.grad is not None}


@pytest.mark.parametrize("name", list(SC.STEP))
@pytest.mark.parametrize("scoring", SC.STEP_SCORERS)
def test_grad_step_equals_the_reference(name, scoring):
    c = SC.STEP[name]
    pre = f"{name}/{scoring}"
    model = _step_model(c, scoring)
    batch = synth.batch_to(cases.model_batch(c), DEV)
    labels = SC.step_labels(c["B"]).to(DEV)
    loss, preds, grads = _step(model, batch, labels, c)
    H.assert_close(loss.reshape(()), GOLD[f"{pre}/loss"], TOL_S, f"{pre} loss")
    H.assert_close(preds, GOLD[f"{pre}/preds"], TOL_S, f"{pre} preds")
    ref = {k[len(pre) + 4:]: v for k, v in GOLD.items() if k.startswith(f"{pre}/dW/")}
    assert set(ref) == set(grads)
    assert any(k.startswith("rec_model.") for k in ref)
    gmax = max(float(GOLD[f"{pre}/max/{k}"]) for k in ref)
    for k, r in ref.items():
        scale = max(float(GOLD[f"{pre}/max/{k}"]), 1e-3 * gmax)
        e = np.abs(SC.sample(grads[k]).astype(np.float64) - r).max() / scale
        assert e <= TOL_G, f"{pre} d{k}: {e:.3e}"
    # two eager steps: the same bits
    loss2, _, grads2 = _step(model, batch, labels, c)
    assert torch.equal(loss, loss2)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k


# ------------------------------------------------------------------------------------------- 4. hipGraph capture
@pytest.mark.parametrize("scoring", SC.STEP_SCORERS)
def test_grad_step_is_captured_in_a_hipgraph_and_replays_bitwise(scoring):
    c = dict(model="standard", B=8, H=6, C=3, S=20, D=64, h=4, E=32, bias=True, seed=7301, min_len=3,
             temperature=0.08, lambda_cl=0.1)
    model = _step_model(c, scoring)
    model.train()
    with torch.no_grad():  # scorer biases that lift the scores above the relu: the scorer's backward carries gradient
        for p in model.rec_model.parameters():
            if p.dim() == 1:
                p.fill_(0.5)
    batch = synth.batch_to(cases.model_batch(c), DEV)
    labels = SC.step_labels(c["B"]).to(DEV)
    params = [p for p in model.parameters() if p.requires_grad]
    for p in params:
        p.grad = torch.zeros_like(p)

    def step():
        for p in params:
            p.grad.zero_()
        preds = torch.relu(model(batch))
        ue = model.get_user_embeddings(batch)
        loss = F.mse_loss(preds, batch["targets"]) + c["lambda_cl"] * contrastive_loss(ue, labels, c["temperature"])
        loss.backward()
        return loss

    # (one side stream for the eager steps and the capture: test_hip_train_step.py explains why)
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
    assert any(p.grad.abs().max() > 0 for p in model.rec_model.parameters())


# ------------------------------------------------------------------------------------------- 5. integrated gradients
@pytest.mark.parametrize("scoring", SC.STEP_SCORERS)
def test_integrated_gradients_batched_equals_the_loop_and_skips_scorer_weight_gradients(scoring, monkeypatch):
    from xnrs_amd.explain import integrated_gradients
    c = dict(model="standard", B=1, H=5, C=3, S=10, D=64, h=4, E=32, bias=True, seed=7401, min_len=3)
    model = _step_model(c, scoring)
    batch = synth.batch_to(cases.model_batch(c), DEV)
    hx, hm = batch["user_features"]["history"]["title_emb"]
    cx, cm = batch["candidate_features"]["title_emb"]
    a = integrated_gradients(model, hx, hm, cx, cm, candidate_idx=1, n_steps=12, batched=True)
    b = integrated_gradients(model, hx, hm, cx, cm, candidate_idx=1, n_steps=12, batched=False)
    scale = b["int_grads"].abs().max().item()
    assert (a["int_grads"] - b["int_grads"]).abs().max().item() <= 1e-5 * scale
    assert all(p.grad is None for p in model.rec_model.parameters())
    # the scorer's backward node is asked for no weight gradient, and launches no weight-gradient product
    calls = []
    lib = hip.lib()
    name = "xnrs_bilinear_scoring_bwd" if scoring == "bilin" else "xnrs_mlp_scoring_bwd"
    real = getattr(lib, name)

    class Spy:
        def __getattr__(self, item):
            return getattr(lib, item)

    def spy(*args):
        calls.append(args)
        return real(*args)
    spy_lib = Spy()
    setattr(spy_lib.__class__, name, staticmethod(spy))
    monkeypatch.setattr(hip, "lib", lambda: spy_lib)
    hxr = hx.clone().requires_grad_()
    batch["user_features"]["history"]["title_emb"] = (hxr, hm)
    r = torch.relu(model(batch)).sum()
    (g,) = torch.autograd.grad(r, hxr)
    assert torch.isfinite(g).all() and g.abs().max() > 0
    assert len(calls) == 1
    weight_slots = (8, 9) if scoring == "bilin" else (9, 10, 11, 12)  # dw, dbias | dw1, db1, dw2, db2
    assert all(calls[0][i] is None for i in weight_slots)
    assert all(p.grad is None for p in model.rec_model.parameters())


# ------------------------------------------------------------------------------------------- 6. the evaluation epoch
def _eval_model(scorer_kind):
    c = dict(model="standard", E=32, bias=True, h=4, D=32, H=8, S=6)
    cfg = Cfg(synth.model_cfg(c))
    torch.manual_seed(11)
    if scorer_kind == "dot_norm":
        model = make_model(Cfg(dict(cfg, scoring="dot")))
        model.rec_model = DotScoring(normalize=True)
    elif scorer_kind == "bilin_norm":
        model = make_model(Cfg(dict(cfg, scoring="dot")))
        model.rec_model = BilinScoring(32, normalize=True)
    else:
        model = make_model(Cfg(dict(cfg, scoring=scorer_kind)))
    return model.to(DEV).eval()


@pytest.mark.parametrize("scorer_kind", ["bilin", "fc", "dot_norm", "bilin_norm"])
def test_evaluate_scores_with_the_models_own_scorer(scorer_kind, monkeypatch):
    from xnrs_amd import evaluation as EV
    from xnrs_amd.data import DeviceBatcher
    store, beh = synth.click_world(n_news=150, n_sess=120)
    store, beh = store.to(DEV), beh.to(DEV)
    model = _eval_model(scorer_kind)
    n_proj = []
    real_proj = ops.mlp_news_proj
    monkeypatch.setattr(ops, "mlp_news_proj", lambda *a: n_proj.append(1) or real_proj(*a))
    res = EV.evaluate(model, store, beh, l_hist=8, batch=32)
    assert len(n_proj) == (1 if scorer_kind == "fc" else 0)  # the news-side projection: once per epoch
    # every impression through forward_store (the model's forward, the scorer's pair kernels)
    bat = DeviceBatcher(beh, 8, store.pad_row)
    sess = torch.arange(len(beh), device=DEV)
    hist, off, rows, csess, targets = bat.eval_batch(sess)
    offs = off.tolist()
    with torch.no_grad():
        ref = torch.cat([torch.relu(model.forward_store(store, hist[i:i + 1], rows[offs[i]:offs[i + 1]].reshape(1, -1))).reshape(-1)
                         for i in range(len(beh))])
        vecs, hm = EV.encode_news_table(model, store)
        table = model.rec_model.prepare_csr(vecs)
        u = model.encode_user(vecs[hist.long()], hm[hist.long()])
        got = model.rec_model.score_csr(table, rows, csess, u, relu=True)
    assert (got - ref).abs().max().item() <= 1e-5 * max(ref.abs().max().item(), 1.0)
    metrics = EV.rank_metrics(ref, targets, off).double().mean(0).tolist()
    for k, v in zip(EV.METRIC_NAMES, metrics):
        assert abs(res[k] - v) <= 1e-6, (k, res[k], v)


def test_evaluate_refuses_a_scorer_without_a_csr_path():
    from xnrs_amd import evaluation as EV

    class Cosine(torch.nn.Module):
        def forward(self, u, c):
            return ops.dot_scoring(u, c, True)
    store, beh = synth.click_world(n_news=40, n_sess=10)
    model = _eval_model("bilin")
    model.rec_model = Cosine()
    with pytest.raises(NotImplementedError, match="Cosine"):
        EV.evaluate(model, store.to(DEV), beh.to(DEV), l_hist=8)


def test_dot_evaluation_is_unchanged(monkeypatch):
    """DotScoring(normalize=False) still scores through evaluation.score_csr on the encoded table itself."""
    from xnrs_amd import evaluation as EV
    store, beh = synth.click_world(n_news=60, n_sess=30)
    model = _eval_model("dot")
    seen = []
    real = EV.score_csr
    monkeypatch.setattr(EV, "score_csr", lambda *a, **k: seen.append(a[0]) or real(*a, **k))
    EV.evaluate(model, store.to(DEV), beh.to(DEV), l_hist=8, batch=16)
    assert len(seen) == 2 and seen[0] is seen[1]


def test_scorer_parameters_are_in_the_first_gradient_bucket():
    from xnrs_amd.distributed import OverlappedGradBuckets
    for kind in ("bilin", "fc"):
        model = _eval_model(kind)
        b = OverlappedGradBuckets.by_tower(model)
        first = {id(p) for p in b.buckets[0].params}
        assert all(id(p) in first for p in model.rec_model.parameters())
