"""GPU: CAUM (xnrs/models/full_models/caum.py:11-172) on the HIP path -- the model against the real reference
(tests/golden/caum.npz: every case of tests/golden/caum_cases.py) in eval mode, through forward and forward_store, and in the
MSE grad step (the fixed-mask dropout case included); the long-attention kernels alone against an fp64 softmax attention
written here; determinism; argument errors.

Bars: the project's for a model against the reference, 1e-4 on scores and 2e-4 on gradients (tests/test_hip_lstur.py), every
gradient against max(its own scale, 1e-3 of the largest parameter gradient) as tests/helpers.py scales them.  The reference
in fp32 sits within a quarter of both bars of itself in fp64 on every recorded case (caum.json "fp32_vs_fp64"; the generator
asserts it).  forward against forward_store: two GPU paths of the same arithmetic, 1e-6 with helpers.ATOL_FLOOR.

(The issue's optional cross-check of the long kernel against xnrs_mha_fwd is not made: that entry point projects its own
Q, K, V from x and cannot be handed a packed image.)"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helpers as H
from tests.golden import caum_cases as CC
from xnrs_amd import hip, ops, synth
from xnrs_amd.models.caum import make_caum

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = H.golden("caum")
META = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caum.json")))
TOL_S, TOL_G = 1e-4, 2e-4


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _model(c):
    model = make_caum(Cfg(CC.model_cfg(c)))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(synth.fill_state_dict(shapes, CC.weight_seed(c)))
    return model.to(DEV)


def _close_sampled(got, name, key, tol):
    """A tensor against its stored sample, on the scale of the WHOLE reference tensor."""
    ref = GOLD[f"{name}/{key}"].astype(np.float64)
    parts = key.split("/")
    scale = max(float(GOLD[f"{name}/{parts[0]}/max/{'/'.join(parts[1:])}"]), 1e-30)
    err = np.abs(CC.sample(got).astype(np.float64) - ref).max()
    print(f"{name} {key}: {err / scale:.3e}")
    assert err <= tol * scale, f"{name} {key}: {err:.3e} vs scale {scale:.3e}"


class _Store:
    """The news of one batch as a table: rows [0, B*H) the history slots, then the candidates."""

    def __init__(self, batch):
        hist, cand = batch["user_features"]["history"], batch["candidate_features"]
        (hx, hm), (cx, cm) = hist["title_emb"], cand["title_emb"]
        S, D = hx.shape[-2:]
        self.x = torch.cat([hx.reshape(-1, S, D), cx.reshape(-1, S, D)])
        self.m = torch.cat([hm.reshape(-1, S), cm.reshape(-1, S)])
        self.cols = {k: torch.cat([hist[k].reshape(-1), cand[k].reshape(-1)]) for k in hist if k != "title_emb"}
        B, Hn, Cn = hx.shape[0], hx.shape[1], cx.shape[1]
        self.hist_ids = torch.arange(B * Hn, dtype=torch.int32, device=hx.device).reshape(B, Hn)
        self.cand_ids = (B * Hn + torch.arange(B * Cn, dtype=torch.int32, device=hx.device)).reshape(B, Cn)

    def text(self, feature):
        assert feature == "title_emb"
        return self.x, self.m

    def column(self, name):
        return self.cols[name]


# ------------------------------------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("name", list(CC.CASES))
def test_scores_equal_the_reference(name):
    c = CC.CASES[name]
    model = _model(c).eval()
    batch = synth.batch_to(CC.batch(c), DEV)
    store = _Store(batch)
    with torch.no_grad():
        r, u, cv = model(batch, return_embeddings=True)
        r2, u2, cv2 = model.forward_store(store, store.hist_ids, store.cand_ids, return_embeddings=True)
    e = CC.emb_dim(c)
    assert r.shape == (c["B"], c["C"], 1) and u.shape == (c["B"], c["C"], e) and cv.shape == (c["B"], c["C"], e)
    assert torch.isfinite(r).all()  # (tiny: ragged histories, all-masked slots included)
    for key, got in (("eval/r", r), ("eval/u", u), ("eval/c", cv)):
        _close_sampled(got, name, key, TOL_S)
    for a, b, what in ((r2, r, "r"), (u2, u, "u"), (cv2, cv, "c")):
        H.assert_close(a, b, 1e-6, f"{name} forward_store {what}")


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


@pytest.mark.parametrize("name", list(CC.CASES))
def test_grad_step_equals_the_reference(name):
    c = CC.CASES[name]
    model = CC.fix_dropouts(_model(c), c)
    batch = synth.batch_to(CC.batch(c), DEV)
    loss, preds, dh, dc = _grad_step(model, batch)
    pre = f"{name}/grad"
    H.assert_close(loss.reshape(1), GOLD[f"{pre}/loss"].reshape(1), TOL_S, f"{pre} loss")
    H.assert_close(preds, GOLD[f"{pre}/preds"], TOL_S, f"{pre} preds")
    no_grad = META["no_grad"][name]
    assert no_grad == ["dW/news_encoder.title_encoder.dummy_param"]
    gmax = max(float(v) for k, v in GOLD.items() if k.startswith(f"{pre}/max/dW/"))
    grads = {"in/hist": dh, "in/cand": dc}
    grads.update({f"dW/{k}": p.grad for k, p in model.named_parameters()})
    checked = 0
    for k, g in grads.items():
        if k in no_grad:
            assert g is None or float(g.abs().max()) == 0.0, f"{pre} {k} must get no gradient"
            continue
        assert g is not None, f"{pre} {k}: no gradient"
        own = float(GOLD[f"{pre}/max/{k}"])
        scale = max(own, 1e-3 * gmax)
        err = np.abs(CC.sample(g).astype(np.float64) - GOLD[f"{pre}/{k}"]).max()
        print(f"{pre} {k}: {err / scale:.3e}")
        assert err <= TOL_G * scale, f"{pre} {k}: {err:.3e} vs scale {scale:.3e}"
        assert abs(float(g.abs().max()) - own) <= TOL_G * scale, f"{pre} max {k}"
        checked += 1
    # every parameter but the news encoder's dummy_param, and both inputs (36 parameters with cfg.bias, 32 without, + 6 with
    # the sub-category encoder)
    assert checked == len(grads) - 1 == len(list(model.parameters())) + 1 and checked >= 31 + 2


# ------------------------------------------------------------------------------------------- 2. long attention vs fp64
def _ref_attention(qkv, heads):
    """fp64 softmax(q k^T / sqrt(d_k)) v per head over a seq-first packed (L, Nb, 3E) image."""
    L, Nb, E3 = qkv.shape
    E = E3 // 3
    q, k, v = (t.reshape(L, Nb, heads, E // heads) for t in qkv.split(E, dim=-1))
    s = torch.einsum("lnhd,mnhd->nhlm", q, k) / (E // heads) ** 0.5
    return torch.einsum("nhlm,mnhd->lnhd", torch.softmax(s, dim=-1), v).reshape(L, Nb, E)


@pytest.mark.parametrize("dk", [1, 8, 17, 64])
@pytest.mark.parametrize("L", [1, 17, 128, 129, 154, 300])
def test_attn_long_matches_fp64(L, dk):
    heads = 2
    E = heads * dk
    for Nb in (1, 3):
        g = torch.Generator().manual_seed(1000 * L + 10 * dk + Nb)
        qkv = torch.randn(L, Nb, 3 * E, generator=g)
        d_o = torch.randn(L, Nb, E, generator=g)
        qd = qkv.double().requires_grad_(True)
        ref = _ref_attention(qd, heads)
        ref.backward(d_o.double())
        qg = qkv.to(DEV).requires_grad_(True)
        with torch.no_grad():
            o_inf = ops.attn_long(qg.detach(), heads)
        o = ops.attn_long(qg, heads)
        o.backward(d_o.to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(o_inf, o.detach()), "inference and training forwards are the same arithmetic"
        assert torch.isfinite(o).all() and torch.isfinite(qg.grad).all()
        print(f"L={L} Nb={Nb} dk={dk}: o {H.rel_err(o, ref.detach()):.3e} dqkv {H.rel_err(qg.grad, qd.grad):.3e}")
        H.assert_close(o, ref.detach(), TOL_S, f"o L={L} Nb={Nb} dk={dk}")
        H.assert_close(qg.grad, qd.grad, TOL_G, f"dqkv L={L} Nb={Nb} dk={dk}")


def test_attn_long_shipped_width_and_widest_head():
    """d_k = 17 at 16 heads (E = 272, LSTUR-style dims) and the widest head the kernel takes (d_k = 128: four column blocks)."""
    for L, Nb, heads, dk in ((70, 2, 16, 17), (45, 1, 1, 128), (40, 2, 2, 96)):
        E = heads * dk
        g = torch.Generator().manual_seed(L + dk)
        qkv = torch.randn(L, Nb, 3 * E, generator=g)
        d_o = torch.randn(L, Nb, E, generator=g)
        qd = qkv.double().requires_grad_(True)
        ref = _ref_attention(qd, heads)
        ref.backward(d_o.double())
        qg = qkv.to(DEV).requires_grad_(True)
        o = ops.attn_long(qg, heads)
        o.backward(d_o.to(DEV))
        H.assert_close(o, ref.detach(), TOL_S, f"o dk={dk}")
        H.assert_close(qg.grad, qd.grad, TOL_G, f"dqkv dk={dk}")


# ------------------------------------------------------------------------------------------- 3. determinism
def test_long_grad_step_twice_is_bitwise_equal():
    c = CC.CASES["long"]
    model = CC.fix_dropouts(_model(c), c)
    outs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        batch = synth.batch_to(CC.batch(c), DEV)
        loss, preds, dh, dc = _grad_step(model, batch)
        outs.append([loss.detach().clone(), preds.detach().clone(), dh.clone(), dc.clone()]
                    + [p.grad.clone() for p in model.parameters() if p.grad is not None])
    assert len(outs[0]) == len(outs[1]) == 4 + len(list(model.parameters())) - 1
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ------------------------------------------------------------------------------------------- 4. argument errors
def test_argument_errors_return_the_error_code_and_launch_nothing():
    l = hip.lib()
    st = hip.stream_ptr(DEV)
    L, Nb = 5, 2
    qkv = torch.randn(L, Nb, 3 * 260, device=DEV)
    o = torch.full((L, Nb, 260), 7.0, device=DEV)

    def fwd(q, out, E, heads):
        return l.xnrs_attn_long_fwd(hip.ptr(q), Nb * 3 * E, 3 * E, hip.ptr(out), Nb * E, E, L, Nb, E, heads, st)

    assert fwd(qkv, o, 260, 3) == -2                       # E % n_heads != 0
    assert fwd(qkv, o, 260, 2) == -4                       # d_k = 130 > 128
    assert fwd(None, o, 260, 4) == -1 and fwd(qkv, None, 260, 4) == -1
    assert l.xnrs_attn_long_fwd_train(hip.ptr(qkv), Nb * 780, 780, hip.ptr(o), Nb * 260, 260, L, Nb, 260, 4, None, 0, st) == -3
    assert l.xnrs_attn_long_bwd(hip.ptr(qkv), Nb * 780, 780, hip.ptr(o), None, Nb * 260, 260, None, 0, hip.ptr(qkv), L, Nb, 260, 4,
                                None, 0, st) == -1
    assert l.xnrs_caum_pair_fwd(None, hip.ptr(qkv), 8, hip.ptr(o), hip.ptr(o), 2, 2, 2, 4, st) == -1
    assert l.xnrs_caum_pair_fwd(hip.ptr(qkv), hip.ptr(qkv), 7, hip.ptr(o), hip.ptr(o), 2, 2, 2, 4, st) == -1   # pitch < 2E
    assert l.xnrs_caum_pool_fwd(hip.ptr(qkv), None, None, hip.ptr(qkv), hip.ptr(o), None, 2, 2, 4, 4, st) == -1
    assert l.xnrs_caum_pool_fwd(hip.ptr(qkv), hip.ptr(qkv), None, hip.ptr(qkv), hip.ptr(o), None, 1, 9000, 1, 1, st) == -4
    assert l.xnrs_act_bwd(hip.ptr(qkv), hip.ptr(qkv), None, 4, hip.ACT_TANH, st) == -1
    assert l.xnrs_act_bwd(hip.ptr(qkv), hip.ptr(qkv), hip.ptr(o), 4, 9, st) == -1
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()), "a refused call writes nothing"
    for code in (-1, -2, -3, -4):
        assert l.xnrs_error_string(code).decode() not in ("", "unknown error")
    with pytest.raises(RuntimeError, match="n_heads"):
        ops.attn_long(qkv, 3)
    with pytest.raises(hip.XnrsHipError, match="code -4"):
        ops.attn_long(qkv, 2)
    # a zero-size call is fine and launches nothing
    assert l.xnrs_attn_long_fwd(None, 0, 0, None, 0, 0, 0, Nb, 260, 4, st) == 0


def test_the_tower_reproduces_the_batch_axis_attention():
    """caum.py:52-54,91-92: the attended axis is batch x candidate, so changing ONE impression's history moves the others'
    scores -- reproduced, not fixed."""
    c = CC.CASES["tiny"]
    model = _model(c).eval()
    batch = synth.batch_to(CC.batch(c), DEV)
    with torch.no_grad():
        r0 = model(batch).clone()
        hx, hm = batch["user_features"]["history"]["title_emb"]
        hx[2] = hx[2].flip(0) * 1.5
        r1 = model(batch)
    assert not torch.equal(r0[0], r1[0])
