"""GPU: integrated gradients with ONE Q|K|V projection -- the two streaming kernels (xnrs_ig_expand,
xnrs_ig_reduce: values, bits, the scalar route behind shifted pointers), the autograd node that encodes from a given image
(ops.text_encoder_from_qkv), the explanation end to end against the CPU oracle and against the batched path, explain_rows /
explain_recommendations over a news store, and the entry points' refusals.

Bars, none of them new: SWITCH_TOL = 2e-6 between two GPU paths of the same arithmetic in another order
(tests/test_hip_topk.py), 2e-5 of the scale against the oracle (tests/test_hip_explain.py), and their triangle 4e-5 between
the one-projection path and the batched path (each within 2e-5 of the oracle; the two differ by fp32 rounding, (a x) W
against a (x W), not only by summation order)."""
import ctypes as C

import pytest
import torch

from oracle import xnrs_oracle as O
from tests.golden import cases, scorer_cases as SC
from tests.test_hip_explain import oracle_ig
from tests.test_hip_grads import Cfg, load
from xnrs_amd import autograd as AG, hip, ops, synth
from xnrs_amd.data import DeviceBatcher, NewsStore
from xnrs_amd.explain import explain_recommendations, explain_rows, integrated_gradients
from xnrs_amd.models import make_model
from xnrs_amd.models.blocks import AdditiveAttention, MultiHeadAttention, TextEncoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWITCH_TOL = 2e-6
ORACLE_TOL = 2e-5
SHAPES = [(1, 1, 4), (5, 7, 36), (3, 130, 18), (4, 257, 192)]   # W = 18: the scalar route by width
GUARD = 8


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _shifted(t):
    """A copy of t one float off an aligned base, between guard floats -> (the view, its buffer)."""
    buf = torch.full((t.numel() + 2 * GUARD + 1,), 777.0, device=DEV)
    view = buf[GUARD + 1:GUARD + 1 + t.numel()].view(t.shape)
    assert view.data_ptr() % 16 == 4
    view.copy_(t)
    return view, buf


def _guards_intact(buf, numel):
    return bool((buf[:GUARD + 1] == 777.0).all() and (buf[GUARD + 1 + numel:] == 777.0).all())


def _expand(p, bias, alphas, out):
    n, (rows, W) = alphas.numel(), p.shape
    hip.check(hip.lib().xnrs_ig_expand(hip.ptr(p), hip.ptr(bias), hip.ptr(alphas), n, rows, W, hip.ptr(out), hip.stream_ptr(DEV)),
              "xnrs_ig_expand")
    return out


def _reduce(g, n, scale, out, accumulate):
    rows, W = out.shape
    hip.check(hip.lib().xnrs_ig_reduce(hip.ptr(g), n, rows, W, scale, hip.ptr(out), accumulate, hip.stream_ptr(DEV)), "xnrs_ig_reduce")
    return out


# ------------------------------------------------------------------------------------------------------------ 1. expand
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("n,rows,W", SHAPES)
def test_expand(n, rows, W, with_bias):
    g = _gen(11 + n + rows + W)
    p = torch.randn((rows, W), device=DEV, generator=g)
    bias = torch.randn((W,), device=DEV, generator=g) if with_bias else None
    alphas = torch.rand((n,), device=DEV, generator=g) + 0.01
    out = _expand(p, bias, alphas, torch.full((n * rows, W), float("nan"), device=DEV))
    assert ops.ig_expand(p, bias, alphas).equal(out)
    b64 = bias.double() if with_bias else 0.0
    ref = (alphas.double()[:, None, None] * p.double()[None] + b64).float().reshape(n * rows, W)
    inf = torch.full_like(ref, float("inf"))
    ok = (out == ref) | (out == torch.nextafter(ref, inf)) | (out == torch.nextafter(ref, -inf))
    assert bool(ok.all())                                                      # within 1 ulp of the fp64 value, rounded
    # p and out one float off an aligned base: the scalar route, the same bits
    ps, pbuf = _shifted(p)
    os_, obuf = _shifted(torch.full((n * rows, W), float("nan"), device=DEV))
    _expand(ps, bias, alphas, os_)
    assert torch.equal(os_, out) and _guards_intact(obuf, out.numel()) and _guards_intact(pbuf, p.numel())
    if with_bias:  # the bias alone off an aligned base: read one float at a time on either route, the same bits
        bs, bbuf = _shifted(bias)
        assert torch.equal(_expand(p, bs, alphas, torch.full_like(out, float("nan"))), out) and _guards_intact(bbuf, W)
        assert torch.equal(_expand(ps, bs, alphas, os_.fill_(float("nan"))), out)
    # small integers, alphas in {0.25, 0.5, 1}: every product and sum is exact
    pi = torch.randint(-8, 9, (rows, W), device=DEV, generator=g).float()
    bi = torch.randint(-8, 9, (W,), device=DEV, generator=g).float() if with_bias else None
    ai = torch.tensor([0.25, 0.5, 1.0], device=DEV)[torch.randint(0, 3, (n,), device=DEV, generator=g)]
    exact = ai[:, None, None] * pi[None] + (bi if with_bias else 0.0)
    assert torch.equal(ops.ig_expand(pi, bi, ai), exact.reshape(n * rows, W))


# ------------------------------------------------------------------------------------------------------------ 2. reduce
@pytest.mark.parametrize("n", [1, 2, 37])
@pytest.mark.parametrize("_n,rows,W", SHAPES)
def test_reduce(n, _n, rows, W):
    gen = _gen(23 + n + rows + W)
    g = torch.randn((n * rows, W), device=DEV, generator=gen)
    old = torch.randn((rows, W), device=DEV, generator=gen)
    scale = 1.0 / 37
    s = g[:rows].clone()
    for i in range(1, n):
        s = s + g[i * rows:(i + 1) * rows]                  # one fp32 chain, ascending
    prod = s * torch.tensor(scale, dtype=torch.float32, device=DEV)
    want = {0: prod, 1: old + prod}                         # the product and the sum rounded one by one
    gs, gbuf = _shifted(g)
    for acc in (0, 1):
        out = _reduce(g, n, scale, old.clone(), acc)
        assert torch.equal(out, want[acc])
        assert torch.equal(_reduce(g, n, scale, old.clone(), acc), out)       # two runs, equal bits
        outs, obuf = _shifted(old)
        _reduce(gs, n, scale, outs, acc)
        assert torch.equal(outs, out) and _guards_intact(obuf, old.numel())   # the scalar route, the same bits
        assert torch.equal(ops.ig_reduce(g, n, scale, old.clone(), bool(acc)), out)
    assert _guards_intact(gbuf, g.numel())


# ---------------------------------------------------------------------------------------------------- 3. the node alone
def _encoder():
    enc = TextEncoder(AdditiveAttention(64, 32), 0.0, out_features=32, in_features=64, head=True, att=MultiHeadAttention(4, 64))
    enc, _ = load(enc, 6301)
    return enc


def _node_inputs():
    g = _gen(6302)
    x = torch.randn((6, 12, 64), device=DEV, generator=g)
    m = (torch.rand((6, 12, 1), device=DEV, generator=g) < 0.7).float()       # holes
    m[:, 0] = 1
    m[2] = 0                                                                  # an all-masked sequence
    m[4] = 0
    m[4, -1] = 1                                                              # its only live token is the last
    r = torch.randn((6, 32), device=DEV, generator=g)
    return x, m, r


def _wcat(att):
    w = torch.cat([att.q_linear.weight, att.k_linear.weight, att.v_linear.weight]).detach().contiguous()
    b = torch.cat([att.q_linear.bias, att.k_linear.bias, att.v_linear.bias]).detach().contiguous()
    return w, b


@pytest.mark.parametrize("fold", ["1", "0"])
def test_node_from_a_given_image(fold, monkeypatch):
    enc = _encoder()
    x, m, r = _node_inputs()
    w, b = _wcat(enc.att)
    real = AG._f32_out
    monkeypatch.setattr(AG, "_f32_out", lambda shape, dev: real(shape, dev).fill_(float("nan")))  # the returned image: NaN first
    with hip.knobs(XNRS_FOLD_TRAIN=fold):
        xd = x.clone().requires_grad_()
        yd, hmd = ops.text_encoder(xd, m, enc)
        (dx,) = torch.autograd.grad((yd * r).sum(), xd)
        qkv = ops.linear(x, w, b).reshape(6 * 12, 192).requires_grad_()
        images_before = len(AG._QKV_IMAGES)
        y, hm = ops.text_encoder_from_qkv(qkv, x, m, enc)
        assert len(AG._QKV_IMAGES) == images_before                            # the node registers no image
        (g1,) = torch.autograd.grad((y * r).sum(), qkv, retain_graph=True)
        (g2,) = torch.autograd.grad((y * r).sum(), qkv)
    ys = yd.abs().max().item()
    ey = (y - yd).abs().max().item()
    assert ey <= SWITCH_TOL * ys and torch.equal(hm, hmd)
    assert bool(torch.isfinite(g1).all())                                      # every row of the image was written
    assert g1.reshape(6, 12, 192)[2].abs().max().item() == 0                   # ... the all-masked sequence's as zeros
    assert g1.abs().max().item() > 0
    assert torch.equal(g1, g2)                                                 # a second backward over the retained graph
    back = ops.linear_input_grad(g1, w).reshape(6, 12, 64)
    ex = (back - dx).abs().max().item()
    print(f"MARGIN node fold={fold}: y {ey / (SWITCH_TOL * ys):.3f}  dx {ex / (SWITCH_TOL * dx.abs().max().item()):.3f}  (error / bar)")
    assert ex <= SWITCH_TOL * dx.abs().max().item()
    assert all(p.grad is None for p in enc.parameters())


# -------------------------------------------------------------------------------------- 4. end to end against the oracle
NRMS = dict(model="NRMS", B=1, H=7, C=3, S=12, D=64, h=4, E=32, bias=True, seed=5101, min_len=4)
_ORACLE = {}


def _nrms_case():
    """The NRMS case of tests/test_hip_explain.py with history slot 1 emptied, and its oracle explanation (computed once)."""
    if not _ORACLE:
        batch = cases.model_batch(NRMS)
        hx, hm = batch["user_features"]["history"]["title_emb"]
        hx, hm = hx.clone(), hm.clone()
        hx[0, 1], hm[0, 1] = 0, 0
        cand = batch["candidate_features"]["title_emb"]
        shapes = {k: tuple(v.shape) for k, v in make_model(Cfg(cases.model_cfg(NRMS))).state_dict().items()}
        sd = synth.fill_state_dict(shapes, NRMS["seed"] + 1)
        with torch.no_grad():
            cidx = int(O.parent_forward((hx, hm), cand, sd, NRMS["h"]).reshape(-1).argmax())
        _ORACLE.update(hist=(hx, hm), cand=cand, cidx=cidx, ref=oracle_ig(sd, NRMS["h"], (hx, hm), cand, cidx, 24))
    return _ORACLE


def test_projection_once_equals_the_reference_loop_on_the_oracle():
    k = _nrms_case()
    model, _ = load(make_model(Cfg(cases.model_cfg(NRMS))), NRMS["seed"] + 1)
    attr_o, ig_o, s_o = k["ref"]
    args = [t.to(DEV) for t in (*k["hist"], *k["cand"])]
    out = integrated_gradients(model, *args, candidate_idx=k["cidx"], n_steps=24, projection_once=True)
    scale = ig_o.abs().max().item()
    assert scale > 0
    e_o = (out["int_grads"].cpu() - ig_o).abs().max().item()
    assert e_o <= ORACLE_TOL * scale
    assert (out["attr"].cpu() - attr_o).abs().max().item() <= ORACLE_TOL * attr_o.abs().max().item()
    assert abs(out["s_true"] - s_o) <= ORACLE_TOL * max(abs(s_o), 1e-3)
    assert out["int_grads"][1].abs().max().item() == 0                         # the emptied slot
    batched = integrated_gradients(model, *args, candidate_idx=k["cidx"], n_steps=24)
    e_b = (out["int_grads"] - batched["int_grads"]).abs().max().item()
    chunk = integrated_gradients(model, *args, candidate_idx=k["cidx"], n_steps=24, steps_per_batch=5, projection_once=True)
    e_c = (chunk["int_grads"] - out["int_grads"]).abs().max().item()
    print(f"MARGIN projection_once: vs oracle {e_o / scale:.3e}  vs batched {e_b / scale:.3e}  chunks of 5 {e_c / scale:.3e}  (of the scale)")
    assert e_b <= 2 * ORACLE_TOL * scale
    assert e_c <= SWITCH_TOL * scale and abs(chunk["s_true"] - out["s_true"]) <= SWITCH_TOL * max(abs(s_o), 1e-3)
    assert all(p.grad is None for p in model.parameters())


@pytest.mark.parametrize("scoring", ["dot", "bilin"])
def test_projection_once_equals_the_batched_path_with_other_scorers(scoring):
    k = _nrms_case()
    model, _ = load(make_model(Cfg(SC.step_cfg(NRMS, scoring))), NRMS["seed"] + 1)
    args = [t.to(DEV) for t in (*k["hist"], *k["cand"])]
    a = integrated_gradients(model, *args, candidate_idx=k["cidx"], n_steps=12, activation=None, projection_once=True)
    b = integrated_gradients(model, *args, candidate_idx=k["cidx"], n_steps=12, activation=None)
    scale = b["int_grads"].abs().max().item()
    assert scale > 0
    assert (a["int_grads"] - b["int_grads"]).abs().max().item() <= 2 * ORACLE_TOL * scale
    assert all(p.grad is None for p in model.parameters())


# ------------------------------------------------------------------------------------------------------ 5. explain_rows
ROWS = dict(model="NRMS", B=1, H=6, C=3, S=12, D=64, h=4, E=32, bias=True, seed=6501)
HIST = [5, 0, 17, 5, 0, 23]     # the pad row twice, row 5 twice
CAND = [9, 31, 2]
_WORLD = {}


def _world():
    if not _WORLD:
        store, beh = synth.click_world(n_news=39, n_sess=3, S=12, D=64, seed=3)
        model, _ = load(make_model(Cfg(cases.model_cfg(ROWS))), ROWS["seed"] + 1)
        _WORLD.update(store=store.to(DEV), beh=beh.to(DEV), model=model)
    return _WORLD


def _rows(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _close(a, b, tol, what):
    scale = b.abs().max().item()
    err = (a - b).abs().max().item()
    assert scale > 0 and err <= tol * scale, (what, err, tol * scale)


def test_explain_rows_equals_integrated_gradients_on_the_gathered_tokens():
    w = _world()
    store, model = w["store"], w["model"]
    assert store.n_rows == 40
    out = explain_rows(model, store, _rows(HIST), _rows(CAND), n_steps=10, activation=None)
    assert out["attr"].shape == (3, 6, 12) and out["news_attribution"].shape == (3, 6) and out["s_true"].shape == (3,)
    hx, hm = store.gather(_rows(HIST)[None])
    cx, cm = store.gather(_rows(CAND)[None])
    for j in range(3):
        one = integrated_gradients(model, hx, hm, cx, cm, candidate_idx=j, n_steps=10, activation=None, projection_once=True)
        _close(out["attr"][j], one["attr"], SWITCH_TOL, f"attr {j}")
        _close(out["news_attribution"][j], one["news_attribution"], SWITCH_TOL, f"news_attribution {j}")
        assert abs(out["s_true"][j].item() - one["s_true"]) <= SWITCH_TOL * max(abs(one["s_true"]), 1e-3)
        assert abs(out["s_attr"][j].item() - one["s_attr"]) <= SWITCH_TOL * one["attr"].abs().sum().item()  # (a sum's scale)
    assert out["attr"][:, 1].abs().max().item() == 0 and out["attr"][:, 4].abs().max().item() == 0   # the pad rows
    assert all(p.grad is None for p in model.parameters())


def test_explain_rows_clamps_rows_outside_the_table_once_for_every_use():
    """A history row outside the table: the tokens AND the projection come from the clamped row (no read out of bounds,
    one consistent explanation) and the sticky status word says so, as NewsStore.gather has it."""
    w = _world()
    store, model = w["store"], w["model"]
    hip.clear_status()
    bad = [5, -1, 17, 5, 43, 23]          # -1 -> row 0 (the pad row), 43 -> row 39
    out = explain_rows(model, store, _rows(bad), _rows(CAND), n_steps=10, activation=None)
    with pytest.raises(hip.XnrsHipError, match="status word"):
        hip.check_status(DEV)
    ref = explain_rows(model, store, _rows([5, 0, 17, 5, 39, 23]), _rows(CAND), n_steps=10, activation=None)
    hip.check_status(DEV)                 # rows inside the table: a clean word
    for key in ("attr", "news_attribution", "s_true", "s_attr"):
        assert torch.equal(out[key], ref[key])
    for s in (store, store.astype(torch.bfloat16)):
        a = explain_rows(model, s, _rows(bad), _rows(CAND), n_steps=10, activation=None)
        hip.clear_status()
        assert bool(torch.isfinite(a["attr"]).all()) and a["attr"][:, 1].abs().max().item() == 0


def test_explain_rows_from_a_bf16_store():
    w = _world()
    store, model = w["store"], w["model"]
    s16 = store.astype(torch.bfloat16)
    wide = NewsStore(s16.x.float(), store.m, store.ids)
    a = explain_rows(model, s16, _rows(HIST), _rows(CAND), n_steps=10, activation=None)
    b = explain_rows(model, wide, _rows(HIST), _rows(CAND), n_steps=10, activation=None)
    _close(a["attr"], b["attr"], SWITCH_TOL, "attr")
    _close(a["s_true"], b["s_true"], SWITCH_TOL, "s_true")


def test_explain_rows_without_an_attention_stage_takes_the_batched_path():
    w = _world()
    store = w["store"]
    model, _ = load(make_model(Cfg(cases.model_cfg(dict(ROWS, model="standard")))), ROWS["seed"] + 2)
    out = explain_rows(model, store, _rows(HIST), _rows(CAND), n_steps=10, activation=None)
    hx, hm = store.gather(_rows(HIST)[None])
    cx, cm = store.gather(_rows(CAND)[None])
    for j in range(3):
        one = integrated_gradients(model, hx, hm, cx, cm, candidate_idx=j, n_steps=10, activation=None)
        _close(out["attr"][j], one["attr"], SWITCH_TOL, f"attr {j}")
        assert abs(out["s_true"][j].item() - one["s_true"]) <= SWITCH_TOL * max(abs(one["s_true"]), 1e-3)


def test_explain_recommendations_gathers_the_history_as_recommend_does():
    w = _world()
    store, beh, model = w["store"], w["beh"], w["model"]
    rows = _rows(CAND)
    out = explain_recommendations(model, store, beh, 6, 1, rows, n_steps=10, activation=None)
    hist = DeviceBatcher(beh, 6, store.pad_row).eval_batch(torch.tensor([1], device=DEV))[0][0]
    ref = explain_rows(model, store, hist, rows, n_steps=10, activation=None)
    for key in ("attr", "news_attribution", "s_true", "s_attr"):
        assert torch.equal(out[key], ref[key])
    with pytest.raises(ValueError, match="filler"):
        explain_recommendations(model, store, beh, 6, 1, _rows([3, -1]))


# ---------------------------------------------------------------------------------------------------------- 6. refusals
def test_entry_points_refuse_bad_arguments_and_write_nothing():
    l = hip.lib()
    st = hip.stream_ptr(DEV)
    p = torch.ones((4, 8), device=DEV)
    al = torch.ones((3,), device=DEV)
    out = torch.full((12, 8), 5.0, device=DEV)
    acc = torch.full((4, 8), 5.0, device=DEV)
    P, A, OUT, ACC = (hip.ptr(t) for t in (p, al, out, acc))
    EINVAL = -1
    assert l.xnrs_ig_expand(P, None, A, -1, 4, 8, OUT, st) == EINVAL
    assert l.xnrs_ig_expand(P, None, A, 3, -4, 8, OUT, st) == EINVAL
    assert l.xnrs_ig_expand(P, None, A, 3, 4, 0, OUT, st) == EINVAL
    assert l.xnrs_ig_expand(None, None, A, 3, 4, 8, OUT, st) == EINVAL
    assert l.xnrs_ig_expand(P, None, None, 3, 4, 8, OUT, st) == EINVAL
    assert l.xnrs_ig_expand(P, None, A, 3, 4, 8, None, st) == EINVAL
    assert l.xnrs_ig_reduce(OUT, -1, 4, 8, 1.0, ACC, 0, st) == EINVAL
    assert l.xnrs_ig_reduce(OUT, 3, -4, 8, 1.0, ACC, 0, st) == EINVAL
    assert l.xnrs_ig_reduce(None, 3, 4, 8, 1.0, ACC, 0, st) == EINVAL
    assert l.xnrs_ig_reduce(OUT, 3, 4, 8, 1.0, None, 0, st) == EINVAL
    assert l.xnrs_ig_reduce(OUT, 3, 4, 8, 1.0, ACC, 2, st) == EINVAL
    # nothing to do: OK, nothing written
    assert l.xnrs_ig_expand(P, None, A, 0, 4, 8, OUT, st) == 0 and l.xnrs_ig_expand(P, None, A, 3, 0, 8, OUT, st) == 0
    assert l.xnrs_ig_reduce(OUT, 0, 4, 8, 1.0, ACC, 0, st) == 0 and l.xnrs_ig_reduce(OUT, 3, 0, 8, 1.0, ACC, 0, st) == 0
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((acc == 5.0).all())
    with pytest.raises(hip.XnrsHipError, match="attention stage"):
        enc = TextEncoder(AdditiveAttention(64, 32), 0.0, out_features=32, in_features=64, head=True).to(DEV)
        ops.text_encoder_from_qkv(torch.zeros((12, 192), device=DEV), torch.zeros((1, 12, 64), device=DEV),
                                  torch.ones((1, 12, 1), device=DEV), enc)
