"""CPU: integrated gradients with ONE Q|K|V projection (xnrs_amd/explain.py) -- the algebra in fp64
against the reference's step-by-step loop over the oracle, the orchestration of xnrs_amd.explain (alphas, chunks, the
reduce's scale and accumulate flag, one backward per candidate, the attribution sums) on plain-torch stand-ins for the device
operations, and the refusals.  The kernels and the autograd node are checked on the GPU in tests/test_hip_ig_linear.py."""
import pytest
import torch

from oracle import xnrs_oracle as O
from tests import ig_linear_ref as R
from tests.golden import cases
from xnrs_amd import synth
from xnrs_amd.explain import explain_rows, integrated_gradients
from xnrs_amd.models import make_model
from xnrs_amd.models.blocks import TextEncoder, UserEncoder


class Cfg(dict):
    __getattr__ = dict.__getitem__


SHAPE = dict(model="NRMS", B=1, H=4, C=3, S=6, D=16, h=2, E=8, bias=True, seed=9101)


def _state(c, dtype=torch.float64):
    model = make_model(Cfg(cases.model_cfg(c)))
    sd = synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, c["seed"] + 1)
    return model, {k: v.to(dtype) for k, v in sd.items()}


def _inputs(c, dtype=torch.float64):
    """hist (1, H, S, D) / (1, H, S, 1) with news 1 all masked and news 2 with a masked tail; cand (1, C, S, D) / mask."""
    g = torch.Generator().manual_seed(c["seed"])
    H, C, S, D = c["H"], c["C"], c["S"], c["D"]
    hx = torch.randn(1, H, S, D, generator=g, dtype=dtype)
    hm = torch.ones(1, H, S, 1, dtype=dtype)
    hm[0, 1] = 0
    hm[0, 2, S // 2:] = 0
    cx = torch.randn(1, C, S, D, generator=g, dtype=dtype)
    cm = torch.ones(1, C, S, 1, dtype=dtype)
    cm[0, 0, S - 2:] = 0
    return (hx, hm), (cx, cm)


# ------------------------------------------------------------------------------------------------ 1. the algebra in fp64
def test_restated_encoder_equals_the_oracle_from_the_image_on():
    _, sd = _state(SHAPE)
    (hx, hm), _ = _inputs(SHAPE)
    nsd = R.sub(sd, "news_encoder")
    y_o, hm_o = O.text_encoder(hx, hm, nsd, SHAPE["h"])
    w, b = R.qkv_weights(nsd)
    y, m = R.encoder_from_qkv(hx[0] @ w.T + b, hm[0], nsd, SHAPE["h"])
    assert (y - y_o[0]).abs().max().item() <= 1e-12 * y_o.abs().max().item()
    assert torch.equal(m, hm_o[0])
    assert y_o[0, 0].abs().max() > 0


def test_one_projection_equals_the_step_by_step_loop_in_fp64():
    _, sd = _state(SHAPE)
    hist, cand = _inputs(SHAPE)
    with torch.no_grad():
        cidx = int(O.parent_forward(hist, cand, sd, SHAPE["h"]).reshape(-1).argmax())
    attr_l, ig_l, s_l = R.ig_step_by_step(sd, SHAPE["h"], hist, cand, cidx, 7)
    attr_p, ig_p, s_p = R.ig_projection_once(sd, SHAPE["h"], hist, cand, cidx, 7)
    scale = ig_l.abs().max().item()
    assert scale > 0 and s_l > 0  # (a score the ReLU cut to 0 would make the comparison vacuous)
    assert (ig_p - ig_l).abs().max().item() <= 1e-10 * scale
    assert (attr_p - attr_l).abs().max().item() <= 1e-10 * attr_l.abs().max().item()
    assert abs(s_p - s_l) <= 1e-12 * abs(s_l)
    assert ig_l[1].abs().max().item() == 0 and ig_p[1].abs().max().item() == 0   # the all-masked news gets nothing


# ------------------------------------------------------------------------------------------- 2. orchestration, stand-ins
class _CpuNews(TextEncoder):
    def forward(self, inpt):
        x, m = inpt
        return O.text_encoder(x, m, dict(self.state_dict()), self.att.h if self.att is not None else None)


class _CpuUser(UserEncoder):
    def forward(self, inpt, add_features=None, return_weights=False):
        x, m = inpt
        return O.user_encoder(x, m, dict(self.state_dict()), self.att.h if self.att is not None else None)


class _CpuDot(torch.nn.Module):
    def forward(self, u, c):
        return O.dot_scoring(u, c)


def _cpu_model(c):
    """The project's model object with its three parts computing on the CPU oracle (the HIP modules cannot run here)."""
    model, sd = _state(c)
    model = model.double()
    model.load_state_dict(sd)
    model.news_encoder.__class__ = _CpuNews
    model.user_encoder.__class__ = _CpuUser
    model.rec_model = _CpuDot()
    return model.eval(), sd


def _best(sd, hist, cand, h):
    with torch.no_grad():
        return int(O.parent_forward(hist, cand, sd, h).reshape(-1).argmax())


@pytest.mark.parametrize("n_steps,per", [(1, 0), (7, 0), (20, 6), (20, 64)])
def test_orchestration_equals_the_reference_loop(n_steps, per):
    model, sd = _cpu_model(SHAPE)
    hist, cand = _inputs(SHAPE)
    cidx = _best(sd, hist, cand, SHAPE["h"])
    attr, ig, s = R.ig_step_by_step(sd, SHAPE["h"], hist, cand, cidx, n_steps)
    be = R.TorchOps()
    out = integrated_gradients(model, hist[0], hist[1], cand[0], cand[1], candidate_idx=cidx, n_steps=n_steps,
                               steps_per_batch=per, projection_once=True, _backend=be)
    scale = ig.abs().max().item()
    assert scale > 0
    assert (out["int_grads"] - ig).abs().max().item() <= 1e-10 * scale
    assert (out["attr"] - attr).abs().max().item() <= 1e-10 * attr.abs().max().item()
    assert torch.allclose(out["news_attribution"], attr.sum(dim=1), rtol=0, atol=1e-10 * attr.abs().max().item())
    assert abs(out["s_true"] - s) <= 1e-12 * abs(s) and abs(out["s_attr"] - float(attr.sum())) <= 1e-10 * attr.abs().max().item() * attr.numel()
    # the reduce: scale da, no alpha weights, accumulate from the second chunk on; one forward per chunk
    chunk = n_steps if per <= 0 else min(per, n_steps)
    sizes = [min(chunk, n_steps - lo) for lo in range(0, n_steps, chunk)]
    assert be.calls == [(nb, 1.0 / n_steps, i > 0) for i, nb in enumerate(sizes)]
    assert be.forwards == len(sizes)
    assert all(p.grad is None for p in model.parameters())


def test_a_reduce_that_weights_by_alpha_is_told_apart():
    model, sd = _cpu_model(SHAPE)
    hist, cand = _inputs(SHAPE)
    cidx = _best(sd, hist, cand, SHAPE["h"])
    _, ig, _ = R.ig_step_by_step(sd, SHAPE["h"], hist, cand, cidx, 7)
    wrong = integrated_gradients(model, hist[0], hist[1], cand[0], cand[1], candidate_idx=cidx, n_steps=7, projection_once=True,
                                 _backend=R.AlphaWeightedOps())
    assert (wrong["int_grads"] - ig).abs().max().item() > 1e-3 * ig.abs().max().item()


class _Store:
    """What explain_rows asks of a NewsStore, on the CPU."""
    pad_row = 0

    def __init__(self, x, m):
        self.x, self.m = x, m

    def text(self, feature):
        return self.x, self.m


def _store(c, n_rows=9):
    g = torch.Generator().manual_seed(c["seed"] + 7)
    x = torch.randn(n_rows, c["S"], c["D"], generator=g, dtype=torch.float64)
    L = torch.randint(1, c["S"] + 1, (n_rows,), generator=g)
    m = (torch.arange(c["S"])[None, :] < L[:, None]).double()
    x[0], m[0] = 0, 0
    return _Store(x, m)


def test_explain_rows_shares_one_forward_between_the_candidates():
    model, sd = _cpu_model(SHAPE)
    store = _store(SHAPE)
    hist_rows = torch.tensor([3, 0, 5, 3], dtype=torch.int32)       # the pad row and a repeated row
    cand_rows = torch.tensor([7, 2, 8], dtype=torch.int32)
    be = R.TorchOps()
    out = explain_rows(model, store, hist_rows, cand_rows, n_steps=20, steps_per_batch=6, activation=None, _backend=be)
    assert out["attr"].shape == (3, 4, SHAPE["S"]) and out["news_attribution"].shape == (3, 4)
    assert out["s_true"].shape == (3,) and out["s_attr"].shape == (3,)
    assert be.forwards == 4 and len(be.calls) == 12                  # 4 chunks: ONE forward each, a reduce per candidate
    assert [c[2] for c in be.calls] == [False] * 3 + [True] * 9
    hist = (store.x[hist_rows.long()][None], store.m[hist_rows.long()][None, ..., None])
    cand = (store.x[cand_rows.long()][None], store.m[cand_rows.long()][None, ..., None])
    for j in range(3):
        one = explain_rows(model, store, hist_rows, cand_rows[j:j + 1], n_steps=20, steps_per_batch=6, activation=None,
                           _backend=R.TorchOps())
        attr, _, s = R.ig_step_by_step(sd, SHAPE["h"], hist, cand, j, 20, act=lambda t: t)
        tol = 1e-10 * attr.abs().max().item()
        assert (out["attr"][j] - one["attr"][0]).abs().max().item() <= tol
        assert (out["attr"][j] - attr).abs().max().item() <= tol
        assert abs(out["s_true"][j].item() - s) <= 1e-12 * abs(s)
        assert abs(out["s_attr"][j].item() - float(attr.sum())) <= tol * attr.numel()
        assert torch.allclose(out["news_attribution"][j], attr.sum(dim=1), rtol=0, atol=tol * attr.shape[1])
    assert out["attr"][:, 1].abs().max().item() == 0                 # the pad row of the history gets nothing


# ------------------------------------------------------------------------------------------------------- 3. refusals
def _plain(name):
    c = dict(SHAPE, model=name)
    return make_model(Cfg(cases.model_cfg(c))).eval()


def test_refusals_come_before_any_device_call():
    hist, cand = _inputs(SHAPE, torch.float32)
    nd = R.NoDevice()
    args = (hist[0], hist[1], cand[0], cand[1])
    rows, crow = torch.tensor([1, 2], dtype=torch.int32), torch.tensor([3], dtype=torch.int32)
    # an attention-free TextEncoder has no Q|K|V image
    with pytest.raises(NotImplementedError, match="attention stage"):
        integrated_gradients(_plain("standard"), *args, projection_once=True, _backend=nd)
    with pytest.raises(NotImplementedError, match="attention stage"):
        explain_rows(_plain("standard"), None, rows, crow, projection_once=True, _backend=nd)
    # a news encoder that is no TextEncoder
    naml = _plain("NAML")
    with pytest.raises(NotImplementedError, match="TextEncoder"):
        integrated_gradients(naml, *args, projection_once=True, _backend=nd)
    with pytest.raises(NotImplementedError, match="TextEncoder"):
        explain_rows(naml, None, rows, crow, _backend=nd)
    # train mode: every copy would draw its own dropout masks
    nrms = _plain("NRMS")
    with pytest.raises(ValueError, match="eval mode"):
        integrated_gradients(nrms.train(), *args, projection_once=True, _backend=nd)
    with pytest.raises(ValueError, match="eval mode"):
        explain_rows(nrms.train(), None, rows, crow, _backend=nd)
    nrms.eval()
    with pytest.raises(ValueError, match="n_steps"):
        integrated_gradients(nrms, *args, n_steps=0, projection_once=True, _backend=nd)
    with pytest.raises(ValueError, match="n_steps"):
        explain_rows(nrms, None, rows, crow, n_steps=0, _backend=nd)
    with pytest.raises(ValueError, match=r"\(H,\)"):
        explain_rows(nrms, None, rows.reshape(1, 2), crow, _backend=nd)
