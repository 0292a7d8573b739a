#!/usr/bin/env python
"""Generate tests/golden/caum.{json,npz} from the REAL reference: its CAUM (xnrs/models/full_models/caum.py:11-172) built by
its make_model with the CAUMScoring scorer, in eval mode (scores, user vectors, candidate vectors) and in the MSE grad step
(training.py:97-113,376-393: relu(model(batch)), mse_loss, backward) for the cases of tests/golden/caum_cases.py; the
state_dict contract of config/mind_small_LSTUR.yml's flat keys + model CAUM / scoring CAUMScoring / n_heads 16; and, per
case, the distance between the reference in fp32 and the same reference in fp64, which must stay within a quarter of the
test bars (1e-4 scores, 2e-4 gradients) -- a case that does not gets another seed or shape, never a wider bar.

Imports the reference exactly as make_golden_lstur.py does.  Stores outputs only: inputs and weights regenerate from the
seeds of caum_cases.py.  Runs only where the reference is present; the GPU machine never needs it.

    python tests/golden/make_golden_caum.py            # rewrites tests/golden/caum.json and caum.npz
"""
import importlib.machinery
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"

for name, path in [("xnrs", f"{REF}/xnrs"), ("xnrs.models", f"{REF}/xnrs/models")]:
    mod = types.ModuleType(name)
    mod.__path__ = [path]
    sys.modules[name] = mod
for name, attrs in [("omegaconf", {"DictConfig": dict}), ("wandb", {})]:
    if name not in sys.modules:
        mod = types.ModuleType(name)
        mod.__spec__ = importlib.machinery.ModuleSpec(name, None)
        for k, v in attrs.items():
            setattr(mod, k, v)
        sys.modules[name] = mod

from xnrs.models.make_model import make_model  # noqa: E402

from xnrs_amd import synth  # noqa: E402
from tests.golden import caum_cases as CC  # noqa: E402

TOL_S, TOL_G = 1e-4, 2e-4


class Cfg(dict):
    __getattr__ = dict.__getitem__


def npy(t):
    return t.detach().cpu().numpy()


def build(c, double=False):
    model = make_model(Cfg(CC.model_cfg(c)))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(synth.fill_state_dict(shapes, CC.weight_seed(c)))
    return model.double() if double else model


def to_double(b):
    if isinstance(b, torch.Tensor):
        return b.double() if b.is_floating_point() else b
    if isinstance(b, dict):
        return {k: to_double(v) for k, v in b.items()}
    if isinstance(b, tuple):
        return tuple(to_double(v) for v in b)
    return b


def run_eval(c, double=False):
    model = build(c, double).eval()
    b = CC.batch(c)
    with torch.no_grad():
        r, u, cv = model(to_double(b) if double else b, return_embeddings=True)
    return dict(r=r, u=u, c=cv)


def run_grad(c, double=False):
    model = CC.fix_dropouts(build(c, double), c)
    b = CC.batch(c)
    if double:
        b = to_double(b)
    h, _ = b["user_features"]["history"]["title_emb"]
    cx, _ = b["candidate_features"]["title_emb"]
    h.requires_grad_(True)
    cx.requires_grad_(True)
    preds = torch.relu(model(b))
    loss = torch.nn.functional.mse_loss(preds, b["targets"])
    loss.backward()
    out = {"loss": loss, "preds": preds}
    grads = {"in/hist": h.grad, "in/cand": cx.grad}
    grads.update({f"dW/{k}": p.grad for k, p in model.named_parameters()})
    out.update({k: v for k, v in grads.items() if v is not None})
    return out, [k for k, v in grads.items() if v is None]


def rel(a, b, floor_scale=0.0):
    return float((a.double() - b.double()).abs().max() / max(float(b.double().abs().max()), floor_scale, 1e-30))


def case(name, c):
    ev, (gr, no_grad) = run_eval(c), run_grad(c)
    ev64, (gr64, _) = run_eval(c, True), run_grad(c, True)
    assert all(torch.isfinite(v).all() for v in ev.values()), name
    arrays = {}
    for k, v in ev.items():
        arrays[f"{name}/eval/{k}"] = CC.sample(v)
        arrays[f"{name}/eval/max/{k}"] = npy(v.abs().max())
    for k, v in gr.items():
        arrays[f"{name}/grad/{k}"] = CC.sample(v) if k.startswith(("dW/", "in/")) else npy(v)
        if k.startswith(("dW/", "in/")):
            arrays[f"{name}/grad/max/{k}"] = npy(v.abs().max())
    # every gradient against max(its own scale, 1e-3 of the largest parameter gradient), as tests/helpers.py scales them:
    # an analytically zero gradient (a bias in front of a softmax) is rounding noise in both precisions
    gmax = max(float(v.abs().max()) for k, v in gr64.items() if k.startswith("dW/"))
    floor = dict(scores=max(rel(ev[k], ev64[k]) for k in ev),
                 grads=max(rel(gr[k], gr64[k], 1e-3 * gmax) for k in gr if k.startswith(("dW/", "in/"))))
    assert floor["scores"] <= TOL_S / 4 and floor["grads"] <= TOL_G / 4, (name, floor)
    return arrays, no_grad, floor


def contract():
    import yaml
    full = yaml.safe_load(open(f"{REF}/config/{CC.INIT['config']}.yml"))
    cfg = Cfg(dict(full, **CC.INIT["extra"]))
    torch.manual_seed(CC.INIT["seed"])
    model = make_model(cfg)
    sd = model.state_dict()
    keys = ("model", "scoring", "n_heads", "title_emb_dim", "total_emb_dim", "cat_emb_dim", "d_backbone", "p_dropout", "bias",
            "hist_len", "seq_len", "n_categories", "n_subcategories", "catg_features", "text_features", "user_features",
            "add_features")
    meta = dict(keys=list(sd), shapes=[list(v.shape) for v in sd.values()], cfg={k: cfg[k] for k in keys},
                n_params=sum(p.numel() for p in model.parameters()), n_param_tensors=len(list(model.parameters())),
                scorer=type(model.rec_model).__name__)
    arrays = {f"init/{k}": CC.sample(v) for k, v in sd.items()}
    arrays.update({f"init_sum/{k}": np.float64(v.double().sum().item()) for k, v in sd.items()})
    return meta, arrays


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    arrays, no_grad, floors = {}, {}, {}
    for name, c in CC.CASES.items():
        a, ng, fl = case(name, c)
        arrays.update(a)
        no_grad[name], floors[name] = ng, fl
        print(name, fl, ng)
    meta, init = contract()
    arrays.update(init)
    np.savez_compressed(os.path.join(HERE, "caum.npz"), **arrays)
    with open(os.path.join(HERE, "caum.json"), "w") as f:
        json.dump(dict(contract=meta, init_case=CC.INIT, cases=CC.CASES, no_grad=no_grad, fp32_vs_fp64=floors,
                       sample=dict(min=CC.SAMPLE_MIN, n=CC.SAMPLE_N), torch=torch.__version__), f, indent=1, sort_keys=True)
    print("caum.npz", len(arrays), "arrays", sum(np.asarray(v).nbytes for v in arrays.values()), "bytes")


if __name__ == "__main__":
    main()
