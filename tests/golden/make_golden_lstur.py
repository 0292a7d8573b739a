#!/usr/bin/env python
"""Generate tests/golden/lstur_model.{json,npz} from the REAL reference: its LSTUR (xnrs/models/full_models/lstur.py:9-159)
built by its make_model, in eval mode (scores, user vectors, candidate vectors) and in the MSE grad step
(training.py:97-113,376-393: relu(model(batch)), mse_loss, backward) for the cases of tests/golden/lstur_cases.py; the
state_dict contract of config/mind_small_LSTUR.yml at a small n_users; and, per case, the distance between the reference in
fp32 and the same reference in fp64 (the floor any fp32 implementation of 25 chained steps lives on).

Imports the reference exactly as make_golden_npa.py does.  Stores outputs only: inputs and weights regenerate from the
seeds of lstur_cases.py.  Runs only where the reference is present; the GPU machine never needs it.

    python tests/golden/make_golden_lstur.py            # rewrites tests/golden/lstur_model.json and lstur_model.npz
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
from tests.golden import lstur_cases as LC  # noqa: E402


class Cfg(dict):
    __getattr__ = dict.__getitem__


def npy(t):
    return t.detach().cpu().numpy()


def build(c, double=False):
    model = make_model(Cfg(LC.model_cfg(c)))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(synth.fill_state_dict(shapes, LC.weight_seed(c)))
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
    b = LC.batch(c)
    with torch.no_grad():
        r, u, cv = model(to_double(b) if double else b, return_embeddings=True)
    return dict(r=r, u=u.reshape(c["B"], -1), c=cv)


def run_grad(c, double=False):
    model = build(c, double).train()
    b = LC.batch(c)
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
    return out, [k for k, v in grads.items() if v is None]  # (lt_only: the GRU, and with the user table the history too)


def rel(a, b, floor_scale=0.0):
    return float((a.double() - b.double()).abs().max() / max(float(b.double().abs().max()), floor_scale, 1e-30))


def case(name, c):
    ev, (gr, no_grad) = run_eval(c), run_grad(c)
    ev64, (gr64, _) = run_eval(c, True), run_grad(c, True)
    arrays = {f"{name}/eval/{k}": npy(v) for k, v in ev.items()}
    for k, v in gr.items():
        arrays[f"{name}/grad/{k}"] = LC.sample(v) if k.startswith(("dW/", "in/")) else npy(v)
        if k.startswith(("dW/", "in/")):
            arrays[f"{name}/grad/max/{k}"] = npy(v.abs().max())
    # every gradient against max(its own scale, 1e-3 of the largest parameter gradient), as tests/helpers.py scales them:
    # an analytically zero gradient (a bias in front of a softmax) is rounding noise in both precisions
    gmax = max(float(v.abs().max()) for k, v in gr64.items() if k.startswith("dW/"))
    floor = dict(scores=max(rel(ev[k], ev64[k]) for k in ev),
                 grads=max(rel(gr[k], gr64[k], 1e-3 * gmax) for k in gr if k.startswith(("dW/", "in/"))))
    return arrays, no_grad, floor


def contract():
    import yaml
    full = yaml.safe_load(open(f"{REF}/config/{LC.INIT['config']}.yml"))
    cfg = Cfg(dict(full, n_users=LC.INIT["n_users"]))
    torch.manual_seed(LC.INIT["seed"])
    model = make_model(cfg)
    sd = model.state_dict()
    keys = ("model", "base_model", "scoring", "long_term_method", "long_short_term_method", "p_user_dropout", "title_emb_dim",
            "total_emb_dim", "cat_emb_dim", "d_backbone", "p_dropout", "bias", "hist_len", "st_hist_len", "seq_len",
            "n_categories", "n_subcategories", "catg_features", "text_features", "user_features", "add_features")
    meta = dict(keys=list(sd), shapes=[list(v.shape) for v in sd.values()], cfg={k: cfg[k] for k in keys},
                n_params=sum(p.numel() for p in model.parameters()))
    arrays = {f"init/{k}": LC.sample(v) for k, v in sd.items()}
    arrays.update({f"init_sum/{k}": np.float64(v.double().sum().item()) for k, v in sd.items()})
    return meta, arrays


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    arrays, no_grad, floors = {}, {}, {}
    for name, c in LC.CASES.items():
        a, ng, fl = case(name, c)
        arrays.update(a)
        no_grad[name], floors[name] = ng, fl
        print(name, fl)
    meta, init = contract()
    arrays.update(init)
    np.savez_compressed(os.path.join(HERE, "lstur_model.npz"), **arrays)
    with open(os.path.join(HERE, "lstur_model.json"), "w") as f:
        json.dump(dict(contract=meta, init_case=LC.INIT, cases=LC.CASES, no_grad=no_grad, fp32_vs_fp64=floors,
                       sample=dict(min=LC.SAMPLE_MIN, n=LC.SAMPLE_N), torch=torch.__version__), f, indent=1, sort_keys=True)
    print("lstur_model.npz", len(arrays), "arrays", sum(np.asarray(v).nbytes for v in arrays.values()), "bytes")


if __name__ == "__main__":
    main()
