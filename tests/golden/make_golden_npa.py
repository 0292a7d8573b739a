#!/usr/bin/env python
"""Generate tests/golden/npa.{json,npz} from the REAL reference: its NPA (xnrs/models/full_models/npa.py:8-95) built by its
make_model, in eval mode (scores, user vectors, candidate vectors) and in the MSE grad step (training.py:97-113,376-393:
relu(model(batch)), mse_loss, backward), for the dot / bilin / fc scorers; and the state_dict contract of
config/mind_small_NPA.yml at a small n_users.

Imports the reference exactly as make_golden_scorers.py does.  Stores outputs only: inputs and weights regenerate from the
seeds of tests/golden/npa_cases.py.  Runs only where the reference is present; the GPU machine never needs it.

    python tests/golden/make_golden_npa.py            # rewrites tests/golden/npa.json and npa.npz
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
from tests.golden import npa_cases as NC  # noqa: E402


class Cfg(dict):
    __getattr__ = dict.__getitem__


def npy(t):
    return t.detach().cpu().numpy()


def build(c, scoring):
    model = make_model(Cfg(NC.model_cfg(c, scoring)))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(synth.fill_state_dict(shapes, NC.weight_seed(c)))
    return model


def eval_case(name, c, scoring):
    """r, and the u / c the scorer saw (hooks on user_encoder and on news_head's second call: the candidates)."""
    model = build(c, scoring).eval()
    seen = {}
    model.user_encoder.register_forward_hook(lambda m, i, o: seen.__setitem__("u", o))
    heads = []
    model.news_head.register_forward_hook(lambda m, i, o: heads.append(o))
    with torch.no_grad():
        r = model(NC.batch(c))
    pre = f"{name}/{scoring}/eval"
    return {f"{pre}/r": npy(r), f"{pre}/u": npy(seen["u"]).reshape(c["B"], -1), f"{pre}/c": npy(heads[1]).reshape(c["B"], c["C"], -1)}


def grad_case(name, c, scoring):
    model = build(c, scoring).train()
    b = NC.batch(c)
    h, hm = b["user_features"]["history"]["title_emb"]
    cx, cm = b["candidate_features"]["title_emb"]
    h.requires_grad_(True)
    cx.requires_grad_(True)
    preds = torch.relu(model(b))
    loss = torch.nn.functional.mse_loss(preds, b["targets"])
    loss.backward()
    pre = f"{name}/{scoring}/grad"
    out = {f"{pre}/loss": npy(loss), f"{pre}/preds": npy(preds), f"{pre}/in/hist": NC.sample(h.grad),
           f"{pre}/in/cand": NC.sample(cx.grad), f"{pre}/max/in/hist": npy(h.grad.abs().max()),
           f"{pre}/max/in/cand": npy(cx.grad.abs().max())}
    for k, p in model.named_parameters():
        out[f"{pre}/dW/{k}"] = NC.sample(p.grad)
        out[f"{pre}/max/{k}"] = npy(p.grad.abs().max())
    return out


def contract():
    import yaml
    full = yaml.safe_load(open(f"{REF}/config/{NC.INIT['config']}.yml"))
    cfg = Cfg(dict(full, n_users=NC.INIT["n_users"]))
    torch.manual_seed(NC.INIT["seed"])
    model = make_model(cfg)
    sd = model.state_dict()
    meta = dict(keys=list(sd), shapes=[list(v.shape) for v in sd.values()],
                cfg={k: cfg[k] for k in ("model", "scoring", "user_emb_dim", "title_emb_dim", "total_emb_dim", "d_backbone",
                                         "p_dropout", "bias")})
    arrays = {f"init/{k}": NC.sample(v) for k, v in sd.items()}
    arrays.update({f"init_sum/{k}": np.float64(v.double().sum().item()) for k, v in sd.items()})
    return meta, arrays


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    arrays = {}
    for name, c in NC.CASES.items():
        for scoring in NC.SCORERS:
            arrays.update(eval_case(name, c, scoring))
            arrays.update(grad_case(name, c, scoring))
    meta, init = contract()
    arrays.update(init)
    np.savez_compressed(os.path.join(HERE, "npa.npz"), **arrays)
    with open(os.path.join(HERE, "npa.json"), "w") as f:
        json.dump(dict(contract=meta, init_case=NC.INIT, cases=NC.CASES, scorers=list(NC.SCORERS),
                       sample=dict(min=NC.SAMPLE_MIN, n=NC.SAMPLE_N), torch=torch.__version__), f, indent=1, sort_keys=True)
    print("npa.npz", len(arrays), "arrays", sum(np.asarray(v).nbytes for v in arrays.values()), "bytes")


if __name__ == "__main__":
    main()
