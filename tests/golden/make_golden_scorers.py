#!/usr/bin/env python
"""Generate tests/golden/scorers.{json,npz} from the REAL reference: its BilinScoring / FCScoring
(xnrs/models/components/scoring.py:41-102), alone and inside the train step, and its make_model's state_dict contract
for the shipped configs with scoring 'bilin' / 'fc'.

Imports the reference exactly as make_golden.py does (sys.modules stand-ins for the two package __init__ files and for
the two absent third-party packages of xnrs/training.py).  Stores outputs only: inputs and weights regenerate from the
seeds of tests/golden/scorer_cases.py.  Runs only where the reference is present; the GPU machine never needs it.

    python tests/golden/make_golden_scorers.py            # rewrites tests/golden/scorers.json and scorers.npz
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

from xnrs.models.components import scoring  # noqa: E402
from xnrs.models.make_model import make_model  # noqa: E402
from xnrs.training import ContrastiveRankingTrainer  # noqa: E402

from xnrs_amd import synth  # noqa: E402
from tests.golden import cases, scorer_cases as SC  # noqa: E402


class Cfg(dict):
    __getattr__ = dict.__getitem__


def npy(t):
    return t.detach().cpu().numpy()


def reference_infonce(emb, labels, temperature):
    holder = types.SimpleNamespace(temperature=temperature)
    return ContrastiveRankingTrainer._compute_contrastive_loss(holder, emb, labels)


def load(module, seed):
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    module.load_state_dict(synth.fill_state_dict(shapes, seed))
    module.eval()
    return module


def reference_scorer(c):
    if c["kind"] == "bilin":
        return scoring.BilinScoring(c["E"], normalize=c["normalize"], bias=c["bias"])
    return scoring.FCScoring(c["E"], hidden_dim=c["H"], bias=c["bias"])


def scorer_cases():
    out = {}
    for name, c in SC.SCORER.items():
        mod = load(reference_scorer(c), c["seed"] + 1)
        u, cv, g = SC.scorer_inputs(c)
        u.requires_grad_(True)
        cv.requires_grad_(True)
        s = mod(u, cv)
        s.backward(g)
        out[f"{name}/s"], out[f"{name}/du"], out[f"{name}/dc"] = npy(s), npy(u.grad), npy(cv.grad)
        for k, p in mod.named_parameters():
            out[f"{name}/d/{k}"] = npy(p.grad)
    return out


def step_cases():
    out = {}
    for name, c in SC.STEP.items():
        for scorer in SC.STEP_SCORERS:
            pre = f"{name}/{scorer}"
            model = load(make_model(Cfg(SC.step_cfg(c, scorer))), c["seed"] + 1)
            batch = cases.model_batch(c)
            labels = SC.step_labels(c["B"])
            preds = torch.relu(model(batch))
            loss_rec = torch.nn.functional.mse_loss(preds, batch["targets"])
            ue = model.get_user_embeddings(batch).reshape(c["B"], -1)
            loss_cl = reference_infonce(ue, labels, c["temperature"])
            loss = loss_rec + c["lambda_cl"] * loss_cl
            loss.backward()
            out[f"{pre}/loss"], out[f"{pre}/loss_rec"], out[f"{pre}/loss_cl"] = npy(loss), npy(loss_rec), npy(loss_cl)
            out[f"{pre}/preds"] = npy(preds)
            for k, p in model.named_parameters():
                if p.grad is not None:
                    out[f"{pre}/dW/{k}"] = SC.sample(p.grad)
                    out[f"{pre}/max/{k}"] = npy(p.grad.abs().max())
    return out


def contract():
    """make_model on the shipped YAMLs with scoring 'bilin' / 'fc': state_dict keys in order, shapes, parameter count."""
    import yaml
    out = {}
    for name in ("mind_small_NRMS", "mind_small_CL", "mind_small_NAML"):
        full = yaml.safe_load(open(f"{REF}/config/{name}.yml"))
        for scorer in SC.STEP_SCORERS:
            model = make_model(Cfg(dict(full, scoring=scorer)))
            sd = model.state_dict()
            out[f"{name}/{scorer}"] = dict(cfg={k: full[k] for k in ("model", "total_emb_dim", "title_emb_dim", "bias")},
                                           keys=list(sd), shapes=[list(v.shape) for v in sd.values()],
                                           n_params=int(sum(p.numel() for p in model.parameters())))
    return out


def init_params():
    """The scorer's parameters right after construction under torch.manual_seed(seed) (nn.Bilinear / nn.Linear init)."""
    E, seed = SC.INIT["E"], SC.INIT["seed"]
    out = {}
    for label, make in [("bilin_bias", lambda: scoring.BilinScoring(E, bias=True)),
                        ("bilin_nobias", lambda: scoring.BilinScoring(E, bias=False)),
                        ("fc_bias", lambda: scoring.FCScoring(E, hidden_dim=E // 2, bias=True)),
                        ("fc_nobias", lambda: scoring.FCScoring(E, hidden_dim=E // 2, bias=False))]:
        torch.manual_seed(seed)
        mod = make()
        out[label] = {k: v.reshape(-1).tolist() for k, v in mod.state_dict().items()}
    return out


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    arrays = dict(scorer_cases(), **step_cases())
    np.savez_compressed(os.path.join(HERE, "scorers.npz"), **arrays)
    meta = dict(contract=contract(), init=init_params(), init_case=SC.INIT, scorer_cases=SC.SCORER, step_cases=SC.STEP,
                sample=dict(min=SC.SAMPLE_MIN, n=SC.SAMPLE_N), torch=torch.__version__)
    with open(os.path.join(HERE, "scorers.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("scorers.npz", len(arrays), "arrays", sum(v.nbytes for v in arrays.values()), "bytes")


if __name__ == "__main__":
    main()
