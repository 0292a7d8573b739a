#!/usr/bin/env python
"""sampled_exposure_table.py -- what one temperature trades: accuracy against exposure, on the synthetic click world of
examples/train_synthetic.py (2000 news, 4000 sessions, 6 topics; NRMS trained for --steps steps of 64 impressions with the
example's default loss).  One JSON file and the table of DESIGN.md section 10m.

    python tools/sampled_exposure_table.py [--steps 300] --out profiles/sampled_exposure.json

Per policy -- recommend(k = 10) and recommend_sampled(k = 10) at temperature 0.05, 0.2 and 1 (seed 1) -- over all sessions:
hit@10 and ndcg@10 of the clicked news within the list (evaluation._list_accuracy_sums, the definitions of evaluate_diversity)
and catalog_coverage@10, gini@10 and ild@10 of evaluation.diversity_metrics.  Needs an MI355X."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xnrs_amd import evaluation as EV  # noqa: E402
from xnrs_amd import synth  # noqa: E402
from xnrs_amd.data import DeviceBatcher  # noqa: E402
from xnrs_amd.losses import contrastive_loss  # noqa: E402
from xnrs_amd.models import make_model  # noqa: E402

K, HIST, TEMPERATURES, SEED = 10, 8, (0.05, 0.2, 1.0), 1


class Cfg(dict):
    __getattr__ = dict.__getitem__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    store, beh = synth.click_world(n_news=2000, n_sess=4000, S=12, D=64, n_topics=6)
    store, beh = store.to(dev), beh.to(dev)
    model = make_model(Cfg(synth.model_cfg(dict(model="NRMS", E=64, bias=True, h=4, D=64, H=HIST, S=12)))).to(dev)
    model.news_encoder.skip_empty = True
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    batcher = DeviceBatcher(beh, l_hist=HIST)
    model.train()
    for step in range(a.steps):  # the default loss of examples/train_synthetic.py
        sess = torch.randint(0, len(beh), (64,), device=dev)
        opt.zero_grad()
        hist, cand, targets = batcher.train_batch(sess, n_neg=4, seed=step)
        r, u, _ = model.forward_ids(store.x, store.m, hist, cand, return_embeddings=True)
        loss = torch.nn.functional.mse_loss(torch.relu(r), targets) + 0.1 * contrastive_loss(u.squeeze(1), beh.theme_labels[sess], 0.08)
        loss.backward()
        opt.step()
    model.eval()
    vecs = EV.encode_news_table(model, store)[0]
    sess = torch.arange(len(beh), device=dev)
    policies = [("recommend", lambda: EV.recommend(model, store, beh, HIST, K)[0])]
    policies += [(f"sampled, temperature {t}", lambda t=t: EV.recommend_sampled(model, store, beh, HIST, K, t, SEED)[0]) for t in TEMPERATURES]
    out = dict(device=torch.cuda.get_device_name(0), steps=a.steps, k=K, seed=SEED, n_news=2000, n_sessions=len(beh), policies={})
    print(f"| policy | hit@{K} | ndcg@{K} | coverage@{K} | gini@{K} | ild@{K} |\n|---|---|---|---|---|---|")
    for name, lists in policies:
        rows = lists()
        m = EV.diversity_metrics(vecs, rows, store.n_rows, store.pad_row)
        m.update(EV._list_accuracy_dict(EV._list_accuracy_sums(beh, sess, rows, store.n_rows, int(store.pad_row)), K))
        out["policies"][name] = m
        print(f"| {name} | {m[f'hit@{K}']:.4f} | {m[f'ndcg@{K}']:.4f} | {m[f'catalog_coverage@{K}']:.4f} | {m[f'gini@{K}']:.4f} | "
              f"{m[f'ild@{K}']:.4f} |")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
