#!/usr/bin/env python
"""bench_calibration.py -- calibrated re-ranking and its measures (ops.calibrated_rerank / list_calibration /
csr_category_counts: xnrs_calibrated_rerank, xnrs_list_calibration, xnrs_csr_category_counts) and
evaluation.recommend_calibrated, one JSON file.

    python tools/bench_calibration.py --out profiles/calibration_bench.json

Shape: B = 4096 sessions x n_rows = 65536 news; pool P in {128, 256, 1024}, k in {10, 100}, n_cat in {18, 285} (MIND's categories
and subcategories); lam = 0.5, alpha = 0.01, rel minmax.  The pools are random rows with scores in descending order, every
place valid and categorised; the targets are the category counts of random histories of 5 to 50 news.  Per (P, k, n_cat):
  calibrated      : xnrs_calibrated_rerank alone
  calibrated_again: the same measurement repeated unchanged: the spread of the method
  torch_composed  : the same greedy from torch operators on the same device: per step a batched (B, n_cat) penalty in the
                    incremental form, a gather to the places and an argmax; alternated call by call with calibrated.
                    picks_equal: the share of (session, step) places where both picked the same place (fp32 sums in another
                    order may break a near-tie the other way; from there on the two lists part)
  list_calibration: xnrs_list_calibration over the (B, k) lists the kernel returned
and once per n_cat  csr_category_counts: xnrs_csr_category_counts over the histories.
Through the public API on a synth.click_world of the same size with an NRMS of E = 256, alternated call by call:
  recommend / recommend_pool / recommend_calibrated : evaluation.recommend(k), recommend(pool), recommend_calibrated(k, lam, pool)
and a QUALITY table on the world and the model of examples/train_synthetic.py (2000 news, 4000 sessions, NRMS E = 64, 300
steps): evaluate_calibration for lam in (None, 0.9, 0.7, 0.5, 0) against the sessions' histories, k = 10, pool 128, 18
categories (each of the world's 6 topics split at random into 3); lam = 0 is what the pool can reach at all.
Every shape is warmed up; each call lies between two device events and ends in a synchronise; a window is the calls of one
route until they add up to --window seconds (at least two calls); figures are medians over the window's calls with the
minimum beside them.  No ratio is a condition: the file states what was measured.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_diversity import Cfg, windows  # noqa: E402

B, N_ROWS = 4096, 65536
POOLS, KS, CATS, LAM, ALPHA = (128, 256, 1024), (10, 100), (18, 285), 0.5, 0.01


def torch_calibrated(pool_cat, scores, p, k, lam, alpha):
    """The greedy (minmax relevance, every place valid and categorised) from torch operators -> the picked places (B, k)."""
    lo, hi = scores.min(dim=1, keepdim=True).values, scores.max(dim=1, keepdim=True).values
    lr = lam * (scores - lo) / (hi - lo)
    at = torch.arange(scores.shape[0], device=scores.device)
    dead = torch.zeros_like(scores, dtype=torch.bool)
    counts = torch.zeros_like(p)
    zero = torch.zeros((), device=p.device)
    floor = alpha * p
    term = lambda n, N: torch.where(p > 0, p * torch.log(p / ((1.0 - alpha) * n / N + floor)), zero)  # noqa: E731
    picks = []
    for t in range(k):
        now = term(counts, t + 1.0)
        pen = (now.sum(dim=1, keepdim=True) - now) + term(counts + 1.0, t + 1.0)
        i = (lr - (1.0 - lam) * pen.gather(1, pool_cat)).masked_fill(dead, float("-inf")).argmax(dim=1)
        picks.append(i)
        dead[at, i] = True
        counts[at, pool_cat[at, i]] += 1.0
    return torch.stack(picks, dim=1)


def quality(dev, steps=300):
    """The lam sweep on the trained model of examples/train_synthetic.py (its default route: sampled negatives)."""
    from xnrs_amd import evaluation as EV
    from xnrs_amd.losses import contrastive_loss
    from xnrs_amd import synth
    from xnrs_amd.data import DeviceBatcher
    from xnrs_amd.models import make_model
    n_news, n_topics, hist, k, pool = 2000, 6, 8, 10, 128
    torch.manual_seed(0)
    store, beh = synth.click_world(n_news=n_news, n_sess=4000, S=12, D=64, n_topics=n_topics)
    rng = np.random.default_rng(0)  # (click_world's own first draws: the topic directions, then the topic of every news)
    rng.standard_normal((n_topics, 64))
    topic = rng.integers(0, n_topics, size=n_news)
    cat = np.concatenate(([-1], topic * 3 + np.random.default_rng(1).integers(0, 3, size=n_news))).astype(np.int32)  # row 0: the pad row
    store, beh, cat = store.to(dev), beh.to(dev), torch.from_numpy(cat).to(dev)
    model = make_model(Cfg(synth.model_cfg(dict(model="NRMS", E=64, bias=True, h=4, D=64, H=hist, S=12)))).to(dev)
    model.news_encoder.skip_empty = True
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    batcher = DeviceBatcher(beh, l_hist=hist)
    model.train()
    for step in range(steps):
        sess = torch.randint(0, len(beh), (64,), device=dev)
        opt.zero_grad()
        h, c, targets = batcher.train_batch(sess, n_neg=4, seed=step)
        r, u, _ = model.forward_ids(store.x, store.m, h, c, return_embeddings=True)
        loss = torch.nn.functional.mse_loss(torch.relu(r), targets) + 0.1 * contrastive_loss(u.squeeze(1), beh.theme_labels[sess], 0.08)
        loss.backward()
        opt.step()
    model.eval()
    out = dict(world="synth.click_world(n_news=2000, n_sess=4000, S=12, D=64, n_topics=6)", model=f"NRMS E=64 h=4, {steps} steps",
               auc=EV.evaluate(model, store, beh, hist, batch=1024)["auc"], k=k, pool=pool, n_categories=18, target="history",
               alpha=ALPHA, rows={})
    # the share of the sessions whose pool holds a news of ANY category of their history: no re-ranking helps the others
    from xnrs_amd import ops
    prow, _ = EV.recommend(model, store, beh, hist, pool)
    tgt = ops.csr_category_counts(beh.hist_off, beh.hist_val, cat, 18, store.pad_row)
    pcat = cat[prow.clamp(min=0).long()].clamp(min=0).long()
    out["sessions_with_a_target_category_in_the_pool"] = float(((tgt.gather(1, pcat) > 0) & (prow >= 0)).any(dim=1).double().mean())
    for lam in (None, 0.9, 0.7, 0.5, 0.0):  # (0: the mix alone -- what this pool can reach at all)
        out["rows"][str(lam)] = EV.evaluate_calibration(model, store, beh, hist, k, lam=lam, row_category=cat, n_categories=18,
                                                        alpha=ALPHA, pool=None if lam is None else pool)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed calls per route and shape (at least 0.5)")
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-api", action="store_true", help="kernels only: no click world, no model")
    a = ap.parse_args()
    if a.window < 0.5:
        raise SystemExit("windows of at least half a second")
    from xnrs_amd import evaluation as EV
    from xnrs_amd import ops, synth
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    res = dict(device=torch.cuda.get_device_name(0), window_s=a.window, B=B, n_rows=N_ROWS, lam=LAM, alpha=ALPHA, rel="minmax", cases={},
               csr_category_counts={})
    lens = torch.randint(5, 51, (B,), generator=gen, device=dev)
    off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=off[1:])
    hist_rows = torch.randint(0, N_ROWS, (int(off[-1]),), generator=gen, device=dev, dtype=torch.int32)
    for C in CATS:
        cat = torch.randint(0, C, (N_ROWS,), generator=gen, device=dev, dtype=torch.int32)
        counts_fn = lambda: ops.csr_category_counts(off, hist_rows, cat, C)  # noqa: E731
        res["csr_category_counts"][f"C{C}"] = dict(windows({"c": counts_fn}, a.window)["c"], history_rows=int(off[-1]))
        target = counts_fn().float()
        p = target / target.sum(dim=1, keepdim=True)
        for P in POOLS:
            pool_rows = torch.randint(0, N_ROWS, (B, P), generator=gen, device=dev, dtype=torch.int32)
            pool_scores = torch.randn((B, P), generator=gen, device=dev).sort(dim=1, descending=True).values.contiguous()
            pool_cat = cat[pool_rows.long()].long()
            for k in KS:
                hip_fn = lambda: ops.calibrated_rerank(pool_rows, pool_scores, k, LAM, cat, C, target, ALPHA, "minmax")  # noqa: E731
                torch_fn = lambda: torch_calibrated(pool_cat, pool_scores, p, k, LAM, ALPHA)  # noqa: E731
                row = dict(P=P, k=k, n_cat=C)
                row.update(windows({"calibrated": hip_fn, "torch_composed": torch_fn}, a.window))
                row["calibrated_again"] = windows({"c": hip_fn}, a.window)["c"]
                row["calibrated_spread"] = abs(row["calibrated_again"]["median_ms"] - row["calibrated"]["median_ms"]) / row["calibrated"]["median_ms"]
                row["calibrated_over_torch_composed"] = row["calibrated"]["median_ms"] / row["torch_composed"]["median_ms"]
                lists, _, pos, kl = hip_fn()
                row["picks_equal"] = float((pos.long() == torch_fn()).float().mean())
                row["mean_kl"] = float(kl.double().mean())
                row["mean_kl_of_the_pool_head"] = float(ops.list_calibration(pool_rows[:, :k].contiguous(), cat, C, target, ALPHA)[0].double().mean())
                row["list_calibration"] = windows({"l": lambda: ops.list_calibration(lists, cat, C, target, ALPHA)}, a.window)["l"]
                res["cases"][f"C{C}_P{P}_k{k}"] = row
                print(json.dumps({f"C{C}_P{P}_k{k}": row}, sort_keys=True), flush=True)
    if not a.skip_api:
        from xnrs_amd.models import make_model
        store, beh = synth.click_world(n_news=N_ROWS - 1, n_sess=B, S=10, D=64, n_topics=16)
        store, beh = store.to(dev), beh.to(dev)
        torch.manual_seed(11)
        model = make_model(Cfg(synth.model_cfg(dict(model="NRMS", E=256, bias=True, h=4, D=64, H=8, S=10)))).to(dev).eval()
        cat = torch.randint(0, 18, (store.n_rows,), generator=gen, device=dev, dtype=torch.int32)
        res["api"] = dict(world="synth.click_world(n_news=65535, n_sess=4096, S=10, D=64, n_topics=16)", model="NRMS E=256 h=4",
                          l_hist=8, n_categories=18, target="history", cases={})
        for P in POOLS:
            for k in KS:
                got = windows({"recommend": lambda: EV.recommend(model, store, beh, 8, k),
                               "recommend_pool": lambda: EV.recommend(model, store, beh, 8, P),
                               "recommend_calibrated": lambda: EV.recommend_calibrated(model, store, beh, 8, k, LAM, cat, 18, pool=P)},
                              a.window, warmup=1)
                got["calibrated_over_recommend"] = got["recommend_calibrated"]["median_ms"] / got["recommend"]["median_ms"]
                got["calibrated_over_recommend_pool"] = got["recommend_calibrated"]["median_ms"] / got["recommend_pool"]["median_ms"]
                res["api"]["cases"][f"P{P}_k{k}"] = got
                print(json.dumps({f"api_P{P}_k{k}": got}, sort_keys=True), flush=True)
        res["quality"] = quality(dev)
        print(json.dumps({"quality": res["quality"]}, sort_keys=True), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
