#!/usr/bin/env python
"""bench_diversity.py -- MMR re-ranking and list diversity (ops.mmr_rerank / ops.list_diversity: xnrs_mmr_rerank,
xnrs_list_diversity) and evaluation.recommend_diverse, one JSON file.

    python tools/bench_diversity.py --out profiles/diversity_bench.json

Shape: B = 4096 sessions x n_rows = 65536 news x E = 256; pool P in {128, 256, 1024}, k in {10, 100}; lam = 0.5, rel minmax; the
pools are mined by ops.topk_deep_dot over a random table.  Per (P, k):
  mmr             : xnrs_mmr_rerank alone, and the bytes k * P * E * 4 * B over its time -- an ALGORITHMIC UPPER BOUND on the
                    traffic of the streaming kernel (every step re-reads the pool's rows; a pool that stays in L2 / Infinity
                    Cache never comes from HBM again), not a bandwidth utilisation
  mmr_again       : the same measurement repeated unchanged: the spread of the method
  torch_composed  : the same selection from torch operators on the same device: gather the pool to (B, P, E) in session
                    chunks, normalise, a bmm Gram matrix, k greedy steps of elementwise ops and argmax; alternated call by
                    call with mmr.  picks_equal: the share of (session, step) places where both picked the same place (fp32
                    sums in another order may break a near-tie the other way; from there on the two lists part)
  list_diversity  : xnrs_list_diversity over the (B, k) lists MMR returned
  topk_deep       : ops.topk_deep_dot(pool) alone; mmr_share = mmr / (topk_deep + mmr): the share of re-ranking in the step
and through the public API on a synth.click_world of the same size with an NRMS of E = 256, alternated call by call:
  recommend       : evaluation.recommend(k)
  recommend_pool  : evaluation.recommend(pool): encoding and mining alone
  recommend_diverse : evaluation.recommend_diverse(k, lam, pool)
Every shape is warmed up; each call lies between two device events and ends in a synchronise; a window is the calls of one
route until they add up to --window seconds (at least two calls); figures are medians over the window's calls with the
minimum beside them.  No ratio is a condition: the file states what was measured.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, N_ROWS, E = 4096, 65536, 256
POOLS, KS, LAM = (128, 256, 1024), (10, 100), 0.5


def one_call_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def windows(fns, window_s, warmup=2):
    """{name: stats} of the routes `fns` = {name: callable}, alternated call by call until every route has run window_s."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    while any(sum(v) < window_s * 1e3 or len(v) < 2 for v in ms.values()):
        for name, fn in fns.items():
            if sum(ms[name]) < window_s * 1e3 or len(ms[name]) < 2:
                ms[name].append(one_call_ms(fn))
    return {name: dict(median_ms=statistics.median(v), min_ms=min(v), calls=len(v), window_s=sum(v) / 1e3) for name, v in ms.items()}


def torch_mmr(table, rows, scores, k, lam, chunk=512):
    """Greedy MMR (minmax relevance, every place valid) from torch operators -> the picked places (B, k) int64."""
    out = []
    for c0 in range(0, rows.shape[0], chunk):
        r, s = rows[c0:c0 + chunk].long(), scores[c0:c0 + chunk]
        x = table[r]
        x = x / x.norm(dim=2, keepdim=True)
        gram = torch.bmm(x, x.transpose(1, 2))
        lo, hi = s.min(dim=1, keepdim=True).values, s.max(dim=1, keepdim=True).values
        lr = lam * (s - lo) / (hi - lo)
        at = torch.arange(r.shape[0], device=r.device)
        dead = torch.zeros_like(s, dtype=torch.bool)
        m = torch.zeros_like(s)
        picks = []
        for t in range(k):
            i = (lr - (1.0 - lam) * m).masked_fill(dead, float("-inf")).argmax(dim=1)
            picks.append(i)
            dead[at, i] = True
            col = gram[at, i]  # (the Gram matrix is symmetric: a row for a column)
            m = col if t == 0 else torch.maximum(m, col)
        out.append(torch.stack(picks, dim=1))
    return torch.cat(out)


class Cfg(dict):
    __getattr__ = dict.__getitem__


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
    table = torch.randn((N_ROWS, E), generator=gen, device=dev)
    u = torch.randn((B, E), generator=gen, device=dev) * (2.0 / E ** 0.5)
    inv = ops.row_inv_norms(table)
    res = dict(device=torch.cuda.get_device_name(0), window_s=a.window, B=B, n_rows=N_ROWS, E=E, lam=LAM, rel="minmax", cases={})
    res["row_inv_norms"] = windows({"row_inv_norms": lambda: ops.row_inv_norms(table)}, a.window)["row_inv_norms"]
    res["l2_normalize_rows"] = windows({"l2": lambda: ops.l2_normalize_rows(table)}, a.window)["l2"]
    for P in POOLS:
        pool_rows, pool_scores = ops.topk_deep_dot(table, u, P)
        mining = windows({"topk_deep": lambda: ops.topk_deep_dot(table, u, P)}, a.window)["topk_deep"]
        for k in KS:
            row = dict(P=P, k=k, topk_deep=mining)
            hip_fn = lambda: ops.mmr_rerank(table, inv, pool_rows, pool_scores, k, LAM, "minmax")  # noqa: E731
            got = windows({"mmr": hip_fn, "torch_composed": lambda: torch_mmr(table, pool_rows, pool_scores, k, LAM)}, a.window)
            row.update(got)
            row["mmr_again"] = windows({"mmr": hip_fn}, a.window)["mmr"]
            row["mmr_spread"] = abs(row["mmr_again"]["median_ms"] - row["mmr"]["median_ms"]) / row["mmr"]["median_ms"]
            bound = k * P * E * 4 * B
            row["mmr_bytes_upper_bound"] = bound
            row["mmr_upper_bound_bytes_per_s"] = bound / (row["mmr"]["median_ms"] / 1e3)
            row["mmr_over_torch_composed"] = row["mmr"]["median_ms"] / row["torch_composed"]["median_ms"]
            row["mmr_share"] = row["mmr"]["median_ms"] / (mining["median_ms"] + row["mmr"]["median_ms"])
            lists, _, pos = hip_fn()
            row["picks_equal"] = float((pos.long() == torch_mmr(table, pool_rows, pool_scores, k, LAM)).float().mean())
            row["list_diversity"] = windows({"d": lambda: ops.list_diversity(table, inv, lists)}, a.window)["d"]
            res["cases"][f"P{P}_k{k}"] = row
            print(json.dumps({f"P{P}_k{k}": row}, sort_keys=True), flush=True)
            torch.cuda.empty_cache()
    if not a.skip_api:
        from xnrs_amd.models import make_model
        store, beh = synth.click_world(n_news=N_ROWS - 1, n_sess=B, S=10, D=64, n_topics=16)
        store, beh = store.to(dev), beh.to(dev)
        torch.manual_seed(11)
        model = make_model(Cfg(synth.model_cfg(dict(model="NRMS", E=E, bias=True, h=4, D=64, H=8, S=10)))).to(dev).eval()
        res["api"] = dict(world="synth.click_world(n_news=65535, n_sess=4096, S=10, D=64, n_topics=16)", model="NRMS E=256 h=4",
                          l_hist=8, cases={})
        for P in POOLS:
            for k in KS:
                got = windows({"recommend": lambda: EV.recommend(model, store, beh, 8, k),
                               "recommend_pool": lambda: EV.recommend(model, store, beh, 8, P),
                               "recommend_diverse": lambda: EV.recommend_diverse(model, store, beh, 8, k, LAM, pool=P)}, a.window,
                              warmup=1)
                got["diverse_over_recommend"] = got["recommend_diverse"]["median_ms"] / got["recommend"]["median_ms"]
                got["diverse_over_recommend_pool"] = got["recommend_diverse"]["median_ms"] / got["recommend_pool"]["median_ms"]
                res["api"]["cases"][f"P{P}_k{k}"] = got
                print(json.dumps({f"api_P{P}_k{k}": got}, sort_keys=True), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
