#!/usr/bin/env python
"""bench_topk_window.py -- what a per-user row window costs and saves (xnrs_topk_deep_win / xnrs_rank_win), one JSON file.

    python tools/bench_topk_window.py [--reps R] [--warmup W] --out profiles/topk_window_bench.json

Shape (tools/bench_topk.py): 4096 users x 65536 news x E 256, the dot form; top-k at k = 10 / 100 / 256 and rank with one
click per user.  Routes, all in one process, alternating call by call, each call between two device events:
  parent, parent_again   the parent entry point (xnrs_topk_deep / xnrs_rank), twice: the difference of the two series is
                         part of the spread
  null                   the _win entry point with both window pointers NULL
  win_F_sorted           windows covering F = 100 / 25 / 5 % of the table, the sessions in time order within the batch (the
                         window's start grows with the user's position: every tile's union is narrow)
  win_F_shuffled         the same windows in random order (every tile's union is nearly the whole table)
  excl_csr_5             the route a caller had before: the 5 % windows (sorted) written as an exclusion CSR of every row
                         outside the window (about 62 000 ids per user), through the parent entry point.  It takes seconds
                         per call and leaves the caches cold, so it is timed in a loop of its own, `--slow-reps` calls,
                         before the others
The order of the routes rotates from call round to call round, so that no route always follows the same neighbour.  The
whole measurement runs `--passes` times (default 2); a route's figure is the median over the calls of a pass, and
`spread` = the largest relative difference among the parent's medians (two series x the passes).  `null` and `win_100_*` must
stay within it: `conditions` says which do, per workload; an excess is a regression to explain, not a number to hide.
Results are compared before anything is timed: null == parent, win_5_sorted == excl_csr_5, bit for bit.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_ROWS, E, B = 65536, 256, 4096
KS = (10, 100, 256)
FRACTIONS = (100, 25, 5)


def windows(frac, shuffled, dev, gen):
    width = N_ROWS * frac // 100
    lo = (torch.arange(B, device=dev, dtype=torch.float64) / (B - 1) * (N_ROWS - width)).to(torch.int32)
    if shuffled:
        lo = lo[torch.randperm(B, device=dev, generator=gen)]
    return lo.contiguous(), (lo + width).contiguous()


def outside_csr(lo, hi, dev):
    """every row outside [lo, hi) per user, all windows of one width: (off int64, rows int32)"""
    width = int(hi[0] - lo[0])
    n = N_ROWS - width
    r = torch.arange(n, device=dev, dtype=torch.int32)[None, :].expand(B, n)
    rows = (r + (r >= lo[:, None]).to(torch.int32) * width).reshape(-1).contiguous()
    return torch.arange(B + 1, device=dev, dtype=torch.int64) * n, rows


def build(dev):
    from xnrs_amd import hip, ops
    gen = torch.Generator(device=dev)
    gen.manual_seed(4096)
    table = torch.randn((N_ROWS, E), generator=gen, device=dev)
    u = torch.randn((B, E), generator=gen, device=dev)
    wins = {f"win_{f}_{'shuffled' if s else 'sorted'}": windows(f, s, dev, gen) for f in FRACTIONS for s in (False, True)}
    csr = outside_csr(*wins["win_5_sorted"], dev)
    # one click per user, inside the user's 5 % window of the sorted case
    lo5, hi5 = wins["win_5_sorted"]
    tgt_rows = (lo5 + torch.randint(0, int(hi5[0] - lo5[0]), (B,), generator=gen, device=dev, dtype=torch.int32)).contiguous()
    tgt_off = torch.arange(B + 1, device=dev, dtype=torch.int64)
    l = hip.lib()

    def null_topk(k):  # (the Python layer never calls a _win entry point without windows)
        rows = torch.empty((B, k), dtype=torch.int32, device=dev)
        scores = torch.empty((B, k), dtype=torch.float32, device=dev)
        nbytes = l.xnrs_topk_deep_workspace_bytes(B, N_ROWS, 0, k)
        ws = hip.workspace(dev, nbytes)
        hip.check(l.xnrs_topk_deep_win(hip.ptr(table), N_ROWS, E, hip.ptr(u), B, None, None, None, None, -1, k, hip.ptr(rows),
                                       hip.ptr(scores), hip.ptr(ws), nbytes, hip.stream_ptr(dev)), "xnrs_topk_deep_win")
        return rows, scores

    def null_rank(_):
        ranks = torch.empty((B,), dtype=torch.int32, device=dev)
        scores = torch.empty((B,), dtype=torch.float32, device=dev)
        hip.check(l.xnrs_rank_win(hip.ptr(table), N_ROWS, E, hip.ptr(u), B, hip.ptr(tgt_off), hip.ptr(tgt_rows), None, None, None, None,
                                  -1, hip.ptr(ranks), hip.ptr(scores), None, 0, hip.stream_ptr(dev)), "xnrs_rank_win")
        return ranks, scores

    topk = {"parent": lambda k: ops.topk_deep_dot(table, u, k), "parent_again": lambda k: ops.topk_deep_dot(table, u, k),
            "null": null_topk, "excl_csr_5": lambda k: ops.topk_deep_dot(table, u, k, csr[0], csr[1])}
    rank = {"parent": lambda _: ops.rank_dot(table, u, tgt_off, tgt_rows), "parent_again": lambda _: ops.rank_dot(table, u, tgt_off, tgt_rows),
            "null": null_rank, "excl_csr_5": lambda _: ops.rank_dot(table, u, tgt_off, tgt_rows, csr[0], csr[1])}
    for name, (lo, hi) in wins.items():
        topk[name] = lambda k, lo=lo, hi=hi: ops.topk_deep_dot(table, u, k, win_lo=lo, win_hi=hi)
        rank[name] = lambda _, lo=lo, hi=hi: ops.rank_dot(table, u, tgt_off, tgt_rows, win_lo=lo, win_hi=hi)
    return topk, rank


def one_call_ms(fn, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def same(x, y):
    return bool(torch.equal(x[0], y[0]) and torch.equal(x[1].view(torch.int32), y[1].view(torch.int32)))


def measure_workload(routes, k, reps, warmup, passes, slow_reps):
    routes = dict(routes)
    with torch.no_grad():
        checks = dict(null_equals_parent=same(routes["null"](k), routes["parent"](k)),
                      win_5_sorted_equals_excl_csr_5=same(routes["win_5_sorted"](k), routes["excl_csr_5"](k)),
                      win_100_equals_parent=same(routes["win_100_shuffled"](k), routes["parent"](k)))
        slow = routes.pop("excl_csr_5")
        slow_ms = [one_call_ms(slow, k) for _ in range(slow_reps)]  # (the call of `checks` was its warm-up)
        for _ in range(warmup):
            for fn in routes.values():
                fn(k)
        torch.cuda.synchronize()
        names = list(routes)
        medians = {name: [] for name in routes}
        mins = {name: [] for name in routes}
        for _ in range(passes):
            ms = {name: [] for name in routes}
            for r in range(reps):
                for name in names[r % len(names):] + names[:r % len(names)]:  # the routes alternate call by call, the order rotates
                    ms[name].append(one_call_ms(routes[name], k))
            for name, v in ms.items():
                medians[name].append(statistics.median(v))
                mins[name].append(min(v))
    par = medians["parent"] + medians["parent_again"]
    spread = (max(par) - min(par)) / min(par)
    base = statistics.median(par)
    out = dict(results_equal=checks, spread=spread, parent_median_ms=base, routes={})
    for name in routes:
        m = statistics.median(medians[name])
        out["routes"][name] = dict(median_ms=m, pass_medians_ms=medians[name], min_ms=min(mins[name]), over_parent=m / base)
    m = statistics.median(slow_ms)
    out["routes"]["excl_csr_5"] = dict(median_ms=m, min_ms=min(slow_ms), over_parent=m / base, calls=slow_reps)
    out["conditions"] = {name: out["routes"][name]["over_parent"] <= 1.0 + spread for name in ("null", "win_100_sorted", "win_100_shuffled")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--slow-reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from xnrs_amd import hip
    dev = torch.device("cuda", 0)
    topk, rank = build(dev)
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, passes=a.passes, slow_reps=a.slow_reps, B=B, n_rows=N_ROWS, E=E,
               slices=hip.lib().xnrs_topk_slices(B, N_ROWS), excl_csr_ids_per_user=N_ROWS - N_ROWS * 5 // 100, workloads={})
    for k in KS:
        res["workloads"][f"topk_k{k}"] = measure_workload(topk, k, a.reps, a.warmup, a.passes, a.slow_reps)
        print(f"topk k = {k}: done", file=sys.stderr, flush=True)
    res["workloads"]["rank"] = measure_workload(rank, 0, a.reps, a.warmup, a.passes, a.slow_reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
