#!/usr/bin/env python
"""bench_topk_sample.py -- what a sampled list costs (xnrs_topk_sample_win: Gumbel top-k inside the top-k sweep), one JSON file.

    python tools/bench_topk_sample.py [--reps R] [--warmup W] --out profiles/topk_sample_bench.json
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_topk_sample.py --sample-only --reps 10
    python tools/bench_topk_sample.py --merge-trace DIR --reps 10 --out profiles/topk_sample_bench.json   (no device: adds the
                                                                                   kernel times of that run to the file)

Shape: B = 4096 users x n_rows = 65536 x E = 256, scores ~ N(0, 1); k in {10, 100, 256} x temperature in {0.05, 1} -- the draw
of a score is skipped when the score cannot reach the user's threshold, and how soon that is depends on the temperature.
  sample : ops.topk_sample_dot
  deep   : ops.topk_deep_dot of the same shape (the sweep without the noise)
  torch  : u @ table.T -> the (B, n_rows) score matrix / temperature, plus -log(-log(U)) of a torch.rand_like, torch.topk
Every (k, temperature) is warmed up; the three routes ALTERNATE call by call in one process, each call between two device
events; the figures are medians over `reps` calls with min, max and the quartiles beside them (the spread).  Kernel times come
from a separate rocprofv3 kernel trace of --sample-only (tracing slows the host), merged by --merge-trace: per configuration the
mean of the last `reps` calls' kernels (partial sweeps, floor, merge).  No ratio is promised: 2.7e8 draws per call have their
price.  `verdict` says in capitals when the sampled call is SLOWER THAN TORCH.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, N_ROWS, E = 4096, 65536, 256
CONFIGS = [(k, tau) for k in (10, 100, 256) for tau in (0.05, 1.0)]
KERNELS = ("topk_partial_kernel", "topk_floor_kernel", "topk_merge_kernel")


def build(dev):
    from xnrs_amd import ops
    gen = torch.Generator(device=dev)
    gen.manual_seed(4096)
    table = torch.randn((N_ROWS, E), generator=gen, device=dev)
    u = torch.randn((B, E), generator=gen, device=dev) / E ** 0.5
    step = [0]

    def sample(k, tau):
        step[0] += 1  # a fresh seed per call, as a caller draws
        return ops.topk_sample_dot(table, u, k, tau, step[0])

    def deep(k, tau):
        return ops.topk_deep_dot(table, u, k)

    def torch_route(k, tau):
        s = (u @ table.t()) / tau
        s -= torch.log(-torch.log(torch.rand_like(s)))
        return torch.topk(s, k, dim=1)
    return dict(sample=sample, deep=deep, torch=torch_route)


def one_call_ms(fn, *args):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(*args)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), q1_ms=q[0], q3_ms=q[2], calls=len(ms))


def measure(reps, warmup, sample_only):
    from xnrs_amd import hip
    dev = torch.device("cuda", 0)
    routes = build(dev)
    names = ["sample"] if sample_only else ["sample", "deep", "torch"]
    out = {}
    for k, tau in CONFIGS:
        with torch.no_grad():
            for _ in range(warmup):
                for n in names:
                    routes[n](k, tau)
            torch.cuda.synchronize()
            ms = {n: [] for n in names}
            for _ in range(reps):
                for n in names:  # the routes alternate call by call
                    ms[n].append(one_call_ms(routes[n], k, tau))
        row = dict(B=B, n_rows=N_ROWS, E=E, k=k, temperature=tau, draws_per_call=B * N_ROWS, executed_flop=2.0 * B * N_ROWS * E,
                   slices=hip.lib().xnrs_topk_slices(B, N_ROWS), workspace_bytes=hip.lib().xnrs_topk_deep_workspace_bytes(B, N_ROWS, 0, k),
                   score_matrix_bytes=4 * B * N_ROWS)
        row.update({n: stats(v) for n, v in ms.items()})
        if not sample_only:
            row["sample_over_deep"] = row["sample"]["median_ms"] / row["deep"]["median_ms"]
            row["sample_over_torch"] = row["sample"]["median_ms"] / row["torch"]["median_ms"]
            row["verdict"] = "SLOWER THAN TORCH" if row["sample_over_torch"] > 1 else "faster than torch"
        out[f"k{k}_tau{tau}"] = row
        torch.cuda.empty_cache()
    return out


def merge_trace(root, res, calls):
    """Kernel times of the --sample-only run under rocprofv3: the dispatches in start order, `calls` calls per configuration,
    each call ending with its merge kernel."""
    files = glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {root}")
    rows = [r for r in csv.DictReader(open(files[0])) if any(n in r["Kernel_Name"] for n in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_call, cur = [], {}
    for r in rows:
        name = next(n for n in KERNELS if n in r["Kernel_Name"])
        cur[name] = cur.get(name, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        if name == "topk_merge_kernel":
            per_call.append(cur)
            cur = {}
    if len(per_call) != calls * len(CONFIGS):
        raise SystemExit(f"{len(per_call)} calls in the trace, expected {calls * len(CONFIGS)}")
    timed = res["trace_reps"]
    res["trace_warmup"] = calls - timed
    for i, (k, tau) in enumerate(CONFIGS):
        mine = per_call[i * calls:(i + 1) * calls][-timed:]
        us = {n.replace("topk_", "").replace("_kernel", "") + "_us": sum(c.get(n, 0) for c in mine) / timed / 1e3 for n in KERNELS}
        us["all_us"] = sum(us.values())
        us["executed_tflops"] = res["shapes"][f"k{k}_tau{tau}"]["executed_flop"] / (us["all_us"] * 1e-6) / 1e12
        res["shapes"][f"k{k}_tau{tau}"]["kernels"] = us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample-only", action="store_true")
    ap.add_argument("--merge-trace", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.merge_trace:
        res = json.load(open(a.out))
        res["trace_reps"] = a.reps
        merge_trace(a.merge_trace, res, a.reps + a.warmup)
    elif a.sample_only:
        measure(a.reps, a.warmup, True)
        return
    else:
        if a.reps < 20:
            raise SystemExit("at least 20 timed calls per route")
        res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, shapes=measure(a.reps, a.warmup, False))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
