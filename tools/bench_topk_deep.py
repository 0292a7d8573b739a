#!/usr/bin/env python
"""bench_topk_deep.py -- deep top-k (xnrs_topk_deep: lists of up to 1024 news per user) against xnrs_topk at its own limit
and against the unfused route through the (B, n_rows) score matrix, one JSON file.

    python tools/bench_topk_deep.py [--reps R] [--warmup W] --out first.json
    python tools/bench_topk_deep.py [--reps R] [--warmup W] --repeat-of first.json --out profiles/topk_deep_bench.json
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_topk_deep.py --deep-only --reps 10
    python tools/bench_topk_deep.py --merge-trace DIR --reps 10 --out profiles/topk_deep_bench.json   (no device: adds the
                                                                                       kernel times of that run to the file)

Shapes: n_rows = 65536, E = 256, a 50-row exclusion list per user, B in {64, 4096} x k in {128, 256, 1024}; the dot scorer
and the MLP scorer (H = 128).
  deep     : ops.topk_deep_dot / ops.topk_deep_mlp at k
  topk128  : ops.topk_dot / ops.topk_mlp at k = 128, the longest list of xnrs_topk
  unfused  : ops.linear(u, table) -> the (B, n_rows) score matrix, the exclusions scattered to -inf, torch.topk at k (dot
             scorer only: the library has no all-pairs MLP route that is not a CSR of B x n_rows entries)
Every shape is warmed up; the routes ALTERNATE call by call in one process (the order rotates from round to round, so that
every route follows every other equally often), each call between two device events; the
figures are medians over `reps` calls (min beside them).  Kernel times come from a separate rocprofv3 kernel trace of
--deep-only (tracing slows the host), merged by --merge-trace: per shape the mean of the last `reps` calls' kernel times
(first sweep and floor kernel where the call has them, partial, merge).

The one condition: through the deep entry, k = 128 is not slower than xnrs_topk(k = 128) of the same run by more than the
run-to-run spread.  --repeat-of FILE makes this run the repeat of an earlier one: the file keeps both (`first_run`), each
shape gets `spread` = the largest relative difference of a route's two medians between the runs, and the tool exits 1 when
deep > topk128 x (1 + spread) in this run at a k = 128 shape (`condition` in the file says which way it fell).  For k = 256
and 1024 the file states `deep_over_unfused`, whichever way it falls.
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

N_ROWS, E, H_MLP, N_EXCL, K_TOPK = 65536, 256, 128, 50, 128
SHAPES = [(kind, B, k) for kind in ("dot", "mlp") for B in (64, 4096) for k in (128, 256, 1024)]


def build(kind, B, dev):
    from xnrs_amd import ops
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 + B)
    W = E if kind == "dot" else H_MLP
    table = torch.randn((N_ROWS, W), generator=gen, device=dev)
    u = torch.randn((B, E), generator=gen, device=dev)
    excl_rows = torch.randint(0, N_ROWS, (B * N_EXCL,), generator=gen, device=dev, dtype=torch.int32)
    excl_off = torch.arange(B + 1, device=dev, dtype=torch.int64) * N_EXCL
    excl_user = torch.arange(B, device=dev).repeat_interleave(N_EXCL)
    if kind == "dot":
        def unfused(k):
            s = ops.linear(u, table)
            s[excl_user, excl_rows.long()] = float("-inf")
            return torch.topk(s, k, dim=1)
        return (lambda k: ops.topk_deep_dot(table, u, k, excl_off, excl_rows),
                lambda k: ops.topk_dot(table, u, K_TOPK, excl_off, excl_rows), unfused)
    w1 = torch.randn((H_MLP, 2 * E), generator=gen, device=dev) / (2 * E) ** 0.5
    b1, w2, b2 = (torch.randn(s, generator=gen, device=dev) for s in ((H_MLP,), (1, H_MLP), (1,)))
    return (lambda k: ops.topk_deep_mlp(table, u, w1, b1, w2, b2, k, excl_off, excl_rows),
            lambda k: ops.topk_mlp(table, u, w1, b1, w2, b2, K_TOPK, excl_off, excl_rows), None)


def one_call_ms(fn, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), calls=len(ms))


def measure(reps, warmup, deep_only):
    from xnrs_amd import hip
    dev = torch.device("cuda", 0)
    out = {}
    for kind, B, k in SHAPES:
        deep, topk128, unfused = build(kind, B, dev)
        routes = [("deep", deep)]
        if not deep_only:
            routes += [("topk128", topk128)] + ([] if unfused is None else [("unfused", unfused)])
        with torch.no_grad():
            for _ in range(warmup):
                for _, fn in routes:
                    fn(k)
            torch.cuda.synchronize()
            ms = {name: [] for name, _ in routes}
            for r in range(reps):
                # the routes alternate call by call, and the order rotates from round to round: what a call finds in the
                # caches depends on the call before it (the unfused route leaves its 1 GB matrix behind, not the table)
                for name, fn in routes[r % len(routes):] + routes[:r % len(routes)]:
                    ms[name].append(one_call_ms(fn, k))
        width = E if kind == "dot" else H_MLP
        row = dict(scorer=kind, B=B, k=k, n_rows=N_ROWS, width=width, slices=hip.lib().xnrs_topk_slices(B, N_ROWS),
                   workspace_bytes=hip.lib().xnrs_topk_deep_workspace_bytes(B, N_ROWS, 0 if kind == "dot" else H_MLP, k),
                   score_matrix_bytes=4 * B * N_ROWS)
        row.update({name: stats(v) for name, v in ms.items()})
        if "topk128" in row:
            row["deep_over_topk128"] = row["deep"]["median_ms"] / row["topk128"]["median_ms"]
        if "unfused" in row:
            row["deep_over_unfused"] = row["deep"]["median_ms"] / row["unfused"]["median_ms"]
            # the two routes sum in different orders: the share of (user, rank) places that hold the same row
            row["rows_agree"] = float((deep(k)[0].long() == unfused(k)[1]).float().mean())
        if "topk128" in row:  # the first 128 places are those of xnrs_topk, bit for bit
            a, b = deep(k), topk128(k)
            row["first_128_equal_topk"] = bool(torch.equal(a[0][:, :K_TOPK], b[0]) and torch.equal(a[1][:, :K_TOPK], b[1]))
        out[f"{kind}_B{B}_k{k}"] = row
        del deep, topk128, unfused
        torch.cuda.empty_cache()
    return out


def merge_trace(root, res, calls):
    """Kernel times of the --deep-only run under rocprofv3: the dispatches in start order, `calls` per shape.  A call ends with
    its one merge dispatch; what precedes it is its partial sweep(s) -- two for the inner-product forms above k = 128 -- and
    the floor kernel between them."""
    files = glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {root}")
    rows = [r for r in csv.DictReader(open(files[0])) if any(n in r["Kernel_Name"] for n in ("topk_partial_kernel", "topk_floor_kernel", "topk_merge_kernel"))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_call, cur = [], dict(first_sweep_us=0.0, floor_us=0.0, partial_us=0.0)
    for r in rows:
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "topk_merge_kernel" in r["Kernel_Name"]:
            cur["merge_us"] = us
            per_call.append(cur)
            cur = dict(first_sweep_us=0.0, floor_us=0.0, partial_us=0.0)
        elif "topk_floor_kernel" in r["Kernel_Name"]:
            cur["floor_us"] += us
            cur["first_sweep_us"], cur["partial_us"] = cur["partial_us"], 0.0  # (the sweep before the floor was the first one)
        else:
            cur["partial_us"] += us
    if len(per_call) != calls * len(SHAPES):
        raise SystemExit(f"{len(per_call)} merge dispatches in the trace, expected {calls * len(SHAPES)}")
    timed = res["trace_reps"]
    res["trace_warmup"] = calls - timed
    for i, (kind, B, k) in enumerate(SHAPES):
        mine = per_call[i * calls:(i + 1) * calls][-timed:]
        kern = {key: sum(c[key] for c in mine) / timed for key in ("first_sweep_us", "floor_us", "partial_us", "merge_us")}
        kern["all_us"] = sum(kern.values())
        res["shapes"][f"{kind}_B{B}_k{k}"]["kernels"] = kern


def check_condition(res, first):
    """spread per shape from the two runs; the condition at k = 128 on this run -> True when it holds"""
    ok = True
    for name, row in res["shapes"].items():
        rel = [abs(row[r]["median_ms"] - first["shapes"][name][r]["median_ms"]) / min(row[r]["median_ms"], first["shapes"][name][r]["median_ms"])
               for r in ("deep", "topk128", "unfused") if r in row]
        row["spread"] = max(rel)
        if row["k"] == K_TOPK:
            row["condition_holds"] = row["deep"]["median_ms"] <= row["topk128"]["median_ms"] * (1.0 + row["spread"])
            ok = ok and row["condition_holds"]
    res["first_run"] = first["shapes"]
    res["condition"] = ("holds" if ok else "FAILS") + ": at k = 128 the deep entry is not slower than xnrs_topk by more than the spread"
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--deep-only", action="store_true")
    ap.add_argument("--merge-trace", default="")
    ap.add_argument("--repeat-of", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ok = True
    if a.merge_trace:
        res = json.load(open(a.out))
        res["trace_reps"] = a.reps
        merge_trace(a.merge_trace, res, a.reps + a.warmup)
    elif a.deep_only:
        measure(a.reps, a.warmup, True)
        return
    else:
        if a.reps < 20:
            raise SystemExit("at least 20 timed calls per route")
        res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, shapes=measure(a.reps, a.warmup, False))
        if a.repeat_of:
            ok = check_condition(res, json.load(open(a.repeat_of)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(res, sort_keys=True))
    if not ok:
        raise SystemExit(res["condition"])


if __name__ == "__main__":
    main()
