#!/usr/bin/env python
"""bench_rank.py -- the rank of given rows within the whole news table: the fused call (xnrs_rank: scores compared with the
targets' while they are formed) against the unfused route that materialises the (B, n_rows) score matrix, one JSON file.

    python tools/bench_rank.py [--reps R] [--warmup W] --out first.json
    python tools/bench_rank.py [--reps R] [--warmup W] --repeat-of first.json --out profiles/rank_bench.json
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_rank.py --fused-only --reps 10
    python tools/bench_rank.py --merge-trace DIR --reps 10 --out profiles/rank_bench.json   (no device: adds the kernel times
                                                                                              of that run to the file)

Shapes: n_rows = 65536, E = 256, a 50-row exclusion list per user; the dot scorer at B in {64, 4096} x {1, 4} targets per user;
the MLP scorer (H = 128) at B = 64.
  fused    : ops.rank_dot / ops.rank_mlp
  unfused  : ops.linear(u, table) -> the (B, n_rows) score matrix, the targets' scores gathered, the exclusions scattered to
             -inf, (s > s_t).sum(1) per target
  topk10   : ops.topk_dot(k = 10) over the same operands, timed in the same run -- for orientation only
Every shape is warmed up; the routes ALTERNATE call by call in one process, each call between two device events; the figures
are medians over `reps` calls (min beside them).  Kernel times come from a separate rocprofv3 kernel trace of --fused-only
(tracing slows the host), merged by --merge-trace: per shape the mean of the last `reps` calls' target + sweep kernel time and
the executed TFLOP/s 2 B n_rows E (MLP: H) of the sweep over it.

The one condition: at B = 4096 the fused call is not slower than the unfused route of the same run by more than the run-to-run
spread.  --repeat-of FILE makes this run the repeat of an earlier one: the file keeps both (`first_run`), each shape gets
`spread` = the larger relative difference of its medians between the runs, and the tool exits 1 when fused > unfused x
(1 + spread) in this run at B = 4096 (`condition` in the file says which).
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

N_ROWS, E, H_MLP, N_EXCL = 65536, 256, 128, 50
PEAK_F32_MATRIX_TF = 157.3
SHAPES = [("dot", B, T) for B in (64, 4096) for T in (1, 4)] + [("mlp", 64, 1), ("mlp", 64, 4)]


def build(kind, B, T, dev):
    from xnrs_amd import ops
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 + B + T)
    W = E if kind == "dot" else H_MLP
    table = torch.randn((N_ROWS, W), generator=gen, device=dev)
    u = torch.randn((B, E), generator=gen, device=dev)
    excl_rows = torch.randint(0, N_ROWS, (B * N_EXCL,), generator=gen, device=dev, dtype=torch.int32)
    excl_off = torch.arange(B + 1, device=dev, dtype=torch.int64) * N_EXCL
    excl_user = torch.arange(B, device=dev).repeat_interleave(N_EXCL)
    tgt = torch.randint(0, N_ROWS, (B, T), generator=gen, device=dev, dtype=torch.int32)
    tgt_off = torch.arange(B + 1, device=dev, dtype=torch.int64) * T
    tgt_rows = tgt.reshape(-1).contiguous()
    if kind == "dot":
        def fused():
            return ops.rank_dot(table, u, tgt_off, tgt_rows, excl_off, excl_rows)

        def unfused():
            s = ops.linear(u, table)
            s_t = s.gather(1, tgt.long())
            s[excl_user, excl_rows.long()] = float("-inf")
            return torch.stack([(s > s_t[:, j:j + 1]).sum(1) for j in range(T)], dim=1), s_t

        def topk10():
            return ops.topk_dot(table, u, 10, excl_off, excl_rows)
        return fused, unfused, topk10
    w1 = torch.randn((H_MLP, 2 * E), generator=gen, device=dev) / (2 * E) ** 0.5
    b1, w2, b2 = (torch.randn(s, generator=gen, device=dev) for s in ((H_MLP,), (1, H_MLP), (1,)))
    return (lambda: ops.rank_mlp(table, u, w1, b1, w2, b2, tgt_off, tgt_rows, excl_off, excl_rows)), None, None


def one_call_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), calls=len(ms))


def measure(reps, warmup, fused_only):
    from xnrs_amd import hip
    dev = torch.device("cuda", 0)
    out = {}
    for kind, B, T in SHAPES:
        fused, unfused, topk10 = build(kind, B, T, dev)
        routes = [("fused", fused)]
        if not fused_only:
            routes += [(n, f) for n, f in (("unfused", unfused), ("topk10", topk10)) if f is not None]
        with torch.no_grad():
            for _ in range(warmup):
                for _, fn in routes:
                    fn()
            torch.cuda.synchronize()
            ms = {name: [] for name, _ in routes}
            for _ in range(reps):
                for name, fn in routes:  # the routes alternate call by call
                    ms[name].append(one_call_ms(fn))
        width = E if kind == "dot" else H_MLP
        row = dict(scorer=kind, B=B, targets_per_user=T, n_rows=N_ROWS, width=width, executed_flop=2.0 * B * N_ROWS * width,
                   slices=hip.lib().xnrs_topk_slices(B, N_ROWS),
                   workspace_bytes=hip.lib().xnrs_rank_workspace_bytes(B, 0 if kind == "dot" else H_MLP),
                   score_matrix_bytes=4 * B * N_ROWS)
        row.update({name: stats(v) for name, v in ms.items()})
        if "unfused" in row:
            row["fused_over_unfused"] = row["fused"]["median_ms"] / row["unfused"]["median_ms"]
            # the two routes sum in different orders (and the unfused one has no tie rule): the share of queries with the same rank
            with torch.no_grad():
                row["ranks_agree"] = float((fused()[0].reshape(B, T).long() == unfused()[0]).float().mean())
        out[f"{kind}_B{B}_T{T}"] = row
        torch.cuda.empty_cache()
    return out


def merge_trace(root, res, calls):
    """Kernel times of the --fused-only run under rocprofv3: the dispatches in start order, `calls` per shape."""
    files = glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {root}")
    rows = [r for r in csv.DictReader(open(files[0])) if "rank_target_kernel" in r["Kernel_Name"] or "rank_sweep_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    tgt = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if "rank_target_kernel" in r["Kernel_Name"]]
    sweep = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if "rank_sweep_kernel" in r["Kernel_Name"]]
    if len(sweep) != calls * len(SHAPES) or len(tgt) != len(sweep):
        raise SystemExit(f"{len(tgt)} target / {len(sweep)} sweep dispatches in the trace, expected {calls * len(SHAPES)} each")
    timed = res["trace_reps"]
    res["trace_warmup"] = calls - timed
    for i, (kind, B, T) in enumerate(SHAPES):
        t = tgt[i * calls:(i + 1) * calls][-timed:]
        s = sweep[i * calls:(i + 1) * calls][-timed:]
        row = res["shapes"][f"{kind}_B{B}_T{T}"]
        sweep_us = sum(s) / timed / 1e3
        tf = row["executed_flop"] / (sweep_us * 1e-6) / 1e12
        row["kernels"] = dict(target_us=sum(t) / timed / 1e3, sweep_us=sweep_us, both_us=(sum(t) + sum(s)) / timed / 1e3,
                              sweep_executed_tflops=tf)
        if kind == "dot":
            row["kernels"]["sweep_share_of_fp32_matrix_peak"] = tf / PEAK_F32_MATRIX_TF


def check_condition(res, first):
    """spread per shape from the two runs; the condition at B = 4096 on this run -> True when it holds"""
    ok = True
    for name, row in res["shapes"].items():
        rel = [abs(row[r]["median_ms"] - first["shapes"][name][r]["median_ms"]) / min(row[r]["median_ms"], first["shapes"][name][r]["median_ms"])
               for r in ("fused", "unfused") if r in row]
        row["spread"] = max(rel)
        if row["B"] == 4096:
            row["condition_holds"] = row["fused"]["median_ms"] <= row["unfused"]["median_ms"] * (1.0 + row["spread"])
            ok = ok and row["condition_holds"]
    res["first_run"] = first["shapes"]
    res["condition"] = ("holds" if ok else "FAILS") + ": at B = 4096 the fused call is not slower than the unfused route by more than the spread"
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--merge-trace", default="")
    ap.add_argument("--repeat-of", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ok = True
    if a.merge_trace:
        res = json.load(open(a.out))
        res["trace_reps"] = a.reps
        merge_trace(a.merge_trace, res, a.reps + a.warmup)
    elif a.fused_only:
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
