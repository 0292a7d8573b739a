#!/usr/bin/env python
"""bench_list_xent.py -- the soft-target loss over listed rows (ops.list_xent: xnrs_list_xent_fwd / _bwd, no copy of the
listed rows) against the ranking loss over the same lists (ops.list_loss, the kernels it shares its walk with) and against
the torch composition, one JSON file.

    python tools/bench_list_xent.py [--reps R] [--warmup W] --out profiles/list_xent_bench.json

Shape: B = 4096 sessions x n_rows = 65536 news x E = 256, L in {16, 128, 1024} rows per session, the lists those of
ops.topk_deep_dot (nothing excluded), the weights the softmax of the student's own scores of the listed rows, perturbed.
Per L, each route in three modes -- fwd; fwd_dup (forward + d_up); fwd_dup_dtable (forward + d_up + d_table, the order's
device sort included):
  xent      : ops.list_xent
  rank      : (i) ops.list_loss on the same lists with one click per session -- the same row traffic minus the (B, L) weights
  composed  : (ii) ops.embedding_rows into a (B, L, E) copy of the listed rows of the DETACHED table, ops.dot_scoring, torch's
              logsumexp and the weighted sum; fwd and fwd_dup only
Every route is warmed up, each call lies between two device events, and every figure is the median over `reps` calls of ONE
run; each route is run TWICE (run_a, run_b) and `spread` = |a - b| / min(a, b) is the run-to-run spread its ratios are to
be read against.  ratio_to_rank = xent / rank and ratio_to_composed = xent / composed use the smaller median of the two
runs.  No ratio is a condition: the file states what was measured."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, N_ROWS, E = 4096, 65536, 256
LS = (16, 128, 1024)
MODES = ("fwd", "fwd_dup", "fwd_dup_dtable")


def one_call_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def one_run(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = [one_call_ms(fn) for _ in range(reps)]
    return dict(median_ms=statistics.median(ms), min_ms=min(ms))


def two_runs(fn, reps, warmup):
    a, b = one_run(fn, reps, warmup), one_run(fn, reps, warmup)
    lo, hi = sorted((a["median_ms"], b["median_ms"]))
    return dict(run_a=a, run_b=b, best_median_ms=lo, spread=(hi - lo) / lo, calls=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("at least 20 timed calls per route")
    from xnrs_amd import hip, ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    table = torch.randn((N_ROWS, E), generator=gen, device=dev)
    up = torch.randn((B, E), generator=gen, device=dev) * (2.0 / E ** 0.5)
    tgt_rows = torch.randint(0, N_ROWS, (B,), generator=gen, device=dev, dtype=torch.int32)
    tgt_off = torch.arange(B + 1, device=dev, dtype=torch.int64)
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, B=B, n_rows=N_ROWS, E=E, cases={})

    def grads(mode):
        return table.detach().requires_grad_(mode == "fwd_dup_dtable"), up.detach().requires_grad_(mode != "fwd")

    def xent_route(rows, w, mode):
        def fn():
            t, u = grads(mode)
            loss = ops.list_xent(t, u, rows, w, -1)[0]
            if mode != "fwd":
                loss.sum().backward()
            return loss.detach()
        return fn

    def rank_route(rows, mode):
        def fn():
            t, u = grads(mode)
            loss = ops.list_loss(t, u, tgt_off, tgt_rows, rows, -1)[0]
            if mode != "fwd":
                loss.sum().backward()
            return loss.detach()
        return fn

    def composed_route(rows, w, mode):
        idx = rows.reshape(-1).contiguous()

        def fn():
            u = up.detach().requires_grad_(mode != "fwd")
            c = ops.embedding_rows(idx, table).reshape(B, -1, E)
            s = ops.dot_scoring(u.reshape(B, 1, E), c).reshape(B, -1)
            loss = (w * (torch.logsumexp(s, dim=1, keepdim=True) - s)).sum(dim=1)
            if mode != "fwd":
                loss.sum().backward()
            return loss.detach()
        return fn

    for L in LS:
        rows, scores = ops.topk_deep_dot(table, up, L, None, None, -1)[:2]
        w = torch.softmax(scores + 0.5 * torch.randn(scores.shape, generator=gen, device=dev), dim=1).contiguous()
        row = dict(L=L, copy_bytes=4 * B * L * E, workspace_bytes=hip.lib().xnrs_list_xent_workspace_bytes(B, L, E, 1),
                   listed_slots_filled=float((rows >= 0).float().mean()))
        want = composed_route(rows, w, "fwd")()
        row["loss_max_rel_diff_vs_composed"] = float((xent_route(rows, w, "fwd")() - want).abs().max() / want.abs().max())
        for mode in MODES:
            m = dict(xent=two_runs(xent_route(rows, w, mode), a.reps, a.warmup),
                     rank=two_runs(rank_route(rows, mode), a.reps, a.warmup))
            m["ratio_to_rank"] = m["xent"]["best_median_ms"] / m["rank"]["best_median_ms"]
            m["spread_of_the_pair"] = max(m["xent"]["spread"], m["rank"]["spread"])
            if mode != "fwd_dup_dtable":
                m["composed"] = two_runs(composed_route(rows, w, mode), a.reps, a.warmup)
                m["ratio_to_composed"] = m["xent"]["best_median_ms"] / m["composed"]["best_median_ms"]
            row[mode] = m
        res["cases"][f"L{L}"] = row
        print(json.dumps({f"L{L}": row}, sort_keys=True), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
