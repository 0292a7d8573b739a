#!/usr/bin/env python
"""bench_list_loss.py -- the ranking loss over mined negatives (ops.list_loss: xnrs_list_loss_fwd / _bwd, no copy of the
listed rows) against the route the parent commit offers for the same lists, and against the full-table loss, one JSON file.

    python tools/bench_list_loss.py [--reps R] [--warmup W] --out profiles/list_loss_bench.json

Shape: B = 4096 sessions x n_rows = 65536 news x E = 256, one click per session, L in {16, 128, 1024} negatives per session,
the lists mined by ops.topk_deep_dot with the click excluded.  Per L:
  a_mining            : topk_deep alone
  b_fwd               : ops.list_loss forward
  c_fwd_dup           : forward + d_up
  d_fwd_dup_dtable    : forward + d_up + d_table (the order's device sort included)
  e_composed          : the parent's operators on the same lists: ops.embedding_rows into a (B, L + 1, E) copy,
                        ops.dot_scoring, torch.logsumexp, forward + backward to `up` and the table
                        (xnrs_embedding_grad_sparse scatters the copy's gradient)
  e_composed_dup_only : the same with the table detached (no scatter)
  f_table_loss        : ops.table_loss forward + backward in the same process, for context (once, it does not depend on L)
  g_same_rows (L=128) : case d with every session listing the SAME 128 rows: the longest runs the d_table walk can meet
Every route is warmed up, each call lies between two device events, the figures are medians over `reps` calls (min beside
them).  The scatter of e_composed scans the id list once per id, so its cost grows with the square of B (L + 1): a route
whose first call takes more than a second is timed over fewer calls (`calls` says how many), and one whose cost, projected
from the next smaller L by that square, passes --skip-over seconds per call is not run; the projection is recorded.
peak_bytes: torch.cuda.max_memory_allocated over one call minus what was allocated before it (operands and lists are there
before; the HIP workspace is grown before).  No ratio is a condition: the file states what was measured.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, N_ROWS, E = 4096, 65536, 256
LS = (16, 128, 1024)


def one_call_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak_bytes(fn):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def measure(fn, reps, warmup, projected_s=None, skip_over=60.0):
    """median / min over `reps` calls; fewer calls for a route whose call takes more than a second"""
    if projected_s is not None and projected_s > skip_over:
        return dict(not_measured=f"projected {projected_s:.0f} s per call from the next smaller L (cost ~ (B (L + 1))^2)")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    first_s = time.perf_counter() - t0
    if first_s > 1.0:
        reps, warmup = max(3, min(reps, int(20.0 / first_s))), 0
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = [one_call_ms(fn) for _ in range(reps)]
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), calls=len(ms), peak_bytes=peak_bytes(fn))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-over", type=float, default=60.0, help="do not run a route projected above this many seconds a call")
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

    def list_route(neg, mode):
        def fn():
            t = table.detach().requires_grad_(mode >= 2)
            u = up.detach().requires_grad_(mode >= 1)
            loss = ops.list_loss(t, u, tgt_off, tgt_rows, neg, -1)[0]
            if mode:
                loss.sum().backward()
            return loss.detach()
        return fn

    def composed_route(neg, with_table):
        idx = torch.cat((tgt_rows.reshape(B, 1), neg), dim=1).reshape(-1).contiguous()

        def fn():
            t = table.detach().requires_grad_(with_table)
            u = up.detach().requires_grad_(True)
            c = ops.embedding_rows(idx, t).reshape(B, -1, E)
            s = ops.dot_scoring(u.reshape(B, 1, E), c).reshape(B, -1)
            loss = torch.logsumexp(s, dim=1) - s[:, 0]
            loss.sum().backward()
            return loss.detach()
        return fn

    def table_route():
        t = table.detach().requires_grad_(True)
        u = up.detach().requires_grad_(True)
        loss = ops.table_loss(t, u, tgt_off, tgt_rows)[0]
        loss.sum().backward()
        return loss.detach()

    res["f_table_loss"] = measure(table_route, a.reps, a.warmup)
    last_composed = None  # (L, seconds per call) of the last measured e_composed
    for L in LS:
        row = dict(L=L, copy_bytes=4 * B * (L + 1) * E, workspace_bytes=hip.lib().xnrs_list_loss_workspace_bytes(B, L, B, E, 1))
        mine = lambda: ops.topk_deep_dot(table, up, L, tgt_off, tgt_rows, -1)[0]  # noqa: E731
        neg = mine()
        row["listed_slots_filled"] = float((neg >= 0).float().mean())
        row["a_mining"] = measure(mine, a.reps, a.warmup)
        row["b_fwd"] = measure(list_route(neg, 0), a.reps, a.warmup)
        row["c_fwd_dup"] = measure(list_route(neg, 1), a.reps, a.warmup)
        row["d_fwd_dup_dtable"] = measure(list_route(neg, 2), a.reps, a.warmup)
        row["e_composed_dup_only"] = measure(composed_route(neg, False), a.reps, a.warmup)
        projected = None if last_composed is None else last_composed[1] * ((L + 1) / (last_composed[0] + 1)) ** 2
        row["e_composed"] = measure(composed_route(neg, True), a.reps, a.warmup, projected, a.skip_over)
        if "median_ms" in row["e_composed"]:
            last_composed = (L, row["e_composed"]["median_ms"] / 1e3)
            want = composed_route(neg, False)()
            row["loss_max_rel_diff_vs_composed"] = float((list_route(neg, 0)() - want).abs().max() / want.abs().max())
        if L == 128:
            same = neg[:1].repeat(B, 1).contiguous()
            row["g_same_rows"] = measure(list_route(same, 2), a.reps, a.warmup)
        step = row["a_mining"]["median_ms"] + row["d_fwd_dup_dtable"]["median_ms"]
        row["a_plus_d_ms"] = step
        row["a_plus_d_over_f"] = step / res["f_table_loss"]["median_ms"]
        if "median_ms" in row["e_composed"]:
            row["a_plus_d_over_a_plus_e"] = step / (row["a_mining"]["median_ms"] + row["e_composed"]["median_ms"])
            row["d_over_e"] = row["d_fwd_dup_dtable"]["median_ms"] / row["e_composed"]["median_ms"]
        row["c_over_e_dup_only"] = row["c_fwd_dup"]["median_ms"] / row["e_composed_dup_only"]["median_ms"]
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
