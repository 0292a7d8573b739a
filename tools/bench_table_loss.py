#!/usr/bin/env python
"""bench_table_loss.py -- the full-table softmax ranking loss (ops.table_loss: xnrs_table_loss_fwd / _bwd, no score matrix)
against the torch route that materialises the (B, n_rows) score matrix, its masked logsumexp and its gradient, one JSON file.

    python tools/bench_table_loss.py [--reps R] [--warmup W] [--big] --out profiles/table_loss_bench.json

Cases: B = 4096 users x n_rows = 65536 news x E = 256, a 50-row exclusion list per user;
  one_click   : one target per user
  four_clicks : four targets per user
  windows_5pct: one target per user, every user a window of 5 % of the table, the users in time order (neighbouring users
                have neighbouring windows: narrow unions per user tile)
  --big       : n_rows = 1048576 (a 17 GB score matrix), one click, the HIP route; the torch route is tried and its
                failure recorded when it does not fit
Routes, each for fwd / fwd + d_up / fwd + d_up + d_table:
  hip   : ops.table_loss (+ backward of the summed loss)
  torch : s = up @ table.T, masked_fill of a precomputed (B, n_rows) bool mask, logsumexp, logaddexp - s_t (+ autograd)
Every route is warmed up; the routes ALTERNATE call by call in one process, each call between two device events; the figures
are medians over `reps` calls (min beside them).  peak_bytes: torch.cuda.max_memory_allocated over one call of the route minus
what was allocated before it (the operands, and for torch the mask, are there before; the HIP workspace is grown before).
No ratio is a condition: the file states what was measured.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, N_ROWS, E, N_EXCL = 4096, 65536, 256, 50
CASES = [("one_click", N_ROWS, 1, False), ("four_clicks", N_ROWS, 4, False), ("windows_5pct", N_ROWS, 1, True)]
MODES = ("fwd", "fwd_dup", "fwd_dup_dtable")


def build(n_rows, T, windowed, dev, want_torch=True):
    from xnrs_amd import ops
    gen = torch.Generator(device=dev)
    gen.manual_seed(7 + T + n_rows)
    table = torch.randn((n_rows, E), generator=gen, device=dev)
    up = torch.randn((B, E), generator=gen, device=dev) * (2.0 / E ** 0.5)
    excl_rows = torch.randint(0, n_rows, (B * N_EXCL,), generator=gen, device=dev, dtype=torch.int32)
    excl_off = torch.arange(B + 1, device=dev, dtype=torch.int64) * N_EXCL
    user = torch.arange(B, device=dev)
    win_lo = win_hi = None
    if windowed:
        width = n_rows // 20
        win_hi = (width + (n_rows - width) * user // (B - 1)).to(torch.int32)
        win_lo = win_hi - width
        tgt = (win_lo[:, None] + torch.randint(0, width, (B, T), generator=gen, device=dev, dtype=torch.int32)).to(torch.int32)
    else:
        tgt = torch.randint(0, n_rows, (B, T), generator=gen, device=dev, dtype=torch.int32)
    tgt_off = torch.arange(B + 1, device=dev, dtype=torch.int64) * T
    tgt_rows = tgt.reshape(-1).contiguous()

    def hip_route(mode):
        t = table.detach().requires_grad_(mode >= 2)
        u = up.detach().requires_grad_(mode >= 1)
        loss, _, _ = ops.table_loss(t, u, tgt_off, tgt_rows, excl_off, excl_rows, -1, win_lo, win_hi)
        if mode:
            loss.sum().backward()
        return loss.detach()

    mask = None

    def torch_route(mode):
        t = table.detach().requires_grad_(mode >= 2)
        u = up.detach().requires_grad_(mode >= 1)
        s = u @ t.T
        lse = torch.logsumexp(s.masked_fill(mask, float("-inf")), dim=1)
        st = s.gather(1, tgt.long())
        loss = torch.logaddexp(st, lse[:, None]) - st
        if mode:
            loss.sum().backward()
        return loss.detach().reshape(-1)

    if want_torch:
        mask = torch.zeros((B, n_rows), dtype=torch.bool, device=dev)  # True: not a negative
        mask[user.repeat_interleave(N_EXCL), excl_rows.long()] = True
        mask[user.repeat_interleave(T), tgt_rows.long()] = True
        if windowed:
            n = torch.arange(n_rows, device=dev)
            mask |= (n[None] < win_lo[:, None]) | (n[None] >= win_hi[:, None])
    return hip_route, torch_route if want_torch else None


def one_call_ms(fn, mode):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(mode)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak_bytes(fn, mode):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn(mode)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def stats(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), calls=len(ms))


def measure_case(name, n_rows, T, windowed, reps, warmup, dev, try_torch=True):
    from xnrs_amd import hip
    row = dict(B=B, n_rows=n_rows, E=E, targets_per_user=T, windowed=windowed, score_matrix_bytes=4 * B * n_rows,
               workspace_bytes=hip.lib().xnrs_table_loss_workspace_bytes(B, n_rows, E, 1))
    try:
        hip_route, torch_route = build(n_rows, T, windowed, dev, try_torch)
    except torch.cuda.OutOfMemoryError as e:
        torch.cuda.empty_cache()
        row["torch"] = f"the mask alone does not fit: {str(e).splitlines()[0]}"
        hip_route, torch_route = build(n_rows, T, windowed, dev, False)
    routes = [("hip", hip_route)] + ([("torch", torch_route)] if torch_route is not None else [])
    try:
        for _ in range(warmup):
            for _, fn in routes:
                for mode in range(3):
                    fn(mode)
    except torch.cuda.OutOfMemoryError as e:
        torch.cuda.empty_cache()
        row["torch"] = f"does not fit: {str(e).splitlines()[0]}"
        routes = routes[:1]
    torch.cuda.synchronize()
    ms = {(r, m): [] for r, _ in routes for m in range(3)}
    for _ in range(reps):
        for mode in range(3):
            for r, fn in routes:  # the routes alternate call by call
                ms[(r, mode)].append(one_call_ms(fn, mode))
    for r, fn in routes:
        row[r] = {MODES[m]: dict(stats(ms[(r, m)]), peak_bytes=peak_bytes(fn, m)) for m in range(3)}
    if len(routes) == 2:
        a, b = hip_route(0), torch_route(0)
        row["loss_max_rel_diff"] = float((a - b).abs().max() / b.abs().max())
        row["hip_over_torch"] = {MODES[m]: row["hip"][MODES[m]]["median_ms"] / row["torch"][MODES[m]]["median_ms"] for m in range(3)}
    del routes, hip_route, torch_route
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--big", action="store_true", help="add the case n_rows = 1048576")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("at least 20 timed calls per route")
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, cases={})
    for name, n_rows, T, windowed in CASES:
        res["cases"][name] = measure_case(name, n_rows, T, windowed, a.reps, a.warmup, dev)
    if a.big:
        res["cases"]["big_one_click"] = measure_case("big_one_click", 16 * N_ROWS, 1, False, a.reps, 1, dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
