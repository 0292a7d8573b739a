"""The news table stored in bf16: what the id path costs on it (a tool, not a test; needs a GPU).

    python tools/bench_bf16_table.py --mode step --variants fp32,bf16,bf16_a16_off --out profiles/bf16_table_bench.json
    python tools/bench_bf16_table.py --mode qkv --out profiles/bf16_table_bench.json

It imports xnrs_amd and bench from the CURRENT DIRECTORY, so `--mode step --variants fp32` also runs from a checkout of an
earlier commit: the yardstick of the bf16 lines is the fp32-table line of the PARENT commit measured in the same session.
--out is ONE JSON document, a list of records: every run reads it, appends its record and writes it back.  --tag names the
build of a record.

step: the benchmark's id path (bench.id_path_extra: B = 512 impressions of 50 + 5 news x 50 x 768 as row ids ~ Zipf(1.1) into
      a table of --n-news news, about half the history slots empty), ParentRec.forward_ids in inference:
        fp32          the fp32 table
        bf16          the same table rounded to bf16 (NewsStore.astype), XNRS_GEMM_A16=1: Q|K|V straight from the bf16 rows
        bf16_a16_off  the bf16 table with XNRS_GEMM_A16=0: every pass widens its rows and runs the fp32 route
      one process, `--reps` repetitions of (5 warm-up + `--steps` timed steps) per variant, the variants alternating; the
      record holds every repetition, the median and the min-max spread, the bytes of each table in HBM, and the launch
      timer's qkv_gemm stage (ms, launches, executed FLOPs -> TF) of one more step per variant.
qkv:  the Q|K|V product alone, 65 500 x 2 304 x 768 over gathered table rows, as ONE nn.Linear of 2 304 outputs:
        gemm_f32 (gathered rows), bf16x3, bf16x2 (xnrs_set_gemm_mode 0 / 1 / 2 on xnrs_linear_fwd; the split modes split the
        weight inside the kernel here, the encoder hands them pre-split planes) and gemm_a16 (xnrs_linear_fwd_bf16: its weight
        split launch is inside the timed region).  Device events around `--launches` launches: us per launch, algorithmic TF.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from xnrs_amd import hip, ops, synth  # noqa: E402


def emit(path, rec):
    rec = dict(rec, build_id=hip.build_id(), device=torch.cuda.get_device_name(0), time=time.strftime("%Y-%m-%dT%H:%M:%S"))
    print(json.dumps(rec), flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        recs = json.load(open(path)) if os.path.exists(path) else []
        recs.append(rec)
        with open(path, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(r) for r in recs) + "\n]\n")


def table(dev, n_news, S, D):
    gen = torch.Generator(device=dev)
    gen.manual_seed(31)
    tx, tm = synth.device_tokens(gen, n_news + 1, S, D, dev)
    tx[0] = 0
    tm[0] = 0
    return tx, tm.reshape(n_news + 1, S)


def to_bf16(tx, rows=4096):
    out = torch.empty(tx.shape, dtype=torch.bfloat16, device=tx.device)
    for lo in range(0, tx.shape[0], rows):  # chunked, as NewsStore.astype does it
        out[lo:lo + rows].copy_(tx[lo:lo + rows])
    return out


def spread(v):
    return {"reps": [round(x, 3) for x in v], "median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def step_mode(args, dev):
    w = bench.WORKLOAD
    model, _ = bench.build_model(w, dev)
    tx, tm = table(dev, args.n_news, w["S"], w["D"])
    rng = np.random.default_rng(5)
    z = np.minimum(rng.zipf(1.1, size=(w["B"], w["H"] + w["C"])), args.n_news).astype(np.int32)
    n_hist = rng.integers(1, w["H"] + 1, size=(w["B"], 1))
    z[:, :w["H"]][np.arange(w["H"])[None, :] >= n_hist] = 0  # empty history slots
    ids = torch.from_numpy(z).to(dev)
    hist_ids, cand_ids = ids[:, :w["H"]].contiguous(), ids[:, w["H"]:].contiguous()
    names = [v for v in args.variants.split(",") if v]
    tables = {"fp32": tx}
    if any(v.startswith("bf16") for v in names):
        tables["bf16"] = to_bf16(tx)
    variants = {"fp32": ("fp32", {}), "bf16": ("bf16", dict(XNRS_GEMM_A16="1")), "bf16_a16_off": ("bf16", dict(XNRS_GEMM_A16="0"))}

    def run(v):
        t, _ = variants[v]
        return model.forward_ids(tables[t], tm, hist_ids, cand_ids)

    ms = {v: [] for v in names}
    with torch.no_grad():
        for _ in range(args.reps):
            for v in names:
                with hip.knobs(**variants[v][1]):
                    ms[v].append(bench.timed(lambda: run(v), args.steps, args.warmup, False) / args.steps * 1e3)
        prof, scores = {}, {}
        for v in names:
            with hip.knobs(**variants[v][1]):
                scores[v] = run(v)
                hip.profile_enable(0b1)
                try:
                    run(v)
                    torch.cuda.synchronize()
                    p_ms, p_n, p_fl = hip.profile_read()["qkv_gemm"]
                finally:
                    hip.profile_enable(0)
                prof[v] = {"ms": round(p_ms, 4), "launches": int(p_n), "us_per_launch": round(p_ms * 1e3 / max(p_n, 1), 1),
                           "executed_tf": round(p_fl / (p_ms * 1e-3) / 1e12, 1) if p_ms > 0 else None}
    rec = {"what": "id_path_step_B512", "workload": w, "table_news": args.n_news, "steps": args.steps, "warmup": args.warmup,
           "empty_history_slots": round(float((hist_ids == 0).float().mean().item()), 4),
           "ms_per_step": {v: spread(ms[v]) for v in names},
           "table_bytes_in_hbm": {k: int(t.numel() * t.element_size()) for k, t in tables.items()},
           "qkv_gemm_launch_timer": prof, "tag": args.tag, "note": args.note}
    if "fp32" in scores:
        ref = scores["fp32"]
        rec["max_abs_score_diff_vs_fp32_table"] = {v: float((s - ref).abs().max().item()) for v, s in scores.items() if v != "fp32"}
        rec["max_abs_score"] = float(ref.abs().max().item())
    emit(args.out, rec)


def qkv_mode(args, dev):
    M, N, K, S = 65500, 2304, 768, 50
    tx, _ = table(dev, args.n_news, S, K)
    tb = to_bf16(tx)
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    wgt = torch.randn(N, K, device=dev, generator=gen) / K ** 0.5
    b = torch.randn(N, device=dev, generator=gen)
    ids = torch.from_numpy(np.random.default_rng(5).integers(1, args.n_news + 1, size=M // S).astype(np.int32)).to(dev)
    y = torch.empty(M, N, device=dev)
    l, st = hip.lib(), hip.stream_ptr(dev)
    nws = l.xnrs_linear_bf16_workspace_bytes(N, K)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)

    def f32(mode):
        def fn():
            hip.check(l.xnrs_linear_fwd(hip.ptr(tx), hip.ptr(ids), S, hip.ptr(wgt), hip.ptr(b), hip.ptr(y), M, N, K, 0, st), "linear")
        return mode, fn

    def a16():
        hip.check(l.xnrs_linear_fwd_bf16(hip.ptr(tb), hip.ptr(ids), S, hip.ptr(wgt), hip.ptr(b), hip.ptr(y), M, N, K, 0, hip.ptr(ws), nws, st),
                  "linear_bf16")

    fns = {"gemm_f32_gath": f32(0), "bf16x3": f32(1), "bf16x2": f32(2), "gemm_a16": (None, a16)}
    flops = 2.0 * M * N * K
    us = {k: [] for k in fns}
    prev = hip.get_gemm_mode()
    try:
        for _ in range(args.reps + 1):  # the first round is the warm-up
            for k, (mode, fn) in fns.items():
                if mode is not None:
                    hip.set_gemm_mode(mode)
                for _ in range(3):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us[k].append(e0.elapsed_time(e1) / args.launches * 1e3)
                hip.set_gemm_mode(0)
    finally:
        hip.set_gemm_mode(prev)
    us = {k: v[1:] for k, v in us.items()}
    emit(args.out, {"what": "qkv_product_65500x2304x768_gathered_rows", "launches": args.launches, "table_news": args.n_news,
                    "us_per_launch": {k: spread(v) for k, v in us.items()},
                    "algorithmic_tf": {k: round(flops / (float(np.median(v)) * 1e-6) / 1e12, 1) for k, v in us.items()},
                    "tag": args.tag, "note": args.note})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("step", "qkv"), required=True)
    ap.add_argument("--variants", default="fp32,bf16,bf16_a16_off")
    ap.add_argument("--out", default="")
    ap.add_argument("--tag", default="")
    ap.add_argument("--note", default="")
    ap.add_argument("--n-news", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bf16_table: no GPU visible (a timing without one says nothing)")
    dev = torch.device("cuda", 0)
    with torch.no_grad():
        (step_mode if args.mode == "step" else qkv_mode)(args, dev)


if __name__ == "__main__":
    main()
