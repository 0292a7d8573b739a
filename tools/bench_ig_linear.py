"""Integrated gradients with ONE Q|K|V projection against the batched path, at the shapes of
bench.py::ig_step_extra: NRMS, one impression, H = 9 and 25 history news, S = 50, D = 768, 16 heads, n_steps = 100.

    python tools/bench_ig_linear.py [--out profiles/ig_linear_bench.json]        # the timings (profiler off)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_ig_linear.py --trace-run --H 25
    python tools/bench_ig_linear.py --summarize DIR --H 25 [--out profiles/ig_linear_trace_H25_summary.txt]

Timings: both paths are warmed, then run ALTERNATELY in one process -- `rounds` rounds of one window per path, `window`
explanations per window, a host clock around work that ends in a device synchronise (every explanation reads its score on
the host anyway).  Per path the mean over the windows and their spread (min / max window).  Also: explain_rows for C = 10
rows with the shared forward against ten single-row calls, and torch.cuda.max_memory_allocated of one explanation per path.

Kernel times come from a rocprofv3 run OF ITS OWN (--trace-run: `calls` explanations of the one-projection path and nothing
else); --summarize reads its kernel_stats.csv.  The bytes of the two streaming kernels are computed here from the shapes:
expand reads rows x W floats and writes n x rows x W, reduce reads n x rows x W and writes rows x W (W = 3 D)."""
import argparse
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_STEPS = 100
HBM_PEAK_TBS = 8.0        # MI355X_MICROARCH: HBM3E peak (spec); a float4 copy reaches 6.29
HBM_COPY_TBS = 6.29


def shape(H):
    return dict(B=1, H=H, C=1, S=50, D=768, h=16, E=256, A=256)


def stream_bytes(H, n=N_STEPS, S=50, D=768):
    """Bytes each of the two kernels moves for one explanation in one chunk (fp32)."""
    image = H * S * 3 * D * 4
    return dict(expand=image * (n + 1), reduce=image * (n + 1), image=image)


def setup(H, device):
    import torch
    import bench
    w = shape(H)
    model, _ = bench.build_model(w, device, model_name="NRMS")
    (hx, hm), (cx, cm) = bench.make_inputs(w, device, seed=50 + H, full_history=True)
    return model, (hx, hm, cx, cm)


def window(fn, count):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / count * 1e3


def ab(fns, rounds, count):
    """fns: {name: callable}; alternating windows -> {name: {ms_mean, ms_min, ms_max, windows}}."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(window(fn, count))
    return {k: dict(ms_mean=sum(v) / len(v), ms_min=min(v), ms_max=max(v), windows=v) for k, v in ms.items()}


def peak_memory(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return dict(peak_bytes=torch.cuda.max_memory_allocated(), resident_before_bytes=base)


def store_for(H, device, n_rows=64):
    import torch
    from xnrs_amd import synth
    from xnrs_amd.data import NewsStore
    gen = torch.Generator(device=device).manual_seed(77)
    x, m = synth.device_tokens(gen, n_rows, 50, 768, device)
    x[0], m[0] = 0, 0
    store = NewsStore(x, m.reshape(n_rows, 50), list(range(n_rows - 1)))
    hist = torch.arange(1, H + 1, dtype=torch.int32, device=device)
    cand = torch.arange(H + 1, H + 11, dtype=torch.int32, device=device)
    return store, hist, cand


def run_timings(args):
    import torch
    from xnrs_amd import hip
    from xnrs_amd.explain import explain_rows, integrated_gradients
    device = "cuda:0"
    out = {"what": "one explanation = 100 interpolation steps of one impression (NRMS, S=50, D=768, 16 heads); ms per explanation, "
                   "host clock around synchronised work, paths alternated in one process",
           "rounds": args.rounds, "explanations_per_window": args.window, "n_steps": N_STEPS, "device": torch.cuda.get_device_name(0)}
    for H in (9, 25):
        model, a = setup(H, device)
        fns = {"batched": lambda: integrated_gradients(model, *a, n_steps=N_STEPS),
               "projection_once": lambda: integrated_gradients(model, *a, n_steps=N_STEPS, projection_once=True)}
        r = ab(fns, args.rounds, args.window)
        for k in r:
            r[k]["it_per_s"] = N_STEPS / r[k]["ms_mean"] * 1e3
            r[k]["memory"] = peak_memory(fns[k])
        # the agreement of the two paths on the raw score (activation=None): the ReLU of the timed calls cuts some impressions'
        # scores to 0, and then every gradient is zero and a comparison says nothing (the kernels run all the same)
        x = integrated_gradients(model, *a, n_steps=N_STEPS, activation=None)["int_grads"]
        y = integrated_gradients(model, *a, n_steps=N_STEPS, activation=None, projection_once=True)["int_grads"]
        r["int_grads_scale"] = x.abs().max().item()
        r["max_abs_difference_over_scale"] = ((x - y).abs().max() / x.abs().max().clamp_min(1e-30)).item()
        r["stream_bytes"] = stream_bytes(H)
        l = hip.lib()
        nsaved = l.xnrs_seq_encoder_saved_bytes(N_STEPS * H, 50, 768, 256, 256, 16, hip.POOL_ADDITIVE, 1)
        r["saved_blob_bytes"] = int(nsaved)
        r["saved_blob_unused_image_bytes"] = stream_bytes(H)["image"] * N_STEPS  # the own Q|K|V region the node never fills
        store, hist, cand = store_for(H, device)
        rows = {"shared_forward_C10": lambda: explain_rows(model, store, hist, cand, n_steps=N_STEPS),
                "ten_single_calls": lambda: [explain_rows(model, store, hist, cand[j:j + 1], n_steps=N_STEPS) for j in range(10)]}
        r["explain_rows_C10"] = ab(rows, args.rounds, max(2, args.window // 10))
        out[f"NRMS_H{H}"] = r
        del model, a, store
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: {p: round(v[p]["ms_mean"], 3) for p in ("batched", "projection_once")}
                      for k, v in out.items() if k.startswith("NRMS")}))


def run_trace(args):
    import torch
    from xnrs_amd.explain import integrated_gradients
    model, a = setup(args.H, "cuda:0")
    for _ in range(args.calls):
        integrated_gradients(model, *a, n_steps=N_STEPS, projection_once=True)
    torch.cuda.synchronize()


def summarize(args):
    import csv
    files = sorted(glob.glob(os.path.join(args.summarize, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {args.summarize}")
    rows = list(csv.DictReader(open(files[-1])))
    calls = args.calls
    b = stream_bytes(args.H)
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    lines = [f"# rocprofv3 --kernel-trace --stats -- python tools/bench_ig_linear.py --trace-run --H {args.H} --calls {calls}  (MI355X)",
             f"# {calls} explanations of the one-projection path (NRMS, H={args.H}, S=50, D=768, n_steps=100, one chunk); kernel time per explanation",
             f"{'kernel':<72} {'calls/expl':>10} {'us/expl':>10} {'share':>7}"]
    new = {}
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        name, ns, cnt = r["Name"], float(r["TotalDurationNs"]), int(r["Calls"])
        lines.append(f"{name[:72]:<72} {cnt / calls:>10.1f} {ns / calls / 1e3:>10.1f} {100 * ns / total:>6.1f}%")
        for key in ("ig_expand", "ig_reduce"):
            if key in name and "Vec4" in name:
                new[key] = ns / cnt
    lines.append(f"all kernels: {total / calls / 1e3:.1f} us per explanation")
    for key, ns in new.items():
        tbs = b[key.split('_')[1]] / ns / 1e3
        lines.append(f"{key}: {ns / 1e3:.1f} us per launch, {b[key.split('_')[1]] / 1e9:.3f} GB from the shapes -> {tbs:.2f} TB/s = "
                     f"{100 * tbs / HBM_PEAK_TBS:.0f} % of the {HBM_PEAK_TBS} TB/s HBM peak ({100 * tbs / HBM_COPY_TBS:.0f} % of the "
                     f"{HBM_COPY_TBS} TB/s a float4 copy reaches)")
    rest = total / calls - sum(new.values())
    lines.append(f"what remains (attention core, pooling, heads, user tower, scorer, their backwards, the two one-off products): "
                 f"{rest / 1e3:.1f} us per explanation = {rest / 1e3 / N_STEPS:.2f} us per step")
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--H", type=int, default=25)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args)
    if args.trace_run:
        return run_trace(args)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "ig_linear_bench.json")
    run_timings(args)


if __name__ == "__main__":
    main()
