"""Input dropout on the id path: what it costs (a tool, not a test; needs a GPU).

    python tools/bench_input_dropout.py --mode kernel --out profiles/input_dropout_bench.json
    python tools/bench_input_dropout.py --mode step --variants ids_dropout,gather_nn_dropout,ids_p0 --out ...

It imports xnrs_amd and bench from the CURRENT DIRECTORY, so both modes also run from a checkout of an earlier commit
(in step mode only the variants that commit can do: gather_nn_dropout, ids_p0).  --out is ONE JSON document, a list of
records: every run reads it, appends its record and writes it back, so the runs of several builds end up in one file.
--tag names the build or the experiment of a record; --note records in words what a run tried (a kernel variant, say).

kernel: xnrs_dropout_rows with ids against xnrs_gather_rows on the same table and ids, in one process, alternating: 64 x 55
        news (the encodes of one NRMS grad step at B = 64: candidates 5, history 25 twice) of 50 x 768 floats.  Algorithmic bytes
        = rows read + rows written; device events around `reps` launches.
step:   the NRMS grad step of bench.make_train_job (scores + MSE, the second history encode + InfoNCE, backward, Adam) at
        B = 64 with the news given as table rows:
          ids_dropout        model.forward_ids / news_encoder.forward_ids with p_dropout = 0.2 (xnrs_dropout_rows + dense path)
          gather_nn_dropout  NewsStore.gather(ids), then forward() with nn.Dropout(0.2): the only way before xnrs_dropout_rows
          ids_p0             the id path with p_dropout = 0 (the gathered-GEMM path this feature does not touch)
        `windows` timed windows of `steps` steps per variant, the variants alternating.
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
from xnrs_amd import hip, synth  # noqa: E402
from xnrs_amd.data import NewsStore  # noqa: E402

P = 0.2


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


def kernel_mode(args, dev):
    w = bench.TRAIN_W
    S, D = w["S"], w["D"]
    n = w["B"] * (w["C"] + 2 * w["H"])
    tx, _ = table(dev, args.n_news, S, D)
    ids = torch.from_numpy(np.random.default_rng(5).integers(1, args.n_news + 1, size=n).astype(np.int32)).to(dev)
    out = torch.empty((n, S, D), dtype=torch.float32, device=dev)
    word = torch.zeros(1, dtype=torch.int64, device=dev)
    st, l = hip.stream_ptr(dev), hip.lib()
    fns = {
        "gather_rows": lambda: hip.check(l.xnrs_gather_rows(hip.ptr(tx), hip.ptr(ids), hip.ptr(out), n, S * D, st), "gather"),
        "dropout_rows": lambda: hip.check(l.xnrs_dropout_rows(hip.ptr(tx), hip.ptr(ids), hip.ptr(out), n, S * D, P, 12345, None, st), "drop"),
        "dropout_rows_seed_word": lambda: hip.check(l.xnrs_dropout_rows(hip.ptr(tx), hip.ptr(ids), hip.ptr(out), n, S * D, P, 12345,
                                                                          hip.ptr(word), st), "drop"),
        "dropout_rows_dense_in_place": lambda: hip.check(l.xnrs_dropout_rows(hip.ptr(out), None, hip.ptr(out), n, S * D, P, 12345, None, st), "drop"),
    }
    nbytes = 2.0 * n * S * D * 4
    res = {k: [] for k in fns}
    for k, fn in fns.items():  # warm-up: code objects loaded
        fn()
    torch.cuda.synchronize()
    for _ in range(args.windows):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[k].append(nbytes / (e0.elapsed_time(e1) / args.reps * 1e-3) / 1e9)
    med = {k: float(np.median(v)) for k, v in res.items()}
    emit(args.out, {"what": "kernel_bandwidth", "rows": n, "row_floats": S * D, "p": P, "table_news": args.n_news, "reps": args.reps,
                    "alg_bytes_per_launch": nbytes, "gbs_windows": {k: [round(x, 1) for x in v] for k, v in res.items()},
                    "gbs_median": {k: round(v, 1) for k, v in med.items()},
                    "ratio_dropout_over_gather": round(med["dropout_rows"] / med["gather_rows"], 4), "tag": args.tag, "note": args.note})


def step_mode(args, dev):
    w = bench.TRAIN_W
    B, H, C, S = w["B"], w["H"], w["C"], w["S"]
    from xnrs_amd.losses import contrastive_loss as infonce
    model, _ = bench.build_model(w, dev, model_name="NRMS")
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4, fused=True)
    tx, tm = table(dev, args.n_news, S, w["D"])
    store = NewsStore(tx, tm, list(range(args.n_news)))
    rng = np.random.default_rng(7)
    hist_np = rng.integers(1, args.n_news + 1, size=(B, H)).astype(np.int32)
    hist_np[np.arange(H)[None, :] >= rng.integers(1, H + 1, size=(B, 1))] = 0  # ragged histories: trailing slots empty
    hist_ids = torch.from_numpy(hist_np).to(dev)
    cand_ids = torch.from_numpy(rng.integers(1, args.n_news + 1, size=(B, C)).astype(np.int32)).to(dev)
    targets = torch.zeros(B, C, 1, device=dev)
    targets[:, 0] = 1.0
    labels = torch.from_numpy(rng.integers(0, 6, size=B)).to(dev)

    def set_p(p):
        model.news_encoder.dropout.p = p
        model.user_encoder.dropout.p = p

    def finish(preds, ue):
        loss = torch.nn.functional.mse_loss(torch.relu(preds), targets) + 0.1 * infonce(ue.reshape(B, -1), labels, 0.08)
        loss.backward()
        opt.step()
        return loss

    def ids_step():
        opt.zero_grad()
        preds = model.forward_ids(tx, tm, hist_ids, cand_ids)
        h, hm = model.news_encoder.forward_ids(tx, tm, hist_ids)  # the reference's second history encode
        return finish(preds, model.user_encoder((h, hm)))

    def gather_step():
        opt.zero_grad()
        batch = {"user_features": {"history": {"title_emb": store.gather(hist_ids, trusted=True)}, "other": {}},
                 "candidate_features": {"title_emb": store.gather(cand_ids, trusted=True)}}
        return finish(model(batch), model.get_user_embeddings(batch))

    variants = {"ids_dropout": (P, ids_step), "gather_nn_dropout": (P, gather_step), "ids_p0": (0.0, ids_step)}
    names = [v for v in args.variants.split(",") if v]
    res = {v: [] for v in names}
    for _ in range(args.windows):
        for v in names:
            p, fn = variants[v]
            set_p(p)
            res[v].append(bench.timed(fn, args.steps, args.warmup, False) / args.steps * 1e3)
    loss = {}
    for v in names:
        p, fn = variants[v]
        set_p(p)
        loss[v] = float(fn().item())
    emit(args.out, {"what": "nrms_grad_step_B64", "p_dropout": P, "steps": args.steps, "warmup": args.warmup, "table_news": args.n_news,
                    "ms_windows": {k: [round(x, 3) for x in v] for k, v in res.items()},
                    "ms_median": {k: round(float(np.median(v)), 3) for k, v in res.items()}, "last_loss": loss, "tag": args.tag, "note": args.note})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernel", "step"), required=True)
    ap.add_argument("--variants", default="ids_dropout,gather_nn_dropout,ids_p0")
    ap.add_argument("--out", default="")
    ap.add_argument("--tag", default="")
    ap.add_argument("--note", default="")
    ap.add_argument("--n-news", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_input_dropout: no GPU visible (a timing without one says nothing)")
    dev = torch.device("cuda", 0)
    (kernel_mode if args.mode == "kernel" else step_mode)(args, dev)


if __name__ == "__main__":
    main()
