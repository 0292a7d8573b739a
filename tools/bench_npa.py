#!/usr/bin/env python
"""bench_npa.py -- NPA (config/mind_small_NPA.yml: 50 x 768 tokens, nh = 25, nc = 5, du = 64, E = 256, n_users = 703 789) on
the HIP path against an eager-torch restatement of the same model, on the same weights, in the same process, outputs
compared.  Writes one JSON document (default profiles/npa_bench.json) and prints it.

    python tools/bench_npa.py [--reps R] [--warmup W] [--out FILE] [--only inference|grad|grad_hip] [--batch B]

  inference : impressions/s of forward(batch) in eval mode at B = 512
  grad_step : ms of the MSE grad step (relu(model(batch)) -> mse_loss -> backward, training.py:97-113,376-393) at B = 64
              (the config's batch_size) and B = 16; the user table's gradient is a dense (n_users + 1, 64) tensor
  x_fc GEMM : FLOP and bytes from the shapes, and the share of the fp32 matrix peak (157.3 TF) that the GEMM's FLOP would
              take at the measured step time
Timing: HIP events around R back-to-back calls after W warm-up calls.  Launch counts and per-kernel times come from a
separate `rocprofv3 --kernel-trace --stats` run of this script (--only keeps that run short and writes no file;
--only grad_hip --batch B runs 1 + W + R HIP grad steps at batch B and nothing else: two such runs with different R give
the launches per step as the difference of their kernel counts over the difference of R).
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xnrs_amd import synth  # noqa: E402
from xnrs_amd.models.npa import make_npa  # noqa: E402

DEV = torch.device("cuda", 0)
PEAK_F32 = 157.3e12
SHAPE = dict(H=25, C=5, S=50, D=768, E=256, du=64, A=128, n_users=703789)


class Cfg(dict):
    __getattr__ = dict.__getitem__


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def eager_npa(model, batch):
    """The NPA forward (npa.py:34-89, layers.py:79-102) restated in stock torch ops on the HIP model's parameters."""
    def pa(mod, q, x, m):
        xa = torch.tanh(F.linear(x, mod.x_fc.weight, mod.x_fc.bias))
        q = F.linear(q, mod.q_fc.weight, mod.q_fc.bias)
        a = torch.exp(torch.bmm(xa, q.transpose(1, 2))) * m
        a = a / (a.sum(1, keepdim=True) + 1e-8)
        return torch.bmm(a.transpose(1, 2), x)

    def head(p):
        h = model.news_head
        return F.linear(torch.relu(F.linear(p, h[0].weight, h[0].bias)), h[2].weight, h[2].bias)

    h, hm = batch["user_features"]["history"]["title_emb"]
    c, cm = batch["candidate_features"]["title_emb"]
    ue = F.embedding(batch["user_features"]["other"]["user_index"].long(), model.user_embedder.weight)  # (B,1,du)
    b, nh, s, d = h.shape
    hv = head(pa(model.title_pooler, ue.repeat_interleave(nh, 0), h.reshape(b * nh, s, d), hm.reshape(b * nh, s, 1)))
    u = pa(model.user_encoder, ue, hv.reshape(b, nh, -1), hm.sum(2).clamp(0, 1))
    nc = c.shape[1]
    cv = head(pa(model.title_pooler, ue.repeat_interleave(nc, 0), c.reshape(b * nc, s, d), cm.reshape(b * nc, s, 1)))
    return torch.bmm(cv.reshape(b, nc, -1), u.transpose(1, 2))  # DotScoring (scoring.py:23)


def make(B, seed=0):
    c = SHAPE
    cfg = Cfg(model="NPA", scoring="dot", n_users=c["n_users"], user_emb_dim=c["du"], d_backbone=c["D"], title_emb_dim=c["E"],
              total_emb_dim=c["E"], p_dropout=0.0, bias=False)
    torch.manual_seed(seed)
    model = make_npa(cfg).to(DEV)
    batch = synth.make_batch(seed + 1, B, c["H"], c["C"], c["S"], c["D"], min_len=5)
    g = torch.Generator().manual_seed(seed + 2)
    batch["user_features"]["other"] = {"user_index": torch.randint(0, c["n_users"] + 1, (B, 1), generator=g, dtype=torch.int32)}
    return model, synth.batch_to(batch, DEV)


def x_fc_cost(B, ms):
    c = SHAPE
    rows = B * (c["H"] + c["C"]) * c["S"]
    flop = 2.0 * rows * c["A"] * c["D"]
    return dict(rows=rows, flop=flop, bytes=4.0 * (rows * c["D"] + rows * c["A"] + c["A"] * c["D"]),
                share_of_peak_at_step_time=flop / (ms * 1e-3) / PEAK_F32)


def inference(B, reps, warmup):
    model, batch = make(B)
    model.eval()
    with torch.no_grad():
        r_hip, r_eager = model(batch), eager_npa(model, batch)
        err = ((r_hip - r_eager).abs().max() / r_eager.abs().max()).item()
        ms_hip = timed(lambda: model(batch), reps, warmup)
        ms_eager = timed(lambda: eager_npa(model, batch), reps, warmup)
    return dict(B=B, hip_ms=ms_hip, eager_ms=ms_eager, hip_impressions_per_s=B / ms_hip * 1e3,
                eager_impressions_per_s=B / ms_eager * 1e3, speedup=ms_eager / ms_hip, max_rel_diff=err,
                x_fc_gemm=x_fc_cost(B, ms_hip))


def grad_step(B, reps, warmup):
    model, batch = make(B)
    model.train()
    params = list(model.parameters())

    def step(fwd):
        for p in params:
            p.grad = None
        loss = F.mse_loss(torch.relu(fwd(batch)), batch["targets"])
        loss.backward()
        return loss

    l_hip = step(model).item()
    g_hip = [p.grad.clone() for p in params]
    l_eager = step(lambda b: eager_npa(model, b)).item()
    g_err = max(((a - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-30)).item() for a, p in zip(g_hip, params))
    del g_hip
    ms_hip = timed(lambda: step(model), reps, warmup)
    ms_eager = timed(lambda: step(lambda b: eager_npa(model, b)), reps, warmup)
    return dict(B=B, hip_ms=ms_hip, eager_ms=ms_eager, speedup=ms_eager / ms_hip, loss_hip=l_hip, loss_eager=l_eager,
                max_rel_grad_diff=g_err, x_fc_gemm=x_fc_cost(B, ms_hip))


def grad_step_hip_only(B, reps, warmup):
    model, batch = make(B)
    model.train()
    params = list(model.parameters())

    def step():
        for p in params:
            p.grad = None
        F.mse_loss(torch.relu(model(batch)), batch["targets"]).backward()

    return dict(B=B, steps=1 + warmup + reps, hip_ms=timed(step, reps, warmup + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "npa_bench.json"))
    ap.add_argument("--only", default="", help="inference | grad | grad_hip (profiling runs; no file written)")
    ap.add_argument("--batch", type=int, default=64, help="batch of --only grad_hip")
    a = ap.parse_args()
    out = dict(shape=SHAPE, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(DEV))
    if a.only in ("", "inference"):
        out["inference"] = inference(512, a.reps, a.warmup)
    if a.only in ("", "grad"):
        out["grad_step"] = [grad_step(B, a.reps, a.warmup) for B in (64, 16)]
    if a.only == "grad_hip":
        out["grad_step_hip"] = grad_step_hip_only(a.batch, a.reps, a.warmup)
    text = json.dumps(out, indent=1)
    if a.out and not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
