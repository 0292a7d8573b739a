#!/usr/bin/env python
"""bench_lstur.py -- LSTUR (config/mind_small_LSTUR.yml's shape: 25 x 50 x 768 tokens, E = 256 + 16, st_hist_len = 25,
n_users = 703 789) with ('embedding', 'con') on the HIP path against an eager-torch restatement of the same model, on the
same weights, in the same process, outputs compared (on the GPU the restatement's nn.GRU is the vendor library's).  Writes
one JSON document (default profiles/lstur_bench.json) and prints it.

    python tools/bench_lstur.py [--reps R] [--warmup W] [--out FILE] [--only inference|grad|grad_hip|gru] [--batch B]

  inference : impressions/s of forward(batch) in eval mode at B = 512
  grad_step : ms of the MSE grad step (relu(model(batch)) -> mse_loss -> backward, training.py:97-113,376-393) at B = 64
              (the config's batch_size) and B = 16; the user table's gradient is a dense (n_users + 1, 136) tensor
  gru_layouts : the GRU alone (ops.gru forward, and forward + backward) at B = 512 and B = 64 under both recurrence
              layouts (XNRS_GRU_LAYOUT=0: one launch per step; 1: one launch, a workgroup owns 32 rows for all steps)
Timing: HIP events around R back-to-back calls after W warm-up calls.  Launch counts come from a separate
`rocprofv3 --kernel-trace --stats` run (--only grad_hip --batch B runs 1 + W + R HIP grad steps and nothing else: two such
runs with different R give the launches per step as the difference of their kernel counts over the difference of R).
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xnrs_amd import hip, ops, synth  # noqa: E402
from xnrs_amd.models.lstur import make_lstur  # noqa: E402

DEV = torch.device("cuda", 0)
TOL_S, TOL_G = 1e-4, 2e-4  # the project's bars (scores, gradients): a timing whose outputs are further apart is not reported as ok
SHAPE = dict(H=25, st=25, C=5, S=50, D=768, Et=256, Ec=16, n_users=703789, ltm="embedding", lstm="con")


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


def eager_lstur(model, batch):
    """The LSTUR forward (lstur.py:18-45,118-154,191-207; layers.py:47-69) restated in stock torch ops on the HIP model's
    parameters, ('embedding', 'con'); the lengths stay on the device until pack_padded_sequence needs them on the host."""
    ne, ue = model.news_encoder, model.user_encoder

    def news(feats, cat):
        x, m = feats
        b, n, s, d = x.shape
        x, m = x.reshape(b * n, s, d), m.reshape(b * n, s, 1)
        p = ne.title_encoder.pooler
        a = torch.exp(F.linear(torch.tanh(F.linear(x, p.fc1.weight, p.fc1.bias)), p.fc2.weight, p.fc2.bias)) * m
        a = a / (a.sum(1, keepdim=True) + 1e-8)
        v = torch.bmm(a.transpose(1, 2), x)
        hd = ne.title_encoder.head
        v = F.linear(torch.relu(F.linear(v, hd[0].weight, hd[0].bias)), hd[2].weight, hd[2].bias).reshape(b, n, -1)
        return torch.cat([v, F.embedding(cat.long(), ne.cat_embedder.weight)], 2), m.reshape(b, n, s).sum(2).clamp(0, 1)

    h, hm = news(batch["user_features"]["history"]["title_emb"], batch["user_features"]["history"]["category_index"])
    c, _ = news(batch["candidate_features"]["title_emb"], batch["candidate_features"]["category_index"])
    u_lt = F.embedding(batch["user_features"]["other"]["user_index"].long(), ue.long_term_encoder.weight, padding_idx=0).squeeze(1)
    st = model.cfg.st_hist_len
    packed = torch.nn.utils.rnn.pack_padded_sequence(h[:, :st], lengths=hm[:, :st].sum(1).cpu(), batch_first=True, enforce_sorted=False)
    _, u_st = ue.gru(packed)
    u = torch.cat((u_st.squeeze(0), u_lt), 1).unsqueeze(1)
    return torch.bmm(c, u.transpose(1, 2))  # DotScoring (scoring.py:23)


def make(B, seed=0):
    c = SHAPE
    cfg = Cfg(model="LSTUR", scoring="dot", long_term_method=c["ltm"], long_short_term_method=c["lstm"], n_users=c["n_users"],
              d_backbone=c["D"], title_emb_dim=c["Et"], cat_emb_dim=c["Ec"], total_emb_dim=c["Et"] + c["Ec"], n_categories=19,
              n_subcategories=264, p_dropout=0.0, p_user_dropout=0.0, bias=False, hist_len=c["H"], st_hist_len=c["st"],
              seq_len=c["S"], catg_features=["category_index"])
    torch.manual_seed(seed)
    model = make_lstur(cfg).to(DEV)
    batch = synth.make_batch(seed + 1, B, c["H"], c["C"], c["S"], c["D"], min_len=5, n_categories=19)
    g = torch.Generator().manual_seed(seed + 2)
    batch["user_features"]["other"] = {"user_index": torch.randint(0, c["n_users"] + 1, (B, 1), generator=g, dtype=torch.int32)}
    return model, synth.batch_to(batch, DEV)


def inference(B, reps, warmup):
    model, batch = make(B)
    model.eval()
    with torch.no_grad():
        r_hip, r_eager = model(batch), eager_lstur(model, batch)
        err = ((r_hip - r_eager).abs().max() / r_eager.abs().max()).item()
        ms_hip = timed(lambda: model(batch), reps, warmup)
        ms_eager = timed(lambda: eager_lstur(model, batch), reps, warmup)
    return dict(B=B, hip_ms=ms_hip, eager_ms=ms_eager, hip_impressions_per_s=B / ms_hip * 1e3,
                eager_impressions_per_s=B / ms_eager * 1e3, speedup=ms_eager / ms_hip, max_rel_diff=err, outputs_ok=err <= TOL_S)


def _params(model):
    return [p for k, p in model.named_parameters() if not k.endswith("dummy_param")]


def grad_step(B, reps, warmup):
    model, batch = make(B)
    model.train()
    params = _params(model)

    def step(fwd):
        for p in params:
            p.grad = None
        loss = F.mse_loss(torch.relu(fwd(batch)), batch["targets"])
        loss.backward()
        return loss

    l_hip = step(model).item()
    g_hip = [p.grad.clone() for p in params]
    l_eager = step(lambda b: eager_lstur(model, b)).item()
    # every gradient against max(its own scale, 1e-3 of the largest), as the tests scale them
    gmax = max(p.grad.abs().max().item() for p in params)
    g_err = max(((a - p.grad).abs().max().item() / max(p.grad.abs().max().item(), 1e-3 * gmax)) for a, p in zip(g_hip, params))
    del g_hip
    ms_hip = timed(lambda: step(model), reps, warmup)
    ms_eager = timed(lambda: step(lambda b: eager_lstur(model, b)), reps, warmup)
    return dict(B=B, hip_ms=ms_hip, eager_ms=ms_eager, speedup=ms_eager / ms_hip, loss_hip=l_hip, loss_eager=l_eager,
                max_rel_grad_diff=g_err, outputs_ok=g_err <= TOL_G and abs(l_hip - l_eager) <= TOL_S * abs(l_eager))


def grad_step_hip_only(B, reps, warmup):
    model, batch = make(B)
    model.train()
    params = _params(model)

    def step():
        for p in params:
            p.grad = None
        F.mse_loss(torch.relu(model(batch)), batch["targets"]).backward()

    return dict(B=B, steps=1 + warmup + reps, hip_ms=timed(step, reps, warmup + 1))


def gru_layouts(reps, warmup):
    """The GRU alone under both recurrence layouts, and the vendor library's nn.GRU on full-length rows beside them."""
    c = SHAPE
    E, Hd, T = c["Et"] + c["Ec"], (c["Et"] + c["Ec"]) // 2, c["st"]
    torch.manual_seed(0)
    gru = torch.nn.GRU(E, Hd, batch_first=True).to(DEV)
    rows = []
    for B in (512, 64):
        x = torch.randn(B, T, E, device=DEV)
        m = torch.ones(B, T, 1, device=DEV)
        dy = torch.randn(B, Hd, device=DEV)
        row = dict(B=B)

        def fwd_bwd(f):
            xg = x.clone().requires_grad_(True)
            gru.zero_grad(set_to_none=True)
            f(xg).backward(dy)

        for layout in ("0", "1"):
            with hip.knobs(XNRS_GRU_LAYOUT=layout):
                with torch.no_grad():
                    row[f"hip_layout{layout}_fwd_ms"] = timed(lambda: ops.gru(x, m, None, gru), reps, warmup)
                row[f"hip_layout{layout}_fwd_bwd_ms"] = timed(lambda: fwd_bwd(lambda xg: ops.gru(xg, m, None, gru)), reps, warmup)
        with torch.no_grad():
            row["vendor_fwd_ms"] = timed(lambda: gru(x), reps, warmup)
        row["vendor_fwd_bwd_ms"] = timed(lambda: fwd_bwd(lambda xg: gru(xg)[1][0]), reps, warmup)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstur_bench.json"))
    ap.add_argument("--only", default="", help="inference | grad | grad_hip | gru (profiling runs; no file written)")
    ap.add_argument("--batch", type=int, default=64, help="batch of --only grad_hip")
    a = ap.parse_args()
    out = dict(shape=SHAPE, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(DEV))
    if a.only in ("", "inference"):
        out["inference"] = inference(512, a.reps, a.warmup)
    if a.only in ("", "grad"):
        out["grad_step"] = [grad_step(B, a.reps, a.warmup) for B in (64, 16)]
    if a.only in ("", "gru"):
        out["gru_layouts"] = gru_layouts(a.reps, a.warmup)
    if a.only == "grad_hip":
        out["grad_step_hip"] = grad_step_hip_only(a.batch, a.reps, a.warmup)
    text = json.dumps(out, indent=1)
    if a.out and not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    bad = [r for r in [out.get("inference")] + out.get("grad_step", []) if r and not r["outputs_ok"]]
    if bad:
        sys.exit(f"HIP and eager outputs differ beyond the {TOL_S:g} / {TOL_G:g} bars: {bad}")


if __name__ == "__main__":
    main()
