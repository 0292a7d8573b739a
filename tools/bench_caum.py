#!/usr/bin/env python
"""bench_caum.py -- CAUM on the HIP path against the same equations in plain torch ops on the same device and weights
(written from the formulas of DESIGN.md section 10c), outputs compared.  Two shapes: the training step's
(B = 64, C = 5, H = 25, S = 50, D = 768, Et = 256, Ec = 16, 16 heads: attention length L = B * C = 320) and an
evaluation-like one (B = 256, C = 20: L = 5120).  Writes one JSON line per measurement to profiles/caum_bench_lines.json
and prints them.

    python tools/bench_caum.py [--reps R] [--warmup W] [--out FILE] [--shapes train,eval]

  inference   ms per forward(batch) in eval mode
  grad_step   ms per MSE grad step (relu(model(batch)) -> mse_loss -> backward); training shape only
  stages      the launch timer's per-stage split of ONE step (xnrs_profile_enable / xnrs_profile_read)
  attn_long   the long-attention kernels alone on a random Q|K|V image of the tower's shape: ms and achieved TFLOP/s
              (4 L^2 E Nb flops forward, 10 L^2 E Nb backward: two products forward, five backward)
Timing: HIP events around R back-to-back calls after W warm-up calls.
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
from xnrs_amd.models.caum import make_caum  # noqa: E402

DEV = torch.device("cuda", 0)
TOL_S, TOL_G = 1e-4, 2e-4
SHAPES = {"train": dict(B=64, C=5), "eval": dict(B=256, C=20)}
COMMON = dict(H=25, S=50, D=768, Et=256, Ec=16, heads=16)


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


def torch_caum(model, batch):
    """The model in plain torch ops on the HIP model's parameters: news encoder (self-attention with the query-row mask,
    additive pooling, head, category encoder), then steps 1-7 of DESIGN.md section 10c as written there."""
    ne, ue = model.news_encoder, model.user_encoder
    te = ne.title_encoder

    def news(feats):
        x, m = feats["title_emb"]
        b, n, s, d = x.shape
        x, m = x.reshape(b * n, s, d), m.reshape(b * n, s, 1)
        att = te.att
        hd, dk = att.h, att.d_k
        q, k, v = (F.linear(x, l.weight, l.bias).reshape(b * n, s, hd, dk).transpose(1, 2)
                   for l in (att.q_linear, att.k_linear, att.v_linear))
        sc = (q @ k.transpose(-1, -2)) / dk ** 0.5
        sc = sc.masked_fill(m.reshape(b * n, 1, s, 1) == 0, -1e9)
        y = F.linear((torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(b * n, s, d), att.out.weight, att.out.bias)
        p = te.pooler
        a = torch.exp(F.linear(torch.tanh(F.linear(y, p.fc1.weight, p.fc1.bias)), p.fc2.weight, p.fc2.bias)) * m
        a = a / (a.sum(1, keepdim=True) + 1e-8)
        t = torch.bmm(a.transpose(1, 2), y)
        t = F.linear(torch.relu(F.linear(t, te.head[0].weight, te.head[0].bias)), te.head[2].weight, te.head[2].bias)
        ce = ne.cat_embedder
        cat = torch.relu(F.linear(F.embedding(feats["category_index"].long(), ce.embedding.weight), ce.linear.weight, ce.linear.bias))
        return torch.cat([t.reshape(b, n, -1), cat], 2)

    h, c = news(batch["user_features"]["history"]), news(batch["candidate_features"])
    B, H, E = h.shape
    C = c.shape[1]
    hr = h[:, None].expand(B, C, H, E)
    cr = c[:, :, None].expand(B, C, H, E)
    h_cnn = F.linear(torch.cat([hr.roll(1, 2), hr, hr.roll(-1, 2), cr], -1), ue.linear1.weight, ue.linear1.bias)
    z = F.linear(torch.cat([cr, hr], -1), ue.linear2.weight, ue.linear2.bias).reshape(B * C, H, E)
    mha = ue.multihead_attention
    nh, dk = mha.num_heads, E // mha.num_heads
    q, k, v = (t.reshape(B * C, H, nh, dk).permute(1, 2, 0, 3) for t in F.linear(z, mha.in_proj_weight, mha.in_proj_bias).split(E, -1))
    o = F.scaled_dot_product_attention(q, k, v).permute(2, 0, 1, 3).reshape(B, C, H, E)   # attended axis: B*C
    h_att = F.linear(o, mha.out_proj.weight, mha.out_proj.bias)
    h_all = F.linear(torch.cat([h_cnn, h_att], -1), ue.linear3.weight, ue.linear3.bias)
    da = ue.dense_att
    s = F.linear(torch.tanh(F.linear(torch.tanh(F.linear(torch.cat([h_all, cr], -1), da.linear.weight, da.linear.bias)),
                                     da.linear2.weight, da.linear2.bias)), da.linear3.weight, da.linear3.bias)
    u = (torch.softmax(s, 2) * h_all).sum(2)
    return (u * c).sum(-1, keepdim=True)


def make(shape, seed=0):
    c = dict(COMMON, **SHAPES[shape])
    cfg = Cfg(model="CAUM", scoring="CAUMScoring", n_heads=c["heads"], d_backbone=c["D"], title_emb_dim=c["Et"],
              cat_emb_dim=c["Ec"], total_emb_dim=c["Et"] + c["Ec"], n_categories=19, n_subcategories=264, p_dropout=0.0,
              bias=False, catg_features=["category_index"])
    torch.manual_seed(seed)
    model = make_caum(cfg).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(seed + 1)

    def side(n):
        x, m = synth.device_tokens(gen, c["B"] * n, c["S"], c["D"], DEV)
        return {"title_emb": (x.reshape(c["B"], n, c["S"], c["D"]), m.reshape(c["B"], n, c["S"], 1)),
                "category_index": torch.randint(1, 20, (c["B"], n), generator=gen, device=DEV, dtype=torch.int32)}

    targets = torch.zeros(c["B"], c["C"], 1, device=DEV)
    targets[:, 0] = 1
    return c, model, {"user_features": {"history": side(c["H"]), "other": {}}, "candidate_features": side(c["C"]), "targets": targets}


def stages(fn):
    hip.profile_enable(hip.PROFILE_ALL)
    try:
        fn()
        rec = hip.profile_read()
    finally:
        hip.profile_enable(0)
    return {k: dict(ms=round(ms, 4), launches=n, tflops=(fl / ms / 1e9 if ms > 0 else 0.0)) for k, (ms, n, fl) in rec.items() if n}


def inference(shape, reps, warmup):
    c, model, batch = make(shape)
    model.eval()
    with torch.no_grad():
        r_hip, r_t = model(batch), torch_caum(model, batch)
        err = ((r_hip - r_t).abs().max() / r_t.abs().max()).item()
        row = dict(kind="inference", shape=shape, **c, L=c["B"] * c["C"], hip_ms=timed(lambda: model(batch), reps, warmup),
                   torch_ms=timed(lambda: torch_caum(model, batch), reps, warmup), max_rel_diff=err, outputs_ok=err <= TOL_S)
        row["speedup"] = row["torch_ms"] / row["hip_ms"]
        row["stages"] = stages(lambda: model(batch))
    return row


def grad_step(shape, reps, warmup):
    c, model, batch = make(shape)
    model.eval()  # (attention-probability dropout of the news encoder off on both sides: the two draws cannot be matched)
    params = [p for k, p in model.named_parameters() if not k.endswith("dummy_param")]

    def step(fwd):
        for p in params:
            p.grad = None
        loss = F.mse_loss(torch.relu(fwd(batch)), batch["targets"])
        loss.backward()
        return loss

    l_hip = step(model).item()
    g_hip = [p.grad.clone() for p in params]
    l_t = step(lambda b: torch_caum(model, b)).item()
    gmax = max(p.grad.abs().max().item() for p in params)
    g_err = max(((a - p.grad).abs().max().item() / max(p.grad.abs().max().item(), 1e-3 * gmax)) for a, p in zip(g_hip, params))
    del g_hip
    row = dict(kind="grad_step", shape=shape, **c, L=c["B"] * c["C"], hip_ms=timed(lambda: step(model), reps, warmup),
               torch_ms=timed(lambda: step(lambda b: torch_caum(model, b)), reps, warmup), loss_hip=l_hip, loss_torch=l_t,
               max_rel_grad_diff=g_err, outputs_ok=g_err <= TOL_G and abs(l_hip - l_t) <= TOL_S * abs(l_t))
    row["speedup"] = row["torch_ms"] / row["hip_ms"]
    row["stages"] = stages(lambda: step(model))
    return row


def attn_alone(shape, reps, warmup):
    c = dict(COMMON, **SHAPES[shape])
    L, Nb, E = c["B"] * c["C"], c["H"], c["Et"] + c["Ec"]
    qkv = torch.randn(L, Nb, 3 * E, device=DEV)
    d_o = torch.randn(L, Nb, E, device=DEV)
    with torch.no_grad():
        fwd_ms = timed(lambda: ops.attn_long(qkv, c["heads"]), reps, warmup)
    qg = qkv.clone().requires_grad_(True)

    def fb():
        qg.grad = None
        ops.attn_long(qg, c["heads"]).backward(d_o)

    fb_ms = timed(fb, reps, warmup)
    f_fl, b_fl = 4.0 * L * L * E * Nb, 10.0 * L * L * E * Nb
    return dict(kind="attn_long", shape=shape, L=L, Nb=Nb, E=E, heads=c["heads"], d_k=E // c["heads"], fwd_ms=fwd_ms,
                fwd_tflops=f_fl / fwd_ms / 1e9, fwd_bwd_ms=fb_ms, bwd_tflops=b_fl / max(fb_ms - fwd_ms, 1e-9) / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="train,eval")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "caum_bench_lines.json"))
    a = ap.parse_args()
    rows = []
    for shape in a.shapes.split(","):
        rows.append(attn_alone(shape, a.reps, a.warmup))
        rows.append(inference(shape, a.reps, a.warmup))
        if shape == "train":
            rows.append(grad_step(shape, a.reps, a.warmup))
        else:
            rows.append(dict(kind="grad_step", shape=shape, unmeasured="the grad step is measured at the training shape only"))
        torch.cuda.empty_cache()
        hip.release_workspaces()
    for r in rows:
        r.update(device=torch.cuda.get_device_name(DEV), reps=a.reps, warmup=a.warmup)
    text = "\n".join(json.dumps(r) for r in rows)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    bad = [r for r in rows if r.get("outputs_ok") is False]
    if bad:
        sys.exit(f"HIP and torch outputs differ beyond the {TOL_S:g} / {TOL_G:g} bars: {[(r['kind'], r['shape']) for r in bad]}")


if __name__ == "__main__":
    main()
