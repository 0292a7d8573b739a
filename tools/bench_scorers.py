#!/usr/bin/env python
"""bench_scorers.py -- what the scorer choice (cfg.scoring 'dot' / 'bilin' / 'fc') costs on the HIP path, one JSON line.

    python tools/bench_scorers.py [--reps R] [--warmup W] [--out FILE]

All numbers come from one process, after warm-up, timed with HIP events around work on the current stream:
  inference   : impressions/s of the bench workload (NRMS, B=512, H=50, C=5, S=50, D=768, 16 heads, E=256: bench.py's
                step, eval mode) per scorer
  grad_step   : ms of the reference's train step (relu scores -> MSE + 0.1 InfoNCE over get_user_embeddings, backward)
                for StandardRec at B=16 / 64 and NRMS at B=64 (H=50, C=5, S=50, D=768) per scorer
  scorer      : the scorer alone at B=512, N=5, E=256: forward and forward+backward us, HIP against the same arithmetic
                written in stock torch ops (the reference's form) on the same device tensors
  eval_epoch  : seconds of xnrs_amd.evaluation.evaluate on a synth.click_world store per scorer
  launches    : library kernels per scorer call (forward, backward, input-gradient-only backward), counted with
                torch.profiler (all_device_kernels adds torch's own gradient accumulation into .grad)
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xnrs_amd import synth  # noqa: E402
from xnrs_amd.losses import contrastive_loss  # noqa: E402
from xnrs_amd.models import make_model  # noqa: E402
from xnrs_amd.models.blocks import BilinScoring, DotScoring, FCScoring  # noqa: E402

DEV = torch.device("cuda", 0)
SCORERS = ("dot", "bilin", "fc")


class Cfg(dict):
    __getattr__ = dict.__getitem__


def timed(fn, reps, warmup):
    """ms per call: HIP events around `reps` back-to-back calls after `warmup` calls."""
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


def model_for(model, scoring, E=256, D=768, S=50, H=50, bias=False):
    cfg = Cfg(synth.model_cfg(dict(model=model, E=E, bias=bias, h=16, D=D, H=H, S=S)))
    torch.manual_seed(0)
    return make_model(Cfg(dict(cfg, scoring=scoring))).to(DEV)


def inference(reps, warmup):
    B, H, C, S, D = 512, 50, 5, 50, 768
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    hx, hm = synth.device_tokens(gen, B * H, S, D, DEV)
    cx, cm = synth.device_tokens(gen, B * C, S, D, DEV)
    hist = (hx.reshape(B, H, S, D), hm.reshape(B, H, S, 1))
    cand = (cx.reshape(B, C, S, D), cm.reshape(B, C, S, 1))
    out = {}
    for sc in SCORERS:
        model = model_for("NRMS", sc).eval()
        with torch.no_grad():
            ms = timed(lambda: model._forward(hist, cand), reps, warmup)
        out[sc] = dict(impressions_per_s=B / ms * 1e3, ms=ms)
        del model
    del hx, cx
    torch.cuda.empty_cache()
    return out


def grad_steps(reps, warmup):
    out = {}
    for model_name, B in (("standard", 16), ("standard", 64), ("NRMS", 64)):
        batch = synth.batch_to(synth.make_batch(5, B, 50, 5, 50, 768, min_len=5), DEV)
        labels = torch.arange(B, device=DEV) % 7
        for sc in SCORERS:
            model = model_for(model_name, sc, bias=model_name == "standard").train()

            def step():
                model.zero_grad(set_to_none=True)
                preds = torch.relu(model(batch))
                loss = F.mse_loss(preds, batch["targets"]) + 0.1 * contrastive_loss(model.get_user_embeddings(batch), labels, 0.08)
                loss.backward()
            out[f"{model_name}_B{B}/{sc}"] = dict(ms=timed(step, max(reps // 4, 5), warmup))
            del model
        del batch
        torch.cuda.empty_cache()
    return out


def torch_form(kind, mod, u, c):
    """The reference's own arithmetic (scoring.py:52-66, 93-102) in stock torch ops."""
    if kind == "bilin":
        return F.bilinear(torch.cat([u] * c.shape[1], dim=1), c, mod.bilin.weight, mod.bilin.bias)
    x = torch.cat([u.repeat((1, c.shape[1], 1)), c], dim=2)
    return F.linear(torch.tanh(F.linear(x, mod.fc1.weight, mod.fc1.bias)), mod.fc2.weight, mod.fc2.bias)


def scorer_alone(reps, warmup):
    B, N, E = 512, 5, 256
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    u = torch.randn((B, 1, E), generator=gen, device=DEV, requires_grad=True)
    c = torch.randn((B, N, E), generator=gen, device=DEV, requires_grad=True)
    g = torch.randn((B, N, 1), generator=gen, device=DEV)
    out = {}
    for kind, mod in (("bilin", BilinScoring(E, bias=False)), ("fc", FCScoring(E, E // 2, bias=False))):
        mod = mod.to(DEV)
        row = {}
        for label, fn in (("hip", lambda: mod(u, c)), ("torch_ops", lambda: torch_form(kind, mod, u, c))):
            with torch.no_grad():
                fwd = timed(fn, reps, warmup)

            def fb():
                s = fn()
                s.backward(g)
            fwd_bwd = timed(fb, reps, warmup)
            row[label] = dict(fwd_us=fwd * 1e3, fwd_bwd_us=fwd_bwd * 1e3)
        with torch.no_grad():
            row["max_abs_diff_vs_torch_ops"] = float((mod(u, c) - torch_form(kind, mod, u, c)).abs().max())
        out[kind] = row
    return out


def eval_epochs():
    from xnrs_amd import evaluation as EV
    store, beh = synth.click_world(n_news=3000, n_sess=4000, S=30, D=256)
    store, beh = store.to(DEV), beh.to(DEV)
    out = {}
    for sc in SCORERS:
        model = model_for("standard", sc, E=128, D=256, S=30, H=20, bias=True).eval()
        EV.evaluate(model, store, beh, l_hist=20, batch=1024)  # warm-up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = EV.evaluate(model, store, beh, l_hist=20, batch=1024)
        b.record()
        torch.cuda.synchronize()
        out[sc] = dict(seconds=a.elapsed_time(b) / 1e3, auc=res["auc"])
    out["store"] = dict(n_news=3000, n_sess=4000, S=30, D=256, E=128, model="standard")
    return out


def count_launches():
    """Kernels the profiler sees in one scorer call (B=512, N=5, E=256)."""
    from torch.profiler import ProfilerActivity, profile
    B, N, E = 512, 5, 256
    u = torch.randn((B, 1, E), device=DEV, requires_grad=True)
    c = torch.randn((B, N, E), device=DEV, requires_grad=True)
    g = torch.randn((B, N, 1), device=DEV)
    out = {}
    for kind, mod in (("dot", DotScoring()), ("bilin", BilinScoring(E, bias=True)), ("bilin_norm", BilinScoring(E, normalize=True)),
                      ("fc", FCScoring(E, E // 2, bias=True))):
        mod = mod.to(DEV)
        s = mod(u, c)
        s.backward(g)  # warm-up (workspaces)
        torch.cuda.synchronize()
        row = {}
        for label in ("forward", "backward", "input_grad_backward"):
            # (an input-gradient pass as integrated gradients runs it: the scorer's inputs come out of earlier nodes)
            s = mod(u * 1, c * 1) if label == "input_grad_backward" else mod(u, c)
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                if label == "forward":
                    mod(u, c)
                elif label == "backward":
                    s.backward(g)
                else:
                    torch.autograd.grad(s, [u, c], g)
                torch.cuda.synchronize()
            kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
            names = [e.name for e in kernels if "xnrs" in e.name]  # the library's launches (not torch's gradient accumulation)
            row[label] = dict(kernels=len(names), names=sorted(set(n[:60] for n in names)),
                              all_device_kernels=len([e for e in kernels if "Memcpy" not in e.name]))
        out[kind] = row
        u.grad = c.grad = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0))
    res["launches"] = count_launches()
    res["scorer"] = scorer_alone(a.reps * 5, a.warmup)
    res["inference"] = inference(a.reps // 2, a.warmup)
    res["grad_step"] = grad_steps(a.reps, a.warmup)
    res["eval_epoch"] = eval_epochs()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
