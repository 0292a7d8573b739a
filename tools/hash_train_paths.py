#!/usr/bin/env python
"""Fingerprint of the training path of xnrs_amd/autograd.py: for a list of seeded cases -- the reference-order train step of
every model, each sharing switch off alone, the id path, an unaligned parameter, frozen parameters, gradients with respect to
the tokens, an unused encode, gradient accumulation, a captured step -- the SHA-256 of the loss, of every output and of every
gradient, the delta of every autograd.STATS key and of the library's launch counters.  Two trees whose autograd.py differ
only in structure give equal files over the same library (the training path has no float atomics).

    python tools/hash_train_paths.py OUT.json
"""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.golden import cases  # noqa: E402
from xnrs_amd import autograd as AG, hip, ops, synth  # noqa: E402
from xnrs_amd.losses import contrastive_loss  # noqa: E402
from xnrs_amd.models import make_model  # noqa: E402
from xnrs_amd.models.components import layers, news_encoding  # noqa: E402

DEV = "cuda:0"
NRMS = dict(model="NRMS", B=8, H=12, C=3, S=50, D=64, h=4, E=32, bias=False, seed=4101, min_len=3)
STD = dict(cases.GRAD_SHIPPED_STD, B=6, H=7, C=3, seed=4505)
NAML = dict(cases.GRAD_SHIPPED_NAML, B=6, H=7, C=3, seed=4606)
LABELS = [0, 1, 0, 2, 1, 0, 2, 2]
COUNTERS = ("xnrs_qkv_launch_count", "xnrs_fc1_in_tail_count", "xnrs_mha_live_o_count")
SWITCHES = ("LIVE_ROWS", "DEVICE_LISTS", "KV_ROWS", "SHARE_QKV", "MERGE_DW", "SUM_SHARED_GRADS", "FOLD_TRAIN_CACHE", "SKIP_UNUSED_DW")


class Cfg(dict):
    __getattr__ = dict.__getitem__


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def make(c, att_dropout=0.1):
    model = make_model(Cfg(cases.model_cfg(c)))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(synth.fill_state_dict(shapes, c["seed"] + 1))
    model.train()
    for mod in model.modules():
        if isinstance(mod, layers.MultiHeadAttention):
            mod.dropout.p = att_dropout
    return model.to(DEV), synth.batch_to(cases.model_batch(c), DEV), torch.tensor(LABELS[:c["B"]], device=DEV)


def forward(model, batch, labels, seed=1234):
    """The reference-order step up to the loss -> {loss, preds, user_emb}.  seed None: the caller has seeded."""
    if seed is not None:
        torch.manual_seed(seed)  # the attention-dropout seeds come from torch's CPU generator
    preds = torch.relu(model(batch))
    ue = model.get_user_embeddings(batch)
    loss = torch.nn.functional.mse_loss(preds, batch["targets"]) + 0.1 * contrastive_loss(ue.reshape(ue.shape[0], -1), labels, 0.08)
    return dict(loss=loss, preds=preds, user_emb=ue)


def grads_of(model, out):
    out.update({"grad/" + k: p.grad for k, p in model.named_parameters() if p.grad is not None})
    return out


def step(c, att_dropout=0.1, prepare=None, off=()):
    """One train step of case c with the switches named in `off` turned off; prepare(model, batch) edits either first."""
    model, batch, labels = make(c, att_dropout)
    if prepare is not None:
        prepare(model, batch)
    saved = {k: getattr(AG, k) for k in off}
    for k in off:
        setattr(AG, k, False)
    try:
        out = forward(model, batch, labels)
        out["loss"].backward()
    finally:
        for k, v in saved.items():
            setattr(AG, k, v)
    return grads_of(model, out)


def misalign_wq(model, batch):
    for k, p in model.named_parameters():
        if k.endswith("q_linear.weight"):
            buf = torch.empty(p.numel() + 8, device=DEV)
            off = ((4 - buf.data_ptr()) % 16) // 4
            p.data = buf[off:off + p.numel()].view_as(p).copy_(p.data)
            assert p.data_ptr() % 16 == 4


def freeze(suffix):
    def prepare(model, batch):
        n = 0
        for k, p in model.named_parameters():
            if k.endswith(suffix):
                p.requires_grad_(False)
                n += 1
        assert n
    return prepare


def mostly_live(model, batch):
    for m in (batch["user_features"]["history"]["title_emb"][1], batch["candidate_features"]["title_emb"][1]):
        m.fill_(1.0)
        m[0, 0, -2:] = 0  # (a mask that still matters; more than LIVE_ROWS_MAX_FRACTION of the rows live)


def id_path(device_lists):
    """A news tower encoding the same id-gathered history twice (the second reads the first's Q|K|V image); 30 % of the table
    rows are empty history slots."""
    S, D, h, E, n_tab, n = 24, 64, 4, 32, 260, 300
    enc = news_encoding.TextEncoder(pooler=layers.AdditiveAttention(D, 48), p_dropout=0.0, out_features=E, in_features=D,
                                    att=layers.MultiHeadAttention(h, D))
    shapes = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    enc.load_state_dict(synth.fill_state_dict(shapes, 171))
    enc.train().to(DEV)
    enc.att.dropout.p = 0.1
    rng = synth.rng_for(172)
    x = torch.from_numpy(rng.standard_normal((n_tab, S, D)).astype("float32")).to(DEV)
    m = torch.from_numpy((rng.random((n_tab, S)) < 0.55).astype("float32"))
    m[torch.from_numpy(rng.random(n_tab) < 0.3)] = 0
    m = m.to(DEV)
    w = torch.from_numpy(rng.standard_normal((2, n, E)).astype("float32")).to(DEV)
    ids = torch.from_numpy(rng.integers(0, n_tab, size=(1, n)).astype("int32")).to(DEV)  # (int32: the call takes them as they are, so two calls share)
    saved, AG.DEVICE_LISTS = AG.DEVICE_LISTS, device_lists
    try:
        torch.manual_seed(31)
        y1, _ = enc.forward_ids(x, m, ids)
        y2, _ = enc.forward_ids(x, m, ids)
        loss = (y1[0] * w[0]).sum() + 0.1 * (y2[0] * w[1]).sum()
        loss.backward()
    finally:
        AG.DEVICE_LISTS = saved
    return grads_of(enc, dict(loss=loss, y1=y1, y2=y2))


def token_grad():
    """torch.autograd.grad(loss, inputs=[tokens]) through the whole model: no parameter product anywhere."""
    model, batch, labels = make(NRMS)
    hx, hm = batch["user_features"]["history"]["title_emb"]
    hx.requires_grad_(True)
    out = forward(model, batch, labels)
    (out["d_tokens"],) = torch.autograd.grad(out["loss"], inputs=[hx])
    assert all(p.grad is None for p in model.parameters())
    return out


def token_grad_from_qkv():
    """... and through the node that starts from a given Q|K|V image: two backward passes over one forward."""
    enc = news_encoding.TextEncoder(pooler=layers.AdditiveAttention(64, 48), p_dropout=0.0, out_features=32, in_features=64,
                                    att=layers.MultiHeadAttention(4, 64))
    shapes = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    enc.load_state_dict(synth.fill_state_dict(shapes, 181))
    enc.eval().to(DEV)
    g = torch.Generator(device=DEV)
    g.manual_seed(6302)
    x = torch.randn((6, 12, 64), device=DEV, generator=g)
    m = (torch.rand((6, 12, 1), device=DEV, generator=g) < 0.7).float()
    m[:, 0] = 1
    m[2] = 0
    r = torch.randn((6, 32), device=DEV, generator=g)
    att = enc.att
    wcat = torch.cat([att.q_linear.weight, att.k_linear.weight, att.v_linear.weight]).detach().contiguous()
    bcat = torch.cat([att.q_linear.bias, att.k_linear.bias, att.v_linear.bias]).detach().contiguous()
    qkv = ops.linear(x, wcat, bcat).reshape(6 * 12, 192).requires_grad_()
    y, hm = ops.text_encoder_from_qkv(qkv, x, m, enc)
    (g1,) = torch.autograd.grad((y * r).sum(), qkv, retain_graph=True)
    (g2,) = torch.autograd.grad((y * r).sum(), qkv)
    return dict(y=y, hm=hm, d_image_1=g1, d_image_2=g2)


def unused_second_encode():
    """The second history encode runs, the loss does not use it: its node never executes and nothing is deferred."""
    model, batch, labels = make(NRMS)
    torch.manual_seed(1234)
    preds = torch.relu(model(batch))
    ue = model.get_user_embeddings(batch)
    loss = torch.nn.functional.mse_loss(preds, batch["targets"])
    loss.backward()
    return grads_of(model, dict(loss=loss, preds=preds, user_emb=ue))


def accumulation():
    model, batch, labels = make(NRMS)
    out = {}
    for i in range(2):  # no zero_grad in between
        o = forward(model, batch, labels, seed=1234 + i)
        o["loss"].backward()
        out.update({f"{k}_{i}": v for k, v in o.items()})
    return grads_of(model, out)


def captured():
    """The step captured on a side stream (eager steps and capture on ONE stream, as tests/test_hip_train_step.py explains):
    two replays, then one after the batch was overwritten in place."""
    model, batch, labels = make(dict(NRMS, seed=4303))
    _, batch2, _ = make(dict(NRMS, seed=4404))
    params = [p for p in model.parameters() if p.requires_grad]
    for p in params:
        p.grad = torch.zeros_like(p)

    def one():
        for p in params:
            p.grad.zero_()
        loss = forward(model, batch, labels, seed=None)["loss"]
        loss.backward()
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.manual_seed(77)
            one()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    torch.manual_seed(77)
    with torch.cuda.graph(graph, stream=side):
        loss_g = one()
    out = {}

    def replay(tag):
        graph.replay()
        torch.cuda.synchronize()
        out["loss_" + tag] = loss_g.clone()
        out.update({f"grad_{tag}/{i}": p.grad.clone() for i, p in enumerate(params)})
    replay("replay0")
    replay("replay1")
    for feat in (lambda b: b["user_features"]["history"]["title_emb"], lambda b: b["candidate_features"]["title_emb"]):
        feat(batch)[0].copy_(feat(batch2)[0])
        feat(batch)[1].copy_(feat(batch2)[1])
    replay("other_batch")
    return out


CASES = [("nrms", lambda: step(NRMS)), ("nrms_bias", lambda: step(dict(NRMS, bias=True))),
         ("standard", lambda: step(STD)), ("naml", lambda: step(NAML))]
CASES += [("nrms_no_" + k, lambda k=k: step(NRMS, off=(k,))) for k in SWITCHES]
CASES += [("standard_no_SHARE_OUTPUTS", lambda: step(STD, off=("SHARE_OUTPUTS",))),
          ("ids_device_lists", lambda: id_path(True)), ("ids_host_lists", lambda: id_path(False)),
          ("unaligned_wq", lambda: step(NRMS, prepare=misalign_wq)),
          ("mostly_live_host_lists", lambda: step(NRMS, prepare=mostly_live, off=("DEVICE_LISTS",))),
          ("frozen_wq", lambda: step(NRMS, prepare=freeze("q_linear.weight"))),
          ("frozen_wo", lambda: step(NRMS, prepare=freeze("out.weight"))),
          ("token_grad", token_grad), ("token_grad_from_qkv", token_grad_from_qkv),
          ("unused_second_encode", unused_second_encode), ("accumulation", accumulation), ("captured", captured)]


def main(path):
    AG.LIVE_ROWS_MIN = 1  # (the row lists at these small shapes)
    l = hip.lib()
    result = {}
    for name, fn in CASES:
        for cache in (AG._QKV_IMAGES, AG._OUTPUTS, AG._TRAIN_FOLDS, AG._PARAM_GROUPS):
            cache.clear()  # (a case must not hit on what an earlier case's freed tensors left at the same address)
        stats = dict(AG.STATS)
        for c in COUNTERS:
            getattr(l, c)(1)
        out = fn()
        torch.cuda.synchronize()
        hip.check_status()
        result[name] = dict(sha256={k: sha(v) for k, v in sorted(out.items())},
                            stats={k: AG.STATS[k] - v for k, v in stats.items()},
                            counters={c: getattr(l, c)(1) for c in COUNTERS})
        print(name, result[name]["stats"], result[name]["counters"], flush=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
