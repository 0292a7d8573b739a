"""Plain-torch helpers for the one-projection form of integrated gradients (xnrs_amd/explain.py):
a restatement of the attention TextEncoder that can START from a given Q|K|V image, the two forms of the explanation
(step by step on the scaled tokens; one projection, expanded and reduced) in whatever dtype the inputs have, and stand-ins
for the device operations of xnrs_amd.explain so that its orchestration runs on the CPU.  No HIP call anywhere."""
import math

import torch

from oracle import xnrs_oracle as O


def sub(sd, prefix):
    p = prefix + "."
    return {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}


def qkv_weights(nsd):
    """[Wq; Wk; Wv] (3D, D) and the three biases (3D,) of a news-encoder state dict."""
    w = torch.cat([nsd["att.q_linear.weight"], nsd["att.k_linear.weight"], nsd["att.v_linear.weight"]])
    b = torch.cat([nsd["att.q_linear.bias"], nsd["att.k_linear.bias"], nsd["att.v_linear.bias"]])
    return w, b


def encoder_from_qkv(qkv, m, nsd, n_heads):
    """The TextEncoder with an attention stage (news_encoding.py:43-60, layers.py:120-156, 47-69) from its Q|K|V image on.
    qkv (n, S, 3D), m (n, S, 1) -> (y (n, E'), hm (n, 1))."""
    n, S, D3 = qkv.shape
    D = D3 // 3
    dk = D // n_heads
    q, k, v = (t.reshape(n, S, n_heads, dk).transpose(1, 2) for t in qkv.split(D, dim=-1))
    att = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(dk)
    att = att.masked_fill(m.unsqueeze(1) == 0, -1e9)             # a QUERY-row mask (layers.py:142-144)
    att = torch.softmax(att, dim=-1)
    o = torch.matmul(att, v).transpose(1, 2).reshape(n, S, D)
    y = o @ nsd["att.out.weight"].T + nsd["att.out.bias"]
    if "pooler.fc1.weight" in nsd:
        e = torch.tanh(y @ nsd["pooler.fc1.weight"].T + nsd["pooler.fc1.bias"]) @ nsd["pooler.fc2.weight"].T + nsd["pooler.fc2.bias"]
        a = torch.exp(e) * m
        a = a / (a.sum(dim=1, keepdim=True) + 1e-8)
        p = (a * y).sum(dim=1)
    else:
        p = (y * m).sum(dim=1) / (m.sum(dim=1) + 1e-8)
    if "head.0.weight" in nsd:
        h = p @ nsd["head.0.weight"].T
        if "head.0.bias" in nsd:
            h = h + nsd["head.0.bias"]
        p = torch.relu(h) @ nsd["head.2.weight"].T
        if "head.2.bias" in nsd:
            p = p + nsd["head.2.bias"]
    return p, torch.clamp(m.sum(dim=1), 0, 1)


def _alphas(n_steps):
    da = 1.0 / n_steps
    return da, torch.arange(da, 1 + da, da)[:n_steps]   # explain.py:160 (fp32 values, as the reference draws them)


def ig_step_by_step(sd, n_heads, hist, cand, cidx, n_steps, act=torch.relu):
    """tests/test_hip_explain.py::oracle_ig in the dtype of its inputs: the reference's loop over the oracle."""
    hx, hm = hist
    nsd, usd = sub(sd, "news_encoder"), sub(sd, "user_encoder")
    c, _ = O.text_encoder(cand[0][:, cidx:cidx + 1], cand[1][:, cidx:cidx + 1], nsd, n_heads)
    da, alphas = _alphas(n_steps)
    grads, sa = [], None
    for a in alphas:
        ga = (a.to(hx.dtype) * hx).requires_grad_()
        ha, ham = O.text_encoder(ga, hm, nsd, n_heads)
        sa = act(O.dot_scoring(O.user_encoder(ha, ham, usd, n_heads), c.detach()))
        grads.append(torch.autograd.grad(sa, ga)[0])
    int_grads = torch.sum(torch.cat(grads) * da, dim=0)
    return (int_grads * hx[0]).sum(dim=2), int_grads, float(sa.item())


def ig_projection_once(sd, n_heads, hist, cand, cidx, n_steps, act=torch.relu):
    """The same explanation with ONE projection: P = x Wcat^T, QKV_i = a_i P + bcat, int_grads = (da sum_i dQKV_i) Wcat."""
    hx, hm = hist
    _, H, S, D = hx.shape
    nsd, usd = sub(sd, "news_encoder"), sub(sd, "user_encoder")
    c, _ = O.text_encoder(cand[0][:, cidx:cidx + 1], cand[1][:, cidx:cidx + 1], nsd, n_heads)
    w, b = qkv_weights(nsd)
    P = hx[0].reshape(H * S, D) @ w.T
    da, alphas = _alphas(n_steps)
    G, sa = torch.zeros_like(P), None
    for a in alphas:
        qkv = (a.to(P.dtype) * P + b).requires_grad_()
        y, ham = encoder_from_qkv(qkv.reshape(H, S, 3 * D), hm[0], nsd, n_heads)
        sa = act(O.dot_scoring(O.user_encoder(y[None], ham[None], usd, n_heads), c.detach()))
        G = G + torch.autograd.grad(sa, qkv)[0]
    int_grads = ((da * G) @ w).reshape(H, S, D)
    return (int_grads * hx[0]).sum(dim=2), int_grads, float(sa.item())


class TorchOps:
    """Stand-ins for the device operations behind xnrs_amd.explain._HipOps, with the contracts of include/xnrs_hip.h
    (xnrs_ig_expand, xnrs_ig_reduce) and of ops.text_encoder_from_qkv, in plain torch.  `calls` logs every reduce."""

    def __init__(self):
        self.calls = []
        self.forwards = 0

    def project(self, x2d, w):
        return x2d @ w.T

    def check_rows(self, store, rows):
        return rows.reshape(-1).to(torch.int32).clamp(0, store.x.shape[0] - 1)

    def project_rows(self, table, rows, w, x):
        return table[rows.long()].reshape(-1, table.shape[-1]).to(w.dtype) @ w.T

    def expand(self, p, bias, alphas):
        self.alphas = alphas
        return (alphas.to(p.dtype)[:, None, None] * p[None] + bias).reshape(-1, p.shape[1])

    def encode(self, qkv, x, m, enc):
        self.forwards += 1
        S = x.shape[-2]
        nsd = {k: v.detach() for k, v in enc.state_dict().items()}
        y, hm = encoder_from_qkv(qkv.reshape(-1, S, qkv.shape[1]), m, nsd, enc.att.h)
        return y, hm.reshape(-1)

    def reduce(self, g, n, scale, out, accumulate):
        self.calls.append((n, scale, bool(accumulate)))
        s = g.reshape(n, *out.shape).sum(dim=0)
        with torch.no_grad():
            out.copy_(out + scale * s if accumulate else scale * s)
        return out

    def input_grad(self, g, w):
        return g @ w

    def gather(self, store, rows, feature):
        return store.x[rows.long()], store.m[rows.long()].unsqueeze(-1)

    def encode_candidates(self, model, store, rows, feature):
        x, m = self.gather(store, rows, feature)
        return model.news_encoder((x[None], m[None]))[0]


class AlphaWeightedOps(TorchOps):
    """A WRONG reduce: it weights the slices by their alphas (the mistake the algebra invites: the a_i of the forward do not
    come back in the backward).  The orchestration tests must tell it from the right one."""

    def reduce(self, g, n, scale, out, accumulate):
        a = self.alphas.to(g.dtype)[:, None, None]
        return super().reduce((g.reshape(n, *out.shape) * a).reshape(g.shape), n, scale, out, accumulate)


class NoDevice:
    """A backend no refusal may reach: every operation fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"device operation {name!r} was reached before the refusal")
