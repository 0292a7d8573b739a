"""Integrated gradients of one score w.r.t. the history's token embeddings -- the compute loop of
Explainer.explain_score_in_batch (xnrs/explain.py:144-182; the one timing the reference publishes).

The reference walks the interpolation path a = 1/n, 2/n, ..., 1 one step at a time: a news-encoder forward over the H
history news scaled by a, the user encoder, the score against the fixed candidate vector, and torch.autograd.grad(score,
scaled tokens) -- n forward + input-gradient passes of ONE impression each, launch-latency bound on any GPU.  The steps are
independent of each other (each score depends on its own scaled copy only), so here they are the BATCH dimension: one
forward and one input-gradient pass over `steps_per_batch` scaled copies of the history, through the same HIP kernels as
the grad step (no parameter gradient is computed: autograd._wanted_inputs).  `batched=False` keeps the reference's loop
(same numbers up to the summation order of the final sums; tests/test_hip_explain.py).

For a TextEncoder with an attention stage the tokens enter through the Q|K|V projection alone, and that projection and its
input-gradient product are linear in the step: `projection_once=True` computes each ONCE per explanation (P = x Wcat^T, the
n images a_i P + bcat by xnrs_ig_expand; the n gradient images summed by xnrs_ig_reduce, then one product with Wcat) -- exact
algebra, DESIGN.md section 10j.  explain_rows / explain_recommendations explain rows of a NewsStore, e.g. what
evaluation.recommend returned for a session, several rows per forward.

Out of scope here as in DESIGN.md section 11: the tokenizer, the backbone that produces the token embeddings, plotting.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch


def _encode_candidate(model, cand_emb, cand_att, cidx):
    # explain.py:155-157: only one candidate is scored
    ce = cand_emb[:, cidx:cidx + 1, :, :]
    ca = cand_att[:, cidx:cidx + 1, :, :]
    c, _ = model.news_encoder((ce, ca))
    return c


class _HipOps:
    """The device operations of the one-projection path, behind one object so that the orchestration
    below -- alphas, chunks, the reduce's scale and accumulate flag, one backward per candidate, the attribution sums -- can
    be run on the CPU against plain-torch stand-ins (tests/test_ig_linear_host.py)."""

    @staticmethod
    def project(x2d, w):                       # P = x W^T, no bias (it is added once per step by expand)
        from . import ops
        return ops.linear(x2d, w)

    @staticmethod
    def check_rows(store, rows):
        """rows as every later use sees them: int32, clamped into the table WITHOUT a host read, an id that had to be clamped
        setting hip.STATUS_ROW_RANGE in the sticky status word (NewsStore.gather's rule) -- no kernel reads out of bounds, and
        the gathered tokens and the projection are taken from the SAME rows."""
        from . import hip
        flat = rows.reshape(-1).to(torch.int32).contiguous()
        if not flat.is_cuda:
            raise hip.XnrsHipError("explain_rows: the rows must live on the HIP device")
        if flat.numel():
            ok = flat.clamp(0, store.n_rows - 1)
            bad = (ok != flat).any().to(torch.int32) * hip.STATUS_ROW_RANGE
            hip.status_word(flat.device).bitwise_or_(bad.reshape(1))
            flat = ok
        return flat

    @staticmethod
    def project_rows(table, rows, w, x):       # the same from the table's token rows by id (rows: checked, see above)
        from . import ops
        S, D = table.shape[1:]
        if table.dtype == torch.bfloat16:       # x: those rows widened (ops.table_rows_f32 under store.gather), never the table
            return ops.linear(x.reshape(-1, D), w)
        if table.shape[0] * S >= 2 ** 31:
            raise ValueError("explain_rows: the token table has more than 2^31 - 1 token rows")
        tok = (rows.long()[:, None] * S + torch.arange(S, device=rows.device)[None, :]).reshape(-1).to(torch.int32)
        return ops.linear(table.reshape(-1, D), w, ids=tok)

    @staticmethod
    def expand(p, bias, alphas):
        from . import ops
        return ops.ig_expand(p, bias, alphas)

    @staticmethod
    def encode(qkv, x, m, enc):
        from . import ops
        return ops.text_encoder_from_qkv(qkv, x, m, enc)

    @staticmethod
    def reduce(g, n, scale, out, accumulate):
        from . import ops
        return ops.ig_reduce(g, n, scale, out, accumulate)

    @staticmethod
    def input_grad(g, w):                      # G . W: one product
        from . import ops
        return ops.linear_input_grad(g, w)

    @staticmethod
    def gather(store, rows, feature):          # dense (x:(n, S, D), m:(n, S, 1)) of table rows
        return store.gather(rows, feature)

    @staticmethod
    def encode_candidates(model, store, rows, feature):  # (1, C, E), from the gathered tokens (a bf16 store: widened rows)
        cx, cm = store.gather(rows, feature)
        c, _ = model.news_encoder((cx[None], cm[None]))
        return c


_HIP = _HipOps()
#: explain_rows(projection_once=None) takes the one-projection path for models that have one
EXPLAIN_ROWS_PROJECTION_ONCE = True


def _text_encoder_of(model):
    """The model's news encoder if it is a TextEncoder (-> it, whether it has an attention stage); NotImplementedError for
    every other news encoder (NAML's views, NPA's personalised attention, ...)."""
    from .models.blocks import TextEncoder
    enc = getattr(model, "news_encoder", None)
    if not isinstance(enc, TextEncoder):
        raise NotImplementedError(f"explanations by store row / with one projection need a news encoder that is a TextEncoder; "
                                  f"{type(model).__name__} has {type(enc).__name__}")
    return enc, enc.att is not None


def _require_projection_once(model):
    enc, has_att = _text_encoder_of(model)
    if not has_att:
        raise NotImplementedError("projection_once needs a TextEncoder WITH an attention stage: only there do the tokens enter "
                                  "through the Q|K|V projection alone (an attention-free tower pools the scaled tokens themselves)")
    if model.training:
        raise ValueError("projection_once explains a model in eval mode: in train mode every scaled copy would draw its own "
                         "dropout masks, and one shared projection cannot reproduce them")
    return enc


def _alphas(n_steps, device):
    da = 1.0 / n_steps
    # explain.py:160: torch.arange(da, 1 + da, da) -- the same fp32 values, cut to n_steps (rounding can add one)
    return da, torch.arange(da, 1 + da, da, device=device)[:n_steps]


def _qkv_weights(enc):
    att = enc.att
    w = torch.cat([att.q_linear.weight, att.k_linear.weight, att.v_linear.weight]).detach().contiguous()   # (3D, D)
    b = torch.cat([att.q_linear.bias, att.k_linear.bias, att.v_linear.bias]).detach().contiguous()         # (3D,)
    return w, b


def _projection_once(model, enc, be, P, bcat, x, m, c, alphas, da, per, act):
    """The per-step part of the one-projection path for C candidates at once.  P (H * S, 3D) = x Wcat^T; x (H, S, D) (its
    shape); m (H, S, 1); c (1, C, E) candidate vectors, fixed along the path.  Per chunk of steps ONE forward scores all
    candidates, then one backward per candidate over the retained graph is reduced into that candidate's own image.
    -> G (C, H * S, 3D) = da * sum_i dQKV_i (no alpha weights: the sum is taken before the one product with Wcat),
    s_true (C,) the scores at a = 1 of the same pass."""
    H, S, _ = x.shape
    C = c.shape[1]
    n = alphas.numel()
    G = torch.zeros((C,) + tuple(P.shape), dtype=P.dtype, device=P.device)
    s_true = None
    for chunk, lo in enumerate(range(0, n, per)):
        al = alphas[lo:lo + per]
        nb = al.numel()
        qkv = be.expand(P, bcat, al).requires_grad_()            # (nb * H * S, 3D): step i is impression i of the batch
        att = m.reshape(1, H, S, 1).expand(nb, -1, -1, -1).reshape(nb * H, S, 1).contiguous()
        y, hm = be.encode(qkv, x, att, enc)
        ha, ham = y.reshape(nb, H, -1), hm.reshape(nb, H, 1)
        ua = model.user_encoder.forward(inpt=(ha, ham))
        sa = act(model.rec_model(ua, c.expand(nb, -1, -1).contiguous())).reshape(nb, C)
        for j in range(C):
            (g,) = torch.autograd.grad(sa[:, j].sum(), qkv, retain_graph=j + 1 < C)  # d sa_ij / d qkv_k = 0 for i != k
            be.reduce(g, nb, da, G[j], chunk > 0)
            del g
        s_true = sa.detach()[-1]
    return G, s_true


def integrated_gradients(model, hist_emb: torch.Tensor, hist_att: torch.Tensor, cand_emb: torch.Tensor,
                         cand_att: torch.Tensor, candidate_idx: int = 0, n_steps: int = 100,
                         activation: Optional[Callable] = torch.relu, batched: bool = True,
                         steps_per_batch: int = 0, projection_once: bool = False, _backend=None) -> Dict[str, object]:
    """hist_emb (1, H, S, D), hist_att (1, H, S, 1), cand_emb (1, C, S, D), cand_att (1, C, S, 1) on the model's device.

    Returns {"attr": (H, S) token attributions, "news_attribution": (H,), "int_grads": (H, S, D), "s_true": score at a = 1,
    "s_attr": sum of the attributions} -- explain.py:167-173 (the dictionary of titles / tokens around them is the
    caller's business).  steps_per_batch: interpolation steps per pass (0 = all n_steps at once; n_steps * H * S * D * 4
    bytes of scaled tokens and as much again of gradients per pass).

    projection_once=True (a TextEncoder with an attention stage, eval mode; NotImplementedError / ValueError otherwise, before
    any launch): the Q|K|V projection and its input-gradient product are linear in the step, so each runs ONCE over the H * S
    token rows instead of once per step -- P = x Wcat^T, QKV_i = a_i P + bcat (xnrs_ig_expand), int_grads =
    (da sum_i dQKV_i) Wcat (xnrs_ig_reduce, then one product).  Exact algebra; the numbers differ from the default path by
    fp32 rounding ((a x) W against a (x W)).  Per pass 3 n_steps H S D floats of images and as much of gradients."""
    if hist_emb.dim() != 4 or hist_emb.size(0) != 1:
        raise ValueError("integrated_gradients explains ONE impression: hist_emb must be (1, H, S, D)")
    if n_steps < 1:
        raise ValueError("n_steps must be >= 1")
    enc = _require_projection_once(model) if projection_once else None
    act = activation if activation is not None else (lambda t: t)
    hist_emb = hist_emb.detach()
    hist_att = hist_att.detach()
    with torch.no_grad():
        c = _encode_candidate(model, cand_emb.detach(), cand_att.detach(), candidate_idx)  # (1, 1, E): fixed along the path
    da, alphas = _alphas(n_steps, hist_emb.device)
    H, S, D = hist_emb.shape[1:]
    if projection_once:
        be = _backend or _HIP
        per = n_steps if steps_per_batch <= 0 else min(int(steps_per_batch), n_steps)
        wcat, bcat = _qkv_weights(enc)
        x = hist_emb[0].contiguous()
        P = be.project(x.reshape(H * S, D), wcat)
        G, s = _projection_once(model, enc, be, P, bcat, x, hist_att[0], c, alphas, da, per, act)
        int_grads = be.input_grad(G[0], wcat).reshape(H, S, D)
        attr = (int_grads * x).sum(dim=2)
        return {"attr": attr, "news_attribution": attr.sum(dim=1), "int_grads": int_grads,
                "s_true": float(s.reshape(-1)[-1].item()), "s_attr": float(attr.sum().item())}
    int_grads = torch.zeros((H, S, D), dtype=hist_emb.dtype, device=hist_emb.device)
    s_true = None
    if not batched:
        for a in alphas:
            ga = (a * hist_emb).requires_grad_()
            ha, ham = model.news_encoder((ga, hist_att))
            ua = model.user_encoder.forward(inpt=(ha, ham))
            sa = act(model.rec_model(ua, c))
            (g,) = torch.autograd.grad(sa, ga)
            int_grads += g[0] * da
            s_true = sa.detach()
    else:
        per = n_steps if steps_per_batch <= 0 else min(int(steps_per_batch), n_steps)
        for lo in range(0, n_steps, per):
            al = alphas[lo:lo + per]
            nb = al.numel()
            ga = (al.view(nb, 1, 1, 1) * hist_emb).requires_grad_()     # (nb, H, S, D): step i is impression i of the batch
            att = hist_att.expand(nb, -1, -1, -1).contiguous()
            ha, ham = model.news_encoder((ga, att))
            ua = model.user_encoder.forward(inpt=(ha, ham))
            sa = act(model.rec_model(ua, c.expand(nb, -1, -1).contiguous()))
            (g,) = torch.autograd.grad(sa.sum(), ga)                     # d sa_i / d ga_j = 0 for i != j
            int_grads += g.sum(dim=0) * da
            s_true = sa.detach().reshape(nb, -1)[-1:]
    attr_full = int_grads * hist_emb[0]                                   # explain.py:169
    attr = attr_full.sum(dim=2)                                           # (H, S): explain.py:170 sums batch and feature axes
    return {"attr": attr, "news_attribution": attr.sum(dim=1), "int_grads": int_grads,
            "s_true": float(s_true.reshape(-1)[-1].item()), "s_attr": float(attr.sum().item())}


def explain_rows(model, store, hist_rows: torch.Tensor, cand_rows: torch.Tensor, n_steps: int = 100,
                 activation: Optional[Callable] = torch.relu, steps_per_batch: int = 0, feature: str = "title_emb",
                 projection_once: Optional[bool] = None, _backend=None) -> Dict[str, torch.Tensor]:
    """Why does ONE session get these rows?  hist_rows (H,): the session's history as rows of `store` (the pad row and
    repeated rows are fine), cand_rows (C,): the rows to explain, e.g. one row of what recommend() returned.
    -> {"attr": (C, H, S) token attributions per explained row, "news_attribution": (C, H), "s_true": (C,) the scores at
    a = 1, "s_attr": (C,) the sums of the attributions}, device tensors.  The one-projection path reads nothing on the host;
    the batched fallback goes through integrated_gradients, which reads two scalars per explained row.  Rows outside the table
    are clamped into it and set hip.STATUS_ROW_RANGE in the sticky status word (hip.check_status() raises at the caller's
    next sync point), as NewsStore.gather does -- the tokens and the projection are taken from the same, checked rows.

    A TextEncoder with an attention stage takes the one-projection path (integrated_gradients(projection_once=True)): P comes
    from the table by row id (a bf16 store: from the widened rows of the history, never the table), per chunk of steps ONE
    forward scores all C candidates and one backward per candidate over the retained graph is reduced into that candidate's
    image, and the C final products run as one call over C H S rows.  projection_once=False, or a TextEncoder without an
    attention stage: the batched path of integrated_gradients on the gathered tokens, candidate by candidate (the capability
    does not depend on the fast path).  None: EXPLAIN_ROWS_PROJECTION_ONCE where the model has the path.
    A news encoder that is not a TextEncoder: NotImplementedError; on the one-projection path a model in train mode:
    ValueError -- all before any launch."""
    if hist_rows.dim() != 1 or cand_rows.dim() != 1:
        raise ValueError("explain_rows explains ONE session: hist_rows must be (H,) and cand_rows (C,)")
    if n_steps < 1:
        raise ValueError("n_steps must be >= 1")
    enc, has_att = _text_encoder_of(model)
    fast = (EXPLAIN_ROWS_PROJECTION_ONCE and has_att) if projection_once is None else bool(projection_once)
    if fast:
        _require_projection_once(model)
    be = _backend or _HIP
    act = activation if activation is not None else (lambda t: t)
    C = cand_rows.numel()
    hist_rows, cand_rows = be.check_rows(store, hist_rows), be.check_rows(store, cand_rows)  # ONE check for every use below
    x, m = be.gather(store, hist_rows, feature)                   # (H, S, D), (H, S, 1)
    H, S, D = x.shape
    if not fast:
        cx, cm = be.gather(store, cand_rows, feature)
        outs = [integrated_gradients(model, x[None], m[None], cx[None], cm[None], candidate_idx=j, n_steps=n_steps,
                                     activation=activation, steps_per_batch=steps_per_batch) for j in range(C)]
        attr = torch.stack([o["attr"] for o in outs]) if C else x.new_zeros((0, H, S))
        s_true = torch.tensor([o["s_true"] for o in outs], dtype=x.dtype, device=x.device)
        return {"attr": attr, "news_attribution": attr.sum(dim=2), "s_true": s_true, "s_attr": attr.sum(dim=(1, 2))}
    with torch.no_grad():
        c = be.encode_candidates(model, store, cand_rows, feature)  # (1, C, E): fixed along the path
    da, alphas = _alphas(n_steps, x.device)
    per = n_steps if steps_per_batch <= 0 else min(int(steps_per_batch), n_steps)
    wcat, bcat = _qkv_weights(enc)
    P = be.project_rows(store.text(feature)[0], hist_rows, wcat, x)  # (H * S, 3D)
    G, s_true = _projection_once(model, enc, be, P, bcat, x, m, c, alphas, da, per, act)
    int_grads = be.input_grad(G.reshape(C * H * S, 3 * D), wcat).reshape(C, H, S, D)   # the C products as one call
    attr = (int_grads * x[None]).sum(dim=3)
    return {"attr": attr, "news_attribution": attr.sum(dim=2), "s_true": s_true.reshape(C), "s_attr": attr.sum(dim=(1, 2))}


def explain_recommendations(model, store, behaviors, l_hist: int, session: int, rows: torch.Tensor, **kwargs):
    """explain_rows for one session of `behaviors` and one row of what recommend() returned for it: the history is the
    last `l_hist` clicks exactly as recommend() gathers them (DeviceBatcher.eval_batch, padded with store.pad_row).
    rows (k,) int32 table rows (a filler -1 -- recommend() had fewer than k eligible news -- is refused: ValueError, one
    host read).  kwargs: n_steps, activation, steps_per_batch, feature, projection_once of explain_rows."""
    from .data import DeviceBatcher
    if rows.dim() != 1:
        raise ValueError("explain_recommendations explains ONE session: rows must be (k,), one row of recommend()'s result")
    _text_encoder_of(model)
    if rows.numel() and bool((rows < 0).any().item()):
        raise ValueError("explain_recommendations: rows holds a filler (-1): recommend() found fewer than k eligible news")
    dev = behaviors.hist_off.device
    sess = torch.tensor([int(session)], dtype=torch.int64, device=dev)
    hist = DeviceBatcher(behaviors, l_hist, store.pad_row).eval_batch(sess)[0][0]   # (l_hist,)
    return explain_rows(model, store, hist, rows.to(torch.int32), **kwargs)
