"""Tensor-level entry points of the HIP hot path (forward).  Each function validates its inputs,
sizes the workspace, and makes ONE call into libxnrs_hip.so on the current HIP stream.

Shapes follow the reference's module contracts; masks are fp32 0/1 with a trailing
singleton dim exactly as the reference passes them.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import hip


def _mask2d(m: Optional[torch.Tensor], rows: int, cols: int, what: str) -> Optional[torch.Tensor]:
    if m is None:
        return None
    m = hip.dev_f32(m, what)
    if m.numel() != rows * cols:
        raise RuntimeError(f"{what}: mask of shape {tuple(m.shape)} does not match ({rows}, {cols}, 1)")
    return m.reshape(rows, cols)


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = hip.ACT_NONE, *,
           ids: Optional[torch.Tensor] = None, table_grad: str = "dense"):
    """nn.Linear forward (+ activation fused into the epilogue) on the fp32 MFMA GEMM.  x:(..., K) -> (..., N); with `ids`, x is
    a table (n_rows, K) whose rows the GEMM gathers by id: -> ids.shape + (N,).  Through autograd when anything needs a
    gradient; table_grad picks the kernel that scatters the table's: "dense" (one workgroup per table row: category tables)
    or "sparse" (one per id: tables far larger than the batch)."""
    if table_grad not in ("dense", "sparse"):
        raise ValueError(f"table_grad {table_grad!r}: 'dense' or 'sparse'")
    if _needs_grad(x, weight, bias):
        from . import autograd
        return autograd.linear(x, ids, weight, bias, act, table_grad)
    x = hip.dev_f32(x, "linear input")
    w = hip.dev_f32(weight, "linear weight")
    b = None if bias is None else hip.dev_f32(bias, "linear bias")
    K = x.shape[-1]
    N = w.shape[0]
    if ids is not None and not ids.is_cuda:
        raise hip.XnrsHipError("row ids must live on the HIP device")
    rows = None if ids is None else ids.to(torch.int32).contiguous()
    M = x.numel() // K if ids is None else rows.numel()
    if w.shape[1] != K:
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({M}x{K} and {w.shape[1]}x{N})")
    y = torch.empty(tuple(x.shape[:-1] if ids is None else ids.shape) + (N,), dtype=torch.float32, device=x.device)
    if M:
        hip.check(hip.lib().xnrs_linear_fwd(hip.ptr(x), hip.ptr(rows), 0 if ids is None else 1, hip.ptr(w), hip.ptr(b), hip.ptr(y),
                                            M, N, K, act, hip.stream_ptr(x.device)), "xnrs_linear_fwd")
    return y


def mha_forward(x: torch.Tensor, m: Optional[torch.Tensor], att, dropout_p: float = 0.0, seed: int = 0):
    """layers.MultiHeadAttention.forward (layers.py:120-156).  x:(B,S,D), m:(B,S,1)|None -> (B,S,D)."""
    x = hip.dev_f32(x, "mha input")
    if x.dim() != 3:
        raise RuntimeError(f"MultiHeadAttention expects (B, S, D), got {tuple(x.shape)}")
    B, S, D = x.shape
    m2 = _mask2d(m, B, S, "mha mask")
    p, keep = hip.mha_params(att, dropout_p, seed)
    y = torch.empty_like(x)
    l = hip.lib()
    nbytes = l.xnrs_mha_workspace_bytes(B, S, D)
    ws = hip.workspace(x.device, nbytes)
    hip.check(l.xnrs_mha_fwd(hip.ptr(x), hip.ptr(m2), hip.ref(p), hip.ptr(y), B, S, D, hip.ptr(ws), nbytes,
                             hip.stream_ptr(x.device)), "xnrs_mha_fwd")
    return y


def additive_forward(x: torch.Tensor, m: Optional[torch.Tensor], pool, return_weights: bool = False):
    """layers.AdditiveAttention.forward (layers.py:47-69).  x:(B,N,D), m:(B,N,1)|None -> (B,1,D) [,(B,N,1)]."""
    x = hip.dev_f32(x, "additive input")
    if x.dim() != 3:
        raise RuntimeError(f"AdditiveAttention expects (B, N, D), got {tuple(x.shape)}")
    B, N, D = x.shape
    m2 = _mask2d(m, B, N, "additive mask")
    p, keep = hip.additive_params(pool)
    y = torch.empty((B, 1, D), dtype=torch.float32, device=x.device)
    a = torch.empty((B, N, 1), dtype=torch.float32, device=x.device) if return_weights else None
    l = hip.lib()
    nbytes = l.xnrs_additive_workspace_bytes(B, N, D, p.hidden)
    ws = hip.workspace(x.device, nbytes)
    hip.check(l.xnrs_additive_attention_fwd(hip.ptr(x), hip.ptr(m2), hip.ref(p), hip.ptr(y), hip.ptr(a), B, N, D,
                                            hip.ptr(ws), nbytes, hip.stream_ptr(x.device)),
              "xnrs_additive_attention_fwd")
    return (y, a) if return_weights else y


def masked_mean(x: torch.Tensor, m: torch.Tensor):
    """layers.MaskedMean.forward (layers.py:26-37).  x:(B,N,D), m:(B,N,1) -> (B,1,D)."""
    if torch.is_grad_enabled() and isinstance(x, torch.Tensor) and x.requires_grad:
        from . import autograd
        return autograd.masked_mean(x, m)
    x = hip.dev_f32(x, "masked_mean input")
    B, N, D = x.shape
    m2 = _mask2d(m, B, N, "masked_mean mask")
    y = torch.empty((B, 1, D), dtype=torch.float32, device=x.device)
    hip.check(hip.lib().xnrs_masked_mean_fwd(hip.ptr(x), hip.ptr(m2), hip.ptr(y), B, N, D, hip.stream_ptr(x.device)),
              "xnrs_masked_mean_fwd")
    return y


def collapse_mask(m: torch.Tensor):
    """xnrs.utils.collaps_mask(m, dim=-2) for m:(..., S, 1) -> (..., 1)  (xnrs/utils.py:74-75)."""
    m = hip.dev_f32(m, "mask")
    S = m.shape[-2]
    rows = m.numel() // S
    hm = torch.empty(m.shape[:-2] + (1,), dtype=torch.float32, device=m.device)
    hip.check(hip.lib().xnrs_collapse_mask(hip.ptr(m), hip.ptr(hm), rows, S, hip.stream_ptr(m.device)),
              "xnrs_collapse_mask")
    return hm


def _encoder_params(att, pooler, head, dropout_p: float = 0.0, seed: int = 0, additive_only: Optional[str] = None):
    """-> (pool_kind, MhaParams|None, AdditiveParams|None, HeadParams|None, keepalive list) of one encoder call.
    Without dropout the cached folds of an inference call ride along: fc1 folded behind the attention stage, and -- behind
    attention + additive pooling -- the out-projection folded into the head's first layer.  additive_only: the encoder
    that needs the additive pooler, named in the error."""
    from .models.components import layers
    fold = att if dropout_p == 0.0 else None
    if isinstance(pooler, layers.AdditiveAttention):
        pool_kind, (pp, keep) = hip.POOL_ADDITIVE, hip.additive_params(pooler, fold)
    elif isinstance(pooler, layers.MaskedMean):
        pool_kind, pp, keep = hip.POOL_MEAN, None, []
    else:
        raise hip.XnrsHipError(f"pooler {type(pooler).__name__} has no HIP implementation "
                               "(supported: AdditiveAttention, MaskedMean)")
    if additive_only and pool_kind != hip.POOL_ADDITIVE:
        raise hip.XnrsHipError(f"the {additive_only} encoder needs the additive pooler")
    ap = hp = None
    if att is not None:
        ap, k2 = hip.mha_params(att, dropout_p, seed)
        keep += k2
    if head is not None:
        hp, k3 = hip.head_params(head, fold if pool_kind == hip.POOL_ADDITIVE else None)
        keep += k3
    return pool_kind, ap, pp, hp, keep


def text_encoder_forward(x: torch.Tensor, m: torch.Tensor, att, pooler, head, ids: Optional[torch.Tensor] = None,
                         chunk: int = 0, dropout_p: float = 0.0, seed: int = 0):
    """TextEncoder.forward core (news_encoding.py:48-59) on (n_news,S,D)/(n_news,S) -> (y:(n,E'), hm:(n,)).

    With ``ids`` (int32, (n,)), ``x``/``m`` are the device-resident news-token table and its mask and
    the rows are gathered inside the first GEMM's load phase.  A table stored in bf16
    (NewsStore.astype) goes to xnrs_text_encoder_fwd_bf16: Q|K|V straight from the bf16 rows, or the rows of a pass
    widened in the workspace -- never the table."""
    bf16_table = _is_bf16_table(x, ids)
    x = _dev_bf16(x, "text encoder table") if bf16_table else hip.dev_f32(x, "text encoder input")
    n_tab, S, D = x.shape
    m2 = _mask2d(m, n_tab, S, "text encoder mask")
    if ids is not None:
        if not ids.is_cuda:
            raise hip.XnrsHipError("ids must live on the HIP device")
        ids = ids.to(torch.int32).contiguous()
        n = ids.numel()
    else:
        n = n_tab
    pool_kind, ap, pp, hp, keep = _encoder_params(att, pooler, head, dropout_p, seed)
    A = pp.hidden if pp is not None else 0
    E = hp.out_features if hp is not None else D
    y = torch.empty((n, E), dtype=torch.float32, device=x.device)
    hm = torch.empty((n,), dtype=torch.float32, device=x.device)
    l = hip.lib()
    size_fn, fwd_fn = ((l.xnrs_text_encoder_bf16_workspace_bytes, l.xnrs_text_encoder_fwd_bf16) if bf16_table else
                       (l.xnrs_text_encoder_workspace_bytes, l.xnrs_text_encoder_fwd))
    nbytes = size_fn(n, S, D, A, E, int(att is not None), pool_kind, int(head is not None), chunk)
    ws = hip.workspace(x.device, nbytes)
    hip.check(fwd_fn(hip.ptr(x), hip.ptr(m2), hip.ptr(ids), n, S, D, hip.ref(ap), pool_kind, hip.ref(pp),
                     hip.ref(hp), hip.ptr(y), hip.ptr(hm), chunk, hip.ptr(ws), nbytes, hip.stream_ptr(x.device)),
              "xnrs_text_encoder_fwd_bf16" if bf16_table else "xnrs_text_encoder_fwd")
    return y, hm


def _is_bf16_table(x, ids) -> bool:
    """Is x a news table stored in bf16, addressed by row ids?  (A dense bf16 batch is not a feature: it is widened whole
    like any other non-fp32 input.)"""
    return isinstance(x, torch.Tensor) and x.dtype == torch.bfloat16 and ids is not None


def _dev_bf16(t: torch.Tensor, what: str) -> torch.Tensor:
    if not t.is_cuda:
        raise hip.XnrsHipError(f"{what}: tensor is on {t.device}; xnrs_amd runs on a HIP device only")
    return t.contiguous()


def table_rows_f32(table: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """table[ids] as dense fp32 rows, (ids.numel(), *table.shape[1:]) -- THE widening gather: every consumer of a bf16
    table with ids other than the encoder's own entry widens only the rows it needs through it (one xnrs_gather_rows_bf16
    launch; an fp32 table: xnrs_gather_rows).  No route converts a whole table."""
    if table.dtype != torch.bfloat16:
        return gather_rows(table, ids)
    tab = _dev_bf16(table, "table_rows_f32 table")
    if not ids.is_cuda:
        raise hip.XnrsHipError("ids must live on the HIP device")
    ids = ids.reshape(-1).to(torch.int32).contiguous()
    out = torch.empty((ids.numel(),) + tuple(tab.shape[1:]), dtype=torch.float32, device=tab.device)
    if out.numel():
        hip.check(hip.lib().xnrs_gather_rows_bf16(hip.ptr(tab), hip.ptr(ids), hip.ptr(out), ids.numel(), tab[0].numel(),
                                                  hip.stream_ptr(tab.device)), "xnrs_gather_rows_bf16")
    return out


def _widen_table_call(x, m, ids):
    """(x, m, ids) of an encoder call for the consumers that have no bf16 entry of their own: a bf16 table with ids becomes
    the dense fp32 rows of those ids and their mask rows (ids: None); anything else passes through."""
    if not _is_bf16_table(x, ids):
        return x, m, ids
    flat = ids.reshape(-1)
    md = None if m is None else gather_rows(m.reshape(x.shape[0], -1), flat)
    return table_rows_f32(x, flat), md, None


def linear_bf16(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = hip.ACT_NONE, *,
                ids: Optional[torch.Tensor] = None, gather_s: int = 1, m_rows: Optional[int] = None):
    """xnrs_linear_fwd_bf16 (inference): rows stored in bf16 against fp32 weights, fp32 out.  x:(..., K) bf16; with `ids`, x
    is a table whose blocks of `gather_s` consecutive rows are gathered by id -> (ids.numel() * gather_s, N), or its first
    `m_rows` rows (the last block then only in part)."""
    x = _dev_bf16(x, "linear_bf16 input")
    if x.dtype != torch.bfloat16:
        raise hip.XnrsHipError("linear_bf16: the rows must be torch.bfloat16")
    w = hip.dev_f32(weight, "linear weight")
    b = None if bias is None else hip.dev_f32(bias, "linear bias")
    N, K = w.shape
    rows = None if ids is None else ids.reshape(-1).to(torch.int32).contiguous()
    M = x.numel() // K if ids is None else rows.numel() * int(gather_s)
    if m_rows is not None:
        if not 0 <= int(m_rows) <= M:
            raise ValueError(f"linear_bf16: m_rows = {m_rows} outside [0, {M}]")
        M = int(m_rows)
    if x.shape[-1] != K:
        raise ValueError(f"linear_bf16: rows of {x.shape[-1]} elements against a weight of {K} columns")
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    l = hip.lib()
    nbytes = l.xnrs_linear_bf16_workspace_bytes(N, K)
    ws = hip.workspace(x.device, nbytes)
    hip.check(l.xnrs_linear_fwd_bf16(hip.ptr(x), hip.ptr(rows), 0 if ids is None else int(gather_s), hip.ptr(w), hip.ptr(b),
                                     hip.ptr(y), M, N, K, int(act), hip.ptr(ws), nbytes, hip.stream_ptr(x.device)),
              "xnrs_linear_fwd_bf16")
    return y


def text_encoder_forward_unpadded(x: torch.Tensor, m: torch.Tensor, att, pooler, head, ids: Optional[torch.Tensor] = None,
                                  news_per_pass: int = 8192):
    """TextEncoder.forward computing only what can reach the output (include/xnrs_hip.h:
    xnrs_text_encoder_fwd_unpadded): the unmasked token rows are compacted (index bookkeeping with torch, one
    host sync for the counts), K/V are projected for every row, everything else for the live rows only.
    Inference, additive pooler, 0/1 masks.  Same signature and results as text_encoder_forward."""
    x, m, ids = _widen_table_call(x, m, ids)  # (a bf16 table: the rows of these ids, widened)
    x = hip.dev_f32(x, "text encoder input")
    n_tab, S, D = x.shape
    m2 = _mask2d(m, n_tab, S, "text encoder mask")
    if ids is not None:
        if not ids.is_cuda:
            raise hip.XnrsHipError("ids must live on the HIP device")
        ids = ids.to(torch.int32).contiguous()
        live = m2[ids.long()].ne(0)                      # (n, S) mask of the gathered news
        base = ids.long().unsqueeze(1) * S               # table token row of (news, 0)
    else:
        live = m2.ne(0)
        base = None
    n = live.shape[0]
    pool_kind, ap, pp, hp, keep = _encoder_params(att, pooler, head, additive_only="unpadded")
    bad = ((m2 != 0) & (m2 != 1)).any()
    A, E = pp.hidden, (hp.out_features if hp is not None else D)
    y = torch.empty((n, E), dtype=torch.float32, device=x.device)
    hm = torch.empty((n,), dtype=torch.float32, device=x.device)
    cnt = live.sum(dim=1)
    off = torch.zeros(n + 1, dtype=torch.int64, device=x.device)
    torch.cumsum(cnt, 0, out=off[1:])
    tok = torch.arange(S, device=x.device).unsqueeze(0)
    l = hip.lib()
    step = max(1, int(news_per_pass))
    bounds = list(range(0, n, step)) + [n]
    off_host = off[bounds].tolist()                       # the one host sync (also surfaces `bad`)
    if bool(bad):
        raise hip.XnrsHipError("the unpadded encoder needs a 0/1 mask")
    for c0, c1, r0, r1 in zip(bounds[:-1], bounds[1:], off_host[:-1], off_host[1:]):
        nc, nv = c1 - c0, r1 - r0
        lv = live[c0:c1]
        if ids is not None:
            rows = (base[c0:c1] + tok)[lv].to(torch.int32)             # table token rows of the live tokens
            xp, idp = x, ids[c0:c1]
        else:
            rows = (torch.arange(nc, device=x.device).unsqueeze(1) * S + tok)[lv].to(torch.int32)  # rows inside this pass
            xp, idp = x[c0:c1], None
        roff = (off[c0:c1 + 1] - r0).contiguous()
        nbytes = l.xnrs_text_encoder_unpadded_workspace_bytes(nc, nv, S, D, A, E, int(att is not None), int(head is not None))
        ws = hip.workspace(x.device, nbytes)
        hip.check(l.xnrs_text_encoder_fwd_unpadded(hip.ptr(xp), hip.ptr(idp), nc, S, D, hip.ptr(rows), hip.ptr(roff), nv,
                                                   hip.ref(ap), hip.ref(pp), hip.ref(hp), hip.ptr(y[c0:c1]), hip.ptr(hm[c0:c1]),
                                                   hip.ptr(ws), nbytes, hip.stream_ptr(x.device)),
                  "xnrs_text_encoder_fwd_unpadded")
    return y, hm


def text_encoder_forward_compact(x: torch.Tensor, m: torch.Tensor, att, pooler, head, ids: Optional[torch.Tensor] = None,
                                 chunk: int = 0):
    """The padding-free encoder with the row lists built on the DEVICE (include/xnrs_hip.h: xnrs_text_encoder_fwd_compact):
    same inputs and results as text_encoder_forward for 0/1 masks, no host sync anywhere -- the call can be captured in a
    hipGraph.  Raises XnrsHipError(code -4) for shapes / modes it does not serve (see compact_supported)."""
    x, m, ids = _widen_table_call(x, m, ids)  # (a bf16 table: the rows of these ids, widened)
    x = hip.dev_f32(x, "text encoder input")
    n_tab, S, D = x.shape
    m2 = _mask2d(m, n_tab, S, "text encoder mask")
    if ids is not None:
        if not ids.is_cuda:
            raise hip.XnrsHipError("ids must live on the HIP device")
        ids = ids.to(torch.int32).contiguous()
        n = ids.numel()
    else:
        n = n_tab
    pool_kind, ap, pp, hp, keep = _encoder_params(att, pooler, head, additive_only="compact")
    A, E = pp.hidden, (hp.out_features if hp is not None else D)
    y = torch.empty((n, E), dtype=torch.float32, device=x.device)
    hm = torch.empty((n,), dtype=torch.float32, device=x.device)
    hip.status_word(x.device)  # (registered once: a non-binary mask sets STATUS_NONBINARY_MASK there; hip.check_status())
    l = hip.lib()
    nbytes = l.xnrs_text_encoder_compact_workspace_bytes(n, S, D, A, E, int(att is not None), int(head is not None), chunk)
    # The default pass (262 144 / S news) needs ~3.2 GB of worst-case scratch at D = 768, and hip.workspace is grow-only per
    # stream: bound it (XNRS_COMPACT_WS_MB, default 4096) by shrinking the pass -- the scratch scales with the news per pass
    cap = int(os.environ.get("XNRS_COMPACT_WS_MB", "4096")) << 20
    if chunk == 0 and nbytes > cap:
        per_pass = max(262144 // max(S, 1), 1)
        while nbytes > cap and per_pass > 64:
            per_pass //= 2
            nbytes = l.xnrs_text_encoder_compact_workspace_bytes(n, S, D, A, E, int(att is not None), int(head is not None), per_pass)
        chunk = per_pass
    ws = hip.workspace(x.device, nbytes)
    hip.check(l.xnrs_text_encoder_fwd_compact(hip.ptr(x), hip.ptr(m2), hip.ptr(ids), n, S, D, hip.ref(ap),
                                              hip.ref(pp), hip.ref(hp), hip.ptr(y), hip.ptr(hm), chunk,
                                              hip.ptr(ws), nbytes, hip.stream_ptr(x.device)), "xnrs_text_encoder_fwd_compact")
    return y, hm


def compact_supported(S: int, D: int, att, pooler, x: Optional[torch.Tensor] = None) -> bool:
    """Mirror of the C entry point's preconditions that can be decided on the host without touching the data.  x (optional):
    the fp32 rows the call will be given -- the entry point's products read their row counts on the device and have no
    scalar-load form, so it refuses rows, fc1 or Q/K/V weights off a 16-byte boundary (parameters viewed out of one flat
    buffer); the caller then takes the host-compacted path, which serves them."""
    from .models.components import layers
    if not isinstance(pooler, layers.AdditiveAttention) or hip.get_gemm_mode() != 0 or D % 4 != 0 or S > 512:
        return False
    operands = [pooler.fc1.weight] + ([att.q_linear.weight, att.k_linear.weight, att.v_linear.weight] if att is not None else [])
    if isinstance(x, torch.Tensor) and x.dtype == torch.float32:
        operands.append(x)
    if any(t.is_cuda and t.data_ptr() % 16 != 0 for t in operands):
        return False
    if os.environ.get("XNRS_FC1_ROWDOT", "1") == "0" or os.environ.get("XNRS_GEMM_BUF", "1") == "0":
        return False
    if att is not None:
        dk = D // att.h
        if S > 64 or dk > 64 or dk % 4 != 0 or os.environ.get("XNRS_FOLD_OUT", "1") == "0":
            return False
    return True


def user_encoder_forward(x: torch.Tensor, m: torch.Tensor, att, pooler, head, return_weights: bool = False,
                         dropout_p: float = 0.0, seed: int = 0):
    """UserEncoder.forward core (user_encoding.py:69-81).  x:(B,H,E), m:(B,H,1) -> (B,1,E) [,(B,H,1)]."""
    x = hip.dev_f32(x, "user encoder input")
    B, H, E = x.shape
    m2 = _mask2d(m, B, H, "user encoder mask")
    pool_kind, ap, pp, hp, keep = _encoder_params(att, pooler, head, dropout_p, seed)
    A = pp.hidden if pp is not None else 0
    y = torch.empty((B, 1, E), dtype=torch.float32, device=x.device)
    a = torch.empty((B, H, 1), dtype=torch.float32, device=x.device) if return_weights else None
    l = hip.lib()
    nbytes = l.xnrs_user_encoder_workspace_bytes(B, H, E, A, int(att is not None), pool_kind, int(head is not None))
    ws = hip.workspace(x.device, nbytes)
    hip.check(l.xnrs_user_encoder_fwd(hip.ptr(x), hip.ptr(m2), B, H, E, hip.ref(ap), pool_kind, hip.ref(pp), hip.ref(hp),
                                      hip.ptr(y), hip.ptr(a), hip.ptr(ws), nbytes, hip.stream_ptr(x.device)),
              "xnrs_user_encoder_fwd")
    return (y, a) if return_weights else y


def dot_scoring(u: torch.Tensor, c: torch.Tensor, normalize: bool = False):
    """DotScoring.forward (scoring.py:12-23).  u:(B,1,E), c:(B,C,E) -> (B,C,1)."""
    if torch.is_grad_enabled() and (getattr(u, "requires_grad", False) or getattr(c, "requires_grad", False)):
        from . import autograd
        return autograd.dot_scoring(u, c, normalize)
    return dot_scoring_forward(u, c, normalize)


def dot_scoring_forward(u: torch.Tensor, c: torch.Tensor, normalize: bool = False):
    u = hip.dev_f32(u, "user vector")
    c = hip.dev_f32(c, "candidate vectors")
    B, Cn, E = c.shape
    if u.numel() != B * E:
        raise RuntimeError(f"batch1 and batch2 shapes do not match: u {tuple(u.shape)} vs c {tuple(c.shape)}")
    r = torch.empty((B, Cn, 1), dtype=torch.float32, device=c.device)
    hip.check(hip.lib().xnrs_dot_scoring_fwd(hip.ptr(u), hip.ptr(c), hip.ptr(r), B, Cn, E, int(normalize),
                                             hip.stream_ptr(c.device)), "xnrs_dot_scoring_fwd")
    return r


def _scorer_inputs(u: torch.Tensor, c: torch.Tensor):
    u = hip.dev_f32(u, "user vector")
    c = hip.dev_f32(c, "candidate vectors")
    if c.dim() != 3:
        raise RuntimeError(f"candidate vectors: expected (B, N, E), got {tuple(c.shape)}")
    B, N, E = c.shape
    if u.numel() != B * E or u.shape[-1] != E:
        raise RuntimeError(f"user vector {tuple(u.shape)} does not match candidates {tuple(c.shape)}: expected ({B}, 1, {E})")
    return u, c, B, N, E


def _saved(device, nbytes: int, keep: bool):
    """Activations a training forward hands to its backward (their own buffer), or the per-stream scratch (inference)."""
    if keep:
        return torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=device)
    return hip.workspace(device, nbytes)


def bilinear_scoring(u: torch.Tensor, c: torch.Tensor, scorer):
    """BilinScoring.forward (scoring.py:52-66).  u:(B,1,E), c:(B,N,E) -> (B,N,1)."""
    w, b = scorer.bilin.weight, scorer.bilin.bias
    if _needs_grad(u, c, w, b):
        from . import autograd
        return autograd.bilinear_scoring(u, c, w, b, scorer.normalize)
    return bilinear_scoring_forward(u, c, w, b, scorer.normalize)[0]


def bilinear_scoring_forward(u, c, w, b, normalize: bool, keep: bool = False):
    """-> (scores (B,N,1), saved buffer for the backward)."""
    u, c, B, N, E = _scorer_inputs(u, c)
    w = hip.dev_f32(w, "bilinear weight")
    if tuple(w.shape) != (1, E, E):
        raise RuntimeError(f"bilinear weight {tuple(w.shape)} does not match the embedding size {E}: expected (1, {E}, {E})")
    b = None if b is None else hip.dev_f32(b, "bilinear bias")
    s = torch.empty((B, N, 1), dtype=torch.float32, device=c.device)
    l = hip.lib()
    nbytes = l.xnrs_bilinear_scoring_saved_bytes(B, E, int(normalize))
    saved = _saved(c.device, nbytes, keep)
    if B * N > 0:
        hip.check(l.xnrs_bilinear_scoring_fwd(hip.ptr(u), hip.ptr(c), hip.ptr(w), hip.ptr(b), hip.ptr(s), B, N, E, int(normalize),
                                              hip.ptr(saved), nbytes, hip.stream_ptr(c.device)), "xnrs_bilinear_scoring_fwd")
    return s, saved


def mlp_scoring(u: torch.Tensor, c: torch.Tensor, scorer):
    """FCScoring.forward (scoring.py:93-102) with activation tanh.  u:(B,1,E), c:(B,N,E) -> (B,N,1)."""
    fc1, fc2 = scorer.fc1, scorer.fc2
    if _needs_grad(u, c, fc1, fc2):
        from . import autograd
        return autograd.mlp_scoring(u, c, fc1.weight, fc1.bias, fc2.weight, fc2.bias)
    return mlp_scoring_forward(u, c, fc1.weight, fc1.bias, fc2.weight, fc2.bias)[0]


def _mlp_weights(E, w1, b1, w2, b2):
    w1 = hip.dev_f32(w1, "fc1 weight")
    H = w1.shape[0]
    if w1.dim() != 2 or w1.shape[1] != 2 * E:
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied (fc1 weight {tuple(w1.shape)}, input width {2 * E})")
    w2 = hip.dev_f32(w2, "fc2 weight")
    if tuple(w2.shape) != (1, H):
        raise RuntimeError(f"fc2 weight {tuple(w2.shape)} does not match the hidden size {H}: expected (1, {H})")
    b1 = None if b1 is None else hip.dev_f32(b1, "fc1 bias")
    b2 = None if b2 is None else hip.dev_f32(b2, "fc2 bias")
    return w1, b1, w2, b2, H


def mlp_scoring_forward(u, c, w1, b1, w2, b2, keep: bool = False):
    """-> (scores (B,N,1), saved buffer q | p for the backward)."""
    u, c, B, N, E = _scorer_inputs(u, c)
    w1, b1, w2, b2, H = _mlp_weights(E, w1, b1, w2, b2)
    s = torch.empty((B, N, 1), dtype=torch.float32, device=c.device)
    l = hip.lib()
    nbytes = l.xnrs_mlp_scoring_saved_bytes(B, N, H)
    saved = _saved(c.device, nbytes, keep)
    if B * N > 0:
        hip.check(l.xnrs_mlp_scoring_fwd(hip.ptr(u), hip.ptr(c), hip.ptr(w1), hip.ptr(b1), hip.ptr(w2), hip.ptr(b2), hip.ptr(s),
                                         B, N, E, H, hip.ptr(saved), nbytes, hip.stream_ptr(c.device)), "xnrs_mlp_scoring_fwd")
    return s, saved


def l2_normalize_rows(x: torch.Tensor):
    """x / ||x|| along the last dim (no epsilon, scoring.py:20-22), as a new tensor."""
    x = hip.dev_f32(x, "vectors")
    y = torch.empty_like(x)
    E = x.shape[-1]
    hip.check(hip.lib().xnrs_l2_normalize_rows(hip.ptr(x), hip.ptr(y), x.numel() // max(E, 1), E, hip.stream_ptr(x.device)),
              "xnrs_l2_normalize_rows")
    return y


def mlp_news_proj(vecs: torch.Tensor, w1: torch.Tensor):
    """P = vecs . W1c^T: the candidate half of FCScoring's fc1 over a whole news table (once per evaluation epoch)."""
    vecs = hip.dev_f32(vecs, "news vectors")
    E = vecs.shape[-1]
    w1 = hip.dev_f32(w1, "fc1 weight")
    if w1.dim() != 2 or w1.shape[1] != 2 * E:
        raise RuntimeError(f"fc1 weight {tuple(w1.shape)} does not match news vectors of width {E}")
    H = w1.shape[0]
    rows = vecs.numel() // E
    P = torch.empty((rows, H), dtype=torch.float32, device=vecs.device)
    hip.check(hip.lib().xnrs_mlp_scoring_news_proj(hip.ptr(vecs), rows, E, hip.ptr(w1), H, hip.ptr(P), hip.stream_ptr(vecs.device)),
              "xnrs_mlp_scoring_news_proj")
    return P


def score_csr_bilinear(vecs, cand_rows, cand_sess, u, w, b, relu: bool = True):
    """r[e] = relu?(u[sess[e]] W[0] vecs[rows[e]] + bias) against a pre-encoded news table."""
    vecs = hip.dev_f32(vecs, "news vectors")
    E = vecs.shape[1]
    u = hip.dev_f32(u, "user vectors").reshape(-1, E)
    w = hip.dev_f32(w, "bilinear weight")
    b = None if b is None else hip.dev_f32(b, "bilinear bias")
    n, n_sess = cand_rows.numel(), u.shape[0]
    r = torch.empty((n,), dtype=torch.float32, device=vecs.device)
    l = hip.lib()
    nbytes = l.xnrs_score_csr_scorer_workspace_bytes(n_sess, E)
    ws = hip.workspace(vecs.device, nbytes)
    hip.check(l.xnrs_score_csr_bilinear(hip.ptr(vecs), hip.ptr(cand_rows), hip.ptr(cand_sess), hip.ptr(u), n_sess, hip.ptr(w),
                                        hip.ptr(b), hip.ptr(r), n, E, int(relu), hip.ptr(ws), nbytes, hip.stream_ptr(vecs.device)),
              "xnrs_score_csr_bilinear")
    return r


def score_csr_mlp(P, cand_rows, cand_sess, u, w1, b1, w2, b2, relu: bool = True):
    """r[e] = relu?(w2 . tanh(W1u u[sess[e]] + b1 + P[rows[e]]) + b2), P = mlp_news_proj(table)."""
    P = hip.dev_f32(P, "projected news table")
    E = w1.shape[1] // 2
    u = hip.dev_f32(u, "user vectors").reshape(-1, E)
    w1, b1, w2, b2, H = _mlp_weights(E, w1, b1, w2, b2)
    if P.shape[-1] != H:
        raise RuntimeError(f"projected news table {tuple(P.shape)} does not match the hidden size {H}")
    n, n_sess = cand_rows.numel(), u.shape[0]
    r = torch.empty((n,), dtype=torch.float32, device=P.device)
    l = hip.lib()
    nbytes = l.xnrs_score_csr_scorer_workspace_bytes(n_sess, H)
    ws = hip.workspace(P.device, nbytes)
    hip.check(l.xnrs_score_csr_mlp(hip.ptr(P), hip.ptr(cand_rows), hip.ptr(cand_sess), hip.ptr(u), n_sess, hip.ptr(w1), hip.ptr(b1),
                                   hip.ptr(w2), hip.ptr(b2), hip.ptr(r), n, E, H, int(relu), hip.ptr(ws), nbytes,
                                   hip.stream_ptr(P.device)), "xnrs_score_csr_mlp")
    return r


def _windows(win_lo, win_hi, B: int, dev) -> tuple:
    """The row-window arguments of an xnrs_*_win entry point: () without windows, else the two pointers.  win_lo / win_hi:
    (B,) int32, contiguous, on the table's device, given together; anything else is refused before the call."""
    if win_lo is None and win_hi is None:
        return ()
    if win_lo is None or win_hi is None:
        raise ValueError("windows: win_lo and win_hi are given together or not at all")
    for t, what in ((win_lo, "win_lo"), (win_hi, "win_hi")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or t.numel() != B:
            raise ValueError(f"windows: {what} is a ({B},) int32 tensor, one row bound per user; got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)} "
                             f"{getattr(t, 'dtype', '')}")
        if t.device != dev or not t.is_contiguous():
            raise hip.XnrsHipError(f"windows: {what} must be a contiguous tensor on {dev}")
    return hip.ptr(win_lo), hip.ptr(win_hi)


def _topk(entry: str, table: torch.Tensor, head: tuple, B: int, proj_width: int, k: int, excl_off, excl_rows, pad_row: int,
          ws_query: str = "xnrs_topk_workspace_bytes", win_lo=None, win_hi=None, noise=None):
    """The call every top-k entry point shares behind its own leading arguments `head` -> (rows:(B,k) int32, scores:(B,k)).
    `entry` and `ws_query` name the entry point and its workspace query (xnrs_topk* or xnrs_topk_deep*); with row windows
    the call goes to `entry`_win (xnrs_topk_deep*_win).  noise = (temperature, seed, user_keys): `entry` is one of
    xnrs_topk_sample*_win, which take the three behind k and the windows as nullable pointers."""
    dev = table.device
    win = _windows(win_lo, win_hi, B, dev)
    if noise is not None:
        win = win or (None, None)
        noise = _noise(*noise, B, dev)
    elif win:
        entry += "_win"
    if (excl_off is None) != (excl_rows is None):
        raise RuntimeError("exclusions: excl_off and excl_rows are given together (a CSR over the users) or not at all")
    if excl_off is not None:
        if excl_off.dtype != torch.int64 or excl_rows.dtype != torch.int32 or excl_off.numel() != B + 1:
            raise RuntimeError(f"exclusions: excl_off (B+1,) int64 and excl_rows int32, got {tuple(excl_off.shape)} {excl_off.dtype} "
                               f"and {excl_rows.dtype} for {B} users")
        if excl_off.device != dev or excl_rows.device != dev or not (excl_off.is_contiguous() and excl_rows.is_contiguous()):
            raise hip.XnrsHipError(f"exclusions must be contiguous tensors on {dev}")
    k = int(k)
    rows = torch.empty((B, max(k, 0)), dtype=torch.int32, device=dev)
    scores = torch.empty((B, max(k, 0)), dtype=torch.float32, device=dev)
    l = hip.lib()
    nbytes = getattr(l, ws_query)(B, table.shape[0], proj_width, k)
    ws = hip.workspace(dev, nbytes)
    hip.check(getattr(l, entry)(*head, hip.ptr(excl_off), hip.ptr(excl_rows), *win, int(pad_row), k, *(noise or ()),
                                hip.ptr(rows), hip.ptr(scores), hip.ptr(ws), nbytes, hip.stream_ptr(dev)), entry)
    return rows, scores


def _noise(temperature, seed, user_keys, B: int, dev) -> tuple:
    """The arguments temperature, seed, user_keys of an xnrs_topk_sample*_win entry point.  temperature: a finite float > 0;
    seed: any integer, taken mod 2^64; user_keys: None (the user's index in the call) or a (B,) int64 tensor on the table's
    device.  Anything else is refused before the call."""
    import math
    temperature = float(temperature)
    if not (math.isfinite(temperature) and temperature > 0):
        raise ValueError(f"topk_sample: temperature = {temperature!r}: a finite number above 0")
    if user_keys is not None:
        if not isinstance(user_keys, torch.Tensor) or user_keys.dtype != torch.int64 or user_keys.dim() != 1 or user_keys.numel() != B:
            raise ValueError(f"topk_sample: user_keys is a ({B},) int64 tensor, one key per user; got "
                             f"{tuple(getattr(user_keys, 'shape', ()))} {getattr(user_keys, 'dtype', type(user_keys))}")
        if user_keys.device != dev or not user_keys.is_contiguous():
            raise hip.XnrsHipError(f"topk_sample: user_keys must be a contiguous tensor on {dev}")
    return temperature, int(seed) % (1 << 64), hip.ptr(user_keys)


def _topk_dot(entry, ws_query, table, u, k, excl_off, excl_rows, pad_row, win_lo=None, win_hi=None, noise=None):
    table = hip.dev_f32(table, "news vectors")
    n_rows, E = table.shape
    u = hip.dev_f32(u, "user vectors").reshape(-1, E)
    B = u.shape[0]
    return _topk(entry, table, (hip.ptr(table), n_rows, E, hip.ptr(u), B), B, 0, k, excl_off, excl_rows, pad_row, ws_query,
                 win_lo, win_hi, noise)


def topk_dot(table, u, k: int, excl_off=None, excl_rows=None, pad_row: int = -1):
    """Per user the k rows of `table` with the highest u . table[row] (include/xnrs_hip.h: xnrs_topk) -> (rows, scores)."""
    return _topk_dot("xnrs_topk", "xnrs_topk_workspace_bytes", table, u, k, excl_off, excl_rows, pad_row)


def _topk_bilinear(entry, ws_query, table, u, w, b, k, excl_off, excl_rows, pad_row, win_lo=None, win_hi=None, noise=None):
    table = hip.dev_f32(table, "news vectors")
    n_rows, E = table.shape
    u = hip.dev_f32(u, "user vectors").reshape(-1, E)
    w = hip.dev_f32(w, "bilinear weight")
    b = None if b is None else hip.dev_f32(b, "bilinear bias")
    B = u.shape[0]
    return _topk(entry, table, (hip.ptr(table), n_rows, E, hip.ptr(u), B, hip.ptr(w), hip.ptr(b)), B, E, k,
                 excl_off, excl_rows, pad_row, ws_query, win_lo, win_hi, noise)


def topk_bilinear(table, u, w, b, k: int, excl_off=None, excl_rows=None, pad_row: int = -1):
    """As topk_dot with the score u W[0] table[row] + bias (xnrs_topk_bilinear)."""
    return _topk_bilinear("xnrs_topk_bilinear", "xnrs_topk_workspace_bytes", table, u, w, b, k, excl_off, excl_rows, pad_row)


def _topk_mlp(entry, ws_query, P, u, w1, b1, w2, b2, k, excl_off, excl_rows, pad_row, win_lo=None, win_hi=None, noise=None):
    P = hip.dev_f32(P, "projected news table")
    E = w1.shape[1] // 2
    u = hip.dev_f32(u, "user vectors").reshape(-1, E)
    w1, b1, w2, b2, H = _mlp_weights(E, w1, b1, w2, b2)
    if P.dim() != 2 or P.shape[1] != H:
        raise RuntimeError(f"projected news table {tuple(P.shape)} does not match the hidden size {H}")
    B = u.shape[0]
    return _topk(entry, P, (hip.ptr(P), P.shape[0], E, H, hip.ptr(u), B, hip.ptr(w1), hip.ptr(b1), hip.ptr(w2), hip.ptr(b2)), B, H, k,
                 excl_off, excl_rows, pad_row, ws_query, win_lo, win_hi, noise)


def topk_mlp(P, u, w1, b1, w2, b2, k: int, excl_off=None, excl_rows=None, pad_row: int = -1):
    """As topk_dot with the score w2 . tanh(W1u u + b1 + P[row]) + b2, P = mlp_news_proj(table) (xnrs_topk_mlp)."""
    return _topk_mlp("xnrs_topk_mlp", "xnrs_topk_workspace_bytes", P, u, w1, b1, w2, b2, k, excl_off, excl_rows, pad_row)


_DEEP_WS = "xnrs_topk_deep_workspace_bytes"


def topk_deep_dot(table, u, k: int, excl_off=None, excl_rows=None, pad_row: int = -1, win_lo=None, win_hi=None):
    """topk_dot for 1 <= k <= 1024 (include/xnrs_hip.h: xnrs_topk_deep): the same order and the same score bits, so the first
    128 places are those of topk_dot and topk_deep_dot(k)[:, :j] is topk_deep_dot(j).
    win_lo, win_hi: (B,) int32 row windows (xnrs_topk_deep_win): user b sees the rows [win_lo[b], win_hi[b]) only -- the result
    of the call with every other row on the user's exclusion list, without the list and without scoring those rows."""
    return _topk_dot("xnrs_topk_deep", _DEEP_WS, table, u, k, excl_off, excl_rows, pad_row, win_lo, win_hi)


def topk_deep_bilinear(table, u, w, b, k: int, excl_off=None, excl_rows=None, pad_row: int = -1, win_lo=None, win_hi=None):
    """topk_bilinear for 1 <= k <= 1024 (xnrs_topk_deep_bilinear; with row windows xnrs_topk_deep_bilinear_win)."""
    return _topk_bilinear("xnrs_topk_deep_bilinear", _DEEP_WS, table, u, w, b, k, excl_off, excl_rows, pad_row, win_lo, win_hi)


def topk_deep_mlp(P, u, w1, b1, w2, b2, k: int, excl_off=None, excl_rows=None, pad_row: int = -1, win_lo=None, win_hi=None):
    """topk_mlp for 1 <= k <= 1024 (xnrs_topk_deep_mlp; with row windows xnrs_topk_deep_mlp_win)."""
    return _topk_mlp("xnrs_topk_deep_mlp", _DEEP_WS, P, u, w1, b1, w2, b2, k, excl_off, excl_rows, pad_row, win_lo, win_hi)


def topk_sample_dot(table, u, k: int, temperature: float, seed: int, user_keys=None, excl_off=None, excl_rows=None,
                    pad_row: int = -1, win_lo=None, win_hi=None):
    """A list of k rows per user DRAWN from the scores of topk_deep_dot (include/xnrs_hip.h: xnrs_topk_sample_win): a sample
    without replacement from the Plackett-Luce distribution P(row first) ~ exp(score / temperature), as Gumbel top-k -- the k
    largest of score / temperature + g, g the Gumbel draw of (seed, user_keys[b], row) -> (rows:(B,k) int32, keys:(B,k) fp32),
    best key first; `keys` are the PERTURBED keys, not the scores.  user_keys: (B,) int64 (None: 0 .. B-1); a user's list depends
    on (seed, its key, its scores, temperature) alone, and topk_sample_dot(k)[:, :j] is topk_sample_dot(j).  Exclusions, pad
    row and windows as topk_deep_dot; 1 <= k <= 1024."""
    return _topk_dot("xnrs_topk_sample_win", _DEEP_WS, table, u, k, excl_off, excl_rows, pad_row, win_lo, win_hi,
                     (temperature, seed, user_keys))


def topk_sample_bilinear(table, u, w, b, k: int, temperature: float, seed: int, user_keys=None, excl_off=None, excl_rows=None,
                         pad_row: int = -1, win_lo=None, win_hi=None):
    """topk_sample_dot over the scores of topk_deep_bilinear (xnrs_topk_sample_bilinear_win)."""
    return _topk_bilinear("xnrs_topk_sample_bilinear_win", _DEEP_WS, table, u, w, b, k, excl_off, excl_rows, pad_row, win_lo,
                          win_hi, (temperature, seed, user_keys))


def topk_sample_mlp(P, u, w1, b1, w2, b2, k: int, temperature: float, seed: int, user_keys=None, excl_off=None,
                    excl_rows=None, pad_row: int = -1, win_lo=None, win_hi=None):
    """topk_sample_dot over the scores of topk_deep_mlp (xnrs_topk_sample_mlp_win)."""
    return _topk_mlp("xnrs_topk_sample_mlp_win", _DEEP_WS, P, u, w1, b1, w2, b2, k, excl_off, excl_rows, pad_row, win_lo, win_hi,
                     (temperature, seed, user_keys))


def _csr_check(what: str, off, rows, B: int, dev):
    if off.dtype != torch.int64 or rows.dtype != torch.int32 or off.numel() != B + 1:
        raise RuntimeError(f"{what}: offsets (B+1,) int64 and rows int32, got {tuple(off.shape)} {off.dtype} "
                           f"and {rows.dtype} for {B} users")
    if off.device != dev or rows.device != dev or not (off.is_contiguous() and rows.is_contiguous()):
        raise hip.XnrsHipError(f"{what} must be contiguous tensors on {dev}")


def _rank(entry: str, table: torch.Tensor, head: tuple, B: int, proj_width: int, tgt_off, tgt_rows, excl_off, excl_rows,
          pad_row: int, out, win_lo=None, win_hi=None):
    """The call every rank entry point shares behind its own leading arguments `head` -> (ranks int32, scores fp32), both
    indexed like tgt_rows.  The call writes the positions [tgt_off[0], tgt_off[B]) only: fresh outputs start at -1 / NaN
    everywhere else, the tensors of `out` = (ranks, scores) keep what they held.  With row windows the call goes to
    `entry`_win."""
    dev = table.device
    win = _windows(win_lo, win_hi, B, dev)
    if win:
        entry += "_win"
    if (excl_off is None) != (excl_rows is None):
        raise RuntimeError("exclusions: excl_off and excl_rows are given together (a CSR over the users) or not at all")
    _csr_check("targets", tgt_off, tgt_rows, B, dev)
    if excl_off is not None:
        _csr_check("exclusions", excl_off, excl_rows, B, dev)
    if out is None:
        ranks = torch.full((tgt_rows.numel(),), -1, dtype=torch.int32, device=dev)
        scores = torch.full((tgt_rows.numel(),), float("nan"), dtype=torch.float32, device=dev)
    else:
        ranks, scores = out
        for t, dt in ((ranks, torch.int32), (scores, torch.float32)):
            if t.dtype != dt or t.device != dev or not t.is_contiguous() or t.numel() != tgt_rows.numel():
                raise RuntimeError(f"out: (ranks int32, scores fp32), contiguous on {dev}, one entry per target row "
                                   f"({tgt_rows.numel()}); got {tuple(t.shape)} {t.dtype} on {t.device}")
    l = hip.lib()
    nbytes = l.xnrs_rank_workspace_bytes(B, proj_width)
    ws = hip.workspace(dev, nbytes)
    hip.check(getattr(l, entry)(*head, hip.ptr(tgt_off), hip.ptr(tgt_rows), hip.ptr(excl_off), hip.ptr(excl_rows), *win,
                                int(pad_row), hip.ptr(ranks), hip.ptr(scores), hip.ptr(ws), nbytes, hip.stream_ptr(dev)), entry)
    return ranks, scores


def rank_dot(table, u, tgt_off, tgt_rows, excl_off=None, excl_rows=None, pad_row: int = -1, out=None, win_lo=None, win_hi=None):
    """For every (user, target row) of the CSR tgt_off / tgt_rows: how many eligible rows of `table` come before the target
    in the order of topk_dot, and the target's score (include/xnrs_hip.h: xnrs_rank) -> (ranks, scores).
    win_lo, win_hi: (B,) int32 row windows (xnrs_rank_win): only the rows [win_lo[b], win_hi[b]) compete; a target outside its
    user's window is ranked all the same."""
    table = hip.dev_f32(table, "news vectors")
    n_rows, E = table.shape
    u = hip.dev_f32(u, "user vectors").reshape(-1, E)
    B = u.shape[0]
    return _rank("xnrs_rank", table, (hip.ptr(table), n_rows, E, hip.ptr(u), B), B, 0, tgt_off, tgt_rows, excl_off, excl_rows,
                 pad_row, out, win_lo, win_hi)


def rank_bilinear(table, u, w, b, tgt_off, tgt_rows, excl_off=None, excl_rows=None, pad_row: int = -1, out=None, win_lo=None,
                  win_hi=None):
    """As rank_dot with the score u W[0] table[row] + bias (xnrs_rank_bilinear; with row windows xnrs_rank_bilinear_win)."""
    table = hip.dev_f32(table, "news vectors")
    n_rows, E = table.shape
    u = hip.dev_f32(u, "user vectors").reshape(-1, E)
    w = hip.dev_f32(w, "bilinear weight")
    b = None if b is None else hip.dev_f32(b, "bilinear bias")
    B = u.shape[0]
    return _rank("xnrs_rank_bilinear", table, (hip.ptr(table), n_rows, E, hip.ptr(u), B, hip.ptr(w), hip.ptr(b)), B, E,
                 tgt_off, tgt_rows, excl_off, excl_rows, pad_row, out, win_lo, win_hi)


def rank_mlp(P, u, w1, b1, w2, b2, tgt_off, tgt_rows, excl_off=None, excl_rows=None, pad_row: int = -1, out=None, win_lo=None,
             win_hi=None):
    """As rank_dot with the score w2 . tanh(W1u u + b1 + P[row]) + b2, P = mlp_news_proj(table) (xnrs_rank_mlp; with row
    windows xnrs_rank_mlp_win)."""
    P = hip.dev_f32(P, "projected news table")
    E = w1.shape[1] // 2
    u = hip.dev_f32(u, "user vectors").reshape(-1, E)
    w1, b1, w2, b2, H = _mlp_weights(E, w1, b1, w2, b2)
    if P.dim() != 2 or P.shape[1] != H:
        raise RuntimeError(f"projected news table {tuple(P.shape)} does not match the hidden size {H}")
    B = u.shape[0]
    return _rank("xnrs_rank_mlp", P, (hip.ptr(P), P.shape[0], E, H, hip.ptr(u), B, hip.ptr(w1), hip.ptr(b1), hip.ptr(w2),
                                      hip.ptr(b2)), B, H, tgt_off, tgt_rows, excl_off, excl_rows, pad_row, out,
                 win_lo, win_hi)


def _table_loss_check(table, up, tgt_off, tgt_rows, excl_off, excl_rows):
    """What can be refused before anything touches the device: the table's shape and the CSRs' dtypes and lengths."""
    if not isinstance(table, torch.Tensor) or table.dim() != 2 or table.shape[1] < 1:
        raise RuntimeError(f"news vectors: a (n_rows, E) table, got {tuple(getattr(table, 'shape', ()))}")
    E = table.shape[1]
    if not isinstance(up, torch.Tensor) or up.numel() % E:
        raise RuntimeError(f"user vectors: (B, {E}) or (B, 1, {E}), got {tuple(getattr(up, 'shape', ()))}")
    B = up.numel() // E
    if (excl_off is None) != (excl_rows is None):
        raise RuntimeError("exclusions: excl_off and excl_rows are given together (a CSR over the users) or not at all")
    _csr_check("targets", tgt_off, tgt_rows, B, table.device)
    if excl_off is not None:
        _csr_check("exclusions", excl_off, excl_rows, B, table.device)


def _table_loss_args(table, up, tgt_off, tgt_rows, excl_off, excl_rows, win_lo, win_hi, bias):
    """The checked operands of xnrs_table_loss_fwd / _bwd: (table, up, bias, B, the pointer tuple of both calls)."""
    _table_loss_check(table, up, tgt_off, tgt_rows, excl_off, excl_rows)
    table = hip.dev_f32(table, "news vectors")
    n_rows, E = table.shape
    up = hip.dev_f32(up, "user vectors").reshape(-1, E)
    bias = None if bias is None else hip.dev_f32(bias, "score bias").reshape(-1)[:1]
    B, dev = up.shape[0], table.device
    win = _windows(win_lo, win_hi, B, dev) or (None, None)
    if (excl_off is None) != (excl_rows is None):
        raise RuntimeError("exclusions: excl_off and excl_rows are given together (a CSR over the users) or not at all")
    _csr_check("targets", tgt_off, tgt_rows, B, dev)
    if excl_off is not None:
        _csr_check("exclusions", excl_off, excl_rows, B, dev)
    if excl_rows is not None and excl_rows.numel() == 0:  # (an empty tensor has no address: no exclusions at all)
        excl_off = excl_rows = None
    # (no target at all: the offsets are all equal and the rows are never read, but the entry point wants an address)
    rows = tgt_rows if tgt_rows.numel() else torch.zeros((1,), dtype=torch.int32, device=dev)
    head = (hip.ptr(table), n_rows, E, hip.ptr(up), hip.ptr(bias), B, hip.ptr(tgt_off), hip.ptr(rows), hip.ptr(excl_off),
            hip.ptr(excl_rows), *win)
    return table, up, bias, B, (head, rows)


def table_loss_forward(table, up, tgt_off, tgt_rows, excl_off=None, excl_rows=None, pad_row: int = -1, win_lo=None, win_hi=None,
                       bias=None):
    """xnrs_table_loss_fwd -> (loss:(T,), scores:(T,), lse:(B,)); positions outside [tgt_off[0], tgt_off[B]) hold 0 / NaN."""
    table, up, bias, B, head = _table_loss_args(table, up, tgt_off, tgt_rows, excl_off, excl_rows, win_lo, win_hi, bias)
    dev, T = table.device, tgt_rows.numel()
    loss = torch.zeros((T,), dtype=torch.float32, device=dev)
    scores = torch.full((T,), float("nan"), dtype=torch.float32, device=dev)
    lse = torch.empty((B,), dtype=torch.float32, device=dev)
    l = hip.lib()
    nbytes = l.xnrs_table_loss_workspace_bytes(B, table.shape[0], table.shape[1], 0)
    ws = hip.workspace(dev, nbytes)
    hip.check(l.xnrs_table_loss_fwd(*head[0], int(pad_row), hip.ptr(scores), hip.ptr(loss), hip.ptr(lse), hip.ptr(ws), nbytes,
                                    hip.stream_ptr(dev)), "xnrs_table_loss_fwd")
    return loss, scores, lse


def table_loss_backward(table, up, tgt_off, tgt_rows, excl_off, excl_rows, pad_row, win_lo, win_hi, bias, scores, lse, g,
                        want_d_up: bool = True, want_d_table: bool = True):
    """xnrs_table_loss_bwd -> (d_up or None, d_table or None): a gradient that is not wanted is not computed."""
    table, up, bias, B, head = _table_loss_args(table, up, tgt_off, tgt_rows, excl_off, excl_rows, win_lo, win_hi, bias)
    dev = table.device
    g = hip.dev_f32(g, "upstream gradient").reshape(-1)
    if g.numel() != tgt_rows.numel() or scores.numel() != tgt_rows.numel() or lse.numel() != B:
        raise RuntimeError(f"table loss backward: g and scores have one entry per target row ({tgt_rows.numel()}), lse one per "
                           f"user ({B}); got {g.numel()}, {scores.numel()}, {lse.numel()}")
    d_up = torch.empty_like(up) if want_d_up else None
    d_table = torch.empty_like(table) if want_d_table else None
    if not (want_d_up or want_d_table):
        return None, None
    l = hip.lib()
    nbytes = l.xnrs_table_loss_workspace_bytes(B, table.shape[0], table.shape[1], int(want_d_table))
    ws = hip.workspace(dev, nbytes)
    hip.check(l.xnrs_table_loss_bwd(*head[0], int(pad_row), hip.ptr(scores), hip.ptr(lse), hip.ptr(g), hip.ptr(d_up), hip.ptr(d_table),
                                    hip.ptr(ws), nbytes, hip.stream_ptr(dev)), "xnrs_table_loss_bwd")
    return d_up, d_table


def table_loss(table, up, tgt_off, tgt_rows, excl_off=None, excl_rows=None, pad_row: int = -1, win_lo=None, win_hi=None, bias=None):
    """The softmax ranking loss of every (user, target row) of the CSR tgt_off / tgt_rows against ALL eligible rows of `table`
    (include/xnrs_hip.h: xnrs_table_loss_fwd) -> (loss:(T,), scores:(T,), lse:(B,)), T = tgt_rows.numel().  The negatives of
    a user are the rows rank_dot counts, minus every target of the user; loss = logaddexp(score, lse) - score, 0 for a query
    without an answer (score NaN) and for a user without negatives (lse -inf).  Differentiable in `table` and `up` (a
    gradient that nobody asks for is not computed); `scores` and `lse` carry no gradient, and neither does `bias`, which
    cancels in the loss."""
    from . import autograd
    _table_loss_check(table, up, tgt_off, tgt_rows, excl_off, excl_rows)
    return autograd.table_loss(table, up, tgt_off, tgt_rows, excl_off, excl_rows, pad_row, win_lo, win_hi, bias)


def _list_loss_check(table, up, tgt_off, tgt_rows, neg_rows):
    """What can be refused before anything touches the device: the table's shape, the target CSR and the lists."""
    _table_loss_check(table, up, tgt_off, tgt_rows, None, None)
    B = up.numel() // table.shape[1]
    if not isinstance(neg_rows, torch.Tensor) or neg_rows.dtype != torch.int32 or neg_rows.dim() != 2 or neg_rows.shape[0] != B:
        raise RuntimeError(f"negative lists: a ({B}, L) int32 tensor, one list of rows per user; got "
                           f"{tuple(getattr(neg_rows, 'shape', ()))} {getattr(neg_rows, 'dtype', type(neg_rows))}")
    if neg_rows.device != table.device or not neg_rows.is_contiguous():
        raise hip.XnrsHipError(f"negative lists must be a contiguous tensor on {table.device}")


def _list_loss_args(table, up, tgt_off, tgt_rows, neg_rows, bias):
    """The checked operands of xnrs_list_loss_fwd / _bwd -> (table, up, B, L, head, keep): head holds the leading arguments of
    both calls as raw addresses; keep holds the tensors behind those addresses that exist only here (the stand-in for an empty
    tgt_rows, the fp32 bias) and must stay referenced by the caller until the call has been enqueued."""
    _list_loss_check(table, up, tgt_off, tgt_rows, neg_rows)
    table = hip.dev_f32(table, "news vectors")
    n_rows, E = table.shape
    up = hip.dev_f32(up, "user vectors").reshape(-1, E)
    bias = None if bias is None else hip.dev_f32(bias, "score bias").reshape(-1)[:1]
    B, L, dev = up.shape[0], neg_rows.shape[1], table.device
    # (no target at all: the offsets are all equal and the rows are never read, but the entry point wants an address)
    rows = tgt_rows if tgt_rows.numel() else torch.zeros((1,), dtype=torch.int32, device=dev)
    head = (hip.ptr(table), n_rows, E, hip.ptr(up), hip.ptr(bias), B, hip.ptr(tgt_off), hip.ptr(rows), hip.ptr(neg_rows), L)
    return table, up, B, L, head, (rows, bias)


def list_loss_forward(table, up, tgt_off, tgt_rows, neg_rows, pad_row: int = -1, bias=None):
    """xnrs_list_loss_fwd -> (loss:(T,), scores:(T,), lse:(B,), neg_scores:(B,L)); positions of loss / scores outside
    [tgt_off[0], tgt_off[B]) hold 0 / NaN."""
    table, up, B, L, head, keep = _list_loss_args(table, up, tgt_off, tgt_rows, neg_rows, bias)
    dev, T = table.device, tgt_rows.numel()
    loss = torch.zeros((T,), dtype=torch.float32, device=dev)
    scores = torch.full((T,), float("nan"), dtype=torch.float32, device=dev)
    lse = torch.empty((B,), dtype=torch.float32, device=dev)
    neg_scores = torch.empty((B, L), dtype=torch.float32, device=dev)
    l = hip.lib()
    nbytes = l.xnrs_list_loss_workspace_bytes(B, L, T, table.shape[1], 0)
    ws = hip.workspace(dev, nbytes)
    # (no target at all: nothing per query is written, but the entry point wants addresses)
    out = (scores, loss) if T else (torch.empty((1,), dtype=torch.float32, device=dev),) * 2
    hip.check(l.xnrs_list_loss_fwd(*head, int(pad_row), hip.ptr(out[0]), hip.ptr(out[1]), hip.ptr(lse), hip.ptr(neg_scores),
                                   hip.ptr(ws), nbytes, hip.stream_ptr(dev)), "xnrs_list_loss_fwd")
    del keep  # (held until here)
    return loss, scores, lse, neg_scores


def list_loss_order(n_rows: int, tgt_rows, neg_rows, scores, neg_scores):
    """The `order` operand of xnrs_list_loss_bwd, built on the device without a host read: the B L slots, then the T queries,
    stably sorted by row, the entries that carry no gradient (NaN in neg_scores / scores) behind all others."""
    key = torch.cat((torch.where(torch.isnan(neg_scores.reshape(-1)), n_rows, neg_rows.reshape(-1)),
                     torch.where(torch.isnan(scores.reshape(-1)), n_rows, tgt_rows.reshape(-1))))
    return torch.sort(key, stable=True).indices.to(torch.int32)


def list_loss_backward(table, up, tgt_off, tgt_rows, neg_rows, pad_row, bias, scores, lse, neg_scores, g, want_d_up: bool = True,
                       want_d_table: bool = True):
    """xnrs_list_loss_bwd -> (d_up or None, d_table or None): a gradient that is not wanted is not computed (and without
    d_table no order is sorted)."""
    table, up, B, L, head, keep = _list_loss_args(table, up, tgt_off, tgt_rows, neg_rows, bias)
    dev, T = table.device, tgt_rows.numel()
    g = hip.dev_f32(g, "upstream gradient").reshape(-1)
    if g.numel() != T or scores.numel() != T or lse.numel() != B or tuple(neg_scores.shape) != (B, L):
        raise RuntimeError(f"list loss backward: g and scores have one entry per target row ({T}), lse one per user ({B}), "
                           f"neg_scores one per slot ({B}, {L}); got {g.numel()}, {scores.numel()}, {lse.numel()}, "
                           f"{tuple(neg_scores.shape)}")
    if not (want_d_up or want_d_table):
        return None, None
    d_up = torch.empty_like(up) if want_d_up else None
    d_table = torch.empty_like(table) if want_d_table else None
    order = list_loss_order(table.shape[0], tgt_rows, neg_rows, scores, neg_scores) if want_d_table else None
    l = hip.lib()
    nbytes = l.xnrs_list_loss_workspace_bytes(B, L, T, table.shape[1], int(want_d_table))
    ws = hip.workspace(dev, nbytes)
    per_query = (scores, g) if T else (torch.empty((1,), dtype=torch.float32, device=dev),) * 2  # (as in the forward)
    hip.check(l.xnrs_list_loss_bwd(*head, int(pad_row), hip.ptr(per_query[0]), hip.ptr(lse), hip.ptr(neg_scores),
                                   hip.ptr(per_query[1]), hip.ptr(order), hip.ptr(d_up), hip.ptr(d_table), hip.ptr(ws), nbytes, hip.stream_ptr(dev)),
              "xnrs_list_loss_bwd")
    del keep  # (held until here)
    return d_up, d_table


def list_loss(table, up, tgt_off, tgt_rows, neg_rows, pad_row: int = -1, bias=None):
    """The softmax ranking loss of every (user, target row) of the CSR tgt_off / tgt_rows against the rows the user LISTS in
    neg_rows:(B, L) int32 (include/xnrs_hip.h: xnrs_list_loss_fwd) -> (loss:(T,), scores:(T,), lse:(B,), neg_scores:(B,L)).
    A slot is a negative when its row is inside the table, not pad_row and no target of the user; every other slot (the -1
    fillers of topk_deep, foreign ids, the pad row, a target) is empty and NaN in neg_scores; a row listed twice counts
    twice.  loss = logaddexp(score, lse) - score, 0 for a query without an answer (score NaN) and for a user without
    negatives (lse -inf).  Differentiable in `table` and `up` (a gradient that nobody asks for is not computed); scores, lse
    and neg_scores carry no gradient, and neither does `bias`, which cancels in the loss."""
    from . import autograd
    _list_loss_check(table, up, tgt_off, tgt_rows, neg_rows)
    return autograd.list_loss(table, up, tgt_off, tgt_rows, neg_rows, pad_row, bias)


def _list_xent_check(table, up, rows, weights):
    """What can be refused before anything touches the device: the table's shape, the lists and their weights."""
    if not isinstance(table, torch.Tensor) or table.dim() != 2 or table.shape[1] < 1:
        raise RuntimeError(f"news vectors: a (n_rows, E) table, got {tuple(getattr(table, 'shape', ()))}")
    E = table.shape[1]
    if not isinstance(up, torch.Tensor) or up.shape[-1:] != (E,):
        raise RuntimeError(f"user vectors: (..., {E}) as the table's rows, got {tuple(getattr(up, 'shape', ()))}")
    B = up.numel() // E
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or rows.dim() != 2 or rows.shape[0] != B:
        raise RuntimeError(f"row lists: a ({B}, L) int32 tensor, one list of rows per user; got "
                           f"{tuple(getattr(rows, 'shape', ()))} {getattr(rows, 'dtype', type(rows))}")
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or tuple(weights.shape) != tuple(rows.shape):
        raise RuntimeError(f"slot weights: a {tuple(rows.shape)} float32 tensor, one weight per slot; got "
                           f"{tuple(getattr(weights, 'shape', ()))} {getattr(weights, 'dtype', type(weights))}")
    if B * rows.shape[1] > 2 ** 31 - 1:
        raise RuntimeError(f"row lists: {B} x {rows.shape[1]} slots, more than 2^31 - 1")
    for t, what in ((rows, "row lists"), (weights, "slot weights")):
        if t.device != table.device or not t.is_contiguous():
            raise hip.XnrsHipError(f"{what} must be a contiguous tensor on {table.device}")


def _list_xent_args(table, up, rows, weights, bias):
    """The checked operands of xnrs_list_xent_fwd / _bwd -> (table, up, B, L, head, keep), as _list_loss_args."""
    _list_xent_check(table, up, rows, weights)
    table = hip.dev_f32(table, "news vectors")
    n_rows, E = table.shape
    up = hip.dev_f32(up, "user vectors").reshape(-1, E)
    bias = None if bias is None else hip.dev_f32(bias, "score bias").reshape(-1)[:1]
    B, L = up.shape[0], rows.shape[1]
    head = (hip.ptr(table), n_rows, E, hip.ptr(up), hip.ptr(bias), B, hip.ptr(rows), hip.ptr(weights), L)
    return table, up, B, L, head, (bias,)


def list_xent_forward(table, up, rows, weights, pad_row: int = -1, bias=None):
    """xnrs_list_xent_fwd -> (loss:(B,), lse:(B,), slot_scores:(B,L))."""
    table, up, B, L, head, keep = _list_xent_args(table, up, rows, weights, bias)
    dev = table.device
    loss = torch.empty((B,), dtype=torch.float32, device=dev)
    lse = torch.empty((B,), dtype=torch.float32, device=dev)
    slot_scores = torch.empty((B, L), dtype=torch.float32, device=dev)
    l = hip.lib()
    nbytes = l.xnrs_list_xent_workspace_bytes(B, L, table.shape[1], 0)
    ws = hip.workspace(dev, nbytes)
    hip.check(l.xnrs_list_xent_fwd(*head, int(pad_row), hip.ptr(loss), hip.ptr(lse), hip.ptr(slot_scores), hip.ptr(ws), nbytes,
                                   hip.stream_ptr(dev)), "xnrs_list_xent_fwd")
    del keep  # (held until here)
    return loss, lse, slot_scores


def list_xent_order(n_rows: int, rows, slot_scores):
    """The `order` operand of xnrs_list_xent_bwd: the B L slots stably sorted by row, the empty ones (NaN in slot_scores)
    behind all others -- list_loss_order without queries."""
    none = rows.new_zeros((0,))
    return list_loss_order(n_rows, none, rows, slot_scores.new_zeros((0,)), slot_scores)


def list_xent_backward(table, up, rows, weights, pad_row, bias, lse, slot_scores, g, want_d_up: bool = True,
                       want_d_table: bool = True):
    """xnrs_list_xent_bwd -> (d_up or None, d_table or None): a gradient that is not wanted is not computed (and without
    d_table no order is sorted)."""
    table, up, B, L, head, keep = _list_xent_args(table, up, rows, weights, bias)
    dev = table.device
    g = hip.dev_f32(g, "upstream gradient").reshape(-1)
    if g.numel() != B or lse.numel() != B or tuple(slot_scores.shape) != (B, L):
        raise RuntimeError(f"list xent backward: g and lse have one entry per user ({B}), slot_scores one per slot ({B}, {L}); "
                           f"got {g.numel()}, {lse.numel()}, {tuple(slot_scores.shape)}")
    if not (want_d_up or want_d_table):
        return None, None
    d_up = torch.empty_like(up) if want_d_up else None
    d_table = torch.empty_like(table) if want_d_table else None
    order = list_xent_order(table.shape[0], rows, slot_scores) if want_d_table else None
    l = hip.lib()
    nbytes = l.xnrs_list_xent_workspace_bytes(B, L, table.shape[1], int(want_d_table))
    ws = hip.workspace(dev, nbytes)
    hip.check(l.xnrs_list_xent_bwd(*head, int(pad_row), hip.ptr(lse), hip.ptr(slot_scores), hip.ptr(g), hip.ptr(order),
                                   hip.ptr(d_up), hip.ptr(d_table), hip.ptr(ws), nbytes, hip.stream_ptr(dev)),
              "xnrs_list_xent_bwd")
    del keep  # (held until here)
    return d_up, d_table


def list_xent(table, up, rows, weights, pad_row: int = -1, bias=None):
    """The soft-target listwise loss: the cross-entropy between the weights a caller gives the rows each user LISTS and the
    softmax of the user's scores over the same slots (include/xnrs_hip.h: xnrs_list_xent_fwd) -> (loss:(B,), lse:(B,),
    slot_scores:(B,L)).  rows:(B, L) int32, weights:(B, L) float32.  A slot is filled when its row is inside the table and
    not pad_row; every other slot (the -1 fillers of topk_deep, foreign ids, the pad row) is empty: NaN in slot_scores, its
    weight ignored.  A row listed twice is two slots.  loss[b] = sum over filled slots of w (lse[b] - s): with weights
    that sum to 1 the cross-entropy of that distribution against softmax(s) (teacher scores: distillation; graded labels:
    ListNet).  A user without a filled slot (lse -inf) or with all weights 0 has loss 0 and no gradient.  Differentiable
    in `table` and `up` (a gradient that nobody asks for is not computed); weights, lse and slot_scores carry no gradient,
    and neither does `bias`, which shifts every score of a user alike."""
    from . import autograd
    _list_xent_check(table, up, rows, weights)
    return autograd.list_xent(table, up, rows, weights, pad_row, bias)


MMR_REL = {"raw": hip._CONSTANTS["MMR_REL_RAW"], "minmax": hip._CONSTANTS["MMR_REL_MINMAX"]}  # include/xnrs_hip.h


def row_inv_norms(vecs: torch.Tensor):
    """inv:(n_rows,) = 1 / ||vecs[r]||, 0 for a zero row (include/xnrs_hip.h: xnrs_row_inv_norms): once per encoded table, the
    `inv` operand of mmr_rerank and list_diversity."""
    vecs = hip.dev_f32(vecs, "news vectors")
    if vecs.dim() != 2:
        raise RuntimeError(f"news vectors: a (n_rows, E) table, got {tuple(vecs.shape)}")
    n_rows, E = vecs.shape
    inv = torch.empty((n_rows,), dtype=torch.float32, device=vecs.device)
    hip.check(hip.lib().xnrs_row_inv_norms(hip.ptr(vecs), n_rows, E, hip.ptr(inv), hip.stream_ptr(vecs.device)), "xnrs_row_inv_norms")
    return inv


def _lists(rows, what: str):
    """The (B, n) int32 check of every list operand: candidate lists and recommended lists."""
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or rows.dim() != 2:
        raise RuntimeError(f"{what}: a (B, n) int32 tensor, one list of rows per session; got "
                           f"{tuple(getattr(rows, 'shape', ()))} {getattr(rows, 'dtype', type(rows))}")


def _row_categories(row_category, dev):
    if not isinstance(row_category, torch.Tensor) or row_category.dtype != torch.int32 or row_category.dim() != 1:
        raise RuntimeError(f"row categories: a (n_rows,) int32 tensor, one category per table row; got "
                           f"{tuple(getattr(row_category, 'shape', ()))} {getattr(row_category, 'dtype', type(row_category))}")
    if row_category.device != dev or not row_category.is_contiguous():
        raise hip.XnrsHipError(f"row categories must be a contiguous tensor on {dev}")


def _pool_scores(who: str, pool_scores, pool_rows, rel: str):
    """(the checked candidate scores of the checked candidate lists, the code of `rel`) of a re-ranker."""
    if rel not in MMR_REL:
        raise ValueError(f"{who}: rel is one of {sorted(MMR_REL)}, got {rel!r}")
    pool_scores = hip.dev_f32(pool_scores, "candidate scores")
    if tuple(pool_scores.shape) != tuple(pool_rows.shape) or pool_scores.device != pool_rows.device:
        raise RuntimeError(f"candidate scores {tuple(pool_scores.shape)} on {pool_scores.device} do not match the candidate lists "
                           f"{tuple(pool_rows.shape)} on {pool_rows.device}")
    return pool_scores, MMR_REL[rel]


def _picks(B: int, k: int, dev):
    """The (rows, scores, pos) outputs of a re-ranker."""
    return tuple(torch.empty((B, max(k, 0)), dtype=t, device=dev) for t in (torch.int32, torch.float32, torch.int32))


def _diversity_operands(vecs, inv, rows, what: str):
    """The checked table, norms and lists of xnrs_mmr_rerank / xnrs_list_diversity."""
    vecs = hip.dev_f32(vecs, "news vectors")
    if vecs.dim() != 2:
        raise RuntimeError(f"news vectors: a (n_rows, E) table, got {tuple(vecs.shape)}")
    inv = hip.dev_f32(inv, "inverse row norms")
    if inv.dim() != 1 or inv.numel() != vecs.shape[0]:
        raise RuntimeError(f"inverse row norms: one per table row ({vecs.shape[0]},), got {tuple(inv.shape)} (row_inv_norms(vecs))")
    _lists(rows, what)
    if rows.device != vecs.device or inv.device != vecs.device or not rows.is_contiguous():
        raise hip.XnrsHipError(f"{what} and the inverse row norms must be contiguous tensors on {vecs.device}")
    return vecs, inv


def mmr_rerank(vecs, inv, pool_rows, pool_scores, k: int, lam: float, rel: str = "minmax"):
    """Greedy MMR over per-session candidate lists (include/xnrs_hip.h: xnrs_mmr_rerank) -> (rows:(B,k) int32, scores:(B,k)
    fp32, pos:(B,k) int32): step by step the valid place of the pool with the largest lam * relevance - (1 - lam) * (largest
    cosine to a place selected so far), equal objectives to the lower place; scores are the pool's own bits, pos the place in
    the pool; -1 / -inf / -1 once the valid places run out.  pool_rows:(B,P) int32 (-1: empty), pool_scores:(B,P) fp32, e.g.
    what topk_deep_* returned; inv = row_inv_norms(vecs); rel "minmax" (per-session min-max of the valid scores) or "raw"."""
    vecs, inv = _diversity_operands(vecs, inv, pool_rows, "candidate lists")
    pool_scores, rel = _pool_scores("mmr_rerank()", pool_scores, pool_rows, rel)
    (B, P), k, dev = pool_rows.shape, int(k), vecs.device
    rows, scores, pos = _picks(B, k, dev)
    hip.check(hip.lib().xnrs_mmr_rerank(hip.ptr(vecs), hip.ptr(inv), vecs.shape[0], vecs.shape[1], hip.ptr(pool_rows),
                                        hip.ptr(pool_scores), B, P, k, float(lam), rel, hip.ptr(rows), hip.ptr(scores),
                                        hip.ptr(pos), hip.stream_ptr(dev)), "xnrs_mmr_rerank")
    return rows, scores, pos


def list_diversity(vecs, inv, rows, row_category=None, n_categories: int = 0):
    """Per list of rows:(B,k) int32 (-1 or out of the table: no place) -> (ild:(B,) fp32, n:(B,) int32, n_cat:(B,) int32,
    diff_cat:(B,) int32) (include/xnrs_hip.h: xnrs_list_diversity): the mean of 1 - cos over the pairs of valid places (0
    below two), the valid places, and -- with row_category:(n_rows,) int32 and its n_categories -- the distinct categories and
    the pairs of differing category (both None without row_category).  inv = row_inv_norms(vecs)."""
    vecs, inv = _diversity_operands(vecs, inv, rows, "lists")
    (B, k), dev = rows.shape, vecs.device
    if row_category is not None:
        _row_categories(row_category, dev)
        if row_category.numel() != vecs.shape[0]:
            raise RuntimeError(f"row categories: one per table row ({vecs.shape[0]},), got {tuple(row_category.shape)}")
    ild = torch.empty((B,), dtype=torch.float32, device=dev)
    n = torch.empty((B,), dtype=torch.int32, device=dev)
    n_cat = None if row_category is None else torch.empty((B,), dtype=torch.int32, device=dev)
    diff_cat = None if row_category is None else torch.empty((B,), dtype=torch.int32, device=dev)
    hip.check(hip.lib().xnrs_list_diversity(hip.ptr(vecs), hip.ptr(inv), vecs.shape[0], vecs.shape[1], hip.ptr(rows), B, k,
                                            hip.ptr(row_category), int(n_categories), hip.ptr(ild), hip.ptr(n), hip.ptr(n_cat),
                                            hip.ptr(diff_cat), hip.stream_ptr(dev)), "xnrs_list_diversity")
    return ild, n, n_cat, diff_cat


def _calibration_operands(rows, row_category, n_categories: int, target, what: str):
    """The checked lists, (n_rows,) int32 categories and (B, n_categories) fp32 target mix of xnrs_calibrated_rerank /
    xnrs_list_calibration -> the target as a contiguous fp32 tensor."""
    _lists(rows, what)
    if not rows.is_cuda:
        raise hip.XnrsHipError(f"{what}: tensor is on {rows.device}; xnrs_amd runs on a HIP device only (there is no CPU fallback)")
    _row_categories(row_category, rows.device)
    target = hip.dev_f32(target, "target mix")
    if tuple(target.shape) != (rows.shape[0], int(n_categories)):
        raise RuntimeError(f"target mix: ({rows.shape[0]}, {int(n_categories)}) weights, one row per session; got {tuple(target.shape)}")
    if target.device != rows.device or not rows.is_contiguous():
        raise hip.XnrsHipError(f"{what} and the target mix must be contiguous tensors on {rows.device}")
    return target


def csr_category_counts(off, rows, row_category, n_categories: int, pad_row: int = -1):
    """counts:(B, n_categories) int32, the category histogram of every list of the CSR off:(B+1) int64 / rows int32 (the shape
    of an exclusion CSR, e.g. the histories) (include/xnrs_hip.h: xnrs_csr_category_counts).  A row outside the table, the pad
    row or a row whose category lies outside [0, n_categories) counts nowhere."""
    if not isinstance(off, torch.Tensor) or off.dtype != torch.int64 or off.dim() != 1 or off.numel() < 1:
        raise RuntimeError(f"CSR offsets: a (B + 1,) int64 tensor, got {tuple(getattr(off, 'shape', ()))} {getattr(off, 'dtype', type(off))}")
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or rows.dim() != 1:
        raise RuntimeError(f"CSR rows: a 1-D int32 tensor, got {tuple(getattr(rows, 'shape', ()))} {getattr(rows, 'dtype', type(rows))}")
    if not off.is_cuda:
        raise hip.XnrsHipError(f"CSR offsets: tensor is on {off.device}; xnrs_amd runs on a HIP device only (there is no CPU fallback)")
    dev = off.device
    _row_categories(row_category, dev)
    if rows.device != dev or not rows.is_contiguous() or not off.is_contiguous():
        raise hip.XnrsHipError(f"the CSR must be contiguous tensors on {dev}")
    B = off.numel() - 1
    counts = torch.empty((B, max(int(n_categories), 0)), dtype=torch.int32, device=dev)
    hip.check(hip.lib().xnrs_csr_category_counts(hip.ptr(off), hip.ptr(rows), B, hip.ptr(row_category), row_category.numel(),
                                                 int(n_categories), int(pad_row), hip.ptr(counts), hip.stream_ptr(dev)),
              "xnrs_csr_category_counts")
    return counts


def calibrated_rerank(pool_rows, pool_scores, k: int, lam: float, row_category, n_categories: int, target, alpha: float = 0.01,
                      rel: str = "minmax"):
    """Greedy calibrated re-ranking of per-session candidate lists (include/xnrs_hip.h: xnrs_calibrated_rerank) -> (rows:(B,k)
    int32, scores:(B,k) fp32, pos:(B,k) int32, kl:(B,) fp32): step by step the valid place of the pool with the largest
    lam * relevance - (1 - lam) * KL(target || mix of the list with that place added), equal objectives to the lower place;
    scores are the pool's own bits, pos the place in the pool, -1 / -inf / -1 once the valid places run out; kl is the
    miscalibration of the final list (0 for a session whose target has no positive weight).  pool_rows:(B,P) int32,
    pool_scores:(B,P) fp32, e.g. what topk_deep_* returned; row_category:(n_rows,) int32, target:(B, n_categories) weights."""
    target = _calibration_operands(pool_rows, row_category, n_categories, target, "candidate lists")
    pool_scores, rel = _pool_scores("calibrated_rerank()", pool_scores, pool_rows, rel)
    (B, P), k, dev = pool_rows.shape, int(k), pool_rows.device
    rows, scores, pos = _picks(B, k, dev)
    kl = torch.empty((B,), dtype=torch.float32, device=dev)
    hip.check(hip.lib().xnrs_calibrated_rerank(hip.ptr(pool_rows), hip.ptr(pool_scores), B, P, k, hip.ptr(row_category),
                                               row_category.numel(), int(n_categories), hip.ptr(target), float(lam), float(alpha),
                                               rel, hip.ptr(rows), hip.ptr(scores), hip.ptr(pos), hip.ptr(kl),
                                               hip.stream_ptr(dev)), "xnrs_calibrated_rerank")
    return rows, scores, pos, kl


def list_calibration(rows, row_category, n_categories: int, target, alpha: float = 0.01, want_counts: bool = False):
    """Per list of rows:(B,k) int32 (-1 or out of the table: no place) -> (kl:(B,) fp32, n:(B,) int32, counts:(B, n_categories)
    int32 or None) (include/xnrs_hip.h: xnrs_list_calibration): the KL divergence of the target mix from the list's smoothed
    category mix (0 for a session without a target), the places that have a category, and their histogram."""
    target = _calibration_operands(rows, row_category, n_categories, target, "lists")
    (B, k), dev = rows.shape, rows.device
    kl = torch.empty((B,), dtype=torch.float32, device=dev)
    n = torch.empty((B,), dtype=torch.int32, device=dev)
    counts = torch.empty((B, int(n_categories)), dtype=torch.int32, device=dev) if want_counts else None
    hip.check(hip.lib().xnrs_list_calibration(hip.ptr(rows), B, k, hip.ptr(row_category), row_category.numel(), int(n_categories),
                                              hip.ptr(target), float(alpha), hip.ptr(kl), hip.ptr(n), hip.ptr(counts),
                                              hip.stream_ptr(dev)), "xnrs_list_calibration")
    return kl, n, counts


# ------------------------------------------------------------------------------------------------
# module-level dispatch: what the nn.Module mirrors call.  Handles train-mode attention dropout and
# routes to the autograd path when gradients are required.
def _needs_grad(*tensors_or_modules) -> bool:
    if not torch.is_grad_enabled():
        return False
    for t in tensors_or_modules:
        if t is None:
            continue
        if isinstance(t, torch.Tensor):
            if t.requires_grad:
                return True
        else:
            for p in t.parameters():
                if p.requires_grad:
                    return True
    return False


#: Optional DEVICE word (int64 tensor of one element) that the attention kernels add to every dropout seed
#: (include/xnrs_hip.h: xnrs_mha_params::seed_dev).  A grad step captured in a hipGraph bakes the host seeds into the graph;
#: a caller that increments this word INSIDE the captured step (`word.add_(1)`) gets a fresh attention-dropout draw per
#: replay, as the reference draws one per call (layers.py:148).  None (default): host seeds alone.
_DROPOUT_SEED_WORD = None


def set_dropout_seed_word(word):
    """word: None, or a one-element int64 tensor on the HIP device.  Do not change it between a forward and its backward."""
    global _DROPOUT_SEED_WORD
    if word is not None and not (isinstance(word, torch.Tensor) and word.is_cuda and word.dtype == torch.int64 and word.numel() == 1):
        raise hip.XnrsHipError("the dropout seed word is a one-element int64 tensor on the HIP device")
    _DROPOUT_SEED_WORD = word


def dropout_seed_word():
    return _DROPOUT_SEED_WORD


def _att_dropout(att):
    """(p, seed) of the attention-probability dropout (layers.py:117,148): active in train mode only.
    The seed is drawn from torch's CPU generator so torch.manual_seed() controls it."""
    if att is None or not att.training or att.dropout.p <= 0.0:
        return 0.0, 0
    return float(att.dropout.p), _draw_seed()


def _draw_seed() -> int:
    return int(torch.empty((), dtype=torch.int64).random_().item())


def dropout_rows(x: torch.Tensor, ids: Optional[torch.Tensor], out: torch.Tensor, p: float, seed: int, word=None):
    """ONE xnrs_dropout_rows launch (include/xnrs_hip.h): out[i] = dropped(x[ids[i]] or x[i]).  x, out: contiguous fp32 on the
    device, rows = everything behind the first dim; word: the device seed word of the call (None: host seed alone)."""
    if out.numel() == 0:  # (n, 0) as well as (0, ...): nothing to draw, as nn.Dropout returns an empty tensor
        return out
    n = out.shape[0] if out.dim() else 1
    row_floats = out.numel() // n
    hip.check(hip.lib().xnrs_dropout_rows(hip.ptr(x), hip.ptr(ids), hip.ptr(out), n, row_floats, float(p),
                                          int(seed) % (1 << 64), hip.ptr(word), hip.stream_ptr(out.device)), "xnrs_dropout_rows")
    return out


def gather_dropout(table: torch.Tensor, ids: torch.Tensor, p: float, seed: int):
    """nn.Dropout(p)(table[ids]) in one launch: table:(n_rows, ...), ids:(n,) -> dense dropped rows (n, ...).  Row i of the
    result draws its mask from (seed, i) -- its position in the call, not its table row -- so two occurrences of one news
    get two masks.  The device seed word (set_dropout_seed_word) is added to the seed."""
    bf16 = table.dtype == torch.bfloat16  # a bf16 news table: gathered, widened and dropped in one launch, the same mask
    tab = _dev_bf16(table, "gather_dropout table") if bf16 else hip.dev_f32(table, "gather_dropout table")
    if not ids.is_cuda:
        raise hip.XnrsHipError("ids must live on the HIP device")
    ids = ids.reshape(-1).to(torch.int32).contiguous()
    out = torch.empty((ids.numel(),) + tuple(tab.shape[1:]), dtype=torch.float32, device=tab.device)
    if bf16:
        if out.numel():
            hip.check(hip.lib().xnrs_dropout_rows_bf16(hip.ptr(tab), hip.ptr(ids), hip.ptr(out), ids.numel(), tab[0].numel(),
                                                       float(p), int(seed) % (1 << 64), hip.ptr(dropout_seed_word()),
                                                       hip.stream_ptr(out.device)), "xnrs_dropout_rows_bf16")
        return out
    return dropout_rows(tab, ids, out, p, seed, dropout_seed_word())


def gather_rows(table: torch.Tensor, ids: torch.Tensor):
    """table[ids] as one xnrs_gather_rows launch: table:(n_rows, ...), ids:(n,) -> (n, ...)."""
    tab = hip.dev_f32(table, "gather_rows table")
    if not ids.is_cuda:
        raise hip.XnrsHipError("ids must live on the HIP device")
    ids = ids.reshape(-1).to(torch.int32).contiguous()
    out = torch.empty((ids.numel(),) + tuple(tab.shape[1:]), dtype=torch.float32, device=tab.device)
    hip.check(hip.lib().xnrs_gather_rows(hip.ptr(tab), hip.ptr(ids), hip.ptr(out), ids.numel(), tab[0].numel(),
                                         hip.stream_ptr(tab.device)), "xnrs_gather_rows")
    return out


def id_path_dropout(table_x: torch.Tensor, table_m: torch.Tensor, ids: torch.Tensor, p: float):
    """The dense batch of an id-path training call with input dropout: (nn.Dropout(p)(table_x[ids]), table_m[ids]) in two
    launches (the dropped rows are never materialised undropped).  Draws the input-dropout seed: call this BEFORE the
    encoder draws its attention-dropout seed (the reference's order: news_encoding.py:51, then layers.py:148)."""
    return gather_dropout(table_x, ids, p, _draw_seed()), gather_rows(table_m, ids)


def input_dropout(x: torch.Tensor, p: float, training: bool, seed: Optional[int] = None):
    """nn.Dropout(p) on a tower's input (news_encoding.py:51, user_encoding.py:69) as one HIP launch; rows = x's first
    dim.  Differentiable: the backward is the same launch on dy, and nothing is saved but (p, seed).  training=False or
    p == 0 returns x itself.  seed=None draws one int64 from torch's CPU generator (torch.manual_seed controls it), as the
    attention dropout does; a caller that runs both draws this one FIRST (the reference's order: news_encoding.py:51, then
    layers.py:148)."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"input_dropout: expected a tensor, got {type(x)}")
    if not training or p == 0:
        return x
    if not x.is_cuda:
        raise hip.XnrsHipError(f"input_dropout: tensor is on {x.device}; xnrs_amd runs on a HIP device only")
    if seed is None:
        seed = _draw_seed()
    from . import autograd
    return autograd.input_dropout(x, float(p), int(seed), dropout_seed_word())


def _check_att(att):
    from .models.components import layers
    if att is not None and not isinstance(att, layers.MultiHeadAttention):
        raise hip.XnrsHipError(f"att module {type(att).__name__} has no HIP implementation "
                               "(supported: xnrs_amd MultiHeadAttention)")


def multi_head_attention(x, m, att):
    p, seed = _att_dropout(att)
    if _needs_grad(x, att):
        from . import autograd
        return autograd.mha(x, m, att, p, seed)
    return mha_forward(x, m, att, p, seed)


def additive_attention(x, m, pool, return_weights=False):
    if _needs_grad(x, pool):
        from . import autograd
        return autograd.additive(x, m, pool, return_weights)
    return additive_forward(x, m, pool, return_weights)


def text_encoder(x, m, enc, ids=None, chunk: int = 0):
    att, pooler, head = enc.att, enc.pooler, getattr(enc, "head", None)
    _check_att(att)
    p, seed = _att_dropout(att)
    if _needs_grad(x, enc):
        from . import autograd
        x, m, ids = _widen_table_call(x, m, ids)  # no bf16 backward: the training path runs on the widened rows of the ids
        return autograd.text_encoder(x, m, enc, ids, p, seed)
    return text_encoder_forward(x, m, att, pooler, head, ids=ids, chunk=chunk, dropout_p=p, seed=seed)


def text_encoder_from_qkv(qkv: torch.Tensor, x: torch.Tensor, m: torch.Tensor, enc):
    """TextEncoder core from a GIVEN Q|K|V image: qkv (n_seq * L, 3D) fp32 = tokens . [Wq; Wk; Wv]^T + [bq; bk; bv], rows of
    sequence i at [i * L, (i + 1) * L); x (..., L, D): the tokens behind it -- read for their shape only, so the unscaled
    (H, L, D) tokens of an explanation serve every step; m: the mask of all n_seq sequences.  -> (y:(n_seq, E'), hm:(n_seq,))
    like text_encoder.  The image is the one differentiable input: its gradient is dQ|dK|dV, every row written; no parameter
    gradient is computed and several backward passes over one forward are fine (integrated gradients with one projection:
    explain.py).  Needs an attention stage."""
    att = enc.att
    if att is None:
        raise hip.XnrsHipError("text_encoder_from_qkv: the encoder has no attention stage, so there is no Q|K|V image to start from")
    _check_att(att)
    p, seed = _att_dropout(att)
    from . import autograd
    return autograd.text_encoder_from_qkv(qkv, x, m, enc, p, seed)


def ig_expand(p: torch.Tensor, bias: Optional[torch.Tensor], alphas: torch.Tensor) -> torch.Tensor:
    """xnrs_ig_expand: p (rows, W), bias (W) or None, alphas (n) on the device -> (n * rows, W),
    out[i * rows + r] = fma(alphas[i], p[r], bias)."""
    p = hip.dev_f32(p, "ig_expand rows")
    alphas = hip.dev_f32(alphas, "ig_expand alphas")
    b = None if bias is None else hip.dev_f32(bias, "ig_expand bias")
    rows, W = p.shape
    n = alphas.numel()
    out = torch.empty((n * rows, W), dtype=torch.float32, device=p.device)
    hip.check(hip.lib().xnrs_ig_expand(hip.ptr(p), hip.ptr(b), hip.ptr(alphas), n, rows, W, hip.ptr(out), hip.stream_ptr(p.device)),
              "xnrs_ig_expand")
    return out


def ig_reduce(g: torch.Tensor, n: int, scale: float, out: torch.Tensor, accumulate: bool) -> torch.Tensor:
    """xnrs_ig_reduce: g (n * rows, W) -> out (rows, W) (=) or (+=) scale * (g[0] + ... + g[n-1]), the slices summed in
    ascending order as one fp32 chain.  out: a contiguous fp32 device tensor, written in place."""
    g = hip.dev_f32(g, "ig_reduce images")
    rows, W = out.shape
    if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()) or g.shape != (n * rows, W):
        raise hip.XnrsHipError(f"ig_reduce: images {tuple(g.shape)} / sum {tuple(out.shape)} for n = {n}")
    hip.check(hip.lib().xnrs_ig_reduce(hip.ptr(g), n, rows, W, float(scale), hip.ptr(out), int(bool(accumulate)),
                                       hip.stream_ptr(out.device)), "xnrs_ig_reduce")
    return out


def linear_input_grad(dy: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """dy . W as ONE product: the input gradient of nn.Linear alone (xnrs_linear_bwd with dx only).  dy (M, N), W (N, K) -> (M, K)."""
    dy, w = hip.dev_f32(dy, "dy"), hip.dev_f32(weight, "linear weight")
    M, N = dy.shape
    K = w.shape[1]
    dx = torch.empty((M, K), dtype=torch.float32, device=dy.device)
    l = hip.lib()
    nws = l.xnrs_linear_bwd_workspace_bytes(M, N, K)
    ws = hip.workspace(dy.device, nws)
    # (x: only the weight gradient reads it; the entry point wants it non-NULL, dy stands in)
    hip.check(l.xnrs_linear_bwd(hip.ptr(dy), None, 0, hip.ptr(w), hip.ptr(dy), hip.ptr(dx), None, None, M, N, K, hip.ptr(ws), nws,
                                hip.stream_ptr(dy.device)), "xnrs_linear_bwd")
    return dx


def text_encoder_unpadded(x, m, enc, ids=None):
    """Inference-only variant of text_encoder that skips the padding work (text_encoder_forward_unpadded).  Falls
    back to the padded kernels -- loudly impossible cases aside -- when attention dropout is active (train mode)."""
    att, pooler, head = enc.att, enc.pooler, getattr(enc, "head", None)
    _check_att(att)
    p, _ = _att_dropout(att)
    S, D = x.shape[-2], x.shape[-1]
    dk = D // att.h if att is not None else 4
    # outside the unpadded kernels' range (S, d_k <= 64, 16-byte aligned head rows) the padded kernels give the same
    # result -- an optional speed-up never turns into an error
    supported = S <= 64 and D % 4 == 0 and (att is None or (dk <= 64 and dk % 4 == 0))
    if _needs_grad(x, enc) or p > 0.0 or not supported:
        return text_encoder(x, m, enc, ids=ids)
    if COMPACT_ON_DEVICE and compact_supported(S, D, att, pooler, x):
        # row lists built on the device: no host sync, capturable; all-masked news cost nothing (so skip_empty's host-side
        # compaction is not needed on top).  A device without room for its scratch falls back to the host-compacted path
        # (the same results) instead of failing: hip.release_workspaces() returns the scratch when eval and train alternate
        try:
            return text_encoder_forward_compact(x, m, att, pooler, head, ids=ids)
        except torch.OutOfMemoryError:
            hip.release_workspaces()
    return text_encoder_forward_unpadded(x, m, att, pooler, head, ids=ids)


def check_binary_mask(m: torch.Tensor, what: str = "mask") -> None:
    """Raise ValueError unless every mask value is 0 or 1 (ONE host sync: set-up code, never the step).  The padding-free
    paths require binary masks (an unmasked row is simply "live"); the host-compacted path checks this per call, the
    device-compacted one (TextEncoder.unpadded on supported shapes) cannot raise from the device -- it writes NaN outputs
    and sets hip.STATUS_NONBINARY_MASK in the sticky status word (hip.check_status()).  Call this once per dataset instead
    (NewsStore.validate_masks)."""
    bad = ((m != 0) & (m != 1)).any()
    if bool(bad.item()):
        raise ValueError(f"{what}: values other than 0 / 1 (the reference's masks are fp32 0/1, news_encoding.py:34-50)")


#: TextEncoder.unpadded compacts on the device when the shape allows (XNRS_COMPACT_ON_DEVICE=0: always the host-compacted path)
COMPACT_ON_DEVICE = os.environ.get("XNRS_COMPACT_ON_DEVICE", "1") != "0"


def user_encoder(x, m, enc, return_weights=False):
    att, pooler, head = enc.att, enc.pooler, getattr(enc, "head", None)
    _check_att(att)
    p, seed = _att_dropout(att)
    if _needs_grad(x, enc):
        from . import autograd
        return autograd.user_encoder(x, m, enc, return_weights, p, seed)
    return user_encoder_forward(x, m, att, pooler, head, return_weights, dropout_p=p, seed=seed)


def personalized_forward(x, m, ids, q, q_idx, x_fc, head, keep: bool = False):
    """layers.PersonalizedAttention (layers.py:72-102) [+ head], include/xnrs_hip.h xnrs_personalized_fwd:
    x:(n_seq,L,D) (or the table with ids:(n_seq,) int32), m:(n_seq,L) or None, q:(n_q,A) query rows (unit column stride),
    q_idx:(n_seq,) int32 -> (y:(n_seq,E), hm:(n_seq,)[, saved blob when keep])."""
    from . import autograd as AG
    x = hip.dev_f32(x, "personalized attention input")
    L, D = x.shape[-2], x.shape[-1]
    if ids is not None:
        ids = ids.to(torch.int32).contiguous()
        if not ids.is_cuda:
            raise hip.XnrsHipError("news ids must live on the HIP device")
    n_seq = ids.numel() if ids is not None else x.numel() // (L * D)
    m = None if m is None else hip.dev_f32(m, "personalized attention mask")
    if m is not None and m.numel() != (x.numel() // D if ids is not None else n_seq * L):
        raise ValueError(f"mask of {m.numel()} values for {n_seq} sequences of {L}")
    if q_idx.numel() != n_seq or q_idx.dtype != torch.int32:
        raise ValueError("q_idx: one int32 query row per sequence")
    keep_alive = []
    pp = AG.personalized_params(x_fc, q, q_idx.contiguous(), keep_alive)
    hp = AG.personalized_head(head, keep_alive)
    E = hp.out_features if hp is not None else D
    l = hip.lib()
    nbytes = l.xnrs_personalized_saved_bytes(n_seq, L, D, pp.hidden, E, int(hp is not None))
    buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device) if keep else hip.workspace(x.device, nbytes)
    y = torch.empty((n_seq, E), dtype=torch.float32, device=x.device)
    hm = torch.empty((n_seq,), dtype=torch.float32, device=x.device)
    fn = l.xnrs_personalized_fwd_train if keep else l.xnrs_personalized_fwd
    hip.check(fn(hip.ptr(x), hip.ptr(m), hip.ptr(ids), n_seq, L, D, C.byref(pp), hip.ref(hp), hip.ptr(y), None, hip.ptr(hm),
                 hip.ptr(buf), nbytes, hip.stream_ptr(x.device)), "xnrs_personalized_fwd")
    return (y, hm, buf) if keep else (y, hm)


def personalized(x, m, ids, q, q_idx, x_fc, head=None):
    """-> (y, hm); through autograd when the input, the queries or the weights need a gradient.  A bf16 table with ids: the
    personalized kernels read fp32 rows, so the rows of the ids are widened first (table_rows_f32)."""
    x, m, ids = _widen_table_call(x, m, ids)
    if _needs_grad(x, q, x_fc, head):
        from . import autograd
        return autograd.personalized(x, m, ids, q, q_idx, x_fc, head)
    return personalized_forward(x, m, ids, q, q_idx, x_fc, head)


def embedding_linear_table(idx: torch.Tensor, table: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor]):
    """table[idx] . w^T + b over a LARGE table (NPA's user table): its gradient costs what the ids cost.  idx:(M,) -> (M, N)."""
    return linear(table, w, b, ids=idx, table_grad="sparse")


def embedding_linear(idx: torch.Tensor, embedder, fc, act: int = hip.ACT_NONE):
    """act(fc(embedder(idx))) (naml.py:82-86; CategoryEncoder, news_encoding.py:63-91) as ONE GEMM whose A rows are gathered
    from the embedding table by index.  idx:(B,N) int -> (B,N,out_features)."""
    return linear(embedder.weight, fc.weight, fc.bias, act, ids=idx)


# ---- nn.GRU, one layer (LSTUR's short-term user tower, lstur.py:113-154): include/xnrs_hip.h xnrs_gru_*
def gru_weights(gru):
    """(w_ih, w_hh, b_ih, b_hh) of a one-layer, unidirectional, batch_first nn.GRU (torch's own layout, gate order r, z, n)."""
    if gru.num_layers != 1 or gru.bidirectional or not gru.batch_first or getattr(gru, "proj_size", 0):
        raise hip.XnrsHipError("the HIP GRU is the one-layer, unidirectional, batch_first nn.GRU of LSTUR")
    return (gru.weight_ih_l0, gru.weight_hh_l0) + tuple(getattr(gru, k) if gru.bias else None for k in ("bias_ih_l0", "bias_hh_l0"))


def gru_params(weights, keep):
    """xnrs_gru_params of (w_ih:(3Hd,E), w_hh:(3Hd,Hd), b_ih, b_hh:(3Hd,) or None)."""
    ts = [hip.dev_f32(weights[0], "gru weight_ih"), hip.dev_f32(weights[1], "gru weight_hh")]
    ts += [None if t is None else hip.dev_f32(t, "gru bias") for t in weights[2:]]
    keep += ts
    return hip.STRUCTS["xnrs_gru_params"](*[None if t is None else t.data_ptr() for t in ts], ts[1].shape[1])


def gru_forward(x, m, h0, weights, keep: bool = False):
    """x:(B,T,E), m:(B,N>=T[,1]) history mask or None, h0:(B,Hd) or None, weights as gru_weights gives them -> final hidden
    state (B,Hd): the state after the first sum(m[b, :T]) slots of row b (a row of length 0 keeps its initial state).
    keep: -> (y, x, saved blob)."""
    x = hip.dev_f32(x, "gru input")
    if x.dim() != 3:
        raise RuntimeError(f"gru: expected (B, T, E), got {tuple(x.shape)}")
    B, T, E = x.shape
    Hd = weights[1].shape[1]
    if tuple(weights[0].shape) != (3 * Hd, E) or tuple(weights[1].shape) != (3 * Hd, Hd):
        raise RuntimeError(f"gru: input width {E} does not match weights {tuple(weights[0].shape)} / {tuple(weights[1].shape)}")
    ldm = 0
    if m is not None:
        m = hip.dev_f32(m, "gru mask").reshape(B, -1)
        ldm = m.shape[1]
        if ldm < T:
            raise RuntimeError(f"gru: mask of {ldm} slots for {T} steps")
    if h0 is not None:
        h0 = hip.dev_f32(h0, "gru initial state")
        if tuple(h0.shape) != (B, Hd):
            raise RuntimeError(f"gru: initial state {tuple(h0.shape)}, expected ({B}, {Hd})")
    keep_alive = []
    p = gru_params(weights, keep_alive)
    y = torch.empty((B, Hd), dtype=torch.float32, device=x.device)
    l = hip.lib()
    nbytes = l.xnrs_gru_saved_bytes(B, T, E, Hd) if keep else l.xnrs_gru_workspace_bytes(B, T, E, Hd)
    buf = _saved(x.device, nbytes, keep)
    fn = l.xnrs_gru_fwd_train if keep else l.xnrs_gru_fwd
    hip.check(fn(hip.ptr(x), hip.ptr(m), ldm, hip.ptr(h0), C.byref(p), hip.ptr(y), B, T, E, hip.ptr(buf), nbytes,
                 hip.stream_ptr(x.device)), "xnrs_gru_fwd")
    return (y, x, buf) if keep else y


def gru(x, m, h0, gru_mod):
    """Final hidden state of nn.GRU over the masked prefix of every row; through autograd when anything needs a gradient."""
    weights = gru_weights(gru_mod)
    if _needs_grad(x, h0, *weights):
        from . import autograd
        return autograd.gru(x, m, h0, weights)
    return gru_forward(x, m, h0, weights)


def embedding_rows(idx: torch.Tensor, table: torch.Tensor, padding_idx: Optional[int] = None):
    """table[idx] for a LARGE table (LSTUR's long-term user table, lstur.py:94-98,134); its gradient costs what the ids cost
    (xnrs_embedding_grad_sparse) and row `padding_idx` receives none.  idx:(M,) int32 -> (M, K)."""
    if not idx.is_cuda:
        raise hip.XnrsHipError("user indices must live on the HIP device")
    if _needs_grad(table):
        from . import autograd
        return autograd.embedding_rows(idx, table, padding_idx)
    return embedding_rows_forward(idx, table)


def embedding_rows_forward(idx, table):
    tab = hip.dev_f32(table, "embedding table")
    ids = idx.reshape(-1).to(torch.int32).contiguous()
    K = tab.shape[1]
    y = torch.empty((ids.numel(), K), dtype=torch.float32, device=tab.device)
    hip.check(hip.lib().xnrs_gather_rows(hip.ptr(tab), hip.ptr(ids), hip.ptr(y), ids.numel(), K, hip.stream_ptr(tab.device)),
              "xnrs_gather_rows")
    return y


# ---- CAUM's candidate-aware user tower (caum.py:31-111): include/xnrs_hip.h xnrs_attn_long_* / xnrs_caum_* / xnrs_act_bwd
def attn_long_forward(qkv: torch.Tensor, n_heads: int, keep: bool = False):
    """qkv:(L, Nb, 3E) seq-first packed q | k | v (nn.MultiheadAttention's in_proj layout) -> o:(L, Nb, E), the heads'
    softmax(q k^T / sqrt(d_k)) v concatenated; no mask, any L.  keep: -> (o, qkv, saved log-sum-exp blob)."""
    qkv = hip.dev_f32(qkv, "attention q|k|v")
    if qkv.dim() != 3 or qkv.shape[-1] % 3:
        raise RuntimeError(f"attn_long: expected (L, Nb, 3E), got {tuple(qkv.shape)}")
    L, Nb, E3 = qkv.shape
    E = E3 // 3
    o = torch.empty((L, Nb, E), dtype=torch.float32, device=qkv.device)
    l = hip.lib()
    st = hip.stream_ptr(qkv.device)
    if keep:
        nbytes = l.xnrs_attn_long_saved_bytes(L, Nb, E, n_heads)
        saved = _saved(qkv.device, nbytes, True)
        hip.check(l.xnrs_attn_long_fwd_train(hip.ptr(qkv), Nb * E3, E3, hip.ptr(o), Nb * E, E, L, Nb, E, n_heads, hip.ptr(saved),
                                             nbytes, st), "xnrs_attn_long_fwd_train")
        return o, qkv, saved
    hip.check(l.xnrs_attn_long_fwd(hip.ptr(qkv), Nb * E3, E3, hip.ptr(o), Nb * E, E, L, Nb, E, n_heads, st), "xnrs_attn_long_fwd")
    return o


def attn_long(qkv: torch.Tensor, n_heads: int):
    """Unmasked multi-head attention over a packed seq-first (L, Nb, 3E) image at any length; autograd when qkv needs it."""
    if _needs_grad(qkv):
        from . import autograd
        return autograd.attn_long(qkv, n_heads)
    return attn_long_forward(qkv, n_heads)


def caum_pair_forward(hp, cp, B: int, C: int, H: int):
    """hp:(B*H, 4E), cp:(B*C, 2E) -> (h_cnn, z), each (B*C*H, E)  (include/xnrs_hip.h: xnrs_caum_pair_fwd)."""
    hp, cp = hip.dev_f32(hp, "history projections"), hip.dev_f32(cp, "candidate projections")
    E = hp.shape[-1] // 4
    if tuple(hp.shape) != (B * H, 4 * E) or tuple(cp.shape) != (B * C, 2 * E):
        raise RuntimeError(f"caum_pair: hp {tuple(hp.shape)} / cp {tuple(cp.shape)} for B={B}, C={C}, H={H}")
    h_cnn = torch.empty((B * C * H, E), dtype=torch.float32, device=hp.device)
    z = torch.empty_like(h_cnn)
    hip.check(hip.lib().xnrs_caum_pair_fwd(hip.ptr(hp), hip.ptr(cp), 2 * E, hip.ptr(h_cnn), hip.ptr(z), B, C, H, E,
                                           hip.stream_ptr(hp.device)), "xnrs_caum_pair_fwd")
    return h_cnn, z


def caum_pair(hp, cp, B: int, C: int, H: int):
    if _needs_grad(hp, cp):
        from . import autograd
        return autograd.caum_pair(hp, cp, B, C, H)
    return caum_pair_forward(hp, cp, B, C, H)


def caum_bias_tanh_forward(pre, cb, H: int):
    pre, cb = hip.dev_f32(pre, "dense attention pre-activation"), hip.dev_f32(cb, "candidate term")
    E = pre.shape[-1]
    P = cb.shape[0]
    if tuple(pre.shape) != (P * H, E) or tuple(cb.shape) != (P, E):
        raise RuntimeError(f"caum_bias_tanh: pre {tuple(pre.shape)} / cb {tuple(cb.shape)} for H={H}")
    t = torch.empty_like(pre)
    hip.check(hip.lib().xnrs_caum_bias_tanh_fwd(hip.ptr(pre), hip.ptr(cb), E, hip.ptr(t), P, H, E, hip.stream_ptr(pre.device)),
              "xnrs_caum_bias_tanh_fwd")
    return t


def caum_bias_tanh(pre, cb, H: int):
    """tanh(pre[p*H + j] + cb[p]): pre:(P*H, E), cb:(P, E)."""
    if _needs_grad(pre, cb):
        from . import autograd
        return autograd.caum_bias_tanh(pre, cb, H)
    return caum_bias_tanh_forward(pre, cb, H)


def caum_pool_forward(t2, w3, b3, h_all, H: int, keep: bool = False):
    t2, w3, h_all = hip.dev_f32(t2, "dense attention hidden"), hip.dev_f32(w3, "dense attention linear3 weight"), hip.dev_f32(h_all, "h_all")
    b3 = None if b3 is None else hip.dev_f32(b3, "dense attention linear3 bias")
    A, E = t2.shape[-1], h_all.shape[-1]
    R = t2.numel() // A
    if R % H or h_all.numel() != R * E or w3.numel() != A:
        raise RuntimeError(f"caum_pool: t2 {tuple(t2.shape)}, h_all {tuple(h_all.shape)}, w3 {tuple(w3.shape)} for H={H}")
    P = R // H
    u = torch.empty((P, E), dtype=torch.float32, device=t2.device)
    a = torch.empty((P, H), dtype=torch.float32, device=t2.device) if keep else None
    hip.check(hip.lib().xnrs_caum_pool_fwd(hip.ptr(t2), hip.ptr(w3), hip.ptr(b3), hip.ptr(h_all), hip.ptr(u), hip.ptr(a), P, H, A, E,
                                           hip.stream_ptr(t2.device)), "xnrs_caum_pool_fwd")
    return (u, a, (t2, w3, h_all)) if keep else u


def caum_pool(t2, w3, b3, h_all, H: int):
    """softmax over the H slots of w3 . t2 + b3, weighted sum of h_all: t2:(P*H, A), h_all:(P*H, E) -> (P, E)."""
    if _needs_grad(t2, w3, b3, h_all):
        from . import autograd
        return autograd.caum_pool(t2, w3, b3, h_all, H)
    return caum_pool_forward(t2, w3, b3, h_all, H)


def caum_user(h, c, enc):
    """CAUMUserEncoder.forward (caum.py:56-111) on h:(B,H,E) history and c:(B,C,E) candidate vectors -> u:(B,C,E).  `enc`
    holds the reference's modules (dropout1-3, linear1-3, dense_att, multihead_attention); none of the Linear /
    MultiheadAttention modules is called.  The dropouts are torch's, on the device."""
    h, c = hip.dev_f32(h, "history vectors"), hip.dev_f32(c, "candidate vectors")
    B, H, E = h.shape
    C = c.shape[1]
    if c.shape[0] != B or c.shape[2] != E:
        raise RuntimeError(f"caum_user: history {tuple(h.shape)} against candidates {tuple(c.shape)}")
    mha, da = enc.multihead_attention, enc.dense_att
    if mha.in_proj_weight is None or mha.bias_k is not None or mha.add_zero_attn or mha.batch_first or mha.dropout != 0.0:
        raise hip.XnrsHipError("the HIP CAUM tower is nn.MultiheadAttention(E, n_heads) as caum.py:52-54 builds it")
    cd, hd = enc.dropout1(c), enc.dropout2(h)
    w1, w2 = enc.linear1.weight, enc.linear2.weight
    # weight blocks side by side (slices and concatenations: data movement, differentiable by torch's own bookkeeping)
    w_h = torch.cat([w1[:, :E], w1[:, E:2 * E], w1[:, 2 * E:3 * E], w2[:, E:]], dim=0)     # [Wl; Wm; Wr; W2h]
    w_c = torch.cat([w1[:, 3 * E:], w2[:, :E], da.linear.weight[:, E:]], dim=0)           # [Wc; W2c; Wdc]
    b_c = torch.cat([enc.linear1.bias, enc.linear2.bias, da.linear.bias], dim=0)
    hp = linear(hd.reshape(B * H, E), w_h, None)                                          # (B*H, 4E)
    cp = linear(cd.reshape(B * C, E), w_c, b_c)                                           # (B*C, 3E)
    h_cnn, z = caum_pair(hp, cp[:, :2 * E], B, C, H)
    # nn.MultiheadAttention without batch_first on the (P, H, E) view: the attended axis is P = B*C, the slot is the batch
    qkv = linear(z, mha.in_proj_weight, mha.in_proj_bias)
    o = attn_long(qkv.reshape(B * C, H, 3 * E), mha.num_heads)
    h_att = linear(o.reshape(B * C * H, E), mha.out_proj.weight, mha.out_proj.bias)
    h_all = linear(enc.dropout3(torch.cat([h_cnn, h_att], dim=1)), enc.linear3.weight, enc.linear3.bias)
    pre = linear(h_all, da.linear.weight[:, :E], None)
    t1 = caum_bias_tanh(pre, cp[:, 2 * E:], H)
    t2 = linear(t1, da.linear2.weight, da.linear2.bias, hip.ACT_TANH)
    u = caum_pool(t2, da.linear3.weight, da.linear3.bias, h_all, H)
    return u.reshape(B, C, E)


def diag_scoring(u, c, normalize: bool = False):
    """CAUMScoring.forward (scoring.py:26-38): r[b, i] = u[b, i] . c[b, i], the diagonal of DotScoring's (C, C) product --
    dot_scoring over (B*C, 1) pairs.  u, c:(B,C,E) -> (B,C,1)."""
    B, C, E = c.shape
    if tuple(u.shape) != (B, C, E):
        raise RuntimeError(f"CAUMScoring: user vectors {tuple(u.shape)} against candidates {tuple(c.shape)}")
    return dot_scoring(u.reshape(B * C, 1, E), c.reshape(B * C, 1, E), normalize).reshape(B, C, 1)
