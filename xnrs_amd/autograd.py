"""Autograd bridge: torch.autograd.Function wrappers around the training entry points of
libxnrs_hip.so (forward that keeps its activations + hand-written backward kernels).

Needed by the grad step (xnrs/training.py:402-431: loss.backward(); Adam) and by integrated
gradients (xnrs/explain.py:160-166: d score / d x).  Everything differentiable on the hot path goes
through HIP kernels; torch only routes gradients between the Functions.
"""
from __future__ import annotations

import ctypes
import os
import weakref
from collections import namedtuple
from typing import List, Optional

import torch

from . import hip

_ATT_NAMES = ("q_linear.weight", "q_linear.bias", "k_linear.weight", "k_linear.bias",
              "v_linear.weight", "v_linear.bias", "out.weight", "out.bias")


def _att_tensors(att) -> List[torch.Tensor]:
    return [att.q_linear.weight, att.q_linear.bias, att.k_linear.weight, att.k_linear.bias,
            att.v_linear.weight, att.v_linear.bias, att.out.weight, att.out.bias]


def _pool_tensors(pool) -> List[torch.Tensor]:
    return [pool.fc1.weight, pool.fc1.bias, pool.fc2.weight, pool.fc2.bias]


def _head_tensors(head) -> List[Optional[torch.Tensor]]:
    return [head[0].weight, head[0].bias, head[2].weight, head[2].bias]


class _Cfg:
    """Static (non-tensor) description of one sequence-encoder call."""

    def __init__(self, n_seq, L, D, n_heads, scaled, pool_kind, A, has_head, E, head_bias, dropout_p, seed, want_a):
        self.n_seq, self.L, self.D = n_seq, L, D
        self.n_heads, self.scaled = n_heads, scaled
        self.pool_kind, self.A = pool_kind, A
        self.has_head, self.E, self.head_bias = has_head, E, head_bias
        self.Eo = E if has_head else D  # the width of a pooled output row
        self.dropout_p, self.seed = dropout_p, seed
        self.want_a = want_a
        self.head_act = hip.ACT_RELU
        from . import ops
        self.seed_word = ops.dropout_seed_word()  # as of the forward: the backward recomputes the same mask


def _param_structs(cfg: _Cfg, params: List[Optional[torch.Tensor]]):
    """Split the flat parameter list (att 8 | pool 4 | head 4) back into the C structs."""
    i = 0
    ap = pp = hp = None
    keep = []
    if cfg.n_heads > 0:
        ts = [hip.dev_f32(t, "mha weight") for t in params[i:i + 8]]
        ap = hip.MhaParams(*[t.data_ptr() for t in ts], cfg.n_heads, 1 if cfg.scaled else 0, float(cfg.dropout_p),
                           int(cfg.seed))
        if cfg.seed_word is not None and cfg.dropout_p > 0:
            ap.seed_dev = cfg.seed_word.data_ptr()  # (ops.set_dropout_seed_word: a fresh draw per hipGraph replay)
            ts = ts + [cfg.seed_word]
        keep += ts
        i += 8
    if cfg.pool_kind == hip.POOL_ADDITIVE:
        ts = [hip.dev_f32(t, "additive weight") for t in params[i:i + 4]]
        pp = hip.AdditiveParams(*[t.data_ptr() for t in ts], cfg.A)
        keep += ts
        i += 4
    if cfg.has_head:
        ts = [None if t is None else hip.dev_f32(t, "head weight") for t in params[i:i + 4]]
        hp = hip.HeadParams(*[None if t is None else t.data_ptr() for t in ts], cfg.E, cfg.head_act)
        keep += ts
        i += 4
    return ap, pp, hp, keep


def _grad_structs(cfg: _Cfg, grads: List[Optional[torch.Tensor]]):
    """The flat gradient list (the layout of the parameter list) as the C structs; None asks for no gradient."""
    ptrs = [_addr(g) for g in grads]
    i = 8 if cfg.n_heads > 0 else 0
    j = i + 4 if cfg.pool_kind == hip.POOL_ADDITIVE else i
    return (hip.MhaGrads(*ptrs[:i]) if i else None, hip.AdditiveGrads(*ptrs[i:j]) if j > i else None,
            hip.HeadGrads(*ptrs[j:j + 4]) if cfg.has_head else None)


#: forward and backward over the unmasked token rows only (exact; include/xnrs_hip.h: xnrs_seq_encoder_fwd_train_live /
#: xnrs_seq_encoder_bwd_live).  Environment
#: XNRS_BWD_LIVE_ROWS=0 turns it off; it is used when at most LIVE_ROWS_MAX_FRACTION of the rows are unmasked.
LIVE_ROWS = os.environ.get("XNRS_BWD_LIVE_ROWS", "1") != "0"
LIVE_ROWS_MAX_FRACTION = 0.9
LIVE_ROWS_MIN = 4096  # token rows from which the live-row path pays for its index bookkeeping (tests lower it)
#: how many training forwards took the live-row path (tests assert that the branch they mean to cover really ran)
STATS = {"live_row_forwards": 0, "kv_row_forwards": 0, "shared_qkv_forwards": 0, "device_list_forwards": 0,
         "deferred_dqkv_backwards": 0, "merged_dqkv_backwards": 0, "shared_output_forwards": 0}
#: the row lists built ON THE DEVICE (include/xnrs_hip.h: xnrs_build_row_lists, xnrs_row_lists::counts_dev): no torch
#: bookkeeping and no host read of the counts -- the grad step has no host synchronisation and can be captured in a hipGraph.
#: Taken whenever the shape allows (fp32 GEMM mode, D and A multiples of 4, 16-byte aligned operands); the lists are then
#: used whatever fraction of the rows is live (LIVE_ROWS_MAX_FRACTION needs the count on the host).  XNRS_DEVICE_LISTS=0:
#: the host bookkeeping of round 3 (one .tolist() per encoder call).
DEVICE_LISTS = os.environ.get("XNRS_DEVICE_LISTS", "1") != "0"
#: K|V projection and dWk / dWv over the token rows of the non-empty news only (rides on the live-row path, exact;
#: include/xnrs_hip.h: xnrs_row_lists).  XNRS_KV_ROWS=0 turns it off.
KV_ROWS = os.environ.get("XNRS_KV_ROWS", "1") != "0"


def _addr(t):
    return None if t is None else t.data_ptr()


def _f32_out(shape, dev):
    return torch.empty(shape, dtype=torch.float32, device=dev)


class _Rows:
    """The row lists of one encoder call (include/xnrs_hip.h: xnrs_row_lists): the unmasked token rows and the token rows of
    the non-empty news, each with its table rows under ids, and their counts -- on the host (n_live, n_kv), or as capacities
    with the counts on the device (counts).  No field set: no lists, the call runs dense."""
    __slots__ = ("live", "live_src", "n_live", "kv", "kv_src", "n_kv", "counts")

    def __init__(self, live=None, live_src=None, n_live=0, kv=None, kv_src=None, n_kv=0, counts=None):
        self.live, self.live_src, self.n_live = live, live_src, n_live
        self.kv, self.kv_src, self.n_kv, self.counts = kv, kv_src, n_kv, counts

    def struct(self, qkv_shared, dqkv_image, dqkv_mode):
        """-> the hip.RowLists of a call that reads the Q|K|V image at address qkv_shared (None: it projects) and defers or
        merges its dQ|dK|dV in the tensor dqkv_image as dqkv_mode says; None when there is nothing to pass."""
        if self.live is None and qkv_shared is None and dqkv_mode == hip.DQKV_OWN:
            return None
        return hip.RowLists(_addr(self.live), _addr(self.live_src), self.n_live, _addr(self.kv), _addr(self.kv_src), self.n_kv,
                            qkv_shared, _addr(self.counts), _addr(dqkv_image), dqkv_mode)


_NO_ROWS = _Rows()  # (never written to: every call without lists shares it)


#: The reference's train step encodes the history twice (training.py:406 scores, :409 get_user_embeddings); with input
#: dropout 0 (every shipped config) the two encodes differ only in their attention-dropout draws, so their Q|K|V images are
#: the same numbers.  A training forward of an attention tower registers its saved blob and row lists here under the
#: identity of everything the image depends on -- data pointer AND version counter of input, mask, ids and the six projection
#: tensors -- and a second forward that finds a LIVE entry reads that image instead of projecting again (and reuses the row
#: lists: no second host read).  Weak references: an entry dies with the first forward's graph.  Bitwise the same step.
#: XNRS_SHARE_QKV=0 turns it off.
SHARE_QKV = os.environ.get("XNRS_SHARE_QKV", "1") != "0"
_QKV_IMAGES = {}
#: ... and their backwards share ONE weight-gradient product per projection: dW = (dQKV_1 + dQKV_2)^T . X (the input X is
#: the same).  Whichever of the two autograd nodes runs first leaves its dQ|dK|dV image in a buffer and returns no gradient
#: for wq/bq/wk/bk/wv/bv (XNRS_DQKV_DEFER) -- but only when the engine says the other node WILL run in this very backward
#: pass (torch._C._will_engine_execute_node) and has not run yet; the second node adds its own dQ|dK|dV to the image and
#: computes the six gradients from the sum (XNRS_DQKV_MERGE).  Same gradients up to summation order.  XNRS_MERGE_DW=0: off.
MERGE_DW = os.environ.get("XNRS_MERGE_DW", "1") != "0"


#: torch.autograd.grad(score, inputs=[tokens]) -- integrated gradients, explain.py:160-166 -- needs no parameter gradient, but
#: ctx.needs_input_grad only says that the parameters REQUIRE grad.  The engine knows what this pass computes: a parameter
#: whose AccumulateGrad node it will not execute gets no weight-gradient product (two thirds of the backward of an IG step).
#: A plain loss.backward() executes every node: nothing changes there.  XNRS_SKIP_UNUSED_DW=0: off.
SKIP_UNUSED_DW = os.environ.get("XNRS_SKIP_UNUSED_DW", "1") != "0"


def _engine_wants(fn) -> bool:
    """torch._C._will_engine_execute_node(fn), asked per node.  Under torch.autograd.grad(..., inputs=[leaves]) the engine
    answers False for the AccumulateGrad node of a leaf that is not among the inputs and RAISES for one that is (a captured
    leaf is not executed, its gradient is handed back: "A leaf node was passed ... not supported"): that leaf is wanted.  Any
    other refusal is answered the same way, on the safe side: the gradient is computed."""
    try:
        return bool(torch._C._will_engine_execute_node(fn))
    except RuntimeError:
        return True


def _wanted_inputs(ctx, is_tensor, first):
    """[will the engine use the gradient of forward input i in THIS backward pass?] for the inputs from `first` on.
    is_tensor: per forward input, whether a tensor was passed -- ctx.next_functions holds one edge per TENSOR input, in order
    (non-tensor arguments and None have none)."""
    count = len(is_tensor) - first
    if not SKIP_UNUSED_DW or torch._C._current_graph_task_id() == -1:
        return [True] * count
    try:
        nf = ctx.next_functions
        if len(nf) != sum(1 for t in is_tensor if t):
            return [True] * count  # (not the layout this rule assumes: compute everything)
        out = []
        e = 0
        for i, t in enumerate(is_tensor):
            fn = nf[e][0] if t else None
            e += 1 if t else 0
            if i >= first:
                out.append(fn is not None and _engine_wants(fn))
        return out
    except (AttributeError, IndexError):  # (an engine without the query: compute everything)
        return [True] * count


class _Pair:
    """The two training forwards that share one Q|K|V image, as seen by their backwards."""
    __slots__ = ("a", "b", "image", "task", "owner", "ran", "__weakref__")

    def __init__(self, a, b):
        self.a, self.b = weakref.ref(a), weakref.ref(b)
        self.image = None   # the deferred dQ|dK|dV of the node that ran first
        self.task = -1      # ... and the backward pass (graph task id) it belongs to
        self.owner = 0      # ... and that node's id
        self.ran = {}       # node id -> graph task id of its last backward

    def decide(self, ctx, task, qkv_all, shape, dev):
        """One dW product per projection for the two backwards over one Q|K|V image (see MERGE_DW above) -> (mode, image) of
        node ctx in backward pass `task`.  qkv_all: ctx computes all six projection gradients and no input gradient.  MERGE:
        the partner ran first in this pass and left its image.  DEFER: it is still to run, ctx leaves a new image of `shape`
        and returns none of the six.  OWN otherwise."""
        mode, image = hip.DQKV_OWN, None
        if self.image is not None and self.task == task and self.owner != id(ctx) and qkv_all:
            mode, image, self.image = hip.DQKV_MERGE, self.image, None
            STATS["merged_dqkv_backwards"] += 1
        else:
            self.image = None  # (an image left by a pass whose second node never ran is dropped)
            partner = self.b() if ctx is self.a() else self.a()
            if (qkv_all and partner is not None and task != -1 and self.ran.get(id(partner)) != task
                    and torch._C._will_engine_execute_node(partner)):
                mode, image = hip.DQKV_DEFER, torch.empty(shape, dtype=torch.float32, device=dev)
                self.image, self.task, self.owner = image, task, id(ctx)
                STATS["deferred_dqkv_backwards"] += 1
        self.ran[id(ctx)] = task
        return mode, image


def _ident(t):
    return None if t is None else (t.data_ptr(), t._version, tuple(t.shape))


def _where(dev):
    """Stream and capture status of a call: a tensor of an EAGER step must never be shared into a step that is being captured
    in a hipGraph (the capture would bake in a pointer to memory outside the graph's pool, freed with the eager step's
    graph), nor across streams."""
    return (torch.cuda.current_stream(dev).cuda_stream, torch.cuda.is_current_stream_capturing())


def _qkv_key(cfg, x, m, ids, params):
    return (_where(x.device), cfg.n_seq, cfg.L, cfg.D, cfg.n_heads, cfg.A, cfg.E, cfg.pool_kind, cfg.has_head, x.device.index, _ident(x), _ident(m),
            _ident(ids), tuple(_ident(p) for p in params[:6]))  # (_att_tensors order: wq, bq, wk, bk, wv, bv, wo, bo)


#: a _QKV_IMAGES entry: the saved blob of a training forward (it holds the Q|K|V image) and that forward's autograd node, both
#: by weak reference -- the entry dies with the forward's graph -- and its row lists
_QkvImage = namedtuple("_QkvImage", "blob rows node")


def _find_qkv_image(key):
    """-> (blob, row lists, node or None) of the live forward under key, or three Nones; a dead entry is dropped."""
    ent = _QKV_IMAGES.get(key) if key is not None else None
    blob = ent.blob() if ent is not None else None
    if blob is None:
        _QKV_IMAGES.pop(key, None)
        return None, None, None
    return blob, ent.rows, ent.node()


def _publish_qkv_image(key, blob, rows, node):
    for k in [k for k, v in _QKV_IMAGES.items() if v.blob() is None]:
        del _QKV_IMAGES[k]
    _QKV_IMAGES[key] = _QkvImage(weakref.ref(blob), rows, weakref.ref(node))


#: A tower's parameters are shared by every call of the tower (the news tower of a grad step is called for the candidates, the
#: history and the history again: training.py:406,409), and autograd adds the calls' parameter gradients pairwise as they
#: arrive -- one elementwise launch per parameter and extra call, 38 per NRMS step.  Here the calls that are NOT the last of
#: their tower in a backward pass keep their parameter gradients back (they return None for them) and the last one -- the
#: engine says which nodes are still to run: torch._C._will_engine_execute_node -- adds the kept sets to its own with ONE
#: multi-tensor launch each (torch._foreach_add_) and returns the sums.  The same gradients up to the order of the additions;
#: a hook on a parameter sees the sum once instead of each contribution.  XNRS_SUM_SHARED_GRADS=0: off.
SUM_SHARED_GRADS = os.environ.get("XNRS_SUM_SHARED_GRADS", "1") != "0"
_PARAM_GROUPS = {}


class _ParamGroup:
    """The live forward nodes of one tower (= one tuple of parameter tensors) and, during a backward pass, the gradient sets
    its earlier nodes kept back."""
    __slots__ = ("nodes", "kept", "task", "ran")

    def __init__(self):
        self.nodes, self.kept, self.task, self.ran = [], [], -1, {}


def _join_group(ctx, params):
    if not SUM_SHARED_GRADS:
        return None
    key = tuple(None if p is None else id(p) for p in params)
    if len(_PARAM_GROUPS) > 64:
        for k in [k for k, g in _PARAM_GROUPS.items() if not any(r() is not None for r in g.nodes)]:
            del _PARAM_GROUPS[k]
    g = _PARAM_GROUPS.get(key)
    if g is None:
        g = _PARAM_GROUPS[key] = _ParamGroup()
    g.nodes = [r for r in g.nodes if r() is not None]
    g.nodes.append(weakref.ref(ctx))
    return g


def _sum_with_group(ctx, grads):
    """Keep this node's parameter gradients back if another node of its tower is still to run in this pass; otherwise add what
    the earlier nodes kept.  -> the list to return to autograd."""
    g = ctx.pgroup
    task = torch._C._current_graph_task_id()
    if g is None or task == -1:
        return grads
    if g.task != task:  # (sets left by a pass that was abandoned are dropped)
        g.kept, g.task = [], task
    g.ran = {k: v for k, v in g.ran.items() if v == task}
    g.ran[id(ctx)] = task
    pending = False
    for r in g.nodes:
        n = r()
        if n is None or n is ctx or g.ran.get(id(n)) == task:
            continue
        try:
            if torch._C._will_engine_execute_node(n):
                pending = True
                break
        except RuntimeError:
            pass
    if pending:
        if any(t is not None for t in grads):
            g.kept.append(grads)
        return [None] * len(grads)
    for kept in g.kept:
        a, b = [], []
        for j, t in enumerate(kept):
            if t is None:
                continue
            if grads[j] is None:
                grads[j] = t          # only an earlier node computed this one (a deferring node leaves its six to the merging one)
            else:
                a.append(grads[j])
                b.append(t)
        if a:
            torch._foreach_add_(a, b)
    g.kept = []
    return grads


#: The folded fc1 pair (W1.Wo, W1.bo + b1: DESIGN.md section 4.6) of a training forward is the same for every call with the
#: same weights: a grad step calls the news tower three times and the user tower twice, so it is computed once per tower and
#: weight version (xnrs_fold_weights; the same routine the in-call fold runs: the same bits) and handed to the forward AND
#: its backward through xnrs_additive_params.w1_folded.  Keyed like every cache here on tensor identity + version counter +
#: stream / capture status.  XNRS_FOLD_TRAIN_CACHE=0: every call folds for itself (three short launches).
FOLD_TRAIN_CACHE = os.environ.get("XNRS_FOLD_TRAIN_CACHE", "1") != "0"
_TRAIN_FOLDS = {}


def _train_fold(l, cfg, params, ap, pp, dev):
    """-> (w1f, b1f) tensors or None when this call does not fold (no attention + additive pair, fold switched off)."""
    if not FOLD_TRAIN_CACHE or cfg.n_heads <= 0 or cfg.pool_kind != hip.POOL_ADDITIVE or not l.xnrs_train_fold_enabled():
        return None
    src = (params[6], params[7], params[8], params[9])  # out.weight, out.bias, fc1.weight, fc1.bias
    key = (_where(dev), dev.index, cfg.D, cfg.A) + tuple(None if t is None else (id(t),) + _ident(t) for t in src)
    hit = _TRAIN_FOLDS.get(key)
    if hit is not None:
        return hit
    if len(_TRAIN_FOLDS) >= 8:  # (every optimizer step retires the entries of the step before)
        _TRAIN_FOLDS.clear()
    w1f = torch.empty((cfg.A, cfg.D), dtype=torch.float32, device=dev)
    b1f = torch.empty((cfg.A,), dtype=torch.float32, device=dev)
    nws = l.xnrs_fold_weights_workspace_bytes(cfg.D, cfg.A)
    ws = hip.workspace(dev, nws)
    hip.check(l.xnrs_fold_weights(hip.ref(ap), hip.ref(pp), cfg.D, hip.ptr(w1f), hip.ptr(b1f), hip.ptr(ws), nws, hip.stream_ptr(dev)),
              "xnrs_fold_weights")
    _TRAIN_FOLDS[key] = (w1f, b1f)
    return w1f, b1f


def _shape_args(cfg):
    """What the library's size queries take."""
    return cfg.n_seq, cfg.L, cfg.D, cfg.A, cfg.Eo, cfg.n_heads, cfg.pool_kind, int(cfg.has_head)


def _forward_prologue(ctx, l, cfg, params, dev):
    """What a training forward of either encoder node prepares -> (ap, pp, hp, keep, saved): the parameter structs with the
    fold pair in place and the blob for the saved activations; on ctx, what _backward_prologue reads."""
    ap, pp, hp, keep = _param_structs(cfg, params)
    ctx.fold_pair = _train_fold(l, cfg, params, ap, pp, dev)
    if ctx.fold_pair is not None:  # (None: the call folds for itself)
        pp.w1_folded, pp.b1_folded = ctx.fold_pair[0].data_ptr(), ctx.fold_pair[1].data_ptr()
    ctx.nsaved = l.xnrs_seq_encoder_saved_bytes(*_shape_args(cfg))
    saved = torch.empty(max(ctx.nsaved, 1), dtype=torch.uint8, device=dev)
    ctx.fold = l.xnrs_train_fold_enabled()  # the saved blob is laid out by this decision (include/xnrs_hip.h)
    ctx.cfg = cfg
    ctx.param_none = [p is None for p in params]
    return ap, pp, hp, keep, saved


def _backward_prologue(ctx, l, ptensors):
    """... and its backward -> (params, ap, pp, hp, keep, nws): the parameter list as the forward took it (ptensors: the saved
    ones, without the None entries), its structs with the forward's fold pair, and the size of the workspace -- which the
    caller takes (hip.workspace) behind its own allocations, so that a growing workspace lands where it always did."""
    cfg = ctx.cfg
    it = iter(ptensors)
    params = [None if isnone else next(it) for isnone in ctx.param_none]
    ap, pp, hp, keep = _param_structs(cfg, params)
    if ctx.fold_pair is not None:  # the pair the forward was given (the saved blob holds no copy then)
        pp.w1_folded, pp.b1_folded = ctx.fold_pair[0].data_ptr(), ctx.fold_pair[1].data_ptr()
    if l.xnrs_train_fold_enabled() != ctx.fold:
        raise hip.XnrsHipError("XNRS_FOLD_TRAIN changed between a training forward and its backward: the saved "
                               "activations were laid out for the other setting (reload the knobs outside a step)")
    return params, ap, pp, hp, keep, l.xnrs_seq_encoder_bwd_workspace_bytes(*_shape_args(cfg))


def _build_rows(l, cfg, x, m, ids, params):
    """The row lists of a training forward that found no earlier forward's to reuse."""
    # Nothing that flows through a masked token row reaches the output or a gradient (its pooling weight is
    # exp(e)*0), so the row-parallel products of an attention tower -- forward (query projection, output projection,
    # fc1) and backward -- run over the unmasked rows only (xnrs_seq_encoder_fwd_train_live / _bwd_live).  Index
    # bookkeeping with torch (one host sync for the count); skipped when few rows are masked.
    if not (LIVE_ROWS and m is not None and cfg.pool_kind == hip.POOL_ADDITIVE and cfg.n_seq * cfg.L >= LIVE_ROWS_MIN):
        return _NO_ROWS
    if DEVICE_LISTS and _device_lists_ok(cfg, x, params):
        return _device_lists(l, cfg, m, ids, x.device)
    return _host_lists(cfg, m, ids, x.device)


class _SeqEncode(torch.autograd.Function):
    """y = head(pool(att(x)))  (any stage optional) with saved activations for the HIP backward."""

    @staticmethod
    def forward(ctx, cfg: _Cfg, x, m, ids, *params):
        x = hip.dev_f32(x, "encoder input")
        dev = x.device
        n, L, D = cfg.n_seq, cfg.L, cfg.D
        pooled = cfg.pool_kind != hip.POOL_NONE
        y = torch.empty((n, cfg.Eo) if pooled else (n, L, D), dtype=torch.float32, device=dev)
        a = torch.empty((n, L), dtype=torch.float32, device=dev) if (cfg.want_a and cfg.pool_kind == hip.POOL_ADDITIVE) else None
        hm = torch.empty((n,), dtype=torch.float32, device=dev) if (pooled and m is not None) else None
        l = hip.lib()
        ap, pp, hp, keep, saved = _forward_prologue(ctx, l, cfg, params, dev)
        # blob of an earlier forward over the same input and projection weights, its row lists, its node
        key = _qkv_key(cfg, x, m, ids, params) if SHARE_QKV and cfg.n_heads > 0 else None
        blob, rows, first = _find_qkv_image(key)
        qkv_shared = None
        if blob is not None:
            STATS["shared_qkv_forwards"] += 1
            qkv_shared = blob.data_ptr() + l.xnrs_seq_encoder_saved_qkv_offset(*_shape_args(cfg))
        else:
            rows = _build_rows(l, cfg, x, m, ids, params)
        lists = rows.struct(qkv_shared, None, hip.DQKV_OWN)
        hip.check(l.xnrs_seq_encoder_fwd_train_rows(hip.ptr(x), hip.ptr(m), hip.ptr(ids), n, L, D, hip.ref(ap), cfg.pool_kind,
                                                    hip.ref(pp), hip.ref(hp), hip.ptr(y), hip.ptr(a), hip.ptr(hm), hip.ptr(saved),
                                                    ctx.nsaved, hip.ref(lists), hip.stream_ptr(dev)),
                  "xnrs_seq_encoder_fwd_train_rows")
        ctx.row_lists, ctx.qkv_shared = rows, qkv_shared
        ctx.qkv_owner = blob  # keeps the other forward's blob alive until our backward
        ctx.pair = None
        if first is not None and first.pair is None:
            ctx.pair = first.pair = _Pair(first, ctx)  # the two backwards share one dW product per projection
        if key is not None and blob is None:
            _publish_qkv_image(key, saved, rows, ctx)
        ctx.pgroup = _join_group(ctx, params)
        ctx.okey = None  # (_run: the key of this forward's _OUTPUTS entry)
        ctx.n_params = len(params)
        ctx.save_for_backward(x, m, ids, saved, *[p for p in params if p is not None])
        outs = [y, a if a is not None else y.new_empty(0), hm if hm is not None else y.new_empty(0)]
        ctx.mark_non_differentiable(outs[1], outs[2])
        ctx.set_materialize_grads(False)  # (the two side outputs never carry a gradient: no zero tensors are made for them)
        return tuple(outs)

    @staticmethod
    def backward(ctx, dy, _da, _dhm):
        _OUTPUTS.pop(ctx.okey, None)  # the graph is being consumed: its outputs are no longer shareable
        if dy is None:  # (nothing flows into the only differentiable output)
            return (None,) * (4 + ctx.n_params)
        cfg = ctx.cfg
        x, m, ids, saved, *ptensors = ctx.saved_tensors
        dev = x.device
        n, L, D = cfg.n_seq, cfg.L, cfg.D
        need = ctx.needs_input_grad  # (cfg, x, m, ids, *params)
        want_dx = need[1]
        if want_dx and ids is not None:
            raise hip.XnrsHipError("no input gradient through an id-gathered news table")
        l = hip.lib()
        params, ap, pp, hp, keep, nws = _backward_prologue(ctx, l, ptensors)
        dy = hip.dev_f32(dy, "grad output")
        dx = torch.empty((n, L, D), dtype=torch.float32, device=dev) if want_dx else None
        wanted = _wanted_inputs(ctx, [False, True, m is not None, ids is not None] + [p is not None for p in params], 4)
        grads = [torch.empty_like(p, dtype=torch.float32) if (p is not None and need[4 + j] and wanted[j]) else None
                 for j, p in enumerate(params)]
        ws = hip.workspace(dev, nws)
        mode, image = hip.DQKV_OWN, None
        if ctx.pair is not None:
            qkv_all = MERGE_DW and not want_dx and all(g is not None for g in grads[:6])
            mode, image = ctx.pair.decide(ctx, torch._C._current_graph_task_id(), qkv_all, (n * L, 3 * D), dev)
            if mode == hip.DQKV_DEFER:
                grads[:6] = [None] * 6  # the merging node returns them (computed from the sum)
        ga, gp, gh = _grad_structs(cfg, grads)
        lists = ctx.row_lists.struct(ctx.qkv_shared, image, mode)  # the row lists built by the forward
        hip.check(l.xnrs_seq_encoder_bwd_rows(hip.ptr(x), hip.ptr(m), hip.ptr(ids), n, L, D, hip.ref(ap), cfg.pool_kind, hip.ref(pp),
                                              hip.ref(hp), hip.ptr(saved), ctx.nsaved, hip.ptr(dy), hip.ptr(dx), hip.ref(ga),
                                              hip.ref(gp), hip.ref(gh), hip.ref(lists), hip.ptr(ws), nws,
                                              hip.stream_ptr(dev)), "xnrs_seq_encoder_bwd_rows")
        return (None, dx, None, None, *_sum_with_group(ctx, grads))


def _host_lists(cfg, m, ids, dev):
    """The row lists by torch bookkeeping: a nonzero and ONE host read for both counts (round 3's path; kept for shapes the
    device-counted kernels do not serve and behind XNRS_DEVICE_LISTS=0)."""
    n, L = cfg.n_seq, cfg.L
    lm = (m[ids.long()] if ids is not None else m).reshape(n, L).ne(0)
    news_live = lm.any(dim=1)
    n_live, n_news_live = (int(v) for v in torch.stack([lm.sum(), news_live.sum()]).tolist())
    if n_live > LIVE_ROWS_MAX_FRACTION * n * L:
        return _NO_ROWS
    rows_live = torch.nonzero_static(lm.reshape(-1), size=n_live).squeeze(1)
    r = _Rows(rows_live.to(torch.int32), n_live=n_live)
    STATS["live_row_forwards"] += 1
    if ids is not None:
        src_news = ids.long()
        seq = torch.div(rows_live, L, rounding_mode="floor")
        r.live_src = (src_news[seq] * L + (rows_live - seq * L)).to(torch.int32)
    # the token rows of the non-empty news: K and V are projected (and their weight gradients summed) over
    # these only -- nobody reads the keys of a news without a live query (include/xnrs_hip.h: xnrs_row_lists)
    if KV_ROWS and cfg.n_heads > 0 and n_news_live < n:
        news_idx = torch.nonzero_static(news_live, size=n_news_live).squeeze(1)
        tok = torch.arange(L, device=dev)
        r.kv, r.n_kv = (news_idx[:, None] * L + tok[None, :]).reshape(-1).to(torch.int32), n_news_live * L
        STATS["kv_row_forwards"] += 1
        if ids is not None:
            r.kv_src = (src_news[news_idx][:, None] * L + tok[None, :]).reshape(-1).to(torch.int32)
    return r


def _device_lists_ok(cfg, x, params) -> bool:
    """Do the kernels that read their row count on the device serve this call?  (The conditions device_counts_ok in
    encoder_fwd.hip checks again: fp32 GEMM mode, D and A multiples of 4, 16-byte aligned input and weights.)"""
    if hip.get_gemm_mode() != 0 or cfg.D % 4 != 0 or cfg.A % 4 != 0 or cfg.n_seq * cfg.L >= 2 ** 31:
        return False
    return x.data_ptr() % 16 == 0 and all(p is None or p.data_ptr() % 16 == 0 for p in params)


def _device_lists(l, cfg, m, ids, dev):
    n, L = cfg.n_seq, cfg.L
    cap = n * L
    buf = torch.empty((4 if ids is not None else 2, cap), dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    live, kv = buf[0], buf[1]
    live_src, kv_src = (buf[2], buf[3]) if ids is not None else (None, None)
    nws = l.xnrs_row_lists_workspace_bytes(n)
    ws = hip.workspace(dev, nws)
    hip.check(l.xnrs_build_row_lists(hip.ptr(m), hip.ptr(ids), n, L, hip.ptr(live), hip.ptr(live_src), hip.ptr(kv),
                                     hip.ptr(kv_src), hip.ptr(counts), hip.ptr(ws), nws, hip.stream_ptr(dev)),
              "xnrs_build_row_lists")
    STATS["device_list_forwards"] += 1
    STATS["live_row_forwards"] += 1
    if KV_ROWS and cfg.n_heads > 0:
        STATS["kv_row_forwards"] += 1
    else:
        kv = kv_src = None
    return _Rows(live, live_src, cap, kv, kv_src, cap, counts)  # capacities: the counts stay on the device


class _SeqEncodeFromQkv(torch.autograd.Function):
    """y = head(pool(att core(qkv))): an attention tower's training forward that READS a given Q|K|V image ((n_seq * L, 3D),
    xnrs_row_lists::qkv_shared) and projects nothing; the image is the one differentiable input.  The backward leaves
    dQ|dK|dV in the gradient it returns (XNRS_DQKV_DEFER) and stops before the projection products: no input gradient, no
    parameter gradient -- the parameters are not even inputs of the node (integrated gradients with one projection,
    explain.py).  No row lists: every row of the returned image is written, the rows of an all-masked
    sequence as zeros.  Neither pass writes the image or the saved blob, so one forward serves any number of backward passes
    (retain_graph=True); nothing is registered in _QKV_IMAGES and no _Pair is formed."""

    @staticmethod
    def forward(ctx, cfg: _Cfg, qkv, m, params):
        qkv = hip.dev_f32(qkv, "Q|K|V image")
        dev = qkv.device
        n, L, D = cfg.n_seq, cfg.L, cfg.D
        if tuple(qkv.shape) != (n * L, 3 * D):
            raise hip.XnrsHipError(f"Q|K|V image {tuple(qkv.shape)}: expected {(n * L, 3 * D)}")
        if qkv.data_ptr() % hip.WORKSPACE_ALIGN:
            raise hip.XnrsHipError(f"Q|K|V image at {qkv.data_ptr():#x} is not {hip.WORKSPACE_ALIGN}-byte aligned")
        y = torch.empty((n, cfg.Eo), dtype=torch.float32, device=dev)
        hm = torch.empty((n,), dtype=torch.float32, device=dev)
        l = hip.lib()
        ap, pp, hp, keep, saved = _forward_prologue(ctx, l, cfg, params, dev)
        lists = _NO_ROWS.struct(qkv.data_ptr(), None, hip.DQKV_OWN)
        # x: the entry points want a non-NULL input; with a given image nothing reads it (project() returns at once, every
        # later stage of an attention tower reads the image or what follows it, and the deferring backward stops before the
        # projection products) -- the image's own address stands in, which is at least as large as the tokens would be
        hip.check(l.xnrs_seq_encoder_fwd_train_rows(hip.ptr(qkv), hip.ptr(m), None, n, L, D, hip.ref(ap), cfg.pool_kind, hip.ref(pp),
                                                    hip.ref(hp), hip.ptr(y), None, hip.ptr(hm), hip.ptr(saved), ctx.nsaved,
                                                    hip.ref(lists), hip.stream_ptr(dev)), "xnrs_seq_encoder_fwd_train_rows")
        ctx.save_for_backward(qkv, m, saved, *[p for p in params if p is not None])
        ctx.mark_non_differentiable(hm)
        ctx.set_materialize_grads(False)
        return y, hm

    @staticmethod
    def backward(ctx, dy, _dhm):
        if dy is None:
            return None, None, None, None
        cfg = ctx.cfg
        qkv, m, saved, *ptensors = ctx.saved_tensors
        dev = qkv.device
        n, L, D = cfg.n_seq, cfg.L, cfg.D
        l = hip.lib()
        params, ap, pp, hp, keep, nws = _backward_prologue(ctx, l, ptensors)
        dy = hip.dev_f32(dy, "grad output")
        ws = hip.workspace(dev, nws)
        image = _f32_out((n * L, 3 * D), dev)
        # no row lists: dead_seq_mode 0, the attention backward writes EVERY row of the image (the reduce sums every row)
        lists = _NO_ROWS.struct(qkv.data_ptr(), image, hip.DQKV_DEFER)
        hip.check(l.xnrs_seq_encoder_bwd_rows(hip.ptr(qkv), hip.ptr(m), None, n, L, D, hip.ref(ap), cfg.pool_kind, hip.ref(pp),
                                              hip.ref(hp), hip.ptr(saved), ctx.nsaved, hip.ptr(dy), None, None, None, None,
                                              hip.ref(lists), hip.ptr(ws), nws, hip.stream_ptr(dev)), "xnrs_seq_encoder_bwd_rows")
        return None, image, None, None


def _encoder_cfg(n, L, D, att, pooler, head, pool_kind, dropout_p, seed, want_a):
    """-> (cfg, params) of a call of n sequences through the modules given (att and head may be None): the static description
    and the flat parameter list (att 8 | pool 4 | head 4) that _param_structs splits again."""
    params: List[Optional[torch.Tensor]] = []
    n_heads, scaled, A, E, has_head = 0, True, 0, D, False
    if att is not None:
        params += _att_tensors(att)
        n_heads, scaled = att.h, att.scaled
    if pool_kind == hip.POOL_ADDITIVE:
        params += _pool_tensors(pooler)
        A = pooler.fc1.out_features
    if head is not None:
        params += _head_tensors(head)
        has_head, E = True, head[0].out_features
    cfg = _Cfg(n, L, D, n_heads, scaled, pool_kind, A, has_head, E, False, dropout_p, seed, want_a)
    if head is not None:
        cfg.head_act = hip.head_activation(head[1])
    return cfg, params


def text_encoder_from_qkv(qkv, x, m, enc, dropout_p, seed):
    """ops.text_encoder_from_qkv: (y:(n_seq, E'), hm:(n_seq,)) of an attention TextEncoder from its Q|K|V image."""
    from . import ops
    L, D = x.shape[-2], x.shape[-1]  # x: the tokens the image was projected from -- for their shape; they are not read
    if qkv.dim() != 2 or qkv.shape[1] != 3 * D or qkv.shape[0] % L:
        raise hip.XnrsHipError(f"Q|K|V image {tuple(qkv.shape)} does not hold sequences of {L} rows of 3 * {D}")
    n = qkv.shape[0] // L
    if m is None:
        raise hip.XnrsHipError("text_encoder_from_qkv needs the token mask")
    m2 = ops._mask2d(m, n, L, "encoder mask")
    cfg, params = _encoder_cfg(n, L, D, enc.att, enc.pooler, getattr(enc, "head", None), _pool_kind(enc.pooler), dropout_p,
                               seed, False)
    # the parameters travel as a tuple: they are no inputs of the node, so no backward pass is ever asked for their gradients
    return _SeqEncodeFromQkv.apply(cfg, qkv, m2, tuple(params))


#: A DETERMINISTIC encode (no attention dropout in play: no attention tower, or p = 0 / eval mode) called again with the very
#: same tensors -- input, mask, ids and every parameter the same objects at the same version -- while the first call's graph
#: is still alive returns the first call's OUTPUT TENSORS (same autograd node).  The reference's train step encodes the
#: history twice (training.py:406 model(batch), :409 get_user_embeddings(batch)); for StandardRec / NAML (no dropout anywhere
#: in the shipped configs) the second encode is bit for bit the first, so it is not computed, and since the user tower then
#: sees the same tensor object again, neither is its second call.  Gradients: the node receives the sum of both uses'
#: gradients and runs ONE backward -- the same gradient up to summation order.  XNRS_SHARE_OUTPUTS=0: off.
SHARE_OUTPUTS = os.environ.get("XNRS_SHARE_OUTPUTS", "1") != "0"
_OUTPUTS = {}
_OUTPUTS_HORIZON = 16  # encoder calls after which an unclaimed entry is dropped (a step's second encode follows within ~8)
#: ... and a cap on the saved activations the unclaimed entries may pin (an entry keeps its graph, i.e. its saved blob, alive
#: until its backward runs or it is dropped): a forward-only loop that forgot torch.no_grad() must not hoard a blob per call
_OUTPUTS_MAX_BYTES = int(os.environ.get("XNRS_SHARE_OUTPUTS_MB", "4096")) << 20
_TICK = 0


def _root(t):
    """The tensor that owns t's storage (views compare by their base: modules reshape their inputs on every call)."""
    return t if (t is None or t._base is None) else t._base


def _alive(refs, objs):
    return all((r is None and o is None) or (r is not None and r() is _root(o)) for r, o in zip(refs, objs))


#: an _OUTPUTS entry: the tick of its last use, the call's tensor arguments by weak reference (a claim needs the very same
#: objects), the outputs (y, a, hm), y's version when they were made and the bytes of saved activations the entry pins
_Output = namedtuple("_Output", "tick refs outs version nbytes")


def _claim_output(okey, objs):
    """One encoder call further: entries unclaimed for _OUTPUTS_HORIZON calls are dropped.  -> the outputs under okey (None:
    this call shares nothing) if they still stand for a call with the tensors objs (else that entry is dropped), or None."""
    global _TICK
    _TICK += 1
    for k in [k for k, v in _OUTPUTS.items() if _TICK - v.tick > _OUTPUTS_HORIZON]:
        del _OUTPUTS[k]  # (never claimed: a forward in grad mode that nobody repeated)
    hit = _OUTPUTS.get(okey) if okey is not None else None
    if hit is None:
        return None
    y = hit.outs[0]
    if _alive(hit.refs, objs) and y._version == hit.version and y.grad_fn is not None:
        STATS["shared_output_forwards"] += 1
        _OUTPUTS[okey] = hit._replace(tick=_TICK)
        return hit.outs
    del _OUTPUTS[okey]
    return None


def _publish_output(okey, objs, outs):
    # the entry holds the outputs themselves (modules drop them: a view of y fed to torch.cat keeps nothing alive) and
    # is dropped by the node's backward, or after _OUTPUTS_HORIZON further encoder calls
    node = outs[0].grad_fn
    refs = [None if o is None else weakref.ref(_root(o)) for o in objs]
    _OUTPUTS[okey] = _Output(_TICK, refs, outs, outs[0]._version, node.nsaved)
    node.okey = okey
    pinned = sum(v.nbytes for v in _OUTPUTS.values())
    for k in sorted(_OUTPUTS, key=lambda k: _OUTPUTS[k].tick):  # oldest first; the entry just made always stays
        if pinned <= _OUTPUTS_MAX_BYTES or k == okey:
            break
        pinned -= _OUTPUTS[k].nbytes
        del _OUTPUTS[k]


def _run(x, m, ids, att, pooler, head, pool_kind, dropout_p, seed, want_a):
    from . import ops
    objs = [x, m, ids]
    x = hip.dev_f32(x, "encoder input")
    n_tab, L, D = x.shape
    m2 = ops._mask2d(m, n_tab, L, "encoder mask")
    if ids is not None:
        ids = ids.to(torch.int32).contiguous()
        n = ids.numel()
    else:
        n = n_tab
    cfg, params = _encoder_cfg(n, L, D, att, pooler, head, pool_kind, dropout_p, seed, want_a)
    okey = None
    if SHARE_OUTPUTS and (cfg.n_heads == 0 or dropout_p == 0.0) and torch.is_grad_enabled():
        objs += params
        okey = (_where(x.device), n, L, D, cfg.n_heads, cfg.scaled, pool_kind, cfg.A, cfg.has_head, cfg.E, cfg.head_act, want_a,
                x.device.index, _ident(x), _ident(m2), _ident(ids), tuple(_ident(p) for p in params))
    outs = _claim_output(okey, objs)
    if outs is not None:
        return outs
    y, a, hm = _SeqEncode.apply(cfg, x, m2, ids, *params)
    outs = (y, a if a.numel() else None, hm if hm.numel() else None)
    if okey is not None and y.grad_fn is not None:
        _publish_output(okey, objs, outs)
    return outs


def _pool_kind(pooler):
    from .models.components import layers
    if isinstance(pooler, layers.AdditiveAttention):
        return hip.POOL_ADDITIVE
    if isinstance(pooler, layers.MaskedMean):
        return hip.POOL_MEAN
    raise hip.XnrsHipError(f"pooler {type(pooler).__name__} has no HIP implementation")


# ------------------------------------------------------------------------- entry points used by ops.py
def mha(x, m, att, dropout_p, seed):
    y, _, _ = _run(x, m, None, att, None, None, hip.POOL_NONE, dropout_p, seed, False)
    return y


def additive(x, m, pool, return_weights):
    y, a, _ = _run(x, m, None, None, pool, None, hip.POOL_ADDITIVE, 0.0, 0, return_weights)
    y = y.unsqueeze(1)
    return (y, a.unsqueeze(-1)) if return_weights else y


def masked_mean(x, m):
    from .models.components import layers
    y, _, _ = _run(x, m, None, None, layers.MaskedMean(), None, hip.POOL_MEAN, 0.0, 0, False)
    return y.unsqueeze(1)


def text_encoder(x, m, enc, ids, dropout_p, seed):
    head = getattr(enc, "head", None)
    y, _, hm = _run(x, m, ids, enc.att, enc.pooler, head, _pool_kind(enc.pooler), dropout_p, seed, False)
    return y, hm


def user_encoder(x, m, enc, return_weights, dropout_p, seed):
    head = getattr(enc, "head", None)
    y, a, _ = _run(x, m, None, enc.att, enc.pooler, head, _pool_kind(enc.pooler), dropout_p, seed, return_weights)
    y = y.unsqueeze(1)
    return (y, a.unsqueeze(-1)) if return_weights else y


class _InputDropout(torch.autograd.Function):
    """nn.Dropout on a tower's input (ops.input_dropout): the mask is a pure function of (seed, row, column), so the backward
    recomputes it on dy -- the same launch -- and nothing is saved."""

    @staticmethod
    def forward(ctx, x, p, seed, word):
        from . import ops
        ctx.p, ctx.seed, ctx.word = p, seed, word  # (the word as of the forward, like _Cfg.seed_word)
        x = hip.dev_f32(x, "input_dropout input")
        return ops.dropout_rows(x, None, torch.empty_like(x), p, seed, word)

    @staticmethod
    def backward(ctx, dy):
        from . import ops
        dy = hip.dev_f32(dy, "grad output")
        return ops.dropout_rows(dy, None, torch.empty_like(dy), ctx.p, ctx.seed, ctx.word), None, None, None


def input_dropout(x, p, seed, word):
    return _InputDropout.apply(x, p, seed, word)


class _Linear(torch.autograd.Function):
    """y = act(rows . w^T + b) (ops.linear): the rows are x's, or -- with ids -- the rows ids gather from the table x.  Backward:
    xnrs_act_bwd when there is an activation, then ONE of xnrs_linear_bwd / xnrs_embedding_linear_bwd (table_grad "dense") /
    xnrs_embedding_linear_bwd_sparse ("sparse": a large table, the gradient costs what the ids cost)."""

    @staticmethod
    def forward(ctx, x, ids, w, b, act, table_grad):
        from . import ops
        x, w = hip.dev_f32(x, "linear input"), hip.dev_f32(w, "linear weight")
        ids = None if ids is None else ids.to(torch.int32).contiguous()
        with torch.no_grad():
            y = ops.linear(x, w, b, act, ids=ids)
        ctx.save_for_backward(x, ids, w, y if act != hip.ACT_NONE else None)
        ctx.has_bias, ctx.act, ctx.table_grad = b is not None, int(act), table_grad
        return y

    @staticmethod
    def backward(ctx, dy):
        x, ids, w, y = ctx.saved_tensors
        dy = hip.dev_f32(dy, "dy")
        dev, l = x.device, hip.lib()
        if y is not None:
            dpre = torch.empty_like(dy)
            hip.check(l.xnrs_act_bwd(hip.ptr(y), hip.ptr(dy), hip.ptr(dpre), dy.numel(), ctx.act, hip.stream_ptr(dev)), "xnrs_act_bwd")
            dy = dpre
        K, N = w.shape[1], w.shape[0]
        M = x.numel() // K if ids is None else ids.numel()
        wanted = _wanted_inputs(ctx, [True, ids is not None, True, ctx.has_bias, False, False], 0)
        need = [n and k for n, k in zip(ctx.needs_input_grad, wanted)]  # x ids w b act table_grad
        dx = torch.empty_like(x) if need[0] else None
        dw = torch.empty_like(w) if need[2] else None
        db = _f32_out((N,), dev) if (ctx.has_bias and need[3]) else None
        if ids is None:
            nws = l.xnrs_linear_bwd_workspace_bytes(M, N, K)
            ws = hip.workspace(dev, nws)
            hip.check(l.xnrs_linear_bwd(hip.ptr(x), None, 0, hip.ptr(w), hip.ptr(dy), hip.ptr(dx), hip.ptr(dw), hip.ptr(db), M, N,
                                        K, hip.ptr(ws), nws, hip.stream_ptr(dev)), "xnrs_linear_bwd")
        else:
            name = "xnrs_embedding_linear_bwd_sparse" if ctx.table_grad == "sparse" else "xnrs_embedding_linear_bwd"
            nws = getattr(l, name + "_workspace_bytes")(M, N, K)
            ws = hip.workspace(dev, nws)
            hip.check(getattr(l, name)(hip.ptr(x), hip.ptr(ids), hip.ptr(w), hip.ptr(dy), hip.ptr(dx), hip.ptr(dw), hip.ptr(db), M, N,
                                       K, x.shape[0], hip.ptr(ws), nws, hip.stream_ptr(dev)), name)
        return dx, None, dw, db, None, None


def linear(x, ids, w, b, act, table_grad):
    return _Linear.apply(x, ids, w, b, act, table_grad)


class _DotScoring(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, c, normalize):
        from . import ops
        u = hip.dev_f32(u, "user vector")
        c = hip.dev_f32(c, "candidate vectors")
        ctx.save_for_backward(u, c)
        ctx.normalize = bool(normalize)
        with torch.no_grad():
            return ops.dot_scoring_forward(u, c, ctx.normalize)

    @staticmethod
    def backward(ctx, dr):
        u, c = ctx.saved_tensors
        dr = hip.dev_f32(dr, "dr")
        B, Cn, E = c.shape
        du = torch.empty_like(u) if ctx.needs_input_grad[0] else None
        dc = torch.empty_like(c) if ctx.needs_input_grad[1] else None
        fn = hip.lib().xnrs_dot_scoring_norm_bwd if ctx.normalize else hip.lib().xnrs_dot_scoring_bwd
        hip.check(fn(hip.ptr(u), hip.ptr(c), hip.ptr(dr), hip.ptr(du), hip.ptr(dc), B, Cn, E, hip.stream_ptr(c.device)),
                  "xnrs_dot_scoring_norm_bwd" if ctx.normalize else "xnrs_dot_scoring_bwd")
        return du, dc, None


def dot_scoring(u, c, normalize):
    return _DotScoring.apply(u, c, normalize)


class _TableLoss(torch.autograd.Function):
    """ops.table_loss: the full-table softmax ranking loss (xnrs_table_loss_fwd / _bwd).  The backward recomputes the scores;
    what is saved is per query and per user only."""

    @staticmethod
    def forward(ctx, table, up, tgt_off, tgt_rows, excl_off, excl_rows, pad_row, win_lo, win_hi, bias):
        from . import ops
        table = hip.dev_f32(table, "news vectors")
        up_shape = tuple(up.shape)
        up = hip.dev_f32(up, "user vectors").reshape(-1, table.shape[-1])
        with torch.no_grad():
            loss, scores, lse = ops.table_loss_forward(table, up, tgt_off, tgt_rows, excl_off, excl_rows, pad_row, win_lo, win_hi,
                                                       bias)
        ctx.save_for_backward(table, up, scores, lse)
        ctx.rest = (tgt_off, tgt_rows, excl_off, excl_rows, int(pad_row), win_lo, win_hi, None if bias is None else bias.detach())
        ctx.up_shape = up_shape
        ctx.is_tensor = [isinstance(t, torch.Tensor) for t in (table, up, tgt_off, tgt_rows, excl_off, excl_rows, pad_row, win_lo,
                                                               win_hi, bias)]
        ctx.mark_non_differentiable(scores, lse)
        return loss, scores, lse

    @staticmethod
    def backward(ctx, g, _g_scores, _g_lse):
        from . import ops
        table, up, scores, lse = ctx.saved_tensors
        tgt_off, tgt_rows, excl_off, excl_rows, pad_row, win_lo, win_hi, bias = ctx.rest
        wanted = _wanted_inputs(ctx, ctx.is_tensor, 0)  # (torch.autograd.grad(inputs=[u]) alone: the table's sweep is not run)
        d_up, d_table = ops.table_loss_backward(table, up, tgt_off, tgt_rows, excl_off, excl_rows, pad_row, win_lo, win_hi, bias,
                                                scores, lse, g, want_d_up=ctx.needs_input_grad[1] and wanted[1],
                                                want_d_table=ctx.needs_input_grad[0] and wanted[0])
        if d_up is not None:
            d_up = d_up.reshape(ctx.up_shape)
        return d_table, d_up, None, None, None, None, None, None, None, None


def table_loss(table, up, tgt_off, tgt_rows, excl_off, excl_rows, pad_row, win_lo, win_hi, bias):
    return _TableLoss.apply(table, up, tgt_off, tgt_rows, excl_off, excl_rows, pad_row, win_lo, win_hi, bias)


class _ListLoss(torch.autograd.Function):
    """ops.list_loss: the softmax ranking loss over per-user row lists (xnrs_list_loss_fwd / _bwd).  What is saved beside the
    operands is per query, per user and per slot -- the slot scores, never the listed rows."""

    @staticmethod
    def forward(ctx, table, up, tgt_off, tgt_rows, neg_rows, pad_row, bias):
        from . import ops
        table = hip.dev_f32(table, "news vectors")
        up_shape = tuple(up.shape)
        up = hip.dev_f32(up, "user vectors").reshape(-1, table.shape[-1])
        with torch.no_grad():
            loss, scores, lse, neg_scores = ops.list_loss_forward(table, up, tgt_off, tgt_rows, neg_rows, pad_row, bias)
        ctx.save_for_backward(table, up, scores, lse, neg_scores)
        ctx.rest = (tgt_off, tgt_rows, neg_rows, int(pad_row), None if bias is None else bias.detach())
        ctx.up_shape = up_shape
        ctx.is_tensor = [isinstance(t, torch.Tensor) for t in (table, up, tgt_off, tgt_rows, neg_rows, pad_row, bias)]
        ctx.mark_non_differentiable(scores, lse, neg_scores)
        return loss, scores, lse, neg_scores

    @staticmethod
    def backward(ctx, g, _g_scores, _g_lse, _g_neg):
        from . import ops
        table, up, scores, lse, neg_scores = ctx.saved_tensors
        tgt_off, tgt_rows, neg_rows, pad_row, bias = ctx.rest
        wanted = _wanted_inputs(ctx, ctx.is_tensor, 0)  # (torch.autograd.grad(inputs=[u]) alone: the table's launches are not run)
        d_up, d_table = ops.list_loss_backward(table, up, tgt_off, tgt_rows, neg_rows, pad_row, bias, scores, lse, neg_scores, g,
                                               want_d_up=ctx.needs_input_grad[1] and wanted[1],
                                               want_d_table=ctx.needs_input_grad[0] and wanted[0])
        if d_up is not None:
            d_up = d_up.reshape(ctx.up_shape)
        return d_table, d_up, None, None, None, None, None


def list_loss(table, up, tgt_off, tgt_rows, neg_rows, pad_row, bias):
    return _ListLoss.apply(table, up, tgt_off, tgt_rows, neg_rows, pad_row, bias)


class _ListXent(torch.autograd.Function):
    """ops.list_xent: the soft-target loss over per-user row lists (xnrs_list_xent_fwd / _bwd).  What is saved beside the
    operands is per user and per slot -- lse and the slot scores, never the listed rows."""

    @staticmethod
    def forward(ctx, table, up, rows, weights, pad_row, bias):
        from . import ops
        table = hip.dev_f32(table, "news vectors")
        up_shape = tuple(up.shape)
        up = hip.dev_f32(up, "user vectors").reshape(-1, table.shape[-1])
        weights = weights.detach()
        with torch.no_grad():
            loss, lse, slot_scores = ops.list_xent_forward(table, up, rows, weights, pad_row, bias)
        ctx.save_for_backward(table, up, lse, slot_scores)
        ctx.rest = (rows, weights, int(pad_row), None if bias is None else bias.detach())
        ctx.up_shape = up_shape
        ctx.is_tensor = [isinstance(t, torch.Tensor) for t in (table, up, rows, weights, pad_row, bias)]
        ctx.mark_non_differentiable(lse, slot_scores)
        return loss, lse, slot_scores

    @staticmethod
    def backward(ctx, g, _g_lse, _g_slots):
        from . import ops
        table, up, lse, slot_scores = ctx.saved_tensors
        rows, weights, pad_row, bias = ctx.rest
        wanted = _wanted_inputs(ctx, ctx.is_tensor, 0)  # (torch.autograd.grad(inputs=[u]) alone: the table's launches are not run)
        d_up, d_table = ops.list_xent_backward(table, up, rows, weights, pad_row, bias, lse, slot_scores, g,
                                               want_d_up=ctx.needs_input_grad[1] and wanted[1],
                                               want_d_table=ctx.needs_input_grad[0] and wanted[0])
        if d_up is not None:
            d_up = d_up.reshape(ctx.up_shape)
        return d_table, d_up, None, None, None, None


def list_xent(table, up, rows, weights, pad_row, bias):
    return _ListXent.apply(table, up, rows, weights, pad_row, bias)


class _BilinScoring(torch.autograd.Function):
    """BilinScoring (scoring.py:41-66): backward G_b = sum_n g_bn c^_bn, dW[0] = U^^T G, du^_b = W[0] G_b, dc^_bn = g_bn v_b,
    dbias = sum g (then through the normalisation when it is on)."""

    @staticmethod
    def forward(ctx, u, c, w, b, normalize):
        from . import ops
        with torch.no_grad():
            s, saved = ops.bilinear_scoring_forward(u, c, w, b, normalize, keep=True)
        ctx.save_for_backward(hip.dev_f32(u, "user vector"), hip.dev_f32(c, "candidate vectors"), hip.dev_f32(w, "bilinear weight"),
                              saved)
        ctx.normalize = bool(normalize)
        ctx.has_bias = b is not None
        ctx.u_shape = tuple(u.shape)
        return s

    @staticmethod
    def backward(ctx, ds):
        u, c, w, saved = ctx.saved_tensors
        ds = hip.dev_f32(ds, "ds")
        B, N, E = c.shape
        wanted = _wanted_inputs(ctx, [True, True, True, ctx.has_bias, False], 0)
        need = [n and k for n, k in zip(ctx.needs_input_grad, wanted)]
        du = torch.empty(ctx.u_shape, dtype=torch.float32, device=c.device) if need[0] else None
        dc = torch.empty_like(c) if need[1] else None
        dw = torch.empty_like(w) if need[2] else None
        db = torch.empty((1,), dtype=torch.float32, device=c.device) if (ctx.has_bias and need[3]) else None
        l = hip.lib()
        nws = l.xnrs_bilinear_scoring_bwd_workspace_bytes(B, E, int(ctx.normalize))
        ws = hip.workspace(c.device, nws)
        hip.check(l.xnrs_bilinear_scoring_bwd(hip.ptr(u), hip.ptr(c), hip.ptr(w), hip.ptr(saved), saved.numel(), hip.ptr(ds),
                                              hip.ptr(du), hip.ptr(dc), hip.ptr(dw), hip.ptr(db), B, N, E, int(ctx.normalize),
                                              hip.ptr(ws), nws, hip.stream_ptr(c.device)), "xnrs_bilinear_scoring_bwd")
        return du, dc, dw, db, None


def bilinear_scoring(u, c, w, b, normalize):
    return _BilinScoring.apply(u, c, w, b, normalize)


class _MlpScoring(torch.autograd.Function):
    """FCScoring with tanh (scoring.py:69-102), factorised: delta_bn = g_bn w2 (1 - t^2), dw2 = sum g t, db2 = sum g,
    db1 = sum delta, dW1 = [sum_b Delta_b (x) u_b | sum_bn delta_bn (x) c_bn], du_b = W1u^T Delta_b, dc_bn = W1c^T delta_bn
    (Delta_b = sum_n delta_bn)."""

    @staticmethod
    def forward(ctx, u, c, w1, b1, w2, b2):
        from . import ops
        with torch.no_grad():
            s, saved = ops.mlp_scoring_forward(u, c, w1, b1, w2, b2, keep=True)
        ctx.save_for_backward(hip.dev_f32(u, "user vector"), hip.dev_f32(c, "candidate vectors"), hip.dev_f32(w1, "fc1 weight"),
                              hip.dev_f32(w2, "fc2 weight"), saved)
        ctx.has_b1, ctx.has_b2 = b1 is not None, b2 is not None
        ctx.u_shape = tuple(u.shape)
        return s

    @staticmethod
    def backward(ctx, ds):
        u, c, w1, w2, saved = ctx.saved_tensors
        ds = hip.dev_f32(ds, "ds")
        B, N, E = c.shape
        H = w1.shape[0]
        wanted = _wanted_inputs(ctx, [True, True, True, ctx.has_b1, True, ctx.has_b2], 0)
        need = [n and k for n, k in zip(ctx.needs_input_grad, wanted)]
        dev = c.device
        du = torch.empty(ctx.u_shape, dtype=torch.float32, device=dev) if need[0] else None
        dc = torch.empty_like(c) if need[1] else None
        dw1 = torch.empty_like(w1) if need[2] else None
        db1 = torch.empty((H,), dtype=torch.float32, device=dev) if (ctx.has_b1 and need[3]) else None
        dw2 = torch.empty_like(w2) if need[4] else None
        db2 = torch.empty((1,), dtype=torch.float32, device=dev) if (ctx.has_b2 and need[5]) else None
        l = hip.lib()
        nws = l.xnrs_mlp_scoring_bwd_workspace_bytes(B, N, H)
        ws = hip.workspace(dev, nws)
        hip.check(l.xnrs_mlp_scoring_bwd(hip.ptr(u), hip.ptr(c), hip.ptr(w1), hip.ptr(w2), hip.ptr(saved), saved.numel(), hip.ptr(ds),
                                         hip.ptr(du), hip.ptr(dc), hip.ptr(dw1), hip.ptr(db1), hip.ptr(dw2), hip.ptr(db2), B, N, E, H,
                                         hip.ptr(ws), nws, hip.stream_ptr(dev)), "xnrs_mlp_scoring_bwd")
        return du, dc, dw1, db1, dw2, db2


def mlp_scoring(u, c, w1, b1, w2, b2):
    return _MlpScoring.apply(u, c, w1, b1, w2, b2)


# ---- layers.PersonalizedAttention (layers.py:72-102) [+ NPA's news head, npa.py:22-26]: include/xnrs_hip.h
#      xnrs_personalized_*.  One node per encoder call; the query rows q are an input like any other (their gradient is
#      summed per query row on the device), q_idx / ids / m are not differentiable.
def personalized_params(x_fc, q, q_idx, keep):
    """xnrs_personalized_params of x_fc + the query rows q:(n_q, A) (row stride q.stride(0), unit column stride).  A q_idx
    outside [0, n_q) reads no query: that sequence's outputs are NaN and hip.STATUS_QUERY_RANGE is set (hip.check_status)."""
    wx = hip.dev_f32(x_fc.weight, "x_fc weight")
    bx = None if x_fc.bias is None else hip.dev_f32(x_fc.bias, "x_fc bias")
    if not q.is_cuda or not q_idx.is_cuda:
        raise hip.XnrsHipError("personalized attention: the query rows and their indices must live on the HIP device")
    if q.dtype != torch.float32 or q.dim() != 2 or q.stride(1) != 1:
        q = hip.dev_f32(q, "query rows").reshape(q.shape[0], -1)
    keep += [wx, bx, q, q_idx]
    return hip.STRUCTS["xnrs_personalized_params"](wx.data_ptr(), _addr(bx), q.data_ptr(), q_idx.data_ptr(), wx.shape[0],
                                                   q.stride(0), q.shape[0])


def personalized_head(head, keep):
    if head is None:
        return None
    ts = [hip.dev_f32(head[0].weight, "head weight"), None if head[0].bias is None else hip.dev_f32(head[0].bias, "head bias"),
          hip.dev_f32(head[2].weight, "head weight"), None if head[2].bias is None else hip.dev_f32(head[2].bias, "head bias")]
    keep += ts
    return hip.HeadParams(*[_addr(t) for t in ts], head[0].weight.shape[0], hip.head_activation(head[1]))


class _Personalized(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mods, x, m, ids, q, q_idx, wx, bx, w0, b0, w2, b2):
        from . import ops
        x_fc, head = mods
        with torch.no_grad():
            y, hm, saved = ops.personalized_forward(x, m, ids, q, q_idx, x_fc, head, keep=True)
        ctx.save_for_backward(x, ids, q, q_idx, saved)
        n_seq = ids.numel() if ids is not None else x.shape[0]
        ctx.mods, ctx.n_q, ctx.dims = mods, q.shape[0], (n_seq, x.shape[-2], x.shape[-1], wx.shape[0], y.shape[1])
        ctx.has = [True, m is not None, ids is not None, True, True, True, bx is not None, w0 is not None,
                   b0 is not None, w2 is not None, b2 is not None]
        ctx.mark_non_differentiable(hm)
        return y, hm

    @staticmethod
    def backward(ctx, dy, _dhm):
        x, ids, q, q_idx, saved = ctx.saved_tensors
        x_fc, head = ctx.mods
        n_seq, L, D, A, E = ctx.dims
        wanted = _wanted_inputs(ctx, [False] + ctx.has, 1)
        need = [n and w for n, w in zip(ctx.needs_input_grad[1:], wanted)]  # x m ids q q_idx wx bx w0 b0 w2 b2
        dev = x.device
        dy = hip.dev_f32(dy, "dy")
        x = hip.dev_f32(x, "personalized attention input")  # (what the forward read: no copy for a contiguous input)
        ids = None if ids is None else ids.to(torch.int32).contiguous()
        keep = []
        pp = personalized_params(x_fc, q, q_idx.contiguous(), keep)
        hp = personalized_head(head, keep)
        dx = torch.empty_like(x) if need[0] and ids is None else None
        dq = torch.empty((ctx.n_q, A), dtype=torch.float32, device=dev) if need[3] else None
        dwx = torch.empty_like(x_fc.weight) if need[5] else None
        dbx = torch.empty_like(x_fc.bias) if need[6] else None
        hw = [head[0].weight, head[0].bias, head[2].weight, head[2].bias] if head is not None else [None] * 4
        g = [torch.empty_like(t) if (t is not None and need[7 + i]) else None for i, t in enumerate(hw)]
        gh = hip.HeadGrads(*[_addr(t) for t in g]) if head is not None else None
        l = hip.lib()
        nws = l.xnrs_personalized_bwd_workspace_bytes(n_seq, L, D, A, E, int(head is not None))
        ws = hip.workspace(dev, nws)
        hip.check(l.xnrs_personalized_bwd(hip.ptr(x), hip.ptr(ids), n_seq, L, D, ctypes.byref(pp), hip.ref(hp), hip.ptr(saved),
                                          saved.numel(), hip.ptr(dy), hip.ptr(dx), hip.ptr(dwx), hip.ptr(dbx), hip.ptr(dq),
                                          ctx.n_q, hip.ref(gh), hip.ptr(ws), nws, hip.stream_ptr(dev)), "xnrs_personalized_bwd")
        return (None, dx, None, None, dq, None, dwx, dbx, *g)


def personalized(x, m, ids, q, q_idx, x_fc, head):
    """Differentiable xnrs_personalized_fwd_train / _bwd: -> (y:(n_seq, E), hm:(n_seq))."""
    hw = [None] * 4 if head is None else [head[0].weight, head[0].bias, head[2].weight, head[2].bias]
    return _Personalized.apply((x_fc, head), x, m, ids, q, q_idx, x_fc.weight, x_fc.bias, *hw)


# ---- nn.GRU, one layer (LSTUR's short-term tower, lstur.py:113-154): include/xnrs_hip.h xnrs_gru_*.  One node per call; the
#      mask is not differentiable, the initial state is an input like any other (LSTUR 'ini': the long-term vector).
class _Gru(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, m, h0, w_ih, w_hh, b_ih, b_hh):
        from . import ops
        with torch.no_grad():
            y, xc, saved = ops.gru_forward(x, m, h0, (w_ih, w_hh, b_ih, b_hh), keep=True)
        # the weights go through save_for_backward: an in-place update between forward and backward raises in autograd
        ctx.save_for_backward(xc, saved, w_ih, w_hh, b_ih, b_hh)
        ctx.has = [True, m is not None, h0 is not None, True, True, b_ih is not None, b_hh is not None]
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import ops
        x, saved, *weights = ctx.saved_tensors
        B, T, E = x.shape
        Hd = weights[1].shape[1]
        wanted = _wanted_inputs(ctx, ctx.has, 0)
        need = [n and w for n, w in zip(ctx.needs_input_grad, wanted)]  # x m h0 w_ih w_hh b_ih b_hh
        dev = x.device
        dy = hip.dev_f32(dy, "dy")
        keep = []
        p = ops.gru_params(weights, keep)
        dx = torch.empty_like(x) if need[0] else None
        dh0 = torch.empty((B, Hd), dtype=torch.float32, device=dev) if (ctx.has[2] and need[2]) else None
        g = [torch.empty_like(t) if (t is not None and need[3 + i]) else None for i, t in enumerate(weights)]
        gg = hip.STRUCTS["xnrs_gru_grads"](*[_addr(t) for t in g])
        l = hip.lib()
        nws = l.xnrs_gru_bwd_workspace_bytes(B, T, E, Hd)
        ws = hip.workspace(dev, nws)
        hip.check(l.xnrs_gru_bwd(hip.ptr(x), ctypes.byref(p), hip.ptr(saved), saved.numel(), hip.ptr(dy), hip.ptr(dx), hip.ptr(dh0),
                                 ctypes.byref(gg), B, T, E, hip.ptr(ws), nws, hip.stream_ptr(dev)), "xnrs_gru_bwd")
        return (dx, None, dh0, *g)


def gru(x, m, h0, weights):
    return _Gru.apply(x, m, h0, *weights)


class _EmbeddingRows(torch.autograd.Function):
    """table[ids] of a large table; backward = xnrs_embedding_grad_sparse (one zero fill + one workgroup per id, no atomics),
    with the padding row's ids dropped (nn.Embedding(padding_idx=...): that row never receives a gradient)."""

    @staticmethod
    def forward(ctx, ids, table, padding_idx):
        from . import ops
        ids = ids.reshape(-1).to(torch.int32).contiguous()
        gids = ids if padding_idx is None else torch.where(ids == padding_idx, torch.full_like(ids, -1), ids)
        ctx.save_for_backward(gids)
        ctx.shape = tuple(table.shape)
        with torch.no_grad():
            return ops.embedding_rows_forward(ids, table)

    @staticmethod
    def backward(ctx, dy):
        gids, = ctx.saved_tensors
        dy = hip.dev_f32(dy, "dy")
        n_rows, K = ctx.shape
        d_tab = torch.empty(ctx.shape, dtype=torch.float32, device=dy.device)
        hip.check(hip.lib().xnrs_embedding_grad_sparse(hip.ptr(dy), hip.ptr(gids), gids.numel(), K, hip.ptr(d_tab), n_rows,
                                                       hip.stream_ptr(dy.device)), "xnrs_embedding_grad_sparse")
        return None, d_tab, None


def embedding_rows(idx, table, padding_idx):
    return _EmbeddingRows.apply(idx, table, padding_idx)


# ---- CAUM's candidate-aware user tower (caum.py:31-111): include/xnrs_hip.h xnrs_attn_long_* / xnrs_caum_* / xnrs_act_bwd.
#      One node per stage; torch only routes gradients between them (weight slices and concatenations are data movement).
class _AttnLong(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, n_heads):
        from . import ops
        with torch.no_grad():
            o, qkv_c, saved = ops.attn_long_forward(qkv, n_heads, keep=True)
        ctx.save_for_backward(qkv_c, o, saved)
        ctx.n_heads = int(n_heads)
        return o

    @staticmethod
    def backward(ctx, d_o):
        qkv, o, saved = ctx.saved_tensors
        d_o = hip.dev_f32(d_o, "d_o")
        L, Nb, E3 = qkv.shape
        E = E3 // 3
        dqkv = torch.empty_like(qkv)
        l = hip.lib()
        nws = l.xnrs_attn_long_workspace_bytes(L, Nb, E, ctx.n_heads)
        ws = hip.workspace(qkv.device, nws)
        hip.check(l.xnrs_attn_long_bwd(hip.ptr(qkv), Nb * E3, E3, hip.ptr(o), hip.ptr(d_o), Nb * E, E, hip.ptr(saved), saved.numel(),
                                       hip.ptr(dqkv), L, Nb, E, ctx.n_heads, hip.ptr(ws), nws, hip.stream_ptr(qkv.device)),
                  "xnrs_attn_long_bwd")
        return dqkv, None


def attn_long(qkv, n_heads):
    return _AttnLong.apply(qkv, n_heads)


class _CaumPair(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hp, cp, B, C, H):
        from . import ops
        ctx.dims = (int(B), int(C), int(H), hp.shape[-1] // 4)
        with torch.no_grad():
            return ops.caum_pair_forward(hp, cp, B, C, H)

    @staticmethod
    def backward(ctx, d_hcnn, d_z):
        B, C, H, E = ctx.dims
        dev = d_hcnn.device
        d_hcnn, d_z = hip.dev_f32(d_hcnn, "d h_cnn"), hip.dev_f32(d_z, "d z")
        d_hp = _f32_out((B * H, 4 * E), dev) if ctx.needs_input_grad[0] else None
        d_cp = _f32_out((B * C, 2 * E), dev) if ctx.needs_input_grad[1] else None
        hip.check(hip.lib().xnrs_caum_pair_bwd(hip.ptr(d_hcnn), hip.ptr(d_z), hip.ptr(d_hp), hip.ptr(d_cp), 2 * E, B, C, H, E,
                                               hip.stream_ptr(dev)), "xnrs_caum_pair_bwd")
        return d_hp, d_cp, None, None, None


def caum_pair(hp, cp, B, C, H):
    return _CaumPair.apply(hp, cp, B, C, H)


class _CaumBiasTanh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pre, cb, H):
        from . import ops
        with torch.no_grad():
            t = ops.caum_bias_tanh_forward(pre, cb, H)
        ctx.save_for_backward(t)
        ctx.H = int(H)
        return t

    @staticmethod
    def backward(ctx, dt):
        t, = ctx.saved_tensors
        dt = hip.dev_f32(dt, "dt")
        E = t.shape[-1]
        P = t.numel() // (E * ctx.H)
        dpre = torch.empty_like(t)
        dcb = _f32_out((P, E), t.device) if ctx.needs_input_grad[1] else None
        hip.check(hip.lib().xnrs_caum_bias_tanh_bwd(hip.ptr(t), hip.ptr(dt), hip.ptr(dpre), hip.ptr(dcb), P, ctx.H, E,
                                                    hip.stream_ptr(t.device)), "xnrs_caum_bias_tanh_bwd")
        return dpre, dcb, None


def caum_bias_tanh(pre, cb, H):
    return _CaumBiasTanh.apply(pre, cb, H)


class _CaumPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t2, w3, b3, h_all, H):
        from . import ops
        with torch.no_grad():
            u, a, ts = ops.caum_pool_forward(t2, w3, b3, h_all, H, keep=True)
        ctx.save_for_backward(*ts, a)
        ctx.H, ctx.has_bias = int(H), b3 is not None
        return u

    @staticmethod
    def backward(ctx, du):
        t2, w3, h_all, a = ctx.saved_tensors
        du = hip.dev_f32(du, "du")
        dev = t2.device
        H, A, E = ctx.H, t2.shape[-1], h_all.shape[-1]
        P = a.numel() // H
        need = ctx.needs_input_grad
        d_t2 = torch.empty_like(t2) if need[0] else None
        d_w3 = torch.empty_like(w3) if need[1] else None
        d_b3 = _f32_out((1,), dev) if (ctx.has_bias and need[2]) else None
        d_hall = torch.empty_like(h_all) if need[3] else None
        l = hip.lib()
        nws = l.xnrs_caum_pool_bwd_workspace_bytes(P, H, A)
        ws = hip.workspace(dev, nws)
        hip.check(l.xnrs_caum_pool_bwd(hip.ptr(t2), hip.ptr(w3), hip.ptr(h_all), hip.ptr(a), hip.ptr(du), hip.ptr(d_t2), hip.ptr(d_w3),
                                       hip.ptr(d_b3), hip.ptr(d_hall), P, H, A, E, hip.ptr(ws), nws, hip.stream_ptr(dev)),
                  "xnrs_caum_pool_bwd")
        return d_t2, d_w3, d_b3, d_hall, None


def caum_pool(t2, w3, b3, h_all, H):
    return _CaumPool.apply(t2, w3, b3, h_all, H)
