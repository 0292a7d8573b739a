"""ops.linear -- the one nn.Linear operator of the bridge (dense rows or rows gathered from a table, optional activation in the
GEMM epilogue) -- and its wrappers ops.embedding_linear / ops.embedding_linear_table, forward and autograd, against torch in
fp64 on the CPU: act(F.linear(table[idx] or x, w, b)) and its autograd.

Bars: outputs helpers.assert_close at RTOL (1e-4); dx, dw, db 2e-4 of each tensor's own maximum (DESIGN.md's gradient bar);
d_table the bound of test_hip_grads.py::test_embedding_table_gradient_vs_index_add.

Shapes: M in {1, 130} (one row; a ragged second 128-row tile), K in {16, 18} (vector / buffer loads; the scalar-load fallback
of K % 4 != 0), N in {5, 24}, bias present and absent, every activation; tables of 7 rows (repeated ids, row 3 never referred
to) and of 40 rows (all-distinct ids: one addend per row in both scatter kernels).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from . import helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRAD_TOL = 2e-4
ACTS = {"none": lambda t: t, "relu": torch.relu, "tanh": torch.tanh}
GRID = [(M, K, N) for M in (1, 130) for K in (16, 18) for N in (5, 24)]
TABLES = [("repeats", 1), ("repeats", 130), ("distinct", 40)]


def _act_code(act):
    from xnrs_amd import hip
    return {"none": hip.ACT_NONE, "relu": hip.ACT_RELU, "tanh": hip.ACT_TANH}[act]


def _max_close(got, ref, what, tol=GRAD_TOL):
    got, ref = got.detach().cpu().double(), ref.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.numel() == 0:
        return
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    assert err <= tol * max(scale, 1e-30), f"{what}: max|d| = {err:.3e} > {tol:.1e} * max|ref| = {tol * scale:.3e}"


def _table_close(got, ref, n_ids, what):
    """The bound of test_embedding_table_gradient_vs_index_add."""
    got, ref = got.detach().cpu().double(), ref.detach().double()
    scale = max(ref.abs().max().item(), 1e-6)
    bound = 5e-6 * scale * max(1.0, (n_ids / ref.shape[0]) ** 0.5)
    err = (got - ref).abs().max().item()
    assert err <= bound, f"{what}: max|d| = {err:.3e} > {bound:.3e}"


@functools.lru_cache(maxsize=None)
def _case(M, K, N, bias, act, table=None):
    """Seeded host operands and the fp64 reference (read-only): y; (dx, dw, db) for a random dy and for dy = 1 (y.sum())."""
    g = torch.Generator().manual_seed(7000 + 131 * M + 17 * K + N + (1000 if table else 0))
    n_rows = {None: M, "repeats": 7, "distinct": 40}[table]
    x = torch.randn(n_rows, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) if bias else None
    idx = None
    if table == "repeats":
        idx = torch.randint(0, 7, (M,), generator=g)
        idx[idx == 3] = 4  # row 3 is never referred to
    elif table == "distinct":
        idx = torch.randperm(40, generator=g).reshape(5, 8)
    dy = torch.randn(*((M,) if idx is None else tuple(idx.shape)), N, generator=g)
    refs = {}
    for name, d in (("dy", dy.double()), ("ones", torch.ones_like(dy).double())):
        xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
        br = None if b is None else b.double().requires_grad_(True)
        yr = ACTS[act](F.linear(xr if idx is None else xr[idx], wr, br))
        yr.backward(d)
        refs[name] = (xr.grad, wr.grad, None if br is None else br.grad)
    return dict(x=x, w=w, b=b, idx=idx, dy=dy, y=yr.detach(), refs=refs)


def _leaves(c):
    x, w = c["x"].to(DEV).requires_grad_(True), c["w"].to(DEV).requires_grad_(True)
    b = None if c["b"] is None else c["b"].to(DEV).requires_grad_(True)
    return x, w, b


def _check_op(c, call, what, n_ids=None):
    """One operator `call(x, w, b) -> y` through every way gradients are asked of it.  -> (y, dx, dw, db) of the random-dy pass."""
    is_table = c["idx"] is not None
    close_x = (lambda got, ref, k: _table_close(got, ref, n_ids, k)) if is_table else _max_close
    x, w, b = _leaves(c)
    with torch.no_grad():
        y0 = call(x, w, b)
    assert not y0.requires_grad
    y = call(x, w, b)
    assert y.requires_grad, f"{what}: the output under grad carries no graph"
    assert torch.equal(y, y0), f"{what}: y under grad differs from y under no_grad"
    H.assert_close(y, c["y"], H.RTOL, f"{what} y")
    # (a) everything, a random dy
    y.backward(c["dy"].to(DEV))
    rx, rw, rb = c["refs"]["dy"]
    close_x(x.grad, rx, f"{what} dx")
    _max_close(w.grad, rw, f"{what} dw")
    if b is not None:
        _max_close(b.grad, rb, f"{what} db")
    # ... and dy = 1: everything, (b) the input only, (c) the weight only -- the same bits whatever else the pass computes
    leaves = [x, w] + ([b] if b is not None else [])
    full = torch.autograd.grad(call(x, w, b).sum(), leaves)
    rx, rw, rb = c["refs"]["ones"]
    close_x(full[0], rx, f"{what} dx (dy = 1)")
    _max_close(full[1], rw, f"{what} dw (dy = 1)")
    if b is not None:
        _max_close(full[2], rb, f"{what} db (dy = 1)")
    only_x, = torch.autograd.grad(call(x, w, b).sum(), [x])
    only_w, = torch.autograd.grad(call(x, w, b).sum(), [w])
    assert torch.equal(only_x, full[0]), f"{what}: dx of an input-only pass differs"
    assert torch.equal(only_w, full[1]), f"{what}: dw of a weight-only pass differs"
    return y.detach(), x.grad, w.grad, None if b is None else b.grad


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("M,K,N", GRID)
def test_dense_rows(M, K, N, act):
    from xnrs_amd import ops
    for bias in (True, False):
        c = _case(M, K, N, bias, act)
        _check_op(c, lambda x, w, b: ops.linear(x, w, b, _act_code(act)), f"linear[{M}x{K}->{N} bias={bias} {act}]")


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("K,N", [(K, N) for K in (16, 18) for N in (5, 24)])
@pytest.mark.parametrize("table,M", TABLES)
def test_table_rows(table, M, K, N, act):
    """ops.linear(ids=...) with either table gradient, ops.embedding_linear and (no activation) ops.embedding_linear_table: all
    four against fp64, and the two table gradients against each other -- y, dw, db bit for bit (the same launches), d_table
    bit for bit when every id occurs once (one addend per row in both scatter kernels)."""
    from xnrs_amd import ops
    code = _act_code(act)

    class Mod:  # what ops.embedding_linear unpacks: embedder.weight, fc.weight, fc.bias
        def __init__(self, **kw):
            self.__dict__.update(kw)

    for bias in (True, False):
        c = _case(M, K, N, bias, act, table)
        ids = c["idx"].to(DEV)
        what = f"[{table} {tuple(ids.shape)} ids, {K}->{N} bias={bias} {act}]"
        got = {}
        for tg in ("dense", "sparse"):
            got[tg] = _check_op(c, lambda x, w, b: ops.linear(x, w, b, code, ids=ids, table_grad=tg), f"linear {tg} {what}", ids.numel())
        got["embedding_linear"] = _check_op(c, lambda x, w, b: ops.embedding_linear(ids, Mod(weight=x), Mod(weight=w, bias=b), code),
                                            f"embedding_linear {what}", ids.numel())
        if act == "none":
            got["embedding_linear_table"] = _check_op(c, lambda x, w, b: ops.embedding_linear_table(ids, x, w, b),
                                                      f"embedding_linear_table {what}", ids.numel())
        for name, same_as in (("sparse", "dense"), ("embedding_linear", "dense"), ("embedding_linear_table", "sparse")):
            if name not in got:
                continue
            for i, k in enumerate(("y", "d_table", "dw", "db")):
                if k == "d_table" and name == "sparse" and table != "distinct":
                    continue  # (the two kernels sum an id's occurrences in different orders)
                if got[name][i] is not None:
                    assert torch.equal(got[name][i], got[same_as][i]), f"{name} vs {same_as} {what}: {k} differs"
        assert tuple(got["dense"][0].shape) == tuple(ids.shape) + (N,)
        if table == "repeats":
            for name, g in got.items():
                assert int(torch.count_nonzero(g[1][3]).item()) == 0, f"{name} {what}: the row nobody refers to has a gradient"


def test_dw_over_more_than_one_k_slice():
    """dW = dy^T . x at (M, N, K) = (2100, 24, 16): one 128 x 128 output tile and a contraction of 2100 rows, which
    gemm_pick_splits cuts into 2100 // 256 = 8 slices (at least 256 contraction steps each) whose slabs a second launch sums.
    The workspace query says so: it reserves N * K floats per slice beyond what a one-row backward needs."""
    from xnrs_amd import hip, ops
    M, N, K = 2100, 24, 16
    l = hip.lib()
    slabs = l.xnrs_linear_bwd_workspace_bytes(M, N, K) - l.xnrs_linear_bwd_workspace_bytes(1, N, K)
    assert slabs >= 2 * N * K * 4, "this shape no longer splits the contraction: pick one that does"
    for act in ACTS:
        _check_op(_case(M, K, N, True, act), lambda x, w, b: ops.linear(x, w, b, _act_code(act)), f"linear[{M}x{K}->{N} {act}]")


def test_no_activation_is_the_plain_linear_backward(monkeypatch):
    """Without an activation the node makes no xnrs_act_bwd launch and its gradients are the bits of xnrs_linear_bwd called
    on the same operands; with one, exactly one xnrs_act_bwd launch.  An input-only pass asks the library for no dw / db
    (autograd.SKIP_UNUSED_DW) and gets the same dx."""
    from xnrs_amd import hip, ops
    l = hip.lib()
    calls = {"act": 0, "dw": []}
    act_bwd, lin_bwd = l.xnrs_act_bwd, l.xnrs_linear_bwd

    def count_act(*a):
        calls["act"] += 1
        return act_bwd(*a)

    def spy_linear(*a):
        calls["dw"].append((a[6] is not None, a[7] is not None))
        return lin_bwd(*a)

    monkeypatch.setattr(l, "xnrs_act_bwd", count_act)
    monkeypatch.setattr(l, "xnrs_linear_bwd", spy_linear)
    M, K, N = 130, 18, 24
    c = _case(M, K, N, True, "none")
    x, w, b = _leaves(c)
    dy = c["dy"].to(DEV)
    ops.linear(x, w, b).backward(dy)
    assert calls == {"act": 0, "dw": [(True, True)]}
    dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
    nws = l.xnrs_linear_bwd_workspace_bytes(M, N, K)
    ws = hip.workspace(x.device, nws)
    hip.check(lin_bwd(hip.ptr(x.detach()), None, 0, hip.ptr(w.detach()), hip.ptr(dy), hip.ptr(dx), hip.ptr(dw), hip.ptr(db), M, N, K,
                      hip.ptr(ws), nws, hip.stream_ptr(x.device)), "xnrs_linear_bwd")
    assert torch.equal(x.grad, dx) and torch.equal(w.grad, dw) and torch.equal(b.grad, db)
    ops.linear(x, w, b, hip.ACT_TANH).backward(dy)
    assert calls["act"] == 1
    # (through a non-leaf input: the engine cannot be asked about a leaf that autograd.grad itself captures, and
    # autograd._wanted_inputs then computes everything)
    calls["dw"].clear()
    x0 = x.detach().clone().requires_grad_(True)
    only_x, = torch.autograd.grad(ops.linear(x0 * 1.0, w, b).sum(), [x0])
    assert calls["dw"] == [(False, False)]
    assert torch.equal(only_x, torch.autograd.grad(ops.linear(x0 * 1.0, w, b).sum(), [x0, w, b])[0])


@pytest.mark.parametrize("variant", ["dense", "dense-table", "sparse-table"])
def test_empty_batch(variant):
    """M == 0: the forward returns an empty tensor of the right shape, and dw, db, d_table are exactly zero.  Blocks of the
    gradients' sizes are filled with a non-zero value and handed back to the caching allocator just before the backward, so
    that a gradient buffer the library does not write cannot pass by luck."""
    from xnrs_amd import ops
    K, N, n_rows = 16, 24, 7
    g = torch.Generator().manual_seed(11)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV).requires_grad_(True)
    b = torch.randn(N, generator=g).to(DEV).requires_grad_(True)
    if variant == "dense":
        x = torch.empty(0, K, device=DEV, requires_grad=True)
        y = ops.linear(x, w, b)
    else:
        x = torch.randn(n_rows, K, generator=g).to(DEV).requires_grad_(True)
        ids = torch.empty(0, dtype=torch.int32, device=DEV)
        y = ops.linear(x, w, b, ids=ids, table_grad=variant.split("-")[0])
    assert tuple(y.shape) == (0, N) and y.requires_grad
    dirty = [torch.full(s, 7.0, device=DEV) for s in ((N, K), (N,), (n_rows, K)) for _ in range(4)]
    torch.cuda.synchronize()
    del dirty
    y.sum().backward()
    assert tuple(x.grad.shape) == tuple(x.shape)
    for name, t in (("dw", w.grad), ("db", b.grad), ("dx / d_table", x.grad)):
        assert t is not None and int(torch.count_nonzero(t).item()) == 0, f"{variant}: {name} of an empty batch is not zero"
