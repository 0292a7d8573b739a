"""GPU: the soft-target loss over per-user row lists (include/xnrs_hip.h: xnrs_list_xent_fwd / _bwd, csrc/list_loss.hip)
through ops.list_xent and the raw entry points.

1. parity of loss, lse, slot_scores, d_up and d_table with the fp64 reference of the definition (tests/list_xent_ref.py)
   at the project's bar for three kinds of weights, non-uniform upstream g, every printed MARGIN = observed error / bar;
2. a walk that gives a wave several pieces; 3. one-hot weights are ops.list_loss; 4. exact checks without a tolerance;
5. large scores; 6. every pointer operand off the 16-byte boundary; 7. autograd plumbing; 8. the bilinear scorer;
9. refusals."""
import functools

import pytest
import torch

from tests import test_hip_list_loss as LL
from tests import test_hip_table_loss as TL
from tests.list_xent_ref import list_xent_ref
from xnrs_amd import hip, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, I32 = torch.float32, torch.int32

# (B, n_rows, E, L): the shapes of tests/test_hip_list_loss.py -- one of everything and the scalar-load path; E % 4 != 0;
# E past one 256-float pass and L past one round of the four waves; runs longer than a 64-position piece and duplicate
# slots; two tiles of users.
SHAPES = LL.SHAPES
KINDS = ("soft", "uniform", "raw")
OUTS = ("loss", "lse", "slot_scores", "d_up", "d_table")
bits, pad_of, check = TL.bits, TL.pad_of, TL.check


def slot_weights(kind, table, up, rows, filled, g, zero_user):
    """(B, L) fp32.  'soft': the softmax over the filled slots of the user's own scores, perturbed (a teacher close to the
    student), NaN in the empty slots (they are ignored); 'uniform': 1 / filled slots, garbage in the empty ones; 'raw':
    unnormalised weights in [0, 3) with exact zeros, all 0 for `zero_user`; 'onehot': weight 1 on the first filled slot."""
    B, L = rows.shape
    if kind == "soft":
        s = (table.double()[rows.long().clamp(0, table.shape[0] - 1)] * up.double()[:, None, :]).sum(-1)
        s = s + 0.5 * torch.randn((B, L), generator=g).double()
        w = torch.softmax(s.masked_fill(~filled, float("-inf")), dim=1)
        return torch.where(filled, w, torch.full_like(w, float("nan"))).float()
    if kind == "uniform":
        n = filled.sum(dim=1, keepdim=True).clamp(min=1)
        return torch.where(filled, 1.0 / n.double(), torch.full((B, L), 7.0, dtype=torch.float64)).float()
    if kind == "raw":
        w = torch.rand((B, L), generator=g) * 3.0
        w = torch.where(torch.rand((B, L), generator=g) < 0.3, torch.zeros_like(w), w)
        if zero_user >= 0:
            w[zero_user] = 0.0
        return w
    assert kind == "onehot"
    w = torch.zeros((B, L))
    for b in range(B):
        j = filled[b].nonzero().reshape(-1)
        if j.numel():
            w[b, j[0]] = 1.0
    return w


@functools.lru_cache(maxsize=None)
def case(B, N, E, L, kind="soft", smax=0.0):
    """One problem and its fp64 reference, computed once and shared.  table ~ N(0, 1), up ~ N(0, 1) 2 / sqrt(E), g = rand +
    0.25 per user; the lists of tests/test_hip_list_loss.py::negative_lists (-1 at the head, the middle and the tail, an id
    below -1, one past the table, the pad row) with the user whose list is empty throughout in the middle of the batch; smax
    scales `up` to max|score| ~ smax."""
    g = TL.gen(2000 * B + N + E + L)
    table = torch.randn((N, E), generator=g)
    up = torch.randn((B, E), generator=g) * (2.0 / E ** 0.5)
    if smax:
        up = up * (smax / (up.double() @ table.double().T).abs().max().item())
    pad_row = pad_of(N)
    empty_user = B // 2 if B > 1 else -1
    zero_user = B - 1 if B > 2 else -1
    rows = LL.negative_lists(B, N, L, g, [[] for _ in range(B)], pad_row, empty_user)
    filled = (rows >= 0) & (rows < N) & (rows != pad_row)
    w = slot_weights(kind, table, up, rows, filled, g, zero_user)
    c = dict(B=B, N=N, E=E, L=L, kind=kind, table=table.to(DEV), up=up.to(DEV), rows=rows.to(DEV), w=w.to(DEV), pad_row=pad_row,
             empty_user=empty_user, zero_user=zero_user if kind == "raw" else -1)
    c["g"] = (torch.rand((B,), generator=g) + 0.25).to(DEV)
    c["ref"] = list_xent_ref(c["table"], c["up"], c["rows"], c["w"], pad_row, None, c["g"])
    return c


def run(c, need_table=True, need_up=True, bias=None, g=None):
    """the outputs and the gradients of sum(g * loss) on the device, as a dict"""
    table = c["table"].clone().requires_grad_(need_table)
    up = c["up"].clone().requires_grad_(need_up)
    loss, lse, slot_scores = ops.list_xent(table, up, c["rows"], c["w"], c["pad_row"], bias)
    if need_table or need_up:
        (loss * (c["g"] if g is None else g)).sum().backward()
    return dict(loss=loss.detach(), lse=lse.detach(), slot_scores=slot_scores.detach(), d_up=up.grad, d_table=table.grad)


def check_against_reference(c, what, got=None, grads=True):
    got, r = run(c) if got is None else got, c["ref"]
    filled = r["filled"]
    for k in ("loss", "d_up", "d_table"):
        assert torch.isfinite(got[k]).all(), f"{what} {k}"
    assert torch.equal(torch.isnan(got["slot_scores"]).cpu(), ~filled), f"{what}: NaN exactly in the empty slots"
    if filled.any():
        check(got["slot_scores"].cpu()[filled], r["slot_scores"][filled], f"{what} slot_scores")
    has = torch.isfinite(r["lse"])
    lse = got["lse"].cpu()
    assert torch.equal(torch.isinf(lse) & (lse < 0), ~has), f"{what}: lse is -inf exactly without filled slots"
    if has.any():
        check(lse[has], r["lse"][has], f"{what} lse")
    check(got["loss"], r["loss"], f"{what} loss")
    if grads:
        check(got["d_up"], r["d_up"], f"{what} d_up")
        check(got["d_table"], r["d_table"], f"{what} d_table")
    return got


# ------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,N,E,L", SHAPES)
def test_matches_fp64_reference(B, N, E, L, kind):
    c = case(B, N, E, L, kind)
    check_against_reference(c, f"{(B, N, E, L)} {kind}")
    r = c["ref"]
    if B > 1:
        e = c["empty_user"]
        assert 0 < e < B - 1 and not r["filled"][e].any() and r["filled"].any() and not r["filled"].all()
    if L > N:  # more slots than rows: some user lists a row twice
        rows = c["rows"].cpu()
        assert any(rows[b][r["filled"][b]].unique().numel() < int(r["filled"][b].sum()) for b in range(B))
    if kind == "raw" and B > 2:
        assert (c["w"][c["zero_user"]] == 0).all() and r["filled"][c["zero_user"]].any()
        assert ((c["w"].cpu() == 0) & r["filled"]).any() and (r["loss"] > 0).any()
    if kind == "soft":
        assert torch.isnan(c["w"].cpu()[~r["filled"]]).all()  # the weight of an empty slot is never read into a sum


def test_spans_of_several_pieces_match_fp64_reference():
    """Past 8192 x 64 slots the d_table walk gives a wave more than one 64-position piece (here 70 positions of 520 x 1100
    slots: a full piece and a short one) and carries its running sum from piece to piece; with 300 rows every run of equal
    rows crosses about 27 spans."""
    B, N, E, L = 520, 300, 8, 1100
    assert B * L > 8192 * 64
    c = case(B, N, E, L, "soft")
    got = check_against_reference(c, f"{(B, N, E, L)}")
    again = run(c)
    assert torch.equal(bits(got["d_table"]), bits(again["d_table"]))


def test_user_vectors_past_the_lds_buffer():
    """E = 4100: a user vector longer than the 4096 floats of LDS is read from global memory; seventeen backward passes"""
    check_against_reference(case(3, 50, 4100, 6, "raw"), "E = 4100")


# ------------------------------------------------------------------------------------------- 3. one-hot weights
@pytest.mark.parametrize("B,N,E,L", SHAPES[1:])
def test_one_hot_weights_are_the_list_loss(B, N, E, L):
    """Weight 1 on one filled slot whose row the user lists once, 0 elsewhere: loss = lse - s_t, which is ops.list_loss with
    that row as the user's single target and the same list as negatives (the target's own slot is no negative there, and
    logaddexp(s_t, lse of the others) is the lse of all).  Within the bar, not in bits: the sums are cut differently."""
    c = dict(case(B, N, E, L, "uniform"))
    rows, filled = c["rows"].cpu(), c["ref"]["filled"]
    w = torch.zeros((B, L))
    targets = []
    for b in range(B):
        once = [j for j in filled[b].nonzero().reshape(-1).tolist() if (rows[b] == rows[b, j]).sum() == 1]
        targets.append([int(rows[b, once[len(once) // 2]])] if once else [])
        if once:
            w[b, once[len(once) // 2]] = 1.0
    has = [b for b in range(B) if targets[b]]
    assert len(has) >= B // 2 and len(has) < B
    c["w"] = w.to(DEV)
    got = run(c)
    tgt = TL.csr(targets)
    table, up = c["table"].clone().requires_grad_(True), c["up"].clone().requires_grad_(True)
    loss = ops.list_loss(table, up, *tgt, c["rows"], c["pad_row"])[0]
    (loss * c["g"][has]).sum().backward()
    what = f"one-hot {(B, N, E, L)}"
    check(got["loss"][has], loss.detach(), f"{what} loss")
    check(got["d_up"], up.grad, f"{what} d_up")
    check(got["d_table"], table.grad, f"{what} d_table")
    none = [b for b in range(B) if not targets[b]]
    assert (got["loss"][none] == 0).all() and (got["d_up"][none] == 0).all()


# ------------------------------------------------------------------------------------------- 4. exact
def sub_case(c, b):
    """the problem of user b alone, nothing else changed"""
    s = dict(c)
    s["B"] = 1
    for k in ("up", "rows", "w", "g"):
        s[k] = c[k][b:b + 1].contiguous()
    return s


@pytest.mark.parametrize("B,N,E,L", SHAPES[1:])
def test_every_user_alone_gives_the_bits_it_gets_in_the_batch(B, N, E, L):
    c = case(B, N, E, L, "raw")
    full = run(c, need_table=False)
    for b in range(B):
        one = run(sub_case(c, b), need_table=False)
        for k in ("loss", "lse", "slot_scores", "d_up"):
            assert torch.equal(bits(one[k]), bits(full[k][b:b + 1])), f"{k} of user {b}"


def test_a_second_run_gives_the_same_bits():
    c = case(70, 40, 32, 130, "soft")
    a, b = run(c), run(c)
    for k in OUTS:
        assert torch.equal(bits(a[k]), bits(b[k])), k


@pytest.mark.parametrize("B,N,E,L", SHAPES[1:])
def test_rows_of_d_table_that_nothing_lists_are_zero(B, N, E, L):
    c = case(B, N, E, L, "soft")
    named = torch.zeros(N, dtype=torch.bool)
    for r in c["rows"].cpu().reshape(-1).tolist():
        if 0 <= r < N:
            named[r] = True
    assert N <= 64 or (~named).sum() > 0
    d_table = run(c)["d_table"].cpu()
    assert (d_table[~named] == 0).all() and (d_table[c["pad_row"]] == 0).all()
    assert (d_table[named].abs().sum(dim=1) > 0).any()


@pytest.mark.parametrize("B,N,E,L", SHAPES[1:])
def test_users_without_filled_slots_and_users_with_zero_weights(B, N, E, L):
    c = case(B, N, E, L, "raw")
    got = run(c)
    e, z = c["empty_user"], c["zero_user"]
    assert got["lse"][e].item() == float("-inf") and torch.isnan(got["slot_scores"][e]).all()
    assert torch.isfinite(got["lse"][z]) and not torch.isnan(got["slot_scores"][z]).all()
    for b in (e, z):
        assert got["loss"][b].item() == 0 and (got["d_up"][b] == 0).all()
    for k in ("loss", "d_up", "d_table"):
        assert not torch.isnan(got[k]).any(), k
    # no contribution: whatever their upstream gradient is, every gradient keeps its bits
    g = c["g"].clone()
    g[e], g[z] = 1e6, -1e6
    other = run(c, g=g)
    assert torch.equal(bits(other["d_up"]), bits(got["d_up"])) and torch.equal(bits(other["d_table"]), bits(got["d_table"]))


# ------------------------------------------------------------------------------------------- 5. large scores
@pytest.mark.parametrize("kind", KINDS)
def test_scores_up_to_30_stay_within_the_bar(kind):
    c = case(5, 300, 260, 65, kind, smax=30.0)
    assert 25 < (c["up"].double() @ c["table"].double().T).abs().max().item() < 35
    check_against_reference(c, f"max|s| ~ 30 {kind}")


@pytest.mark.parametrize("kind", ["uniform", "onehot"])
def test_scores_up_to_300_stay_within_the_bar(kind):
    c = case(5, 300, 260, 65, kind, smax=300.0)
    assert 250 < (c["up"].double() @ c["table"].double().T).abs().max().item() < 350
    check_against_reference(c, f"max|s| ~ 300 {kind}")


def test_scores_up_to_300_with_softmax_weights_stay_finite():
    """W p - w is then a difference of nearly equal numbers (the weights ARE the softmax of almost these scores): an fp32
    evaluation of the definition itself misses the bar on the gradients there.  Everything is finite, the loss at the bar."""
    c = case(5, 300, 260, 65, "soft", smax=300.0)
    got = check_against_reference(c, "max|s| ~ 300 soft", grads=False)
    assert torch.isfinite(got["d_up"]).all() and torch.isfinite(got["d_table"]).all()


# ------------------------------------------------------------------------------------------- 6. operand alignment
ALIGN_SHAPE = (5, 300, 260, 65)
ALIGN_INS = ("table", "up", "bias", "rows", "weights", "g", "order")
ALIGN_OUTS = ("loss", "lse", "slot_scores", "d_up", "d_table")


@functools.lru_cache(maxsize=None)
def align_family():
    """xnrs_list_xent_fwd + _bwd on one problem in the case style of tests/test_hip_pointer_alignment.py: every pointer
    operand is a guarded view (tests/align_ref.py) at a chosen offset from a 16-byte boundary."""
    from tests import test_hip_pointer_alignment as PA
    B, N, E, L = ALIGN_SHAPE
    c = case(B, N, E, L, "raw")
    bias = torch.tensor([0.75])
    r = list_xent_ref(c["table"], c["up"], c["rows"], c["w"], c["pad_row"], bias, c["g"])
    key = torch.where(r["filled"].reshape(-1), c["rows"].cpu().reshape(-1).long(), N)
    order = torch.sort(key, stable=True).indices.to(I32)

    def call(o):
        l = hip.lib()
        nws = l.xnrs_list_xent_workspace_bytes(B, L, E, 1)
        ws = hip.workspace(DEV, nws)
        head = (hip.ptr(o["table"]), N, E, hip.ptr(o["up"]), hip.ptr(o["bias"]), B, hip.ptr(o["rows"]), hip.ptr(o["weights"]), L,
                c["pad_row"])
        rc = l.xnrs_list_xent_fwd(*head, hip.ptr(o["loss"]), hip.ptr(o["lse"]), hip.ptr(o["slot_scores"]), hip.ptr(ws), nws,
                                  PA.stream())
        if rc:
            return rc
        return l.xnrs_list_xent_bwd(*head, hip.ptr(o["lse"]), hip.ptr(o["slot_scores"]), hip.ptr(o["g"]), hip.ptr(o["order"]),
                                    hip.ptr(o["d_up"]), hip.ptr(o["d_table"]), hip.ptr(ws), nws, PA.stream())
    ins = dict(table=c["table"].cpu(), up=c["up"].cpu(), bias=bias, rows=c["rows"].cpu(), weights=c["w"].cpu(), g=c["g"].cpu(),
               order=order)
    outs = dict(loss=((B,), F32), lse=((B,), F32), slot_scores=((B, L), F32), d_up=((B, E), F32), d_table=((N, E), F32))
    assert tuple(ins) == ALIGN_INS and tuple(outs) == ALIGN_OUTS
    return PA, PA.Family(ins, outs, call, {k: r[k] for k in outs}, bitwise=tuple(outs))


@functools.lru_cache(maxsize=None)
def align_base():
    PA, fam = align_family()
    return PA.run_case(fam, {})


@pytest.mark.parametrize("case_", ["aligned"] + [f"{k}+4" for k in ALIGN_INS + ALIGN_OUTS] + ["table+8", "d_table+12", "all"])
def test_operand_off_a_16_byte_boundary(case_):
    """Every pointer operand of both entry points shifted by one element (and all at once) gives the results of the aligned
    call -- the same bits -- and leaves the guards around every operand intact."""
    PA, fam = align_family()
    base, _ = align_base()
    if case_ == "aligned":
        shifts = {}
    elif case_ == "all":
        shifts = {k: 4 for k in ALIGN_INS + ALIGN_OUTS}
    else:
        k, n = case_.split("+")
        shifts = {k: int(n)}
    got = PA.run_case(fam, shifts)[0] if shifts else base
    PA.check_case(fam, "list_xent", case_, got, base)


# ------------------------------------------------------------------------------------------- 7. autograd
def test_gradients_that_nobody_asks_for_are_not_computed(monkeypatch):
    c = case(70, 40, 32, 130, "soft")
    asked, sorted_orders = [], []
    real, real_order = ops.list_xent_backward, ops.list_xent_order

    def spy(*a, **k):
        asked.append((k["want_d_up"], k["want_d_table"]))
        return real(*a, **k)

    def order_spy(*a, **k):
        sorted_orders.append(1)
        return real_order(*a, **k)

    monkeypatch.setattr(ops, "list_xent_backward", spy)
    monkeypatch.setattr(ops, "list_xent_order", order_spy)
    full = run(c)
    assert asked[-1] == (True, True) and len(sorted_orders) == 1
    got = run(c, need_table=False)  # a detached table: no d_table, None for it, no order sorted
    assert got["d_table"] is None and asked[-1] == (True, False) and torch.equal(bits(got["d_up"]), bits(full["d_up"]))
    assert len(sorted_orders) == 1
    got = run(c, need_up=False)
    assert got["d_up"] is None and asked[-1] == (False, True) and torch.equal(bits(got["d_table"]), bits(full["d_table"]))
    table, up = c["table"].clone().requires_grad_(True), c["up"].clone().requires_grad_(True)
    w = c["w"].clone().requires_grad_(True)
    loss, lse, slot_scores = ops.list_xent(table, up, c["rows"], w, c["pad_row"])
    assert loss.requires_grad and not lse.requires_grad and not slot_scores.requires_grad
    (du,) = torch.autograd.grad((loss * c["g"]).sum(), [up])
    assert asked[-1] == (True, False) and table.grad is None and w.grad is None and torch.equal(bits(du), bits(full["d_up"]))
    n = len(asked)
    with torch.no_grad():
        l2 = ops.list_xent(table, up, c["rows"], c["w"], c["pad_row"])[0]
    assert not l2.requires_grad and torch.equal(bits(l2), bits(full["loss"])) and len(asked) == n


def test_what_the_autograd_node_saves():
    """table, up, lse and the slot scores: nothing of the size of the listed rows (B, L, E)"""
    c = case(70, 40, 32, 130, "soft")
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(tuple(t.shape)) or t, lambda t: t):
        ops.list_xent(c["table"].clone().requires_grad_(True), c["up"].clone().requires_grad_(True), c["rows"], c["w"], c["pad_row"])
    assert sorted(saved) == sorted([(40, 32), (70, 32), (70,), (70, 130)])


# ------------------------------------------------------------------------------------------- 8. the scorers
@pytest.mark.parametrize("B,N,E,L", [(70, 40, 32, 130), (5, 300, 260, 65)])
def test_bilinear_scorer(B, N, E, L):
    from xnrs_amd.models.blocks import BilinScoring
    c = case(B, N, E, L, "soft")
    torch.manual_seed(5)
    sc = BilinScoring(E).to(DEV)
    with torch.no_grad():
        sc.bilin.weight.mul_(E ** 0.5 * 0.5)
        sc.bilin.bias.fill_(0.75)
    table = c["table"].clone().requires_grad_(True)
    u = c["up"].clone().reshape(B, 1, E).requires_grad_(True)
    loss, lse, slot_scores = sc.list_xent(table, u, c["rows"], c["w"], c["pad_row"])
    (loss * c["g"]).sum().backward()
    # the reference: the same definition on v = u W[0] in fp64, autograd down to u, W and the table
    W = sc.bilin.weight.detach().double().cpu().requires_grad_(True)
    u64 = c["up"].double().cpu().requires_grad_(True)
    v = u64 @ W[0]
    r = list_xent_ref(c["table"], v, c["rows"], c["w"], c["pad_row"], sc.bilin.bias, c["g"])
    d_u, d_W = torch.autograd.grad(v, [u64, W], grad_outputs=r["d_up"])
    what = f"bilinear {(B, N, E, L)}"
    check(loss, r["loss"], f"{what} loss")
    check(slot_scores.cpu()[r["filled"]], r["slot_scores"][r["filled"]], f"{what} slot_scores")
    check(u.grad.reshape(B, E), d_u, f"{what} d_u")
    check(sc.bilin.weight.grad, d_W, f"{what} d_W")
    check(table.grad, r["d_table"], f"{what} d_table")
    assert sc.bilin.bias.grad is None
    with pytest.raises(NotImplementedError, match="normalize=True"):
        BilinScoring(E, normalize=True).to(DEV).list_xent(table, u, c["rows"], c["w"], c["pad_row"])


def test_dot_scorer_is_ops_list_xent():
    from xnrs_amd.models.blocks import DotScoring
    c = case(70, 40, 32, 130, "soft")
    got = DotScoring().list_xent(c["table"], c["up"].reshape(70, 1, 32), c["rows"], c["w"], c["pad_row"])
    want = run(c, False, False)
    assert torch.equal(bits(got[0]), bits(want["loss"])) and torch.equal(bits(got[1]), bits(want["lse"]))
    with pytest.raises(NotImplementedError, match="normalize=True"):
        DotScoring(normalize=True).list_xent(c["table"], c["up"], c["rows"], c["w"], c["pad_row"])


def test_listed_soft_target_loss_reductions():
    from xnrs_amd import losses
    from xnrs_amd.models.blocks import DotScoring, FCScoring
    c = case(70, 40, 32, 130, "soft")
    per_user = run(c, False, False)
    args = (DotScoring(), c["table"], c["up"], c["rows"], c["w"], c["pad_row"])
    none = losses.listed_soft_target_loss(*args, reduction="none")
    assert torch.equal(bits(none), bits(per_user["loss"]))
    n = int(torch.isfinite(per_user["lse"]).sum())
    assert n == 69  # (the user in the middle has no filled slot and does not count)
    check(losses.listed_soft_target_loss(*args, reduction="sum"), c["ref"]["loss"].sum(), "sum")
    check(losses.listed_soft_target_loss(*args), c["ref"]["loss"].sum() / n, "mean")
    with pytest.raises(NotImplementedError, match="FCScoring"):
        losses.listed_soft_target_loss(FCScoring(32, 8), *args[1:])
    with pytest.raises(ValueError, match="reduction"):
        losses.listed_soft_target_loss(*args, reduction="max")


# ------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_write_nothing():
    c = case(70, 40, 32, 130, "soft")
    B, N, E, L = 70, 40, 32, 130
    l = hip.lib()
    EINVAL, EWORKSPACE = hip._CONSTANTS["EINVAL"], hip._CONSTANTS["EWORKSPACE"]
    ok = run(c, False, False)
    need = l.xnrs_list_xent_workspace_bytes(B, L, E, 1)
    assert need > 0 and l.xnrs_list_xent_workspace_bytes(B, L, E, 0) == 0
    assert l.xnrs_list_xent_workspace_bytes(4096, 128, 256, 1) <= 4096 * 128 * 256 * 4 // 16  # never the (B, L, E) copy
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    st = hip.stream_ptr(torch.device(DEV))
    p = hip.ptr

    def fwd(table=c["table"], up=c["up"], rows=c["rows"], w=c["w"], L_=L, E_=E, skip=None):
        out = dict(loss=torch.full((B,), 7.0, device=DEV), lse=torch.full((B,), 7.0, device=DEV),
                   slot_scores=torch.full((B, L), 7.0, device=DEV))
        a = {k: (None if k == skip else p(t)) for k, t in out.items()}
        rc = l.xnrs_list_xent_fwd(p(table), N, E_, p(up), None, B, p(rows), p(w), L_, c["pad_row"], a["loss"], a["lse"],
                                  a["slot_scores"], None, 0, st)
        torch.cuda.synchronize()
        return rc, out

    rc, out = fwd()
    assert rc == 0 and all(torch.equal(bits(out[k]), bits(ok[k])) for k in out)
    for bad in (dict(L_=-1), dict(E_=0), dict(table=None), dict(up=None), dict(rows=None), dict(w=None), dict(skip="loss"),
                dict(skip="lse"), dict(skip="slot_scores")):
        rc, out = fwd(**bad)
        assert rc == EINVAL and all((t == 7.0).all() for t in out.values()), bad

    order = ops.list_xent_order(N, c["rows"], ok["slot_scores"])

    def bwd(order_=order, d_table="out", g=c["g"], lse=ok["lse"], ws_=ws, nbytes=need, L_=L, E_=E):
        d_up, d_tab = torch.full_like(c["up"], 7.0), torch.full_like(c["table"], 7.0)
        rc = l.xnrs_list_xent_bwd(p(c["table"]), N, E_, p(c["up"]), None, B, p(c["rows"]), p(c["w"]), L_, c["pad_row"], p(lse),
                                  p(ok["slot_scores"]), p(g), p(order_), p(d_up), p(d_tab) if d_table == "out" else None,
                                  p(ws_), nbytes, st)
        torch.cuda.synchronize()
        return rc, d_up, d_tab

    rc, d_up, d_tab = bwd()
    full = run(c)
    assert rc == 0 and torch.equal(bits(d_up), bits(full["d_up"])) and torch.equal(bits(d_tab), bits(full["d_table"]))
    for bad, want in ((dict(order_=None), EINVAL), (dict(d_table=None), EINVAL), (dict(g=None), EINVAL), (dict(lse=None), EINVAL),
                      (dict(L_=-1), EINVAL), (dict(E_=0), EINVAL), (dict(nbytes=need - 1), EWORKSPACE),
                      (dict(ws_=None), EWORKSPACE)):
        rc, d_up, d_tab = bwd(**bad)
        assert rc == want and (d_up == 7.0).all() and (d_tab == 7.0).all(), bad
    rc, d_up, d_tab = bwd(order_=None, d_table=None, ws_=None, nbytes=0)  # d_up alone needs neither an order nor a workspace
    assert rc == 0 and torch.equal(bits(d_up), bits(full["d_up"])) and (d_tab == 7.0).all()
    # an order with values outside [0, B L): skipped, never dereferenced (the gradients of the rows concerned are unspecified)
    wild = order.clone()
    wild[::7] = 2 ** 31 - 1
    wild[3::7] = -5
    rc, d_up, d_tab = bwd(order_=wild)
    assert rc == 0 and torch.isfinite(d_tab).all()
    # B == 0: XNRS_OK, nothing to write; L == 0: every user is without a filled slot
    out = ops.list_xent(c["table"], torch.zeros((0, E), device=DEV), torch.zeros((0, L), dtype=I32, device=DEV),
                        torch.zeros((0, L), device=DEV))
    assert all(t.numel() == 0 for t in out)
    up = c["up"].clone().requires_grad_(True)
    loss, lse, ss = ops.list_xent(c["table"], up, torch.zeros((B, 0), dtype=I32, device=DEV), torch.zeros((B, 0), device=DEV))
    loss.sum().backward()
    assert (loss == 0).all() and (lse == float("-inf")).all() and ss.numel() == 0 and (up.grad == 0).all()
