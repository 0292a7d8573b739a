"""GPU: the softmax ranking loss over per-user row lists (include/xnrs_hip.h: xnrs_list_loss_fwd / _bwd, csrc/list_loss.hip)
through ops.list_loss and the raw entry points.

1. parity of scores, neg_scores, lse, loss, d_up and d_table with the fp64 reference of the definition
   (tests/list_loss_ref.py) at the project's bar, non-uniform upstream g, every printed MARGIN = observed error / bar;
2. exact checks without a tolerance: every user alone, run-to-run bits, unlisted d_table rows, users without negatives,
   queries without an answer;
3. the list of ALL rows is the full-table loss (tests/table_loss_ref.py); 4. large scores; 5. autograd plumbing and the
   bilinear scorer; 6. every pointer operand off the 16-byte boundary; 7. refusals."""
import functools

import pytest
import torch

from tests import helpers as H
from tests import test_hip_table_loss as TL
from tests.list_loss_ref import list_loss_ref
from tests.table_loss_ref import table_loss_ref
from xnrs_amd import hip, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, I32 = torch.float32, torch.int32

# (B, n_rows, E, L), the smallest shapes that reach each edge: one of everything; the scalar-load path (E % 4 != 0); E past
# one 256-float pass of a wave and L past one 64-slot round of the four waves; a 40-row table listed by 70 users -- every run
# of equal rows is longer than a 64-position piece and L > n_rows forces duplicate slots; the LSTUR width over two tiles of
# users.
SHAPES = [(1, 1, 4, 1), (3, 127, 37, 5), (5, 300, 260, 65), (70, 40, 32, 130), (130, 1153, 272, 16)]
OUTS = ("loss", "scores", "lse", "neg_scores", "d_up", "d_table")
bits, csr, pad_of, check = TL.bits, TL.csr, TL.pad_of, TL.check


def negative_lists(B, N, L, g, targets, pad_row, empty_user):
    """Per user L slots of real rows (drawn with replacement: duplicates) with, where the list has room, -1 fillers at the
    head, in the middle and at the tail, an id below -1, one past the table, the pad row and the user's own first target;
    a short list (L < 16) takes two of those per user, by turns.  `empty_user`: a list that is empty throughout."""
    rows = torch.randint(0, N, (B, L), generator=g).to(I32)
    for b in range(B):
        own = next((t for t in targets[b] if 0 <= t < N), -1)
        special = [(0, -1), (L // 2, -1), (L - 1, -1), (1, -7), (2, N + 3), (3, pad_row), (4, own)]
        if b == empty_user:
            for j in range(L):
                rows[b, j] = special[j % 7][1] if special[j % 7][1] != own else -1
        elif L >= 16:
            for j, r in special:
                rows[b, j] = r
        elif L >= 5:
            for j, r in (special[b % 7], special[(b + 3) % 7]):
                rows[b, j % L] = r
    return rows


@functools.lru_cache(maxsize=None)
def case(B, N, E, L, smax=0.0):
    """One problem and its fp64 reference, computed once and shared.  The inputs are those of tests/test_hip_table_loss.py:
    table ~ N(0, 1), up ~ N(0, 1) 2 / sqrt(E), g = rand + 0.25, its target lists; smax scales `up` to max|score| ~ smax."""
    g = TL.gen(1000 * B + N + E + L)
    table = torch.randn((N, E), generator=g)
    up = torch.randn((B, E), generator=g) * (2.0 / E ** 0.5)
    if smax:
        up = up * (smax / (up.double() @ table.double().T).abs().max().item())
    targets = TL.target_lists(B, N, g)
    pad_row = pad_of(N)
    answerable = lambda b: [t for t in targets[b] if 0 <= t < N and t != pad_row]  # noqa: E731
    with_answer = [b for b in range(B) if answerable(b)]
    # the user whose list is empty throughout sits in the MIDDLE of the batch, and the next user that has clicks (and
    # negatives) clicks the same row: in the sorted order the empty user's query lies inside the run of that row, between
    # entries that carry a gradient
    empty_user = with_answer[len(with_answer) // 2] if B > 1 else -1
    if B > 1:
        later = with_answer[len(with_answer) // 2 + 1]
        targets[later][0] = answerable(empty_user)[0]
    neg = negative_lists(B, N, L, g, targets, pad_row, empty_user)
    c = dict(B=B, N=N, E=E, L=L, table=table.to(DEV), up=up.to(DEV), targets=targets, pad_row=pad_row, neg=neg.to(DEV),
             empty_user=empty_user, tgt=csr(targets))
    T = c["tgt"][1].numel()
    c["g"] = (torch.rand((T,), generator=g) + 0.25).to(DEV)
    c["ref"] = list_loss_ref(c["table"], c["up"], *c["tgt"], c["neg"], pad_row, None, c["g"])
    return c


def run(c, need_table=True, need_up=True, bias=None, g=None):
    """the outputs and the gradients of sum(g * loss) on the device, as a dict"""
    table = c["table"].clone().requires_grad_(need_table)
    up = c["up"].clone().requires_grad_(need_up)
    loss, scores, lse, neg_scores = ops.list_loss(table, up, *c["tgt"], c["neg"], c["pad_row"], bias)
    if need_table or need_up:
        (loss * (c["g"] if g is None else g)).sum().backward()
    return dict(loss=loss.detach(), scores=scores.detach(), lse=lse.detach(), neg_scores=neg_scores.detach(), d_up=up.grad,
                d_table=table.grad)


def check_against_reference(c, what, got=None, r=None):
    got, r = run(c) if got is None else got, c["ref"] if r is None else r
    valid, filled = r["valid"], r["filled"]
    for k in ("loss", "d_up", "d_table"):
        assert torch.isfinite(got[k]).all(), f"{what} {k}"
    assert torch.equal(torch.isnan(got["scores"]).cpu(), ~valid), f"{what}: NaN exactly where a query has no answer"
    assert torch.equal(torch.isnan(got["neg_scores"]).cpu(), ~filled), f"{what}: NaN exactly in the empty slots"
    assert (got["loss"].cpu()[~valid] == 0).all()
    if valid.any():
        check(got["scores"].cpu()[valid], r["scores"][valid], f"{what} scores")
    if filled.any():
        check(got["neg_scores"].cpu()[filled], r["neg_scores"][filled], f"{what} neg_scores")
    has = torch.isfinite(r["lse"])
    lse = got["lse"].cpu()
    assert torch.equal(torch.isinf(lse) & (lse < 0), ~has), f"{what}: lse is -inf exactly without negatives"
    if has.any():
        check(lse[has], r["lse"][has], f"{what} lse")
    check(got["loss"], r["loss"], f"{what} loss")
    check(got["d_up"], r["d_up"], f"{what} d_up")
    check(got["d_table"], r["d_table"], f"{what} d_table")
    return got


# ------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("B,N,E,L", SHAPES)
def test_matches_fp64_reference(B, N, E, L):
    c = case(B, N, E, L)
    check_against_reference(c, f"{(B, N, E, L)}")
    r = c["ref"]
    if B > 1:
        assert r["valid"].any() and not r["valid"].all() and r["filled"].any() and not r["filled"].all()
        e = c["empty_user"]
        assert not r["filled"][e].any() and torch.isfinite(r["lse"]).any()
        shared = [b for b in range(e + 1, B) if r["filled"][b].any() and set(c["targets"][b]) & set(c["targets"][e])]
        assert 0 < e < B - 1 and shared, "a later user with negatives clicks a row of the user without negatives"
    if L > N:  # more slots than rows: some user lists a row twice
        rows = c["neg"].cpu()
        assert any(rows[b][r["filled"][b]].unique().numel() < int(r["filled"][b].sum()) for b in range(B))


def test_spans_of_several_pieces_match_fp64_reference():
    """Past 8192 x 64 entries the d_table walk gives a wave more than one 64-position piece (here 70 positions of 520 x 1101
    entries: a full piece and a short one) and carries its running sum from piece to piece; with 300 rows every run of equal
    rows crosses about 27 spans.  The smallest shape on the far side of that threshold, at a narrow E."""
    B, N, E, L = 520, 300, 8, 1100
    assert B * (L + 1) > 8192 * 64
    c = case(B, N, E, L)
    got = check_against_reference(c, f"{(B, N, E, L)}")
    again = run(c)
    assert torch.equal(bits(got["d_table"]), bits(again["d_table"]))


def test_a_query_of_a_user_without_negatives_inside_a_run_of_its_row():
    """Row 5 is listed by user 3 and clicked by users 0, 1 and 2; user 1 lists fillers only.  Sorted by row, the entries of row 5
    are [slot of user 3, query of user 0, query of user 1 (no gradient), query of user 2]: d_table[5] is the sum over ALL of
    them, the query in the middle adds exactly 0 and cuts nothing off."""
    N, E = 9, 8
    g = TL.gen(77)
    c = dict(B=4, N=N, E=E, L=3, table=torch.randn((N, E), generator=g).to(DEV), up=torch.randn((4, E), generator=g).to(DEV),
             targets=[[5], [5], [5, 2], [7]], pad_row=-1, empty_user=1)
    c["neg"] = torch.tensor([[1, 2, 3], [-1, -1, -1], [4, 6, -1], [5, 0, 5]], dtype=I32, device=DEV)
    c["tgt"] = csr(c["targets"])
    c["g"] = (torch.rand((5,), generator=g) + 0.25).to(DEV)
    c["ref"] = list_loss_ref(c["table"], c["up"], *c["tgt"], c["neg"], -1, None, c["g"])
    got = check_against_reference(c, "no-negatives query inside a run")
    assert (got["d_up"][1] == 0).all() and got["loss"][1].item() == 0 and got["lse"][1].item() == float("-inf")
    # the same with the user's upstream gradient changed: it contributes nothing, to no row
    g2 = c["g"].clone()
    g2[1] = 1e6
    other = run(c, g=g2)
    assert torch.equal(bits(other["d_table"]), bits(got["d_table"])) and torch.equal(bits(other["d_up"]), bits(got["d_up"]))


def test_user_vectors_past_the_lds_buffer():
    """E = 4100: the forward keeps a user vector in LDS up to 4096 floats and reads a longer one from global memory; the
    backward makes seventeen 256-feature passes"""
    check_against_reference(case(3, 50, 4100, 6), "E = 4100")


# ------------------------------------------------------------------------------------------- 2. exact
def sub_case(c, b):
    """the problem of user b alone, nothing else changed"""
    off = c["tgt"][0].tolist()
    s = dict(c)
    s["B"], s["up"], s["neg"] = 1, c["up"][b:b + 1].contiguous(), c["neg"][b:b + 1].contiguous()
    s["tgt"], s["g"] = csr([c["targets"][b]]), c["g"][off[b]:off[b + 1]].contiguous()
    return s


@pytest.mark.parametrize("B,N,E,L", SHAPES[1:])
def test_every_user_alone_gives_the_bits_it_gets_in_the_batch(B, N, E, L):
    c = case(B, N, E, L)
    full = run(c, need_table=False)
    off = c["tgt"][0].tolist()
    for b in range(B):
        one = run(sub_case(c, b), need_table=False)
        for k in ("loss", "scores"):
            assert torch.equal(bits(one[k]), bits(full[k][off[b]:off[b + 1]])), f"{k} of user {b}"
        for k in ("lse", "neg_scores", "d_up"):
            assert torch.equal(bits(one[k]), bits(full[k][b:b + 1])), f"{k} of user {b}"


def test_a_second_run_gives_the_same_bits():
    c = case(70, 40, 32, 130)
    a, b = run(c), run(c)
    for k in OUTS:
        assert torch.equal(bits(a[k]), bits(b[k])), k


@pytest.mark.parametrize("B,N,E,L", SHAPES[1:])
def test_rows_of_d_table_that_nothing_lists_are_zero(B, N, E, L):
    c = case(B, N, E, L)
    named = torch.zeros(N, dtype=torch.bool)
    for r in c["neg"].cpu().reshape(-1).tolist() + c["tgt"][1].cpu().tolist():
        if 0 <= r < N:
            named[r] = True
    assert N <= 64 or (~named).sum() > 0
    d_table = run(c)["d_table"].cpu()
    assert (d_table[~named] == 0).all() and (d_table[c["pad_row"]] == 0).all()
    assert (d_table[named].abs().sum(dim=1) > 0).any()


@pytest.mark.parametrize("B,N,E,L", SHAPES)
def test_users_without_negatives_and_queries_without_an_answer(B, N, E, L):
    c = case(B, N, E, L)
    got = run(c)
    off, r = c["tgt"][0].tolist(), c["ref"]
    none = [b for b in range(B) if not r["filled"][b].any()]
    assert none and (B == 1 or c["empty_user"] in none)
    for b in none:
        assert got["lse"][b].item() == float("-inf")
        assert (got["loss"][off[b]:off[b + 1]] == 0).all() and (got["d_up"][b] == 0).all()
    for k in OUTS:
        if k not in ("scores", "neg_scores"):
            assert not torch.isnan(got[k]).any(), k
    rows = c["tgt"][1].cpu()
    no_answer = (rows < 0) | (rows >= N) | (rows == c["pad_row"])
    assert torch.equal(torch.isnan(got["scores"]).cpu(), no_answer) and (got["loss"].cpu()[no_answer] == 0).all()
    if no_answer.any():  # no contribution: whatever their upstream gradient is, every gradient keeps its bits
        g = torch.where(no_answer.to(DEV), torch.full_like(c["g"], 1e6), c["g"])
        other = run(c, g=g)
        assert torch.equal(bits(other["d_up"]), bits(got["d_up"])) and torch.equal(bits(other["d_table"]), bits(got["d_table"]))
    else:
        assert B == 1


# ------------------------------------------------------------------------------------------- 3. every row listed
@pytest.mark.parametrize("B,N,E", [(5, 300, 260), (70, 40, 32)])
def test_the_list_of_all_rows_is_the_full_table_loss(B, N, E):
    c = dict(case(B, N, E, {300: 65, 40: 130}[N]))
    c["neg"] = torch.arange(N, dtype=I32, device=DEV).repeat(B, 1).contiguous()
    r = table_loss_ref(c["table"], c["up"], *c["tgt"], None, None, c["pad_row"], None, None, None, c["g"])
    got = run(c)
    what = f"all rows {(B, N, E)}"
    assert torch.equal(torch.isnan(got["scores"]).cpu(), ~r["valid"])
    check(got["scores"].cpu()[r["valid"]], r["scores"][r["valid"]], f"{what} scores")
    check(got["lse"], r["lse"], f"{what} lse")
    check(got["loss"], r["loss"], f"{what} loss")
    check(got["d_up"], r["d_up"], f"{what} d_up")
    check(got["d_table"], r["d_table"], f"{what} d_table")


# ------------------------------------------------------------------------------------------- 4. large scores
def test_large_scores_stay_finite_and_within_the_bar():
    c = case(5, 300, 260, 65, smax=300.0)
    assert 250 < (c["up"].double() @ c["table"].double().T).abs().max().item() < 350
    check_against_reference(c, "max|s| ~ 300")


# ------------------------------------------------------------------------------------------- 5. autograd, the scorers
def test_gradients_that_nobody_asks_for_are_not_computed(monkeypatch):
    c = case(70, 40, 32, 130)
    asked = []
    real = ops.list_loss_backward

    def spy(*a, **k):
        asked.append((k["want_d_up"], k["want_d_table"]))
        return real(*a, **k)

    monkeypatch.setattr(ops, "list_loss_backward", spy)
    full = run(c)
    assert asked[-1] == (True, True)
    got = run(c, need_table=False)  # a detached table: no d_table, None for it
    assert got["d_table"] is None and asked[-1] == (True, False) and torch.equal(bits(got["d_up"]), bits(full["d_up"]))
    got = run(c, need_up=False)
    assert got["d_up"] is None and asked[-1] == (False, True) and torch.equal(bits(got["d_table"]), bits(full["d_table"]))
    table, up = c["table"].clone().requires_grad_(True), c["up"].clone().requires_grad_(True)
    loss, scores, lse, neg_scores = ops.list_loss(table, up, *c["tgt"], c["neg"], c["pad_row"])
    assert loss.requires_grad and not scores.requires_grad and not lse.requires_grad and not neg_scores.requires_grad
    (du,) = torch.autograd.grad((loss * c["g"]).sum(), [up])
    assert asked[-1] == (True, False) and table.grad is None and torch.equal(bits(du), bits(full["d_up"]))
    with torch.no_grad():
        l2 = ops.list_loss(table, up, *c["tgt"], c["neg"], c["pad_row"])[0]
    assert not l2.requires_grad and torch.equal(bits(l2), bits(full["loss"]))


@pytest.mark.parametrize("B,N,E,L", [(70, 40, 32, 130), (5, 300, 260, 65)])
def test_bilinear_scorer(B, N, E, L):
    from xnrs_amd.models.blocks import BilinScoring
    c = case(B, N, E, L)
    torch.manual_seed(5)
    sc = BilinScoring(E).to(DEV)
    with torch.no_grad():
        sc.bilin.weight.mul_(E ** 0.5 * 0.5)
        sc.bilin.bias.fill_(0.75)
    table = c["table"].clone().requires_grad_(True)
    u = c["up"].clone().reshape(B, 1, E).requires_grad_(True)
    loss, scores, lse, neg_scores = sc.list_loss(table, u, *c["tgt"], c["neg"], c["pad_row"])
    (loss * c["g"]).sum().backward()
    # the reference: the same definition on v = u W[0] in fp64, autograd down to u, W and the table
    W = sc.bilin.weight.detach().double().cpu().requires_grad_(True)
    u64 = c["up"].double().cpu().requires_grad_(True)
    v = u64 @ W[0]
    r = list_loss_ref(c["table"], v, *c["tgt"], c["neg"], c["pad_row"], sc.bilin.bias, c["g"])
    d_u, d_W = torch.autograd.grad(v, [u64, W], grad_outputs=r["d_up"])
    what = f"bilinear {(B, N, E, L)}"
    check(loss, r["loss"], f"{what} loss")
    check(scores.cpu()[r["valid"]], r["scores"][r["valid"]], f"{what} scores")
    check(neg_scores.cpu()[r["filled"]], r["neg_scores"][r["filled"]], f"{what} neg_scores")
    check(u.grad.reshape(B, E), d_u, f"{what} d_u")
    check(sc.bilin.weight.grad, d_W, f"{what} d_W")
    check(table.grad, r["d_table"], f"{what} d_table")
    assert sc.bilin.bias.grad is None


def test_dot_scorer_is_ops_list_loss():
    from xnrs_amd.models.blocks import DotScoring
    c = case(70, 40, 32, 130)
    got = DotScoring().list_loss(c["table"], c["up"].reshape(70, 1, 32), *c["tgt"], c["neg"], c["pad_row"])
    want = run(c, False, False)
    assert torch.equal(bits(got[0]), bits(want["loss"])) and torch.equal(bits(got[2]), bits(want["lse"]))
    with pytest.raises(NotImplementedError, match="normalize=True"):
        DotScoring(normalize=True).list_loss(c["table"], c["up"], *c["tgt"], c["neg"], c["pad_row"])


# ------------------------------------------------------------------------------------------- 6. operand alignment
ALIGN_SHAPE = (5, 300, 260, 65)
ALIGN_INS = ("table", "up", "neg_rows", "tgt_rows", "g", "order")
ALIGN_OUTS = ("scores", "loss", "lse", "neg_scores", "d_up", "d_table")


@functools.lru_cache(maxsize=None)
def align_family():
    """xnrs_list_loss_fwd + _bwd on one problem in the case style of tests/test_hip_pointer_alignment.py: every pointer
    operand is a guarded view at a chosen offset from a 16-byte boundary.  `order` follows from the rows and from which
    entries are empty, so the reference gives it."""
    from tests import test_hip_pointer_alignment as PA
    B, N, E, L = ALIGN_SHAPE
    c = case(B, N, E, L)
    r = c["ref"]
    T = c["tgt"][1].numel()
    key = torch.cat((torch.where(r["filled"].reshape(-1), c["neg"].cpu().reshape(-1).long(), N),
                     torch.where(r["valid"], c["tgt"][1].cpu().long(), N)))
    order = torch.sort(key, stable=True).indices.to(I32)

    def call(o):
        l = hip.lib()
        nws = l.xnrs_list_loss_workspace_bytes(B, L, T, E, 1)
        ws = hip.workspace(DEV, nws)
        head = (hip.ptr(o["table"]), N, E, hip.ptr(o["up"]), None, B, hip.ptr(c["tgt"][0]), hip.ptr(o["tgt_rows"]),
                hip.ptr(o["neg_rows"]), L, c["pad_row"])
        o["loss"].zero_()  # (the entry point writes the positions of the CSR; ops.list_loss_forward starts from zeros / NaN)
        o["scores"].fill_(float("nan"))
        rc = l.xnrs_list_loss_fwd(*head, hip.ptr(o["scores"]), hip.ptr(o["loss"]), hip.ptr(o["lse"]), hip.ptr(o["neg_scores"]),
                                  hip.ptr(ws), nws, PA.stream())
        if rc:
            return rc
        return l.xnrs_list_loss_bwd(*head, hip.ptr(o["scores"]), hip.ptr(o["lse"]), hip.ptr(o["neg_scores"]), hip.ptr(o["g"]),
                                    hip.ptr(o["order"]), hip.ptr(o["d_up"]), hip.ptr(o["d_table"]), hip.ptr(ws), nws, PA.stream())
    ins = dict(table=c["table"].cpu(), up=c["up"].cpu(), neg_rows=c["neg"].cpu(), tgt_rows=c["tgt"][1].cpu(), g=c["g"].cpu(),
               order=order)
    outs = dict(scores=((T,), F32), loss=((T,), F32), lse=((B,), F32), neg_scores=((B, L), F32), d_up=((B, E), F32),
                d_table=((N, E), F32))
    assert tuple(ins) == ALIGN_INS and tuple(outs) == ALIGN_OUTS
    return PA, PA.Family(ins, outs, call, {k: r[k] for k in outs}, bitwise=tuple(outs))


@functools.lru_cache(maxsize=None)
def align_base():
    PA, fam = align_family()
    return PA.run_case(fam, {})


@pytest.mark.parametrize("case_", ["aligned"] + [f"{k}+4" for k in ALIGN_INS + ALIGN_OUTS] + ["table+8", "d_table+12", "all"])
def test_operand_off_a_16_byte_boundary(case_):
    """Every pointer operand shifted by one element (and all at once) gives the results of the aligned call -- the same bits:
    the scalar-load forms add the same elements in the same order."""
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
    PA.check_case(fam, "list_loss", case_, got, base)


# ------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_write_nothing():
    c = case(70, 40, 32, 130)
    B, N, E, L = 70, 40, 32, 130
    l = hip.lib()
    EINVAL, EWORKSPACE = hip._CONSTANTS["EINVAL"], hip._CONSTANTS["EWORKSPACE"]
    T = c["tgt"][1].numel()
    ok = run(c, False, False)
    need = l.xnrs_list_loss_workspace_bytes(B, L, T, E, 1)
    assert need > 0 and l.xnrs_list_loss_workspace_bytes(B, L, T, E, 0) == 0
    assert l.xnrs_list_loss_workspace_bytes(4096, 128, 4096, 256, 1) <= 4096 * 128 * 256 * 4 // 16  # never the (B, L, E) copy
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    st = hip.stream_ptr(torch.device(DEV))
    p = hip.ptr

    def fwd(table=c["table"], up=c["up"], off=c["tgt"][0], rows=c["tgt"][1], neg=c["neg"], L_=L, loss="out"):
        out = [torch.full(s, 7.0, device=DEV) for s in ((T,), (T,), (B,), (B, L))]
        rc = l.xnrs_list_loss_fwd(p(table), N, E, p(up), None, B, p(off), p(rows), p(neg), L_, c["pad_row"], p(out[0]),
                                  p(out[1]) if loss == "out" else None, p(out[2]), p(out[3]), p(ws), need, st)
        torch.cuda.synchronize()
        return rc, out

    rc, out = fwd()
    assert rc == 0 and torch.equal(bits(out[1]), bits(ok["loss"])) and torch.equal(bits(out[3]), bits(ok["neg_scores"]))
    for bad in (dict(L_=-1), dict(table=None), dict(up=None), dict(off=None), dict(rows=None), dict(neg=None), dict(loss=None)):
        rc, out = fwd(**bad)
        assert rc == EINVAL and all((t == 7.0).all() for t in out), bad

    order = ops.list_loss_order(N, c["tgt"][1], c["neg"], ok["scores"], ok["neg_scores"])

    def bwd(order_=order, d_table="out", g=c["g"], nbytes=need, L_=L):
        d_up, d_tab = torch.full_like(c["up"], 7.0), torch.full_like(c["table"], 7.0)
        rc = l.xnrs_list_loss_bwd(p(c["table"]), N, E, p(c["up"]), None, B, p(c["tgt"][0]), p(c["tgt"][1]), p(c["neg"]), L_,
                                  c["pad_row"], p(ok["scores"]), p(ok["lse"]), p(ok["neg_scores"]), p(g), p(order_), p(d_up),
                                  p(d_tab) if d_table == "out" else None, p(ws), nbytes, st)
        torch.cuda.synchronize()
        return rc, d_up, d_tab

    rc, d_up, d_tab = bwd()
    full = run(c)
    assert rc == 0 and torch.equal(bits(d_up), bits(full["d_up"])) and torch.equal(bits(d_tab), bits(full["d_table"]))
    for bad, want in ((dict(order_=None), EINVAL), (dict(d_table=None), EINVAL), (dict(g=None), EINVAL), (dict(L_=-1), EINVAL),
                      (dict(nbytes=need - 1), EWORKSPACE)):
        rc, d_up, d_tab = bwd(**bad)
        assert rc == want and (d_up == 7.0).all() and (d_tab == 7.0).all(), bad
    rc, d_up, d_tab = bwd(order_=None, d_table=None, nbytes=0)  # d_up alone needs neither an order nor a workspace
    assert rc == 0 and torch.equal(bits(d_up), bits(full["d_up"])) and (d_tab == 7.0).all()
    # an order with values outside [0, B L + T): skipped, never dereferenced (the gradients of the rows concerned are unspecified)
    wild = order.clone()
    wild[::7] = 2 ** 31 - 1
    wild[3::7] = -5
    rc, d_up, d_tab = bwd(order_=wild)
    assert rc == 0 and torch.isfinite(d_tab).all()
    empty = torch.zeros((0, E), device=DEV)
    off0 = torch.zeros((1,), dtype=torch.int64, device=DEV)
    out = ops.list_loss(c["table"], empty, off0, torch.zeros((0,), dtype=I32, device=DEV), torch.zeros((0, L), dtype=I32, device=DEV))
    assert all(t.numel() == 0 for t in out)  # B == 0: XNRS_OK
    # L == 0: every user is without negatives
    loss, scores, lse, ns = ops.list_loss(c["table"], c["up"], *c["tgt"], torch.zeros((B, 0), dtype=I32, device=DEV), c["pad_row"])
    assert (loss == 0).all() and (lse == float("-inf")).all() and ns.numel() == 0
    assert torch.equal(torch.isnan(scores), torch.isnan(ok["scores"]))
