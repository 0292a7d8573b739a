"""GPU: the full-table softmax ranking loss (include/xnrs_hip.h: xnrs_table_loss_fwd / _bwd, csrc/table_loss.hip) through
ops.table_loss and the raw entry points.

1. parity of loss, d_up and d_table with the fp64 reference of the definition (tests/table_loss_ref.py) at the project's bar,
   non-uniform upstream g, every printed MARGIN = observed error / bar;
2. exact checks without a tolerance: score bits, batch and position invariance, run-to-run bits, window == complement
   exclusions, users without negatives, queries without an answer, untouched d_table rows;
3. autograd plumbing, 4. the bilinear scorer, 5. refusals."""
import functools

import pytest
import torch

from tests import helpers as H
from tests.table_loss_ref import table_loss_ref
from xnrs_amd import hip, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the smallest shapes that reach every edge of the tile code (B, n_rows, E): one row; the scalar-load path (E % 4 != 0); the
# feature tail behind one 32-block, two user tiles, a ragged last chunk; 9 chunks + 1 row at the LSTUR width (two feature
# passes of the backward); one user tile at 256.  The last one is the smallest at which a slice of the d_up sweep walks
# several chunks (9 user tiles x 63 chunks > 256 workgroups) and a group of the d_table sweep several user tiles.
SHAPES = [(1, 1, 4), (3, 127, 37), (130, 300, 40), (129, 1153, 272), (5, 1153, 256), (1100, 8000, 8)]
CONFIGS = ["plain", "messy", "own"]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def csr(lists):
    off = [0]
    for l in lists:
        off.append(off[-1] + len(l))
    rows = [r for l in lists for r in l]
    return (torch.tensor(off, dtype=torch.int64, device=DEV), torch.tensor(rows, dtype=torch.int32, device=DEV).reshape(-1))


def pad_of(N):
    return N // 2 if N > 2 else -1


def target_lists(B, N, g):
    """Per user 0, 1, 3 or 6 targets: duplicates and the three kinds without an answer (below 0, past the table, the pad row)"""
    draw = lambda n: torch.randint(0, N, (n,), generator=g).tolist()  # noqa: E731
    out = []
    for b in range(B):
        kind = (b + 1) % 4 if B > 1 else 1
        if kind == 0:
            out.append([])
        elif kind == 1:
            out.append(draw(1))
        elif kind == 2:
            r = draw(2)
            out.append([r[0], r[1], r[0]])
        else:
            r = draw(2)
            out.append([r[0], -3, r[1], N + 2, pad_of(N), r[0]])
    return out


def exclusion_lists(B, N, g, targets, config):
    if config == "plain":
        return None
    out = []
    for b in range(B):
        n = int(torch.randint(0, 24, (1,), generator=g))
        l = torch.randint(0, N, (n,), generator=g).tolist()
        l = l + l[:3] + [-5, N + 100]  # unsorted, duplicates, foreign ids
        if config == "own":
            l = l + [t for t in targets[b]]  # the user's own targets
        out.append(l if b % 5 != 4 else [])
    return out


def window_lists(B, N, g):
    """narrow ones in the first quarter, empty (lo >= hi), the two ends of the table and a stretch in the middle (disjoint
    within a tile: gaps, and whole chunks that no window touches), bounds outside the table"""
    lo, hi = [], []
    for b in range(B):
        kind = b % 5
        a = int(torch.randint(0, max(N // 4, 1), (1,), generator=g))
        if kind == 0:
            w = (a, a + 40)
        elif kind == 1:
            w = (a + 7, a)
        elif kind == 2:
            w = (-9, min(50, N))
        elif kind == 3:
            w = (max(N - 60, 0), N + 1000)
        else:
            w = (N // 3, N // 3 + 200)
        lo.append(w[0])
        hi.append(w[1])
    return (torch.tensor(lo, dtype=torch.int32, device=DEV), torch.tensor(hi, dtype=torch.int32, device=DEV))


@functools.lru_cache(maxsize=None)
def case(B, N, E, config, smax=0.0):
    """One problem and its fp64 reference, computed once and shared.  config: 'plain' (no exclusions, no windows, no pad row),
    'messy' (messy exclusion lists, windows of every kind, a pad row inside the table), 'own' (lists that hold the user's own
    targets, a pad row).  smax: scale `up` so that max|score| is about smax."""
    g = gen(1000 * B + N + E + len(config))
    table = torch.randn((N, E), generator=g)
    up = torch.randn((B, E), generator=g) * (2.0 / E ** 0.5)
    if smax:
        up = up * (smax / (up.double() @ table.double().T).abs().max().item())
    targets = target_lists(B, N, g)
    excl = exclusion_lists(B, N, g, targets, config)
    c = dict(B=B, N=N, E=E, table=table.to(DEV), up=up.to(DEV), targets=targets, excl=excl, pad_row=-1 if config == "plain" else pad_of(N))
    c["tgt"] = csr(targets)
    c["excl_csr"] = csr(excl) if excl is not None else (None, None)
    c["win"] = window_lists(B, N, g) if config == "messy" else (None, None)
    T = c["tgt"][1].numel()
    c["g"] = (torch.rand((T,), generator=g) + 0.25).to(DEV)
    c["ref"] = table_loss_ref(c["table"], c["up"], *c["tgt"], *c["excl_csr"], c["pad_row"], *c["win"], None, c["g"])
    return c


def run(c, need_table=True, need_up=True, win="case", excl="case", bias=None):
    """loss, scores, lse and the gradients of sum(g * loss) on the device"""
    table = c["table"].clone().requires_grad_(need_table)
    up = c["up"].clone().requires_grad_(need_up)
    wl, wh = c["win"] if win == "case" else win
    eo, er = c["excl_csr"] if excl == "case" else excl
    loss, scores, lse = ops.table_loss(table, up, *c["tgt"], eo, er, c["pad_row"], wl, wh, bias)
    if need_table or need_up:
        (loss * c["g"]).sum().backward()
    return loss.detach(), scores.detach(), lse.detach(), up.grad, table.grad


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def check(got, ref, what):
    e = H.assert_close(got, ref, what=what)
    print(f"MARGIN {what}: {e / H.RTOL:.3f} of the bar, elementwise {H.elementwise_excess(got, ref, H.RTOL):.3f}")


def check_against_reference(c, what):
    loss, scores, lse, d_up, d_table = run(c)
    r = c["ref"]
    valid = r["valid"]
    assert torch.isfinite(loss).all() and torch.isfinite(d_up).all() and torch.isfinite(d_table).all(), what
    assert torch.equal(torch.isnan(scores).cpu(), ~valid), f"{what}: NaN exactly where a query has no answer"
    assert (loss.cpu()[~valid] == 0).all()
    if valid.any():
        check(scores.cpu()[valid], r["scores"][valid], f"{what} scores")
    has = torch.isfinite(r["lse"])
    assert torch.equal(torch.isinf(lse).cpu() & (lse.cpu() < 0), ~has), f"{what}: lse is -inf exactly without negatives"
    if has.any():
        check(lse.cpu()[has], r["lse"][has], f"{what} lse")
    check(loss, r["loss"], f"{what} loss")
    check(d_up, r["d_up"], f"{what} d_up")
    check(d_table, r["d_table"], f"{what} d_table")
    return loss, scores, lse, d_up, d_table


# ------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("B,N,E", SHAPES)
def test_matches_fp64_reference(B, N, E, config):
    c = case(B, N, E, config)
    check_against_reference(c, f"{(B, N, E)} {config}")
    if N > 1:
        assert c["ref"]["valid"].any() and (B == 1 or not c["ref"]["valid"].all())


def test_large_scores_stay_finite_and_within_the_bar():
    c = case(5, 1153, 272, "messy", smax=300.0)
    assert 250 < (c["up"].double() @ c["table"].double().T).abs().max().item() < 350
    check_against_reference(c, "max|s| ~ 300")


# ------------------------------------------------------------------------------------------- 2. exact
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("B,N,E", SHAPES[:5])
def test_scores_are_the_bits_of_rank_dot(B, N, E, config):
    c = case(B, N, E, config)
    _, scores, _, _, _ = run(c, need_table=False, need_up=False)
    _, want = ops.rank_dot(c["table"], c["up"], *c["tgt"], *c["excl_csr"], c["pad_row"], win_lo=c["win"][0], win_hi=c["win"][1])
    assert torch.equal(torch.isnan(scores), torch.isnan(want))
    ok = ~torch.isnan(want)
    assert torch.equal(bits(scores[ok]), bits(want[ok]))


def sub_case(c, users):
    """the problem of `users` (in that order) of case c, nothing else changed"""
    idx = torch.tensor(users, device=DEV)
    s = dict(c)
    s["B"] = len(users)
    s["up"] = c["up"][idx].contiguous()
    s["tgt"] = csr([c["targets"][b] for b in users])
    s["excl_csr"] = csr([c["excl"][b] for b in users]) if c["excl"] is not None else (None, None)
    s["win"] = tuple(w[idx].contiguous() for w in c["win"]) if c["win"][0] is not None else (None, None)
    return s


@pytest.mark.parametrize("config", ["messy", "own"])
def test_a_user_does_not_depend_on_the_batch_or_the_position(config):
    c = case(130, 300, 40, config)
    loss, _, lse, _, _ = run(c, False, False)
    off = c["tgt"][0].tolist()
    order = list(range(129, -1, -1))  # every user at another position, in the other tile
    rl, _, rlse, _, _ = run(sub_case(c, order), False, False)
    roff = sub_case(c, order)["tgt"][0].tolist()
    for pos, b in enumerate(order):
        assert torch.equal(bits(lse[b:b + 1]), bits(rlse[pos:pos + 1])), f"lse of user {b}"
        assert torch.equal(bits(loss[off[b]:off[b + 1]]), bits(rl[roff[pos]:roff[pos + 1]])), f"loss of user {b}"
    for b in (2, 77, 129):  # alone
        al, _, alse, _, _ = run(sub_case(c, [b]), False, False)
        assert torch.equal(bits(alse), bits(lse[b:b + 1])) and torch.equal(bits(al), bits(loss[off[b]:off[b + 1]])), f"user {b} alone"


@pytest.mark.parametrize("B,N,E", [(130, 300, 40), (129, 1153, 272), (1100, 8000, 8)])
def test_a_second_run_gives_the_same_bits(B, N, E):
    c = case(B, N, E, "messy")
    a, b = run(c), run(c)
    for x, y, what in zip(a, b, ("loss", "scores", "lse", "d_up", "d_table")):
        assert torch.equal(bits(x), bits(y)), what


@pytest.mark.parametrize("B,N,E", [(130, 300, 40), (129, 1153, 272)])
def test_a_window_equals_its_complement_on_the_exclusion_list(B, N, E):
    c = case(B, N, E, "messy")
    lo, hi = (w.tolist() for w in c["win"])
    listed = [c["excl"][b] + [n for n in range(N) if not lo[b] <= n < hi[b]] for b in range(B)]
    a = run(c, False, False)
    b = run(c, False, False, win=(None, None), excl=csr(listed))
    for x, y, what in zip(a[:3], b[:3], ("loss", "scores", "lse")):
        assert torch.equal(bits(x), bits(y)), what


def raw_forward(c, win=(None, None), ws_bytes=None, fill=7.0):
    l = hip.lib()
    T = c["tgt"][1].numel()
    out = [torch.full((n,), fill, dtype=torch.float32, device=DEV) for n in (T, T, c["B"])]
    need = l.xnrs_table_loss_workspace_bytes(c["B"], c["N"], c["E"], 0)
    ws = torch.empty((need + 256,), dtype=torch.uint8, device=DEV)
    rc = l.xnrs_table_loss_fwd(hip.ptr(c["table"]), c["N"], c["E"], hip.ptr(c["up"]), None, c["B"], hip.ptr(c["tgt"][0]),
                               hip.ptr(c["tgt"][1]), hip.ptr(c["excl_csr"][0]), hip.ptr(c["excl_csr"][1]), hip.ptr(win[0]),
                               hip.ptr(win[1]), c["pad_row"], hip.ptr(out[0]), hip.ptr(out[1]), hip.ptr(out[2]), hip.ptr(ws),
                               need if ws_bytes is None else ws_bytes, hip.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, out, need


def test_null_windows_are_the_call_without_windows():
    c = case(130, 300, 40, "own")
    rc, (scores, loss, lse), _ = raw_forward(c)
    assert rc == 0
    want = run(c, False, False)
    assert torch.equal(bits(loss), bits(want[0])) and torch.equal(bits(lse), bits(want[2]))
    ok = ~torch.isnan(want[1])
    assert torch.equal(bits(scores[ok]), bits(want[1][ok]))


def test_users_without_negatives_and_queries_without_an_answer():
    c = dict(case(130, 300, 40, "messy"))
    N = c["N"]
    excl = [list(l) for l in c["excl"]]
    excl[2] = list(range(N))  # every row excluded
    excl[5] = list(range(N - 1, -1, -1))
    c["excl"], c["excl_csr"] = excl, csr(excl)
    lo, hi = (w.tolist() for w in c["win"])
    empty = [b for b in range(c["B"]) if lo[b] >= hi[b]]
    assert empty and any(c["targets"][b] for b in empty) and c["targets"][2] and c["targets"][5]
    c["ref"] = table_loss_ref(c["table"], c["up"], *c["tgt"], *c["excl_csr"], c["pad_row"], *c["win"], None, c["g"])
    loss, scores, lse, d_up, d_table = check_against_reference(c, "no negatives")
    off = c["tgt"][0].tolist()
    for b in empty + [2, 5]:
        assert lse[b].item() == float("-inf")
        assert (loss[off[b]:off[b + 1]] == 0).all() and (d_up[b] == 0).all()
    assert not torch.isnan(loss).any() and not torch.isnan(lse).any() and not torch.isnan(d_up).any() and not torch.isnan(d_table).any()
    rows = c["tgt"][1].cpu()
    no_answer = (rows < 0) | (rows >= N) | (rows == c["pad_row"])
    assert no_answer.any() and torch.isnan(scores.cpu()[no_answer]).all() and (loss.cpu()[no_answer] == 0).all()
    assert not torch.isnan(scores.cpu()[~no_answer]).any()


@pytest.mark.parametrize("B,N,E", [(130, 300, 40), (129, 1153, 272)])
def test_rows_of_d_table_that_nobody_may_touch_are_zero(B, N, E):
    c = case(B, N, E, "messy")
    lo, hi = (torch.tensor(w.tolist()).clamp(0, N) for w in c["win"])
    n = torch.arange(N)
    in_a_window = ((n[None] >= lo[:, None]) & (n[None] < hi[:, None])).any(dim=0)
    is_target = torch.zeros(N, dtype=torch.bool)
    for t in c["tgt"][1].tolist():
        if 0 <= t < N:
            is_target[t] = True
    untouched = ~in_a_window & ~is_target
    untouched[c["pad_row"]] = True
    if N > 1000:
        assert untouched.sum() > 128  # whole chunks between the windows
    d_table = run(c)[4].cpu()
    assert (d_table[untouched] == 0).all() and (d_table[c["pad_row"]] == 0).all()
    assert (d_table[~untouched].abs().sum(dim=1) > 0).any()


# ------------------------------------------------------------------------------------------- 3. autograd plumbing
def test_gradients_that_nobody_asks_for_are_not_computed(monkeypatch):
    c = case(130, 300, 40, "messy")
    asked = []
    real = ops.table_loss_backward

    def spy(*a, **k):
        asked.append((k["want_d_up"], k["want_d_table"]))
        return real(*a, **k)

    monkeypatch.setattr(ops, "table_loss_backward", spy)
    full = run(c)
    assert asked[-1] == (True, True)
    _, _, _, d_up, d_table = run(c, need_table=False)
    assert d_table is None and asked[-1] == (True, False) and torch.equal(bits(d_up), bits(full[3]))
    _, _, _, d_up, d_table = run(c, need_up=False)
    assert d_up is None and asked[-1] == (False, True) and torch.equal(bits(d_table), bits(full[4]))
    table, up = c["table"].clone().requires_grad_(True), c["up"].clone().requires_grad_(True)
    loss, scores, lse = ops.table_loss(table, up, *c["tgt"], *c["excl_csr"], c["pad_row"], *c["win"])
    assert loss.requires_grad and not scores.requires_grad and not lse.requires_grad
    (du,) = torch.autograd.grad((loss * c["g"]).sum(), inputs=[up])
    assert asked[-1] == (True, False) and table.grad is None and torch.equal(bits(du), bits(full[3]))
    with torch.no_grad():
        l2, _, _ = ops.table_loss(table, up, *c["tgt"], *c["excl_csr"], c["pad_row"], *c["win"])
    assert not l2.requires_grad and torch.equal(bits(l2), bits(full[0]))


# ------------------------------------------------------------------------------------------- 4. the scorers
@pytest.mark.parametrize("B,N,E", [(130, 300, 40), (5, 1153, 256)])
def test_bilinear_scorer(B, N, E):
    from xnrs_amd.models.blocks import BilinScoring
    c = case(B, N, E, "messy")
    torch.manual_seed(5)
    sc = BilinScoring(E).to(DEV)
    with torch.no_grad():
        sc.bilin.weight.mul_(E ** 0.5 * 0.5)
        sc.bilin.bias.fill_(0.75)
    table = c["table"].clone().requires_grad_(True)
    u = c["up"].clone().reshape(B, 1, E).requires_grad_(True)
    loss, scores, lse = sc.table_loss(table, u, *c["tgt"], *c["excl_csr"], c["pad_row"], *c["win"])
    (loss * c["g"]).sum().backward()
    # the reference: the same definition on v = u W[0] in fp64, autograd down to u, W and the table
    W = sc.bilin.weight.detach().double().cpu().requires_grad_(True)
    u64 = c["up"].double().cpu().requires_grad_(True)
    v = u64 @ W[0]
    r = table_loss_ref(c["table"], v, *c["tgt"], *c["excl_csr"], c["pad_row"], *c["win"], sc.bilin.bias, c["g"])
    d_u, d_W = torch.autograd.grad(v, [u64, W], grad_outputs=r["d_up"])
    check(loss, r["loss"], f"bilinear {(B, N, E)} loss")
    check(scores.cpu()[r["valid"]], r["scores"][r["valid"]], f"bilinear {(B, N, E)} scores")
    check(u.grad.reshape(B, E), d_u, f"bilinear {(B, N, E)} d_u")
    check(sc.bilin.weight.grad, d_W, f"bilinear {(B, N, E)} d_W")
    check(table.grad, r["d_table"], f"bilinear {(B, N, E)} d_table")
    assert sc.bilin.bias.grad is None or (sc.bilin.bias.grad == 0).all()


def test_dot_scorer_is_ops_table_loss():
    from xnrs_amd.models.blocks import DotScoring
    c = case(130, 300, 40, "own")
    got = DotScoring().table_loss(c["table"], c["up"].reshape(130, 1, 40), *c["tgt"], *c["excl_csr"], c["pad_row"])
    want = run(c, False, False)
    assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[2]), bits(want[2]))


# ------------------------------------------------------------------------------------------- 5. refusals
def test_a_short_workspace_and_a_single_window_pointer_are_refused_and_write_nothing():
    c = case(130, 300, 40, "messy")
    l = hip.lib()
    consts = hip._CONSTANTS
    rc, out, need = raw_forward(c)
    assert rc == 0 and need >= 8 * 3 * 130  # one (max, sum) pair per user and 128-row chunk
    assert l.xnrs_table_loss_workspace_bytes(130, 300, 40, 1) > l.xnrs_table_loss_workspace_bytes(130, 300, 40, 0)
    assert l.xnrs_table_loss_workspace_bytes(4096, 65536, 256, 1) < 4096 * 65536 * 4 // 16  # never the score matrix
    rc, out, _ = raw_forward(c, ws_bytes=need - 1)
    assert rc == consts["EWORKSPACE"] and all((t == 7.0).all() for t in out)
    for win in ((c["win"][0], None), (None, c["win"][1])):
        rc, out, _ = raw_forward(c, win=win)
        assert rc == consts["EINVAL"] and all((t == 7.0).all() for t in out)
    # the backward: the same two refusals, the gradients untouched
    _, scores, lse, _, _ = run(c, False, False)
    d_up, d_table = torch.full_like(c["up"], 7.0), torch.full_like(c["table"], 7.0)
    need = l.xnrs_table_loss_workspace_bytes(130, 300, 40, 1)
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    for win, nbytes, want in (((None, None), need - 1, "EWORKSPACE"), ((c["win"][0], None), need, "EINVAL")):
        rc = l.xnrs_table_loss_bwd(hip.ptr(c["table"]), 300, 40, hip.ptr(c["up"]), None, 130, hip.ptr(c["tgt"][0]), hip.ptr(c["tgt"][1]),
                                   hip.ptr(c["excl_csr"][0]), hip.ptr(c["excl_csr"][1]), hip.ptr(win[0]), hip.ptr(win[1]),
                                   c["pad_row"], hip.ptr(scores), hip.ptr(lse), hip.ptr(c["g"]), hip.ptr(d_up), hip.ptr(d_table),
                                   hip.ptr(ws), nbytes, hip.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        assert rc == consts[want] and (d_up == 7.0).all() and (d_table == 7.0).all()
    empty = torch.zeros((0, 40), device=DEV)
    off0 = torch.zeros((1,), dtype=torch.int64, device=DEV)
    loss, scores, lse = ops.table_loss(c["table"], empty, off0, torch.zeros((0,), dtype=torch.int32, device=DEV))
    assert loss.numel() == 0 and scores.numel() == 0 and lse.numel() == 0  # B == 0: XNRS_OK
