"""CPU: what the mined-negatives loss does around its kernels -- the merged exclusion CSR, the arguments topk_deep and
list_loss receive (stub scorers), the refusals raised before anything is encoded, the malformed lists ops.list_loss refuses
before the device, and the C ABI's argument and workspace checks."""
import ctypes

import pytest
import torch

from xnrs_amd import hip, losses, ops, synth
from xnrs_amd.models.blocks import BilinScoring, DotScoring, FCScoring
from xnrs_amd.models.caum import CAUMScoring

EINVAL, EWORKSPACE = -1, -3


def _csr(lists):
    off = [0]
    for l in lists:
        off.append(off[-1] + len(l))
    return torch.tensor(off, dtype=torch.int64), torch.tensor([r for l in lists for r in l], dtype=torch.int32)


def test_merged_exclusions_are_history_then_clicks_per_session():
    hist = [[5, 3, 5], [], [9], [1, 2, 3, 4]]
    clicks = [[7], [8, 8], [], [6]]
    off, rows = losses.merged_exclusions(_csr(hist), _csr(clicks))
    assert off.dtype == torch.int64 and rows.dtype == torch.int32
    assert off.tolist() == [0, 4, 6, 7, 12]
    assert rows.tolist() == [5, 3, 5, 7, 8, 8, 9, 1, 2, 3, 4, 6]  # unsorted, duplicates kept: the header allows both
    off, rows = losses.merged_exclusions((None, None), _csr(clicks))  # exclude_history=False: the clicks alone
    assert off.tolist() == [0, 1, 3, 3, 4] and rows.tolist() == [7, 8, 8, 6]
    off, rows = losses.merged_exclusions(_csr([[], []]), _csr([[], []]))
    assert off.tolist() == [0, 0, 0] and rows.numel() == 0


class _Stub:
    """a scorer that records what it is asked and returns what it was given"""

    def __init__(self, loss, scores, rows):
        self.loss, self.scores, self.rows, self.mined, self.listed = loss, scores, rows, [], []

    def topk_deep(self, table, u, k, excl_off=None, excl_rows=None, pad_row=-1, win_lo=None, win_hi=None):
        assert not torch.is_grad_enabled() and not table.requires_grad and not u.requires_grad
        self.mined.append((k, excl_off.tolist(), excl_rows.tolist(), pad_row, win_lo, win_hi))
        return self.rows[:, :k], torch.zeros(self.rows[:, :k].shape)

    def list_loss(self, table, u, tgt_off, tgt_rows, neg_rows, pad_row=-1):
        assert torch.is_grad_enabled() and table.requires_grad and u.requires_grad
        self.listed.append((tgt_off.tolist(), tgt_rows.tolist(), neg_rows, pad_row))
        return self.loss, self.scores, torch.zeros(2), torch.zeros(neg_rows.shape)


def test_the_arguments_of_topk_deep_and_list_loss():
    nan = float("nan")
    loss = torch.tensor([1.5, 0.0, 2.5], dtype=torch.float64, requires_grad=True)
    scores = torch.tensor([0.1, nan, -3.0])
    rows = torch.arange(2 * 6, dtype=torch.int32).reshape(2, 6)
    stub = _Stub(loss, scores, rows)
    table, u = torch.zeros((20, 4), requires_grad=True), torch.zeros((2, 4), requires_grad=True)
    hist, tgt = _csr([[5, 3], [9]]), _csr([[7], [8, 2]])
    got = losses.mine_and_rank(stub, table, u, hist, tgt, 11, 4)
    assert got.item() == 4.0 / 2  # the mean over the two queries that have an answer
    assert stub.mined == [(4, [0, 3, 6], [5, 3, 7, 9, 8, 2], 11, None, None)]
    assert stub.listed[-1][:2] == ([0, 1, 3], [7, 8, 2]) and stub.listed[-1][3] == 11
    assert torch.equal(stub.listed[-1][2], rows[:, :4])
    # windows reach the mining step as keywords; without history the clicks alone are excluded; the lists come back
    lo, hi = torch.tensor([0, 5], dtype=torch.int32), torch.tensor([10, 20], dtype=torch.int32)
    got, used = losses.mine_and_rank(stub, table, u, (None, None), tgt, 11, 6, (lo, hi), "sum", None, True)
    assert got.item() == 4.0 and torch.equal(used, rows)
    assert stub.mined[-1][:4] == (6, [0, 1, 3], [7, 8, 2], 11) and stub.mined[-1][4] is lo and stub.mined[-1][5] is hi
    # given lists: topk_deep is not called
    mine = torch.tensor([[3, -1, 4], [1, 1, -1]], dtype=torch.int32)
    got = losses.mine_and_rank(stub, table, u, hist, tgt, 11, 4, reduction="none", neg_rows=mine)
    assert got is loss and len(stub.mined) == 2 and stub.listed[-1][2] is mine
    # the loss over listed rows on its own
    assert losses.listed_ranking_loss(stub, table, u, *tgt, mine, 11).item() == 2.0 and stub.listed[-1][2] is mine
    with pytest.raises(ValueError, match="reduction"):
        losses.listed_ranking_loss(stub, table, u, *tgt, mine, 11, reduction="max")


class _Model(torch.nn.Module):
    def __init__(self, scorer):
        super().__init__()
        self.rec_model = scorer

    def encode_news_ids(self, store, ids):
        raise AssertionError("refused before anything is encoded")

    def encode_user(self, *a):
        raise AssertionError("refused before anything is encoded")


def test_refusals_come_before_anything_is_encoded():
    assert callable(DotScoring.list_loss) and callable(BilinScoring.list_loss)
    assert not hasattr(FCScoring, "list_loss") and not callable(getattr(CAUMScoring, "list_loss", None))
    table, u = torch.zeros((10, 4)), torch.zeros((2, 4))
    off, rows = _csr([[1], [2]])
    neg = torch.zeros((2, 3), dtype=torch.int32)

    class Cosine(torch.nn.Module):
        pass
    for scorer in (FCScoring(4, 8), Cosine(), CAUMScoring()):
        with pytest.raises(NotImplementedError, match=type(scorer).__name__):
            losses.listed_ranking_loss(scorer, table, u, off, rows, neg)
    for scorer in (DotScoring(normalize=True), BilinScoring(4, normalize=True)):
        with pytest.raises(NotImplementedError, match="normalize=True"):
            losses.listed_ranking_loss(scorer, table, u, off, rows, neg)
    store, beh = synth.click_world(n_news=20, n_sess=5)
    npa_like = _Model(DotScoring())
    npa_like.user_dependent_news = True
    lstur_like = _Model(DotScoring())
    lstur_like.uses_user_index = True
    call = lambda m, **k: losses.mined_negatives_loss(m, store, beh, [0, 1], l_hist=8, **k)  # noqa: E731
    with pytest.raises(NotImplementedError, match="depend on the user"):
        call(npa_like)
    with pytest.raises(NotImplementedError, match="CAUMScoring"):
        call(_Model(CAUMScoring()))
    with pytest.raises(NotImplementedError, match="FCScoring"):
        call(_Model(FCScoring(4, 8)))
    with pytest.raises(NotImplementedError, match="Cosine"):
        call(_Model(Cosine()))
    with pytest.raises(NotImplementedError, match="normalize=True"):
        call(_Model(DotScoring(normalize=True)))
    with pytest.raises(ValueError, match="user index"):
        call(lstur_like)
    with pytest.raises(ValueError, match="reduction"):
        call(_Model(DotScoring()), reduction="median")
    for bad in (0, -1, 1025, 2.5, True):
        with pytest.raises(ValueError, match="n_negatives"):
            call(_Model(DotScoring()), n_negatives=bad)
    for bad in (torch.zeros((3, 4), dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int64), torch.zeros((8,), dtype=torch.int32),
                [[1, 2], [3, 4]]):
        with pytest.raises(ValueError, match="neg_rows"):
            call(_Model(DotScoring()), neg_rows=bad)


def test_list_checks_come_before_the_device():
    table, u = torch.zeros((10, 4)), torch.zeros((3, 1, 4))
    off, rows = _csr([[1], [2], []])
    neg = torch.zeros((3, 5), dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r"targets: offsets \(B\+1,\) int64 and rows int32"):
        ops.list_loss(table, u, off.int(), rows, neg)
    with pytest.raises(RuntimeError, match="for 3 users"):
        ops.list_loss(table, u, off[:-1], rows, neg)
    for bad in (neg.long(), neg[:2], neg.reshape(-1), None):
        with pytest.raises(RuntimeError, match="negative lists"):
            ops.list_loss(table, u, off, rows, bad)
    with pytest.raises(RuntimeError, match="news vectors"):
        ops.list_loss(table[0], u, off, rows, neg)
    with pytest.raises(hip.XnrsHipError, match="cpu"):  # everything well-formed: the only thing missing is the device
        ops.list_loss(table, u, off, rows, neg)


def test_order_puts_entries_without_a_gradient_behind_all_others():
    nan = float("nan")
    neg_rows = torch.tensor([[4, -1, 2], [2, 9, 4]], dtype=torch.int32)
    neg_scores = torch.tensor([[0.5, nan, 0.1], [0.2, nan, 0.3]])
    tgt_rows = torch.tensor([2, 7, 0], dtype=torch.int32)
    scores = torch.tensor([1.0, nan, 2.0])
    order = ops.list_loss_order(9, tgt_rows, neg_rows, scores, neg_scores)
    # entries: slots 0..5, queries 6..8; rows 4 - 2 | 2 - 4 | 2 - 0
    assert order.dtype == torch.int32 and order.tolist() == [8, 2, 3, 6, 0, 5, 1, 4, 7]


def test_workspace_is_a_pure_host_call_and_never_the_copy_of_the_rows():
    w = hip.lib().xnrs_list_loss_workspace_bytes
    up = lambda x: -(-x // 256) * 256  # noqa: E731
    assert w(5, 65, 5, 260, 0) == 0 and w(-1, 8, 1, 8, 1) == 0 and w(4, -1, 1, 8, 1) == 0 and w(4, 8, 1, 0, 1) == 0
    G = -(-5 * 66 // 64)  # one span per 64 entries of the B (L + 1) slots and queries
    assert w(5, 65, 5, 260, 1) == up(4 * 5) + 2 * up(4 * G * 260) + 2 * up(4 * G)
    assert w(5, 65, 5, 260, 1) == w(5, 65, 500, 260, 1)  # (T does not enter)
    # the measured case: 8192 spans at most; 1/32 of the 0.54 GB copy of the listed rows
    assert w(4096, 128, 4096, 256, 1) == up(4 * 4096) + 2 * 4 * 8192 * 256 + 2 * 4 * 8192
    assert w(4096, 128, 4096, 256, 1) <= 4096 * 129 * 256 * 4 // 32 + 3 * 65536


def test_the_entry_points_refuse_on_the_host_before_any_launch():
    l = hip.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = l.xnrs_list_loss_workspace_bytes(3, 5, 3, 8, 1)
    fwd = lambda table=p, n=1000, E=8, up=p, B=3, off=p, rows=p, neg=p, L=5, out=p: \
        l.xnrs_list_loss_fwd(table, n, E, up, None, B, off, rows, neg, L, -1, out, out, out, out, None, 0, None)  # noqa: E731
    bwd = lambda g=p, order=p, d_table=p, nb=need, ws=p, L=5, B=3: \
        l.xnrs_list_loss_bwd(p, 1000, 8, p, None, B, p, p, p, L, -1, p, p, p, g, order, p, d_table, ws, nb, None)  # noqa: E731
    for bad in (dict(n=-1), dict(n=2 ** 31), dict(E=0), dict(B=-1), dict(L=-1), dict(table=None), dict(up=None), dict(off=None),
                dict(rows=None), dict(neg=None), dict(out=None), dict(B=2 ** 26, L=63)):
        assert fwd(**bad) == EINVAL, bad
    assert bwd(g=None) == EINVAL and bwd(L=-1) == EINVAL and bwd(order=None) == EINVAL and bwd(d_table=None) == EINVAL
    assert bwd(nb=need - 1) == EWORKSPACE and bwd(ws=None) == EWORKSPACE
    # B == 0: nothing to do, whatever else is missing
    assert l.xnrs_list_loss_fwd(None, 1000, 8, None, None, 0, None, None, None, 5, -1, None, None, None, None, None, 0, None) == 0
    assert l.xnrs_list_loss_bwd(None, 1000, 8, None, None, 0, None, None, None, 5, -1, None, None, None, None, None, None, None,
                                None, 0, None) == 0
    assert buf.raw == bytes(64)
