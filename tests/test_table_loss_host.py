"""CPU: what the full-table ranking loss refuses before any device work (scorers and models without a table loss, malformed
CSRs, the C ABI's argument and workspace checks), the workspace formula, and the reduction arithmetic against a stub scorer."""
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


class _Model(torch.nn.Module):
    def __init__(self, scorer):
        super().__init__()
        self.rec_model = scorer

    def encode_news_ids(self, store, ids):
        raise AssertionError("refused before anything is encoded")

    def encode_user(self, *a):
        raise AssertionError("refused before anything is encoded")


def test_scorers_and_models_without_a_table_loss_are_refused():
    assert callable(DotScoring.table_loss) and callable(BilinScoring.table_loss)
    assert not hasattr(FCScoring, "table_loss") and CAUMScoring.table_loss is None
    table, u = torch.zeros((10, 4)), torch.zeros((2, 4))
    off, rows = _csr([[1], [2]])

    class Cosine(torch.nn.Module):
        pass
    for scorer in (FCScoring(4, 8), Cosine(), CAUMScoring()):
        with pytest.raises(NotImplementedError, match=type(scorer).__name__):
            losses.table_ranking_loss(scorer, table, u, off, rows)
    for scorer in (DotScoring(normalize=True), BilinScoring(4, normalize=True)):
        with pytest.raises(NotImplementedError, match="normalize=True"):
            losses.table_ranking_loss(scorer, table, u, off, rows)
    store, beh = synth.click_world(n_news=20, n_sess=5)
    npa_like = _Model(DotScoring())
    npa_like.user_dependent_news = True
    lstur_like = _Model(DotScoring())
    lstur_like.uses_user_index = True
    call = lambda m, **k: losses.full_table_loss(m, store, beh, [0, 1], l_hist=8, **k)  # noqa: E731
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


def test_csr_dtype_and_length_checks_come_before_the_device():
    table, u = torch.zeros((10, 4)), torch.zeros((3, 1, 4))
    off, rows = _csr([[1], [2], []])
    with pytest.raises(RuntimeError, match=r"targets: offsets \(B\+1,\) int64 and rows int32"):
        ops.table_loss(table, u, off.int(), rows)
    with pytest.raises(RuntimeError, match=r"targets: offsets \(B\+1,\) int64 and rows int32"):
        ops.table_loss(table, u, off, rows.long())
    with pytest.raises(RuntimeError, match="for 3 users"):
        ops.table_loss(table, u, off[:-1], rows)
    with pytest.raises(RuntimeError, match=r"exclusions: offsets \(B\+1,\) int64 and rows int32"):
        ops.table_loss(table, u, off, rows, off, rows.long())
    with pytest.raises(RuntimeError, match="given together"):
        ops.table_loss(table, u, off, rows, off, None)
    with pytest.raises(RuntimeError, match="news vectors"):
        ops.table_loss(table[0], u, off, rows)
    with pytest.raises(hip.XnrsHipError, match="cpu"):  # everything well-formed: the only thing missing is the device
        ops.table_loss(table, u, off, rows)


class _Stub:
    """a scorer whose table_loss returns what it was given"""

    def __init__(self, loss, scores):
        self.loss, self.scores, self.calls = loss, scores, []

    def table_loss(self, table, u, tgt_off, tgt_rows, excl_off=None, excl_rows=None, pad_row=-1, win_lo=None, win_hi=None):
        self.calls.append((excl_off, excl_rows, pad_row, win_lo, win_hi))
        return self.loss, self.scores, torch.zeros(2)


def test_reduction_arithmetic():
    nan = float("nan")
    loss = torch.tensor([1.5, 0.0, 2.5, 0.0, 4.0], dtype=torch.float64, requires_grad=True)
    scores = torch.tensor([0.1, nan, -3.0, nan, 7.0])
    stub = _Stub(loss, scores)
    args = (stub, torch.zeros((4, 2)), torch.zeros((2, 2)), torch.zeros(3, dtype=torch.int64), torch.zeros(5, dtype=torch.int32))
    assert losses.table_ranking_loss(*args, reduction="none") is loss
    assert losses.table_ranking_loss(*args, reduction="sum").item() == 8.0
    mean = losses.table_ranking_loss(*args, 1, 2, 3, 4, 5)  # the default: over the three queries that have an answer
    assert mean.item() == 8.0 / 3 and stub.calls[-1] == (1, 2, 3, 4, 5)
    mean.backward()
    assert torch.equal(loss.grad, torch.full((5,), 1 / 3, dtype=torch.float64))
    none = _Stub(torch.zeros(2), torch.tensor([nan, nan]))
    assert losses.table_ranking_loss(none, *args[1:]).item() == 0.0  # no query has an answer: 0, not a division by zero
    empty = _Stub(torch.zeros(0), torch.zeros(0))
    assert losses.table_ranking_loss(empty, *args[1:]).item() == 0.0
    with pytest.raises(ValueError, match="reduction"):
        losses.table_ranking_loss(*args, reduction="max")
    assert not stub.calls[3:]  # (refused before the scorer is called)


def test_workspace_is_a_pure_host_call_and_never_the_score_matrix():
    w = hip.lib().xnrs_table_loss_workspace_bytes
    assert w(0, 100, 8, 1) == 0 and w(-1, 100, 8, 1) == 0 and w(4, 100, 0, 1) == 0
    up = lambda x: -(-x // 256) * 256  # noqa: E731
    # one user tile, 10 chunks: forward 8 B per (user, chunk); d_up over 10 slices; d_table straight into the gradient
    assert w(5, 1153, 256, 0) == w(5, 1153, 256, 1) == max(up(8 * 10 * 5), up(4 * 10 * 5 * 256))
    # two user tiles, 3 chunks: 3 slices; 2 user groups of the d_table sweep
    assert w(130, 300, 40, 0) == max(up(8 * 3 * 130), up(4 * 3 * 130 * 40))
    assert w(130, 300, 40, 1) == up(4 * 3 * 130 * 40) + up(4 * 2 * 300 * 40)
    # the measured case: 32 user tiles -> 8 slices, 512 chunks -> one group; 1/32 of the 1.07 GB score matrix
    assert w(4096, 65536, 256, 1) == 4 * 8 * 4096 * 256 == 4096 * 65536 * 4 // 32


def _buf():
    b = ctypes.create_string_buffer(64)
    return b, ctypes.cast(b, ctypes.c_void_p)


def test_the_entry_points_refuse_on_the_host_before_any_launch():
    l = hip.lib()
    buf, p = _buf()
    need = l.xnrs_table_loss_workspace_bytes(3, 1000, 8, 1)
    fwd = lambda table=p, n=1000, E=8, up=p, B=3, off=p, rows=p, eo=None, er=None, lo=None, hi=None, out=p, ws=p, nb=need: \
        l.xnrs_table_loss_fwd(table, n, E, up, None, B, off, rows, eo, er, lo, hi, -1, out, out, out, ws, nb, None)  # noqa: E731
    bwd = lambda lo=None, hi=None, g=p, nb=need, B=3: \
        l.xnrs_table_loss_bwd(p, 1000, 8, p, None, B, p, p, None, None, lo, hi, -1, p, p, g, p, p, p, nb, None)  # noqa: E731
    for bad in (dict(n=-1), dict(n=2 ** 31), dict(E=0), dict(B=-1), dict(table=None), dict(up=None), dict(off=None), dict(rows=None),
                dict(eo=p), dict(out=None), dict(lo=p), dict(hi=p)):
        assert fwd(**bad) == EINVAL, bad
    assert fwd(nb=need - 1) == EWORKSPACE and fwd(ws=None) == EWORKSPACE
    assert bwd(lo=p) == EINVAL and bwd(hi=p) == EINVAL and bwd(g=None) == EINVAL and bwd(nb=need - 1) == EWORKSPACE
    # B == 0: nothing to do, whatever else is missing
    assert l.xnrs_table_loss_fwd(None, 1000, 8, None, None, 0, None, None, None, None, None, None, -1, None, None, None, None, 0,
                                 None) == 0
    assert l.xnrs_table_loss_bwd(None, 1000, 8, None, None, 0, None, None, None, None, None, None, -1, None, None, None, None,
                                 None, None, 0, None) == 0
    assert buf.raw == bytes(64)
