"""CPU: what the soft-target loss does around its kernels -- the refusals of distillation_loss raised before anything is
encoded (stub models), the targets built from teacher scores, the operands ops.list_xent refuses before the device, the C
ABI's argument and workspace checks, and list_recall."""
import ctypes

import pytest
import torch

from xnrs_amd import evaluation, hip, losses, ops, synth
from xnrs_amd.models.blocks import BilinScoring, DotScoring, FCScoring
from xnrs_amd.models.caum import CAUMScoring

EINVAL, EWORKSPACE = -1, -3


class _Model(torch.nn.Module):
    def __init__(self, scorer):
        super().__init__()
        self.rec_model = scorer

    def encode_news_ids(self, store, ids):
        raise AssertionError("refused before anything is encoded")

    def encode_user(self, *a):
        raise AssertionError("refused before anything is encoded")


def test_scorer_classes():
    assert callable(DotScoring.list_xent) and callable(BilinScoring.list_xent)
    assert not hasattr(FCScoring, "list_xent") and not callable(getattr(CAUMScoring, "list_xent", None))
    assert not hasattr(FCScoring, "list_loss") and not hasattr(FCScoring, "table_loss")
    table, u = torch.zeros((10, 4)), torch.zeros((2, 4))
    rows, w = torch.zeros((2, 3), dtype=torch.int32), torch.zeros((2, 3))

    class Cosine(torch.nn.Module):
        pass
    for scorer in (FCScoring(4, 8), Cosine(), CAUMScoring()):
        with pytest.raises(NotImplementedError, match=type(scorer).__name__):
            losses.listed_soft_target_loss(scorer, table, u, rows, w)
    for scorer in (DotScoring(normalize=True), BilinScoring(4, normalize=True)):
        with pytest.raises(NotImplementedError, match="normalize=True"):
            losses.listed_soft_target_loss(scorer, table, u, rows, w)
    with pytest.raises(ValueError, match="reduction"):
        losses.listed_soft_target_loss(DotScoring(), table, u, rows, w, reduction="max")


def test_refusals_come_before_anything_is_encoded():
    store, beh = synth.click_world(n_news=20, n_sess=5)
    teacher = _Model(DotScoring())
    npa_like = _Model(DotScoring())
    npa_like.user_dependent_news = True
    lstur_like = _Model(DotScoring())
    lstur_like.uses_user_index = True
    call = lambda s, t=teacher, table=store, **k: losses.distillation_loss(s, t, table, beh, [0, 1], l_hist=8, **k)  # noqa: E731
    good = _Model(DotScoring())
    # the student: everything the mined-negatives loss refuses, worded for this loss
    with pytest.raises(NotImplementedError, match="FCScoring.*list_xent"):
        call(_Model(FCScoring(4, 8)))
    with pytest.raises(NotImplementedError, match="CAUMScoring"):
        call(_Model(CAUMScoring()))
    with pytest.raises(NotImplementedError, match=r"normalize=True\) has no soft-target loss"):
        call(_Model(DotScoring(normalize=True)))
    with pytest.raises(NotImplementedError, match=r"distillation_loss\(\).*depend on the user"):
        call(npa_like)
    with pytest.raises(ValueError, match="user index"):
        call(lstur_like)
    with pytest.raises(ValueError, match="reduction"):
        call(good, reduction="median")
    # the teacher: CAUM has no user vector of its own and no score_impressions; an NPA-like one without the hook neither
    with pytest.raises(NotImplementedError, match="teacher _Model"):
        call(good, _Model(CAUMScoring()))
    with pytest.raises(NotImplementedError, match="teacher _Model"):
        call(good, npa_like)
    with pytest.raises(ValueError, match="teacher .* user index"):
        call(good, lstur_like)
    npa_like.score_impressions = lambda *a, **k: None
    with pytest.raises(ValueError, match="teacher .* user index"):  # (this world's sessions carry no user index)
        call(good, npa_like)
    for bad in (0, -1.0, float("inf"), float("nan"), True, "1", None):
        with pytest.raises(ValueError, match="temperature"):
            call(good, temperature=bad)
    for bad in (0, -1, 1025, 2.5, True):
        with pytest.raises(ValueError, match="pool"):
            call(good, pool=bad)
    for bad in (torch.zeros((3, 4), dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int64), torch.zeros((8,), dtype=torch.int32),
                [[1, 2], [3, 4]]):
        with pytest.raises(ValueError, match="rows is a"):
            call(good, rows=bad)
    with pytest.raises(ValueError, match="store="):
        call(good, table=(torch.zeros((21, 4)), torch.ones((21, 1))))


def test_soft_targets_are_a_softmax_over_the_filled_slots():
    t = torch.tensor([[1.0, 3.0, -2.0, 0.5], [200.0, -300.0, 100.0, 0.0], [5.0, 5.0, 5.0, 5.0]])
    filled = torch.tensor([[True, False, True, True], [True, True, False, True], [False, False, False, False]])
    w, h = losses.soft_targets(t, filled, 2.0)
    want = torch.softmax((t.double() / 2.0).masked_fill(~filled, float("-inf")), dim=1)
    assert torch.isfinite(w).all() and torch.isfinite(h).all() and w.dtype == torch.float32
    assert (w[~filled] == 0).all() and (w[2] == 0).all() and h[2].item() == 0
    assert torch.allclose(w[:2].double(), want[:2], rtol=1e-6, atol=1e-12)
    assert torch.allclose(w[:2].sum(dim=1), torch.ones(2), atol=1e-6)
    ent = -(want[:2] * torch.where(want[:2] > 0, want[:2].log(), torch.zeros(()).double())).sum(dim=1)
    assert torch.allclose(h[:2].double(), ent, rtol=1e-5, atol=1e-7)


def test_operand_checks_come_before_the_device():
    table, u = torch.zeros((10, 4)), torch.zeros((3, 1, 4))
    rows, w = torch.zeros((3, 5), dtype=torch.int32), torch.zeros((3, 5))
    for bad in (rows.long(), rows[:2], rows.reshape(-1), None):
        with pytest.raises(RuntimeError, match="row lists"):
            ops.list_xent(table, u, bad, w)
    for bad in (w.double(), w[:, :4], w.reshape(-1), None):
        with pytest.raises(RuntimeError, match="slot weights"):
            ops.list_xent(table, u, rows, bad)
    with pytest.raises(RuntimeError, match="news vectors"):
        ops.list_xent(table[0], u, rows, w)
    with pytest.raises(RuntimeError, match="user vectors"):
        ops.list_xent(table, torch.zeros((3, 5)), rows, w)
    with pytest.raises(hip.XnrsHipError, match="cpu"):  # everything well-formed: the only thing missing is the device
        ops.list_xent(table, u, rows, w)


def test_order_is_the_list_loss_order_without_queries():
    nan = float("nan")
    rows = torch.tensor([[4, -1, 2], [2, 9, 4]], dtype=torch.int32)
    slot_scores = torch.tensor([[0.5, nan, 0.1], [0.2, nan, 0.3]])
    order = ops.list_xent_order(9, rows, slot_scores)
    assert order.dtype == torch.int32 and order.tolist() == [2, 3, 0, 5, 1, 4]  # rows 2 2 4 4, then the empty slots


def test_workspace_is_a_pure_host_call_and_follows_its_formula():
    w = hip.lib().xnrs_list_xent_workspace_bytes
    up = lambda x: -(-x // 256) * 256  # noqa: E731
    assert w(5, 65, 260, 0) == 0 and w(-1, 8, 8, 1) == 0 and w(4, -1, 8, 1) == 0 and w(4, 8, 0, 1) == 0
    for B, L, E in ((5, 65, 260), (1, 1, 4), (3, 0, 8), (70, 130, 32), (4096, 128, 256), (4096, 1024, 256)):
        G = max(1, min(8192, -(-B * L // 64)))  # one span per 64 slots
        assert w(B, L, E, 1) == up(4 * B) + 2 * up(4 * G * E) + 2 * up(4 * G), (B, L, E)
    assert w(4096, 128, 256, 1) <= 4096 * 128 * 256 * 4 // 32 + 3 * 65536  # 1/32 of the copy of the listed rows


def test_the_entry_points_refuse_on_the_host_before_any_launch():
    l = hip.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = l.xnrs_list_xent_workspace_bytes(3, 5, 8, 1)
    fwd = lambda table=p, n=1000, E=8, up=p, B=3, rows=p, w=p, L=5, loss=p, lse=p, ss=p: \
        l.xnrs_list_xent_fwd(table, n, E, up, None, B, rows, w, L, -1, loss, lse, ss, None, 0, None)  # noqa: E731
    bwd = lambda g=p, order=p, d_table=p, nb=need, ws=p, L=5, B=3, E=8, lse=p, rows=p, w=p, ss=p: \
        l.xnrs_list_xent_bwd(p, 1000, E, p, None, B, rows, w, L, -1, lse, ss, g, order, p, d_table, ws, nb, None)  # noqa: E731
    for bad in (dict(n=-1), dict(n=2 ** 31), dict(E=0), dict(B=-1), dict(L=-1), dict(table=None), dict(up=None), dict(rows=None),
                dict(w=None), dict(loss=None), dict(lse=None), dict(ss=None), dict(B=2 ** 26, L=64)):
        assert fwd(**bad) == EINVAL, bad
    for bad in (dict(g=None), dict(L=-1), dict(E=0), dict(order=None), dict(d_table=None), dict(lse=None), dict(rows=None),
                dict(w=None), dict(ss=None), dict(B=2 ** 26, L=64)):
        assert bwd(**bad) == EINVAL, bad
    assert bwd(nb=need - 1) == EWORKSPACE and bwd(ws=None) == EWORKSPACE
    # B == 0: nothing to do, whatever else is missing
    assert l.xnrs_list_xent_fwd(None, 1000, 8, None, None, 0, None, None, 5, -1, None, None, None, None, 0, None) == 0
    assert l.xnrs_list_xent_bwd(None, 1000, 8, None, None, 0, None, None, 5, -1, None, None, None, None, None, None, None, 0,
                                None) == 0
    assert buf.raw == bytes(64)


def test_list_recall_against_a_loop():
    g = torch.Generator().manual_seed(5)
    n, P, k = 37, 12, 5
    found = torch.randint(-1, 30, (n, P), generator=g).to(torch.int32)
    wanted = torch.randint(-1, 30, (n, k), generator=g).to(torch.int32)
    wanted[3] = -1  # nothing wanted
    found[4] = -1   # nothing found
    wanted[5, :2] = wanted[5, 2]  # a row wanted twice counts twice
    got = evaluation.list_recall(found, wanted)
    assert got.shape == (n,) and got.dtype == torch.float32
    for i in range(n):
        want = [r for r in wanted[i].tolist() if r >= 0]
        have = set(found[i].tolist())
        assert got[i].item() == pytest.approx(sum(r in have for r in want) / max(len(want), 1), abs=1e-6), i
    assert got[3].item() == 0 and got[4].item() == 0
    old = evaluation.LIST_RECALL_CHUNK
    evaluation.LIST_RECALL_CHUNK = 4 * P * k  # four sessions per chunk, a ragged last one
    try:
        assert torch.equal(evaluation.list_recall(found, wanted), got)
    finally:
        evaluation.LIST_RECALL_CHUNK = old
    with pytest.raises(ValueError, match="list_recall"):
        evaluation.list_recall(found, wanted[:5])
