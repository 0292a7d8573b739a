"""CPU: the top-k reference on a hand-written case, the pure host calls of the top-k C ABI (slice count, workspace size,
refusals before any launch), and the Python surface that needs no device."""
import ctypes

import numpy as np
import pytest
import torch

from tests.topk_ref import topk_reference
from xnrs_amd import hip

EINVAL, EWORKSPACE = -1, -3


def test_reference_on_a_hand_written_case():
    nan, inf = float("nan"), float("inf")
    #                 0    1    2     3    4     5     6
    s = np.array([[1.0, 3.0, 3.0, nan, -inf, -0.0, 0.0],
                  [2.0, 2.0, nan, nan, 2.0, -inf, 5.0]], dtype=np.float32)
    rows, sc = topk_reference(s, 4)
    assert rows.tolist() == [[1, 2, 0, 5], [6, 0, 1, 4]]  # ties by row; -0 == +0 ties, row 5 before row 6
    assert sc[0].tolist() == [3.0, 3.0, 1.0, 0.0] and sc[1].tolist() == [5.0, 2.0, 2.0, 2.0]
    rows, sc = topk_reference(s, 7)  # six / five eligible rows: fillers behind the real -inf
    assert rows.tolist() == [[1, 2, 0, 5, 6, 4, -1], [6, 0, 1, 4, 5, -1, -1]]
    assert sc[0, 5] == -inf and sc[0, 6] == -inf and np.all(sc[1, 4:] == -inf)
    rows, _ = topk_reference(s, 3, excl=[[1, 1, 99, -4], [6, 0]], pad_row=2)  # duplicates and ids outside the table
    assert rows.tolist() == [[0, 5, 6], [1, 4, 5]]
    rows, _ = topk_reference(s[:1], 2, excl=[range(7)])
    assert rows.tolist() == [[-1, -1]]


def test_slices_and_workspace_are_pure_host_calls():
    l = hip.lib()
    assert hip._CONSTANTS["TOPK_MAX_K"] == 128
    assert l.xnrs_topk_slices(3, 1000) > 1
    for B in (1, 3, 130, 4096):
        assert l.xnrs_topk_slices(B, 100) == 1
        assert l.xnrs_topk_slices(B, 128) == 1
    assert l.xnrs_topk_slices(3, 129) == 2
    assert l.xnrs_topk_slices(0, 1000) == 1 and l.xnrs_topk_slices(5, 0) == 1
    # user tiles x slices fills the chip, and a slice is a whole number of 128-row chunks
    for B, N in ((1, 65536), (64, 65536), (4096, 65536), (130, 1000), (3, 2100)):
        s = l.xnrs_topk_slices(B, N)
        chunks = -(-N // 128)
        per = -(-chunks // s)
        assert 1 <= s <= chunks and (s - 1) * per < chunks <= s * per, (B, N, s)
    assert l.xnrs_topk_slices(4096, 65536) * 32 >= 256
    assert 1 < l.xnrs_topk_slices(1, 65536) <= 256 and 1 < l.xnrs_topk_slices(1, 2 ** 31 - 1) <= 256  # capped: the merge is serial
    w = l.xnrs_topk_workspace_bytes
    assert w(0, 1000, 0, 10) == 0 and w(0, 0, 64, 10) == 0
    assert w(3, 1000, 0, 10) >= l.xnrs_topk_slices(3, 1000) * 3 * 10 * 8
    assert w(6, 1000, 0, 10) > w(3, 1000, 0, 10)      # grows with B
    assert w(3, 1000, 0, 100) > w(3, 1000, 0, 10)     # ... with k
    assert w(3, 1000, 0, 10) > w(3, 100, 0, 10)       # ... with the slices
    assert w(3, 1000, 70, 10) > w(3, 1000, 0, 10)     # ... with the projected user side
    assert w(4096, 65536, 0, 100) < 4 * 4096 * 65536 // 10  # far below the score matrix it replaces


@pytest.mark.parametrize("k,E,outputs", [(0, 8, True), (129, 8, True), (-1, 8, True), (10, 0, True), (10, 8, False)])
def test_refusals_need_no_device(k, E, outputs):
    """Argument errors are found on the host before any launch: null device pointers never reach a kernel."""
    l = hip.lib()
    buf = ctypes.create_string_buffer(64)
    out = ctypes.cast(buf, ctypes.c_void_p) if outputs else None
    assert l.xnrs_topk(None, 1000, E, None, 3, None, None, -1, k, out, out, None, 0, None) == EINVAL
    assert l.xnrs_topk_bilinear(None, 1000, E, None, 3, None, None, None, None, -1, k, out, out, None, 0, None) == EINVAL
    assert l.xnrs_topk_mlp(None, 1000, E, max(E, 1), None, 3, None, None, None, None, None, None, -1, k, out, out, None, 0,
                           None) == EINVAL
    assert buf.raw == bytes(64)


def test_more_refusals_and_the_empty_batch():
    l = hip.lib()
    assert l.xnrs_topk(None, 2 ** 31, 8, None, 3, None, None, -1, 10, None, None, None, 0, None) == EINVAL
    assert l.xnrs_topk(None, -1, 8, None, 3, None, None, -1, 10, None, None, None, 0, None) == EINVAL
    assert l.xnrs_topk(None, 1000, 8, None, -1, None, None, -1, 10, None, None, None, 0, None) == EINVAL
    assert l.xnrs_topk_mlp(None, 1000, 8, 0, None, 3, None, None, None, None, None, None, -1, 10, None, None, None, 0, None) == EINVAL
    assert l.xnrs_topk(None, 1000, 8, None, 0, None, None, -1, 10, None, None, None, 0, None) == 0  # B == 0: nothing to do
    # valid arguments, no workspace: refused on the host as well (the pointers are never dereferenced there)
    one = ctypes.cast(ctypes.create_string_buffer(8), ctypes.c_void_p)
    assert l.xnrs_topk(one, 1000, 8, one, 3, None, None, -1, 10, one, one, None, 0, None) == EWORKSPACE
    assert l.xnrs_topk(one, 1000, 8, one, 3, None, None, -1, 10, one, one, one, 8, None) == EWORKSPACE


def test_scorers_have_topk_and_recommend_refuses_what_it_cannot_rank():
    from xnrs_amd import evaluation as EV
    from xnrs_amd import synth
    from xnrs_amd.models.blocks import BilinScoring, DotScoring, FCScoring
    from xnrs_amd.models.caum import CAUMScoring
    for cls in (DotScoring, BilinScoring, FCScoring):
        assert callable(getattr(cls, "topk"))
    assert CAUMScoring.topk is None

    class Cosine(torch.nn.Module):
        pass

    class Model(torch.nn.Module):
        def __init__(self, scorer):
            super().__init__()
            self.rec_model = scorer
    store, beh = synth.click_world(n_news=20, n_sess=5)
    with pytest.raises(NotImplementedError, match="Cosine"):
        EV.recommend(Model(Cosine()), store, beh, l_hist=8, k=5)
    with pytest.raises(NotImplementedError, match="CAUMScoring"):
        EV.recommend(Model(CAUMScoring()), store, beh, l_hist=8, k=5)
    npa_like = Model(DotScoring())
    npa_like.user_dependent_news = True
    with pytest.raises(NotImplementedError, match="depend on the user"):
        EV.recommend(npa_like, store, beh, l_hist=8, k=5)
