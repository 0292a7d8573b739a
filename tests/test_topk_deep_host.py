"""CPU: the pure host side of deep top-k (include/xnrs_hip.h: xnrs_topk_deep*) -- the constant, refusals before any launch,
the workspace query -- and the refusals of evaluation.recommend that need no device."""
import ctypes

import pytest
import torch

from xnrs_amd import hip

EINVAL = -1


def test_the_constants():
    assert hip._CONSTANTS["TOPK_DEEP_MAX_K"] == 1024
    assert hip._CONSTANTS["TOPK_MAX_K"] == 128


@pytest.mark.parametrize("k,E,outputs", [(0, 8, True), (-1, 8, True), (1025, 8, True), (10, 0, True), (300, 8, False)])
def test_refusals_need_no_device(k, E, outputs):
    l = hip.lib()
    buf = ctypes.create_string_buffer(64)
    out = ctypes.cast(buf, ctypes.c_void_p) if outputs else None
    assert l.xnrs_topk_deep(None, 1000, E, None, 3, None, None, -1, k, out, out, None, 0, None) == EINVAL
    assert l.xnrs_topk_deep_bilinear(None, 1000, E, None, 3, None, None, None, None, -1, k, out, out, None, 0, None) == EINVAL
    assert l.xnrs_topk_deep_mlp(None, 1000, E, max(E, 1), None, 3, None, None, None, None, None, None, -1, k, out, out, None, 0,
                                None) == EINVAL
    assert buf.raw == bytes(64)


def test_the_old_entry_points_keep_their_limit():
    l = hip.lib()
    assert l.xnrs_topk(None, 1000, 8, None, 3, None, None, -1, 129, None, None, None, 0, None) == EINVAL
    assert l.xnrs_topk_workspace_bytes(3, 1000, 0, 129) == 0
    # valid deep arguments, no workspace: refused on the host (the pointers are never dereferenced there)
    one = ctypes.cast(ctypes.create_string_buffer(8), ctypes.c_void_p)
    assert l.xnrs_topk_deep(one, 1000, 8, one, 3, None, None, -1, 1024, one, one, None, 0, None) == -3  # XNRS_EWORKSPACE
    assert l.xnrs_topk_deep(None, 1000, 8, None, 0, None, None, -1, 1024, None, None, None, 0, None) == 0  # B == 0


def test_the_workspace_query():
    l = hip.lib()
    w = l.xnrs_topk_deep_workspace_bytes
    assert w(3, 1000, 0, 0) == 0 and w(3, 1000, 0, 1025) == 0 and w(0, 1000, 0, 300) == 0
    ks = (1, 10, 128, 129, 256, 300, 1000, 1024)
    for B, N, pw in ((3, 1000, 0), (130, 40000, 64), (4096, 65536, 256)):
        sizes = [w(B, N, pw, k) for k in ks]
        assert all(a > 0 for a in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]  # monotone in k
        assert w(B, N, pw, 1024) >= l.xnrs_topk_slices(B, N) * B * 1024 * 8
        for k in (1, 10, 128):
            assert w(B, N, pw, k) == l.xnrs_topk_workspace_bytes(B, N, pw, k)
    # n_rows counts through the slice count alone
    assert l.xnrs_topk_slices(4096, 65536) == l.xnrs_topk_slices(4096, 60000)
    assert w(4096, 65536, 0, 1024) == w(4096, 60000, 0, 1024)
    assert l.xnrs_topk_slices(1, 65536) == l.xnrs_topk_slices(1, 2 ** 31 - 1) and w(1, 65536, 0, 1024) == w(1, 2 ** 31 - 1, 0, 1024)
    assert w(4096, 65536, 0, 1024) < 4096 * 65536 * 4  # below the score matrix


def test_recommend_refuses_before_anything_is_encoded():
    from xnrs_amd import evaluation as EV
    from xnrs_amd import synth
    from xnrs_amd.models.blocks import BilinScoring, DotScoring, FCScoring
    from xnrs_amd.models.caum import CAUMScoring
    for cls in (DotScoring, BilinScoring, FCScoring):
        assert callable(getattr(cls, "topk_deep"))

    class Model(torch.nn.Module):  # (no news encoder: encoding it would raise AttributeError, not the refusal)
        def __init__(self, scorer):
            super().__init__()
            self.rec_model = scorer

    class ShallowOnly(torch.nn.Module):
        prepare_csr = topk = staticmethod(lambda *a, **k: None)

    class NPALike(Model):
        user_dependent_news = True

        def score_impressions(self, *a, **k):
            raise AssertionError("nothing is scored before the refusals")

    store, beh = synth.click_world(n_news=20, n_sess=5)
    gen, npa = Model(DotScoring()), NPALike(DotScoring())
    with pytest.raises(ValueError, match="1024"):
        EV.recommend(gen, store, beh, l_hist=8, k=2000)
    with pytest.raises(ValueError, match="1024"):
        EV.recommend(npa, store, beh, l_hist=8, k=2000, generator=gen)
    with pytest.raises(NotImplementedError, match="128"):
        EV.recommend(Model(ShallowOnly()), store, beh, l_hist=8, k=200)
    with pytest.raises(ValueError, match="pool"):
        EV.recommend(npa, store, beh, l_hist=8, k=20, generator=gen, pool=19)
    with pytest.raises(ValueError, match="pool"):
        EV.recommend(npa, store, beh, l_hist=8, k=20, generator=gen, pool=1025)
    with pytest.raises(ValueError, match="pool"):
        EV.recommend(gen, store, beh, l_hist=8, k=20, pool=100)
    with pytest.raises(NotImplementedError, match="depend on the user"):
        EV.recommend(npa, store, beh, l_hist=8, k=5, generator=NPALike(DotScoring()))
    with pytest.raises(NotImplementedError, match="generator"):  # alone, the message names the two-stage form
        EV.recommend(npa, store, beh, l_hist=8, k=5)
    with pytest.raises(NotImplementedError, match="CAUMScoring"):
        EV.recommend(npa, store, beh, l_hist=8, k=5, generator=Model(CAUMScoring()))
    with pytest.raises(NotImplementedError, match="score_impressions"):  # a table-ranking model (CAUM too) is no second stage
        EV.recommend(Model(CAUMScoring()), store, beh, l_hist=8, k=5, generator=gen)
    assert getattr(beh, "user_index", None) is None
    with pytest.raises(ValueError, match="user index"):
        EV.recommend(npa, store, beh, l_hist=8, k=5, generator=gen)
