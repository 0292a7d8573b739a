"""CPU: the host side of the sampled top-k (include/xnrs_hip.h: xnrs_topk_sample*_win) -- the draw restated in
tests/sample_ref.py on fixed vectors and against the dropout stream it shares, the range of the Gumbel draw, the statistical
case of tests/test_hip_sample.py on the fp64 reference alone, the refusals of recommend_sampled and mined_negatives_loss that
need no device, and the C ABI's refusals before any launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import input_dropout_ref as DR
from tests import sample_ref as SR
from xnrs_amd import evaluation as EV
from xnrs_amd import hip, losses, ops, synth
from xnrs_amd.models.blocks import BilinScoring, DotScoring, FCScoring
from xnrs_amd.models.caum import CAUMScoring

EINVAL, EWORKSPACE = -1, -3


def _word(seed, key, row):
    """drop_word of kernels.h for ONE pair in Python integers (masks written out: nothing wraps by itself)."""
    M64, M32 = (1 << 64) - 1, (1 << 32) - 1
    z = (seed + 0x9E3779B97F4A7C15 * ((key + 1) & M64)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    x = (z & M32) ^ ((row * 0x9E3779B9) & M32)
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x ^ (z >> 32)


def test_the_word_is_the_dropout_stream_before_its_shift():
    for seed in DR.SEEDS + (0, -5):
        x = SR.draw_words(seed, np.arange(6), 50)
        assert x.dtype == np.uint32 and x.shape == (6, 50)
        # the uniform of xnrs_dropout_rows is (x >> 8) * 2^-24 of the same word: user key = row of the call, table row = element
        assert np.array_equal((x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24), DR.input_drop_uniform(seed, 6, 50))
        for key, row in ((0, 0), (5, 49), (3, 17)):
            assert int(x[key, row]) == _word(seed % (1 << 64), key, row)
    # keys are int64 session ids: any value, negative ones as two's complement; rows can be picked
    keys = np.array([2 ** 40 + 3, -1, -2 ** 63, 7], dtype=np.int64)
    x = SR.draw_words(99, keys, 2 ** 31 - 1, rows=[0, 12345, 2 ** 31 - 2])
    for i, key in enumerate(keys.tolist()):
        for j, row in enumerate((0, 12345, 2 ** 31 - 2)):
            assert int(x[i, j]) == _word(99, key % (1 << 64), row)
    assert np.array_equal(SR.draw_words(99, keys, 40)[:, 5:9], SR.draw_words(99, keys, 40, rows=[5, 6, 7, 8]))
    assert not np.array_equal(SR.draw_words(99, keys, 40), SR.draw_words(100, keys, 40))


def test_the_uniform_and_the_gumbel_draw_on_fixed_words():
    x = np.array([0, 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31, 2 ** 32 - 256, 2 ** 32 - 1], dtype=np.uint32)
    w = SR.uniform32(x)
    assert w.dtype == np.float32
    # x = 0: 2^-33, the relative precision of an fp32 towards 0; 2^24 + 1 rounds to 2^24 (the fp32 of a word holds 24 bits);
    # the top of the range is clamped to the last fp32 below 1
    want = [2.0 ** -33, 1.5 * 2.0 ** -32, 2.0 ** -8, 2.0 ** -8, 0.5, 1 - 2.0 ** -24, 1 - 2.0 ** -24]
    assert w.tolist() == want
    assert (w > 0).all() and (w < 1).all()
    g = SR.gumbel64(x)
    assert g[0] == pytest.approx(33 * math.log(2), abs=1e-9)            # -log(2^-33 (1 + 2^-34))
    assert g[2] == pytest.approx(-math.log(-math.log1p(-2.0 ** -8)), abs=1e-12)
    assert g[4] == pytest.approx(-math.log(math.log(2)), abs=1e-12)
    assert g[-1] == pytest.approx(-math.log(24 * math.log(2)), abs=1e-12)
    assert (np.diff(g) <= 0).all()                                       # g falls as the word grows
    # the bounds the header states, and the constant the kernel skips by: above every draw, with room for the logarithms' ulps
    assert SR.GUMBEL_MIN < g[-1] < SR.GUMBEL_MIN + 1e-4 and g[0] < SR.GUMBEL_MAX and SR.GUMBEL_MAX - g[0] > 50 * 2.0 ** -20
    assert float(np.float32(SR.GUMBEL_MAX)) > g[0]
    assert SR.GUMBEL_MAX - SR.GUMBEL_MIN < 26  # what the cold-limit test leans on
    # the bound the kernel tries before it takes a logarithm: above the draw by more than the logarithms' ulps (2e-6 each) for
    # every exponent of w -- at both ends of each binade and on random words -- and never more than log(2) + 1 above -log(w)
    edges = [0] + [v for e in range(1, 33) for v in (2 ** e - 1, 2 ** e, 2 ** e + 1)]
    xs = np.concatenate([np.array(edges, dtype=np.uint64) % 2 ** 32, synth.rng_for(5).integers(0, 2 ** 32, size=200000, dtype=np.uint64)])
    xs = xs.astype(np.uint32)
    b, g64 = SR.gumbel_bound32(xs).astype(np.float64), SR.gumbel64(xs)
    assert b.dtype == np.float64 and (b - g64 >= 5e-5).all() and (b <= -np.log(SR.uniform32(xs).astype(np.float64)) + math.log(2) + 2e-4).all()
    assert SR.gumbel_bound32(np.array([0], dtype=np.uint32))[0] == pytest.approx(33 * math.log(2) + 1e-4, abs=1e-5)
    assert SR.gumbel_bound32(np.array([2 ** 32 - 1], dtype=np.uint32))[0] == pytest.approx(math.log(2) + 1e-4, abs=1e-6)


def test_keys_tolerance_and_validator_on_a_small_case():
    rng = synth.rng_for(4242)
    s = rng.standard_normal((4, 30))
    s[1, 3], s[2, 14], s[3, 5] = np.nan, -np.inf, np.inf
    keys = SR.keys64(s, 0.5, 7, np.arange(4))
    assert np.isnan(keys[1, 3]) and np.isneginf(keys[2, 14]) and np.isposinf(keys[3, 5])
    g = SR.gumbel64(SR.draw_words(7, np.arange(4), 30))
    assert np.allclose(keys[0], s[0] / 0.5 + g[0], rtol=0, atol=0)
    ok = SR.eligible_mask(4, 30, excl=[[0, 1], [], [29, 77, -3], [5]], pad_row=2, win=([0, 0, 10, 0], [30, 0, 40, 30]))
    assert not ok[:, 2].any() and not ok[0, :2].any() and not ok[1].any() and ok[2].sum() == 19 and not ok[3, 5]
    tol = SR.tolerance(keys, ok)
    assert tol == 32 * 2.0 ** -23 * np.abs(keys[ok & np.isfinite(keys)]).max()
    k = 25
    rows = SR.reference_lists(keys, ok, k)
    dev_keys = np.where(rows >= 0, np.take_along_axis(keys, np.maximum(rows, 0), axis=1), -np.inf).astype(np.float32)
    worst = SR.check_sampled_topk(rows.astype(np.int32), dev_keys, keys, ok, k, tol)
    assert worst <= tol / 8 and (rows[1] == -1).all() and (rows[2, 19:] == -1).all() and rows[2, 18] == 14  # -inf: last real place
    # the validator refuses: an ineligible row, a wrong order, a key off by more than tol, a better row left out
    bad = rows.astype(np.int32).copy()
    bad[0, 0] = 2
    with pytest.raises(AssertionError):
        SR.check_sampled_topk(bad, dev_keys, keys, ok, k, tol)
    swapped = rows.astype(np.int32).copy()
    swapped[0, [0, 1]] = swapped[0, [1, 0]]
    with pytest.raises(AssertionError):
        SR.check_sampled_topk(swapped, dev_keys, keys, ok, k, tol)
    off = dev_keys.copy()
    off[0, 0] += np.float32(4 * tol)
    with pytest.raises(AssertionError):
        SR.check_sampled_topk(rows.astype(np.int32), off, keys, ok, k, tol)
    r5 = rows[:, :5].astype(np.int32).copy()
    k5 = dev_keys[:, :5].copy()
    r5[0, 4], k5[0, 4] = rows[0, 9], dev_keys[0, 9]
    with pytest.raises(AssertionError):
        SR.check_sampled_topk(r5, k5, keys, ok, 5, tol)


@pytest.mark.parametrize("tau", [0.5, 2.0])
def test_the_reference_draws_plackett_luce_inside_four_sigma(tau):
    """The statistical case of the GPU test on the fp64 reference alone: 8 rows, 8192 identical users with the keys 0 .. 8191,
    seed 1234.  The device's bar is 5 sigma; the reference has to sit inside 4 so that the bar has room."""
    scores = SR.PL_SCORES
    n = 8192
    keys = SR.keys64(np.tile(scores, (n, 1)), tau, 1234, np.arange(n))
    rows = SR.reference_lists(keys, np.ones((n, 8), dtype=bool), 2)
    z1, z2 = SR.worst_sigma(rows, scores, tau)
    print(f"tau {tau}: first places within {z1:.2f} sigma, ordered pairs within {z2:.2f} sigma")
    assert z1 <= 4 and z2 <= 4
    p1, p2 = SR.plackett_luce_first_two(scores, tau)
    assert p1.sum() == pytest.approx(1) and p2.sum() == pytest.approx(1) and n * p2[p2 > 0].min() > 20  # every cell is populated


class _Model(torch.nn.Module):
    def __init__(self, scorer):
        super().__init__()
        self.rec_model = scorer

    def encode_news_ids(self, store, ids):
        raise AssertionError("refused before anything is encoded")

    def encode_user(self, *a):
        raise AssertionError("refused before anything is encoded")


def test_recommend_sampled_refuses_before_anything_is_encoded():
    for cls in (DotScoring, BilinScoring, FCScoring):
        assert callable(cls.topk_sample)
    assert CAUMScoring.topk_sample is None
    store, beh = synth.click_world(n_news=20, n_sess=5)
    call = lambda m, k=5, t=1.0, **kw: EV.recommend_sampled(m, store, beh, 8, k, t, 3, **kw)  # noqa: E731
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), None, "1", True):
        with pytest.raises(ValueError, match="temperature"):
            call(_Model(DotScoring()), t=bad)
    with pytest.raises(ValueError, match="1024"):
        call(_Model(DotScoring()), k=1025)

    class Cosine(torch.nn.Module):
        prepare_csr = topk = topk_deep = score_csr = staticmethod(lambda *a, **k: None)
    with pytest.raises(NotImplementedError, match="Cosine"):
        call(_Model(Cosine()))
    with pytest.raises(NotImplementedError, match="CAUMScoring"):
        call(_Model(CAUMScoring()))
    npa_like = _Model(DotScoring())
    npa_like.user_dependent_news = True
    with pytest.raises(NotImplementedError, match="depend on the user"):
        call(npa_like)
    with pytest.raises(NotImplementedError, match="generator"):
        call(_Model(DotScoring()), generator=_Model(DotScoring()))
    from xnrs_amd.models.caum import CAUM
    caum = CAUM.__new__(CAUM)
    torch.nn.Module.__init__(caum)
    caum.rec_model = DotScoring()
    with pytest.raises(NotImplementedError, match="CAUM"):
        call(caum)
    lstur_like = _Model(DotScoring())
    lstur_like.uses_user_index = True
    with pytest.raises(ValueError, match="user index"):
        call(lstur_like)

    class NoWindows(DotScoring):
        def topk_sample(self, table, u, k, temperature, seed, user_keys=None, excl_off=None, excl_rows=None, pad_row=-1):
            raise AssertionError("not reached")
    win = (torch.zeros(5, dtype=torch.int32), torch.full((5,), 20, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="row windows"):
        call(_Model(NoWindows()), windows=win)
    with pytest.raises(ValueError, match="windows"):
        call(_Model(DotScoring()), windows=(win[0][:3], win[1]))


def test_mined_negatives_loss_checks_temperature_and_seed_before_anything_is_encoded():
    store, beh = synth.click_world(n_news=20, n_sess=5)
    call = lambda m, **k: losses.mined_negatives_loss(m, store, beh, [0, 1], l_hist=8, **k)  # noqa: E731
    for bad in (0, -0.5, float("inf"), float("nan"), "hot", True):
        with pytest.raises(ValueError, match="temperature"):
            call(_Model(DotScoring()), temperature=bad, seed=1)
    for bad in (None, 1.5, "7", True):
        with pytest.raises(ValueError, match="seed"):
            call(_Model(DotScoring()), temperature=0.5, seed=bad)
    with pytest.raises(ValueError, match="without a temperature"):
        call(_Model(DotScoring()), seed=3)

    class Old(DotScoring):
        topk_sample = None
    with pytest.raises(NotImplementedError, match="topk_sample"):
        call(_Model(Old()), temperature=0.5, seed=1)
    # the refusals of the existing call still come first
    with pytest.raises(NotImplementedError, match="FCScoring"):
        call(_Model(FCScoring(4, 8)), temperature=0.5, seed=1)
    with pytest.raises(ValueError, match="n_negatives"):
        call(_Model(DotScoring()), n_negatives=0, temperature=0.5, seed=1)


class _Stub:
    def __init__(self, rows):
        self.rows, self.calls = rows, []

    def topk_deep(self, table, u, k, excl_off=None, excl_rows=None, pad_row=-1, win_lo=None, win_hi=None):
        self.calls.append(("deep", k))
        return self.rows[:, :k], None

    def topk_sample(self, table, u, k, temperature, seed, user_keys=None, excl_off=None, excl_rows=None, pad_row=-1, win_lo=None,
                    win_hi=None):
        assert not torch.is_grad_enabled() and not table.requires_grad and not u.requires_grad
        self.calls.append(("sample", k, temperature, seed, user_keys, excl_off.tolist(), excl_rows.tolist(), pad_row, win_lo, win_hi))
        return self.rows[:, :k], None

    def list_loss(self, table, u, tgt_off, tgt_rows, neg_rows, pad_row=-1):
        self.calls.append(("list", neg_rows))
        return torch.ones(3, requires_grad=True), torch.zeros(3), None, None


def test_mine_and_rank_draws_through_topk_sample_with_the_minings_arguments():
    rows = torch.arange(12, dtype=torch.int32).reshape(2, 6)
    stub = _Stub(rows)
    table, u = torch.zeros((20, 4), requires_grad=True), torch.zeros((2, 4), requires_grad=True)
    hist = (torch.tensor([0, 2, 3]), torch.tensor([5, 3, 9], dtype=torch.int32))
    tgt = (torch.tensor([0, 1, 3]), torch.tensor([7, 8, 2], dtype=torch.int32))
    keys = torch.tensor([40, 41])
    lo, hi = torch.tensor([0, 5], dtype=torch.int32), torch.tensor([10, 20], dtype=torch.int32)
    _, used = losses.mine_and_rank(stub, table, u, hist, tgt, 11, 4, (lo, hi), "mean", None, True, 0.25, 9, keys)
    assert stub.calls[0][:4] == ("sample", 4, 0.25, 9) and stub.calls[0][4] is keys
    assert stub.calls[0][5:8] == ([0, 3, 6], [5, 3, 7, 9, 8, 2], 11) and stub.calls[0][8] is lo and stub.calls[0][9] is hi
    assert stub.calls[1][0] == "list" and torch.equal(stub.calls[1][1], rows[:, :4]) and torch.equal(used, rows[:, :4])
    # no temperature: the existing call, and nothing else
    losses.mine_and_rank(stub, table, u, hist, tgt, 11, 4)
    assert stub.calls[2] == ("deep", 4)


def test_the_binding_and_the_ops_refuse_before_the_device():
    c = hip.parse_header(open(hip.HEADER_PATH).read())
    assert c[0]["ABI_VERSION"] == 6  # new entry points only
    twins = {"xnrs_topk_sample_win": "xnrs_topk_deep_win", "xnrs_topk_sample_bilinear_win": "xnrs_topk_deep_bilinear_win",
             "xnrs_topk_sample_mlp_win": "xnrs_topk_deep_mlp_win"}
    for name, twin in twins.items():
        args, targs = c[2][name][1], c[2][twin][1]
        # the twin's list with (float temperature, uint64 seed, const int64* user_keys) behind k
        assert args[:-5] == targs[:-5] + [ctypes.c_float, ctypes.c_uint64, ctypes.c_void_p] and args[-5:] == targs[-5:], name
    table, u = torch.zeros((10, 4)), torch.zeros((3, 4))
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            ops._noise(bad, 1, None, 3, table.device)
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), [0, 1, 2]):
        with pytest.raises(ValueError, match="user_keys"):
            ops._noise(1.0, 1, bad, 3, table.device)
    assert ops._noise(0.5, -1, None, 3, table.device)[:2] == (0.5, 2 ** 64 - 1)
    with pytest.raises(hip.XnrsHipError, match="cpu"):  # everything well-formed: the only thing missing is the device
        ops.topk_sample_dot(table, u, 2, 1.0, 0)


def test_the_entry_points_refuse_on_the_host_before_any_launch():
    l = hip.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 40
    dot = lambda t=1.0, k=10, lo=p, hi=p, nb=big, B=3, rows=p: \
        l.xnrs_topk_sample_win(p, 1000, 8, p, B, None, None, lo, hi, -1, k, t, 7, None, rows, p, p, nb, None)  # noqa: E731
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1e-45):
        assert dot(t=bad) == EINVAL, bad
        assert l.xnrs_topk_sample_bilinear_win(p, 1000, 8, p, 3, p, p, None, None, None, None, -1, 10, bad, 7, p, p, p, p, big,
                                               None) == EINVAL
        assert l.xnrs_topk_sample_mlp_win(p, 1000, 8, 8, p, 3, p, p, p, p, None, None, None, None, -1, 10, bad, 7, p, p, p, p, big,
                                          None) == EINVAL
        assert dot(t=bad, B=0) == EINVAL  # (a bad temperature is refused even where nothing would run)
    assert dot(k=0) == EINVAL and dot(k=1025) == EINVAL and dot(lo=None) == EINVAL and dot(hi=None) == EINVAL and dot(rows=None) == EINVAL
    need = l.xnrs_topk_deep_workspace_bytes(3, 1000, 0, 300)
    assert need > 0 and dot(k=300, nb=need - 1) == EWORKSPACE
    assert l.xnrs_topk_sample_win(None, 1000, 8, None, 0, None, None, None, None, -1, 10, 1.0, 7, None, None, None, None, 0, None) == 0
    assert buf.raw == bytes(64)
