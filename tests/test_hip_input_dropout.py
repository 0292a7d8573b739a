"""GPU: the towers' input dropout on the HIP path (xnrs_dropout_rows; ops.gather_dropout / ops.input_dropout; the id path
of TextEncoder / NAML / NPA in train mode with p_dropout > 0; the hip_dropout opt-in of the dense towers).

The kernel's draw is restated in integer numpy (tests/input_dropout_ref.py, held to the attention dropout's oracle in
tests/test_input_dropout_host.py), so every kernel result is compared BIT FOR BIT: a kept element is one fp32 rounding.
The encoders are compared with a twin without input dropout that runs the dense entry points on the restated dropped rows
(the same kernels on the same numbers) and with the fp64 oracle on those rows, at the project's bars (H.RTOL, GTOL).

Observed on an MI355X: see the docstrings of the id-path tests.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import xnrs_oracle as O
from tests import helpers as H
from tests import input_dropout_ref as R
from tests.golden import cases
from tests.test_hip_attention_dropout import f64, fc2_bias_bar, grad_excess
from tests.test_hip_grads import GTOL, load
from xnrs_amd import hip, ops, synth
from xnrs_amd.models import make_model
from xnrs_amd.models.components import layers, news_encoding, user_encoding

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = R.SEEDS[0]
EINVAL = hip._CONSTANTS["EINVAL"]


class Cfg(dict):
    __getattr__ = dict.__getitem__


# ------------------------------------------------------------------------------------------------ the kernel, bit for bit
def launch(x, ids, out, p, seed, word=None, n=None, row_floats=None):
    """xnrs_dropout_rows as the header declares it -> return code."""
    n = out.shape[0] if n is None else n
    row_floats = (out[0].numel() if out.shape[0] else 1) if row_floats is None else row_floats
    return hip.lib().xnrs_dropout_rows(hip.ptr(x), hip.ptr(ids), hip.ptr(out), n, row_floats, p, int(seed) % 2 ** 64,
                                       hip.ptr(word), hip.stream_ptr(torch.device(DEV)))


@functools.lru_cache(maxsize=None)
def table(n_tab, row_floats):
    """Seeded rows without zeros (so a dropped element is told from a kept one)."""
    x = synth.rng_for(9100 + 7 * n_tab + row_floats).standard_normal((n_tab, row_floats)).astype(np.float32)
    x[x == 0] = 1
    return x


def make_ids(kind, n, n_tab):
    rng = synth.rng_for(9200 + n)
    if kind == "perm":
        return rng.permutation(n_tab)[:n].astype(np.int32)
    ids = rng.integers(0, min(3, n_tab), size=n).astype(np.int32)  # repeats of rows 0..2
    ids[0] = 0
    if n > 1:
        ids[-1] = ids[0]  # row 0 at least twice
    return ids


# (n, row_floats): smallest; scalar path; vector path; vector path across the 1 024-f32x4 piece boundary; scalar path across the
# 4 096-float piece boundary; more workgroups than one wave of the grid
SHAPES = [(1, 1), (3, 20), (7, 600), (4, 4120), (3, 4099), (3000, 32)]


@pytest.mark.parametrize("kind", ["dense", "perm", "repeats"])
@pytest.mark.parametrize("n,rf", SHAPES)
def test_kernel_equals_the_restatement_bit_for_bit(n, rf, kind):
    """p in {0, 0.1, 0.5, 1}: out == dropped(x[src], p, seed) with torch.equal; p = 0 is xnrs_gather_rows (or a copy), p = 1
    all zeros; two occurrences of one table row carry different masks (the draw is by position in the call)."""
    n_tab = n if kind == "dense" else n + 3
    tab = table(n_tab, rf)
    ids = None if kind == "dense" else make_ids(kind, n, n_tab)
    src = tab if ids is None else tab[ids]
    x_d = torch.from_numpy(tab).to(DEV)
    ids_d = None if ids is None else torch.from_numpy(ids).to(DEV)
    for p in (0.0, 0.1, 0.5, 1.0):
        out = torch.full((n, rf), float("nan"), device=DEV)
        assert launch(x_d, ids_d, out, p, SEED) == 0
        assert torch.equal(out.cpu(), torch.from_numpy(R.dropped(src, p, SEED))), (n, rf, kind, p)
        if p == 0.0 and ids is not None:
            g = torch.empty_like(out)
            hip.check(hip.lib().xnrs_gather_rows(hip.ptr(x_d), hip.ptr(ids_d), hip.ptr(g), n, rf, hip.stream_ptr(torch.device(DEV))), "gather")
            assert torch.equal(out, g)
        if p == 1.0:
            assert not out.any()
        if p == 0.5 and kind == "repeats" and n > 1 and rf >= 20:
            o = out.cpu().numpy()
            assert ids[0] == ids[-1] and not np.array_equal(o[0] != 0, o[-1] != 0)


@pytest.mark.parametrize("n,rf", [(3, 20), (7, 600), (4, 4120)])
def test_dense_call_in_place(n, rf):
    x = torch.from_numpy(table(n, rf)).to(DEV)
    assert launch(x, None, x, 0.5, SEED) == 0
    assert torch.equal(x.cpu(), torch.from_numpy(R.dropped(table(n, rf), 0.5, SEED)))
    y = x.clone()
    assert launch(x, None, x, 0.0, SEED) == 0 and torch.equal(x, y)  # p = 0 in place: nothing to do


@pytest.mark.parametrize("which", ["out", "x"])
def test_misaligned_pointer_takes_the_scalar_path(which):
    """row_floats % 4 == 0 but one pointer 4 bytes off a 16-byte boundary: the scalar variant, the same bits."""
    n, rf = 7, 600
    tab = table(n, rf)
    buf = torch.zeros(n * rf + 1, device=DEV)
    if which == "out":
        x, out = torch.from_numpy(tab).to(DEV), buf[1:].view(n, rf)
    else:
        buf[1:] = torch.from_numpy(tab).to(DEV).reshape(-1)
        x, out = buf[1:].view(n, rf), torch.empty(n, rf, device=DEV)
    assert (x.data_ptr() | out.data_ptr()) % 16 != 0
    assert launch(x, None, out, 0.1, SEED) == 0
    assert torch.equal(out.cpu(), torch.from_numpy(R.dropped(tab, 0.1, SEED)))
    if which == "out":
        assert buf[0].item() == 0  # nothing written in front of the view


def test_seed_above_2_63_and_the_device_seed_word():
    """A seed >= 2^63; and a launch with seed s and device word w equals a launch with host seed s + w (mod 2^64) and no word."""
    n, rf = 7, 600
    tab = table(n, rf)
    x = torch.from_numpy(tab).to(DEV)
    big = R.SEEDS[2]
    assert big >= 2 ** 63
    out = torch.empty(n, rf, device=DEV)
    assert launch(x, None, out, 0.5, big) == 0
    assert torch.equal(out.cpu(), torch.from_numpy(R.dropped(tab, 0.5, big)))
    for s, w in ((SEED, 5), (big, 2 ** 63 + 9)):  # (the second sum wraps)
        word = torch.tensor([w - 2 ** 64 if w >= 2 ** 63 else w], dtype=torch.int64, device=DEV)
        a, b = torch.empty(n, rf, device=DEV), torch.empty(n, rf, device=DEV)
        assert launch(x, None, a, 0.5, s, word) == 0 and launch(x, None, b, 0.5, (s + w) % 2 ** 64) == 0
        assert torch.equal(a, b) and torch.equal(a.cpu(), torch.from_numpy(R.dropped(tab, 0.5, (s + w) % 2 ** 64)))
        assert not torch.equal(a.cpu(), torch.from_numpy(R.dropped(tab, 0.5, s)))


def test_edge_arguments():
    x = torch.ones(2, 8, device=DEV)
    out = torch.full((2, 8), 7.0, device=DEV)
    assert launch(x, None, out, 0.5, SEED, n=0) == 0
    for p in (1.5, -0.1, float("nan")):
        assert launch(x, None, out, p, SEED) == EINVAL
        assert launch(x, None, out, p, SEED, n=0) == EINVAL
    assert launch(x, None, out, 0.5, SEED, row_floats=2 ** 32) == EINVAL
    assert launch(x, None, out, 0.5, SEED, row_floats=0) == EINVAL
    assert launch(None, None, out, 0.5, SEED) == EINVAL and launch(x, None, None, 0.5, SEED, n=2, row_floats=8) == EINVAL
    torch.cuda.synchronize()
    assert (out == 7).all()  # no refused call wrote anything


def test_gather_dropout_bridge_adds_the_seed_word():
    tab = table(10, 600)
    ids = make_ids("repeats", 7, 10)
    t, i = torch.from_numpy(tab).to(DEV).reshape(10, 30, 20), torch.from_numpy(ids).to(DEV)
    y = ops.gather_dropout(t, i, 0.1, SEED)
    assert y.shape == (7, 30, 20) and torch.equal(y.cpu().reshape(7, 600), torch.from_numpy(R.dropped(tab[ids], 0.1, SEED)))
    ops.set_dropout_seed_word(torch.tensor([3], dtype=torch.int64, device=DEV))
    try:
        y = ops.gather_dropout(t, i, 0.1, SEED)
    finally:
        ops.set_dropout_seed_word(None)
    assert torch.equal(y.cpu().reshape(7, 600), torch.from_numpy(R.dropped(tab[ids], 0.1, SEED + 3)))


# ------------------------------------------------------------------------------------------------ autograd
def test_input_dropout_backward_is_the_same_mask_on_dy():
    rng = synth.rng_for(9300)
    x = rng.standard_normal((5, 7, 12)).astype(np.float32)
    dy = rng.standard_normal((5, 7, 12)).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    y = ops.input_dropout(xd, 0.5, True, seed=SEED)
    assert tuple(y.grad_fn.saved_tensors) == ()  # nothing saved but (p, seed)
    y.backward(torch.from_numpy(dy).to(DEV))
    assert torch.equal(y.detach().cpu(), torch.from_numpy(R.dropped(x, 0.5, SEED)))
    assert torch.equal(xd.grad.cpu(), torch.from_numpy(R.dropped(dy, 0.5, SEED)))
    # seed=None: drawn from torch's CPU generator
    seeds = R.draw_seeds(R.TORCH_SEEDS[0], 2)
    torch.manual_seed(R.TORCH_SEEDS[0])
    y1, y2 = ops.input_dropout(xd, 0.1, True), ops.input_dropout(xd, 0.1, True)
    torch.manual_seed(R.TORCH_SEEDS[0])
    y3 = ops.input_dropout(xd, 0.1, True)
    assert torch.equal(y1, y3) and not torch.equal(y1, y2)
    assert torch.equal(y1.detach().cpu(), torch.from_numpy(R.dropped(x, 0.1, seeds[0])))
    assert torch.equal(y2.detach().cpu(), torch.from_numpy(R.dropped(x, 0.1, seeds[1])))
    assert ops.input_dropout(xd, 0.1, False) is xd and ops.input_dropout(xd, 0.0, True) is xd


@pytest.mark.parametrize("shape", [(3, 0), (0, 4), (2, 0, 5)])
def test_input_dropout_of_an_empty_tensor_is_empty(shape):
    """nn.Dropout returns an empty tensor for an empty input; so does this, forward and backward (no launch at all)."""
    x = torch.empty(shape, device=DEV, requires_grad=True)
    y = ops.input_dropout(x, 0.5, True, seed=SEED)
    assert y.shape == x.shape and y.numel() == 0
    y.sum().backward()
    assert x.grad.shape == x.shape
    t = torch.ones(4, 0, device=DEV)
    assert ops.gather_dropout(t, torch.tensor([1, 3, 3], dtype=torch.int32, device=DEV), 0.5, SEED).shape == (3, 0)


# ------------------------------------------------------------------------------------------------ the id path
P_IN = 0.3
N_TAB, IDS = 12, [[3, 0, 7, 3, 11], [5, 7, 0, 1, 3]]  # a repeat inside a row, across the rows, and the empty row 0
# (S, D, heads, attention dropout)
ID_CASES = [(7, 20, 0, 0.0), (9, 24, 2, 0.0), (9, 24, 2, 0.1)]


def make_encoder(S, D, h, pa, p_in, seed=81):
    att = layers.MultiHeadAttention(h, D, dropout=pa) if h else None
    enc = news_encoding.TextEncoder(pooler=layers.AdditiveAttention(D, 8), p_dropout=p_in, out_features=12, in_features=D, att=att)
    return load(enc, seed, train=True)


@functools.lru_cache(maxsize=None)
def id_table(S, D):
    """[12, S, D] tokens and [12, S, 1] masks: row 0 all-masked (the empty history slot), ragged tails, one hole."""
    rng = synth.rng_for(9400 + S)
    x = rng.standard_normal((N_TAB, S, D)).astype(np.float32)
    lens = rng.integers(1, S + 1, size=(N_TAB,))
    m = (np.arange(S)[None, :] < lens[:, None]).astype(np.float32)
    m[3, 0] = 0
    m[0] = 0
    x[0] = 0
    return torch.from_numpy(x), torch.from_numpy(m).reshape(N_TAB, S, 1)


def id_inputs(S, D):
    tx, tm = id_table(S, D)
    ids = torch.tensor(IDS, dtype=torch.int32)
    flat = ids.reshape(-1).long()
    return tx, tm, ids, tx[flat], tm[flat]


def run_id_path(enc, S, D, k):
    tx, tm, ids, _, _ = id_inputs(S, D)
    enc.zero_grad()
    torch.manual_seed(k)
    y, hm = enc.forward_ids(tx.to(DEV), tm.to(DEV), ids.to(DEV))
    return y, hm


@pytest.mark.parametrize("S,D,h,pa", ID_CASES)
def test_forward_ids_equals_the_dense_path_on_the_dropped_rows(S, D, h, pa):
    """TextEncoder.forward_ids in train mode with p_dropout = 0.3 == a twin with the same weights and p_dropout = 0, also in
    train mode, called as forward((xd, md)) with xd = dropped(tx[ids], p, seed_k): outputs at H.RTOL, every parameter gradient
    at GTOL.  With attention dropout on, the twin's run first discards one draw: the input seed is drawn BEFORE the attention
    seed.  Both sides run the same dense entry points on the same numbers.  Observed on an MI355X: difference 0 (outputs and
    all gradients bitwise equal) in all three cases."""
    k = R.TORCH_SEEDS[0]
    enc, sd = make_encoder(S, D, h, pa, P_IN)
    twin, _ = make_encoder(S, D, h, pa, 0.0)
    tx, tm, ids, xg, mg = id_inputs(S, D)
    y, hm = run_id_path(enc, S, D, k)
    y.sum().backward()
    seed_in = R.draw_seeds(k)[0]
    xd = torch.from_numpy(R.dropped(xg, P_IN, seed_in)).reshape(2, 5, S, D)
    torch.manual_seed(k)
    if pa > 0:
        torch.empty((), dtype=torch.int64).random_()  # the draw the id path spent on its input dropout
    yt, hmt = twin((xd.to(DEV), mg.reshape(2, 5, S, 1).to(DEV)))
    yt.sum().backward()
    worst = H.assert_close(y, yt.detach(), H.RTOL, "news vectors")
    assert torch.equal(hm, hmt)
    gmax = max(p.grad.abs().max().item() for n, p in twin.named_parameters() if p.grad is not None)
    for (n1, p1), (n2, p2) in zip(enc.named_parameters(), twin.named_parameters()):
        if n1.endswith("dummy_param"):
            continue
        assert n1 == n2 and p1.grad is not None and p2.grad is not None, n1
        e = (p1.grad - p2.grad).abs().max().item() / max(p2.grad.abs().max().item(), 1e-3 * gmax)
        assert e <= GTOL, f"{n1}: {e:.3e}"
        worst = max(worst, e)
    print(f"OBSERVED id path vs twin ({S},{D},{h},{pa}): largest relative difference {worst:.3e}")
    # not vacuous: without the input dropout the vectors are others
    with torch.no_grad():
        enc.dropout.p = 0.0
        torch.manual_seed(k)
        if pa > 0:
            torch.empty((), dtype=torch.int64).random_()
        y0, _ = enc.forward_ids(tx.to(DEV), tm.to(DEV), ids.to(DEV))
    assert H.rel_err(y0, yt.detach()) > 100 * H.RTOL


@pytest.mark.parametrize("S,D,h,pa", ID_CASES[:2])
def test_forward_ids_matches_fp64_oracle_on_the_dropped_rows(S, D, h, pa):
    """The same call against oracle text_encoder in fp64 on xd: news vectors at H.RTOL, the parameter gradients at GTOL (+ the
    derived extra bar of pooler.fc2.bias, tests/test_hip_attention_dropout.py).  Observed on an MI355X, error / bar: see the
    MARGIN lines (y and dW both below 0.1)."""
    k = R.TORCH_SEEDS[1]
    enc, sd = make_encoder(S, D, h, pa, P_IN)
    _, _, _, xg, mg = id_inputs(S, D)
    w = torch.from_numpy(synth.rng_for(9500).standard_normal((2, 5, 12)).astype(np.float32))
    y, hm = run_id_path(enc, S, D, k)
    (y * w.to(DEV)).sum().backward()
    xd = torch.from_numpy(R.dropped(xg, P_IN, R.draw_seeds(k)[0])).double().reshape(2, 5, S, D)
    osd = f64(sd)
    yo, hmo = O.text_encoder(xd, mg.double().reshape(2, 5, S, 1), osd, h or None)
    (yo * w.double()).sum().backward()
    ey = H.assert_close(y, yo.detach(), H.RTOL, "news vectors")
    assert torch.equal(hm.cpu().double(), hmo)
    eg, cnt = grad_excess(enc, osd, fc2_bias_bar(osd, 10 * S))
    assert cnt == (16 if h else 8)
    print(f"MARGIN id path vs fp64 ({S},{D},{h}): y {ey / H.RTOL:.3f}  dW {eg:.3f}  (error / bar)")


@pytest.mark.parametrize("S,D,h,pa", ID_CASES[:2])
def test_two_encodes_of_the_same_ids_share_nothing(S, D, h, pa):
    """Every encode gets its own dropped copy: neither the Q|K|V image nor the output reuse of xnrs_amd.autograd fires, and the
    two results differ.  With p_dropout = 0 the same two calls DO share (the control that the counters see this path)."""
    from xnrs_amd import autograd as AG
    enc, _ = make_encoder(S, D, h, pa, P_IN)
    tx, tm, ids, _, _ = id_inputs(S, D)
    txd, tmd, idd = tx.to(DEV), tm.to(DEV), ids.to(DEV)
    before = dict(AG.STATS)
    torch.manual_seed(R.TORCH_SEEDS[0])
    y1, _ = enc.forward_ids(txd, tmd, idd)
    y2, _ = enc.forward_ids(txd, tmd, idd)
    assert AG.STATS["shared_qkv_forwards"] == before["shared_qkv_forwards"]
    assert AG.STATS["shared_output_forwards"] == before["shared_output_forwards"]
    assert y1 is not y2 and y1.grad_fn is not y2.grad_fn and not torch.equal(y1, y2)
    (y1.sum() + y2.sum()).backward()
    del y1, y2
    enc.dropout.p = 0.0
    y1, _ = enc.forward_ids(txd, tmd, idd)
    y2, _ = enc.forward_ids(txd, tmd, idd)
    shared = sum(AG.STATS[s] - before[s] for s in ("shared_qkv_forwards", "shared_output_forwards"))
    assert shared == 1 and torch.equal(y1, y2)


def test_dedup_with_active_input_dropout_is_refused():
    enc, _ = make_encoder(7, 20, 0, 0.0, P_IN)
    tx, tm, ids, _, _ = id_inputs(7, 20)
    with pytest.raises(hip.XnrsHipError, match="dedup"):
        enc.forward_ids(tx.to(DEV), tm.to(DEV), ids.to(DEV), dedup=True)
    enc.eval()
    with torch.no_grad():
        a, _ = enc.forward_ids(tx.to(DEV), tm.to(DEV), ids.to(DEV), dedup=True)
        b, _ = enc.forward_ids(tx.to(DEV), tm.to(DEV), ids.to(DEV))
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ models
def tiny_model(name, p):
    c = cases.MODELS[name]
    model = make_model(Cfg(dict(cases.model_cfg(c), p_dropout=p)))
    model.load_state_dict(synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, c["seed"] + 1))
    return model.to(DEV), c


def tiny_store(c, naml):
    """A device NewsStore of 10 rows (row 0 empty) at the case's token shape, and (hist, cand) ids with repeats and a 0."""
    from xnrs_amd.data import NewsStore
    rng = synth.rng_for(9600)
    n, S, D = 10, c["S"], c["D"]
    feats = {}
    for i in range(1, n):
        f = {}
        for name in (("title_emb", "abstract_emb") if naml else ("title_emb",)):
            L = int(rng.integers(1, S + 1))
            f[name] = (rng.standard_normal((1, S, D)).astype(np.float32), (np.arange(S)[None, :] < L).astype(np.float32))
        if naml:
            f["category_index"], f["subcategory_index"] = int(rng.integers(1, 19)), int(rng.integers(1, 300))
        feats[f"N{i}"] = f
    store = NewsStore.from_news_feat(feats, "title_emb", ["category_index", "subcategory_index"] if naml else [],
                                     ["abstract_emb"] if naml else [])
    hist = torch.tensor([[3, 0, 7, 3], [5, 7, 0, 0], [1, 2, 3, 4]], dtype=torch.int32)[:c["B"]]
    cand = torch.tensor([[2, 9, 2], [4, 1, 8], [6, 6, 5]], dtype=torch.int32)[:c["B"]]
    return store.to(DEV), hist.to(DEV), cand.to(DEV)


@pytest.mark.parametrize("name", ["nrms_tiny", "naml_tiny"])
def test_models_train_through_the_id_path_with_input_dropout(name):
    """p_dropout = 0.25: train-mode forward_store gives finite scores and backward fills every parameter's .grad; in eval mode
    the scores are exactly those of the model with p_dropout = 0; dedup=True in train mode is refused."""
    model, c = tiny_model(name, 0.25)
    plain, _ = tiny_model(name, 0.0)
    store, hist, cand = tiny_store(c, name == "naml_tiny")
    model.train()
    torch.manual_seed(R.TORCH_SEEDS[0])
    r = model.forward_store(store, hist, cand)
    assert r.shape[:2] == (c["B"], 3) and torch.isfinite(r).all()
    r.sum().backward()
    for n, p in model.named_parameters():
        if not n.endswith("dummy_param"):
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
    r2 = model.forward_store(store, hist, cand)
    assert not torch.equal(r, r2)  # a fresh draw per call
    with pytest.raises(hip.XnrsHipError, match="dedup"):
        model.forward_store(store, hist, cand, dedup=True)
    model.eval(), plain.eval()
    with torch.no_grad():
        assert torch.equal(model.forward_store(store, hist, cand), plain.forward_store(store, hist, cand))
        assert torch.equal(model.forward_store(store, hist, cand, dedup=True), plain.forward_store(store, hist, cand))


def test_npa_trains_through_the_id_path_with_input_dropout():
    """NPA.forward_store takes the dense dropped rows as it is: train mode with p_dropout = 0.2 equals the dense personalized
    encoder on dropped(tx[ids]) (one draw over history + candidates), and eval mode is untouched."""
    from tests.golden import npa_cases as NC
    from xnrs_amd.models.npa import make_npa
    c = NC.CASES["tiny"]
    model = make_npa(Cfg(dict(NC.model_cfg(c), p_dropout=0.2)))
    model.load_state_dict(synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 97))
    model = model.to(DEV).train()
    S, D = c["S"], c["D"]
    rng = synth.rng_for(9700)
    x = rng.standard_normal((9, S, D)).astype(np.float32)
    lens = rng.integers(1, S + 1, size=9)
    lens[0] = 0
    x[0] = 0

    class Store:
        tx, tm = torch.from_numpy(x).to(DEV), torch.from_numpy((np.arange(S)[None, :] < lens[:, None]).astype(np.float32)).to(DEV)

        def text(self, feature):
            return self.tx, self.tm
    store = Store()
    hist = torch.tensor([[3, 0, 7, 3], [5, 7, 0, 0]], dtype=torch.int32, device=DEV)
    cand = torch.tensor([[2, 8, 2], [4, 1, 8]], dtype=torch.int32, device=DEV)
    uid = torch.tensor([1, 2], dtype=torch.int32, device=DEV)
    k = R.TORCH_SEEDS[0]
    torch.manual_seed(k)
    r = model.forward_store(store, hist, cand, uid)
    assert torch.isfinite(r).all()
    r.sum().backward()
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    assert grads and all(torch.isfinite(g).all() for g in grads.values())
    # the dense restatement: the same personalized encoder on the dropped rows
    tx, tm = store.text("title_emb")
    flat = torch.cat([hist.reshape(-1), cand.reshape(-1)]).long()
    xd = torch.from_numpy(R.dropped(tx[flat].cpu(), 0.2, R.draw_seeds(k)[0])).to(DEV)
    model.zero_grad()
    model.dropout.p = 0.0
    h, c_ = xd[:8].reshape(2, 4, S, D), xd[8:].reshape(2, 3, S, D)
    hm, cm = tm[flat[:8]].reshape(2, 4, S, 1), tm[flat[8:]].reshape(2, 3, S, 1)
    rt = model._forward((h, hm), (c_, cm), uid)
    H.assert_close(r, rt.detach(), H.RTOL, "NPA scores")
    model.dropout.p = 0.2
    model.eval()
    with torch.no_grad():
        re = model.forward_store(store, hist, cand, uid)
        model.dropout.p = 0.0
        assert torch.equal(re, model.forward_store(store, hist, cand, uid))


# ------------------------------------------------------------------------------------------------ the opt-in of the dense towers
def test_user_encoder_hip_dropout_matches_the_twin_on_the_dropped_input():
    """UserEncoder with hip_dropout = True, p = 0.5, (B, H, E) = (3, 6, 16): user vectors, dx and the parameter gradients equal the
    twin's (p_dropout = 0) on dropped(x) -- dx through the kernel's backward: dx == dropped(twin's dx)."""
    B, Hn, E, p, k = 3, 6, 16, 0.5, R.TORCH_SEEDS[1]
    mk = lambda pd: load(user_encoding.UserEncoder(pooler=layers.AdditiveAttention(E, 8), p_dropout=pd, emb_dim=E, head=True,  # noqa: E731
                                                   att=layers.MultiHeadAttention(2, E, dropout=0.0)), 83, train=True)[0]
    enc, twin = mk(p), mk(0.0)
    enc.hip_dropout = True
    rng = synth.rng_for(9800)
    x = rng.standard_normal((B, Hn, E)).astype(np.float32)
    m = np.ones((B, Hn, 1), dtype=np.float32)
    m[0, 4:] = 0
    w = torch.from_numpy(rng.standard_normal((B, 1, E)).astype(np.float32)).to(DEV)
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    torch.manual_seed(k)
    u = enc((xd, torch.from_numpy(m).to(DEV)))
    (u * w).sum().backward()
    seed = R.draw_seeds(k)[0]
    xt = torch.from_numpy(R.dropped(x, p, seed)).to(DEV).requires_grad_(True)
    ut = twin((xt, torch.from_numpy(m).to(DEV)))
    (ut * w).sum().backward()
    H.assert_close(u, ut.detach(), H.RTOL, "user vectors")
    H.assert_close(xd.grad, R.dropped(xt.grad, p, seed), GTOL, "dx")
    gmax = max(q.grad.abs().max().item() for q in twin.parameters() if q.grad is not None)
    for (n1, p1), (_, p2) in zip(enc.named_parameters(), twin.named_parameters()):
        if n1.endswith("dummy_param"):
            continue
        e = (p1.grad - p2.grad).abs().max().item() / max(p2.grad.abs().max().item(), 1e-3 * gmax)
        assert e <= GTOL, f"{n1}: {e:.3e}"
    # eval mode: the input object goes through untouched
    enc.eval(), twin.eval()
    with torch.no_grad():
        assert torch.equal(enc((xd.detach(), torch.from_numpy(m).to(DEV))), twin((xd.detach(), torch.from_numpy(m).to(DEV))))


def test_text_encoder_hip_dropout_opt_in_and_default(monkeypatch):
    """hip_dropout = True: forward() == the twin on dropped(x); hip_dropout = False (default): self.dropout is the op that runs
    (its forward is patched and seen called) and ops.input_dropout is not."""
    S, D, k = 7, 20, R.TORCH_SEEDS[0]
    enc, _ = make_encoder(S, D, 0, 0.0, P_IN)
    twin, _ = make_encoder(S, D, 0, 0.0, 0.0)
    _, _, _, xg, mg = id_inputs(S, D)
    x, m = xg.reshape(2, 5, S, D).to(DEV), mg.reshape(2, 5, S, 1).to(DEV)
    calls = []
    monkeypatch.setattr(enc.dropout, "forward", lambda t: (calls.append("nn"), t)[1])
    real = ops.input_dropout
    monkeypatch.setattr(ops, "input_dropout", lambda *a, **kw: (calls.append("hip"), real(*a, **kw))[1])
    assert enc.hip_dropout is False
    y0, _ = enc((x, m))
    assert calls == ["nn"]
    enc.hip_dropout = True
    torch.manual_seed(k)
    y, _ = enc((x, m))
    assert calls == ["nn", "hip"]
    yt, _ = twin((torch.from_numpy(R.dropped(xg, P_IN, R.draw_seeds(k)[0])).reshape(2, 5, S, D).to(DEV), m))
    H.assert_close(y, yt.detach(), H.RTOL, "news vectors")
    assert not torch.equal(y, y0)
    # the user tower's default, too
    ue = load(user_encoding.UserEncoder(pooler=layers.AdditiveAttention(16, 8), p_dropout=0.5, emb_dim=16), 85, train=True)[0]
    monkeypatch.setattr(ue.dropout, "forward", lambda t: (calls.append("nn-user"), t)[1])
    ue((torch.randn(2, 3, 16, device=DEV), torch.ones(2, 3, 1, device=DEV)))
    assert calls[-1] == "nn-user"
