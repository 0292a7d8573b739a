"""GPU tests of the bf16 news table: the widening gather / dropout kernels, the primitive
xnrs_linear_fwd_bf16 (gemm_a16_kernel: bf16 rows against the exact three-way bf16 split of the fp32 weights), the two routes
of xnrs_text_encoder_fwd_bf16, and the models, the evaluation epoch and a grad step on a bf16 NewsStore.

Which shapes reach gemm_a16_kernel: K % 8 == 0 and 16-byte aligned rows.  The golden `news_nrms_300` tower has D = 300
(300 % 8 = 4): its calls take the widening route whatever the knob says, so the direct-route tests run it AND a D = 768
tower that does reach the kernel; only the latter can show that the direct route ran (its bits differ from the widening
route's)."""
import numpy as np
import pytest
import torch

from oracle import xnrs_oracle as O
from tests import helpers as H
from tests.golden import cases
from tests.golden import npa_cases as NC
from tests.test_hip_grads import GTOL
from tests.test_hip_split_gemm import _fp64_err
from xnrs_amd import evaluation as EV
from xnrs_amd import hip, ops, synth
from xnrs_amd.data import Behaviors, NewsStore
from xnrs_amd.models import make_model
from xnrs_amd.models.components import layers, news_encoding
from xnrs_amd.models.npa import make_npa

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
FORCE = dict(XNRS_GEMM_SPLIT_MIN_TILES="0")  # the a16 kernel on every eligible shape, also the tiny ones


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


# ------------------------------------------------------------------------------------------------ 1. primitive, exact
def _int_operands(M, N, K, seed):
    """x: integers in [-8, 8] stored as bf16 (a table of M rows, padded to whole blocks of 3), w, b: integers in [-4, 4]:
    every product and partial sum is an integer below 2^24, exact in fp32 in any order."""
    g = _gen(seed)
    rows = (M + 2) // 3 * 3
    x = torch.randint(-8, 9, (rows, K), device=DEV, generator=g).to(BF16)
    w = torch.randint(-4, 5, (N, K), device=DEV, generator=g).float()
    b = torch.randint(-4, 5, (N,), device=DEV, generator=g).float()
    return x, w, b


def _src_rows(ids, S, M):
    m = torch.arange(M, device=DEV)
    return ids.long()[m // S] * S + m % S


EXACT_SHAPES = [(129, 129, 24), (130, 260, 40), (1, 1, 8), (257, 384, 256)]


@pytest.mark.parametrize("act", [hip.ACT_NONE, hip.ACT_RELU, hip.ACT_TANH])
@pytest.mark.parametrize("shape", EXACT_SHAPES)
def test_linear_bf16_is_exact_on_integers(shape, act):
    """1-row M tail, 1-column N tail in a second column tile, K % 16 = 8, a single half k step; dense by ids and shuffled
    repeating ids at gather_S = 1 and 3."""
    M, N, K = shape
    x, w, b = _int_operands(M, N, K, M + N + K)
    g = _gen(7)
    with hip.knobs(**FORCE):
        for S in (1, 3):
            n_blocks = x.shape[0] // S
            n_ids = (M + S - 1) // S
            for ids in (torch.arange(n_ids, device=DEV, dtype=torch.int32),
                        torch.randint(0, n_blocks, (n_ids,), device=DEV, generator=g, dtype=torch.int32)):
                y = ops.linear_bf16(x, w, b, act, ids=ids, gather_s=S, m_rows=M)
                ref = ops.linear(x.float()[_src_rows(ids, S, M)], w, b, act)
                assert y.shape == (M, N) and torch.equal(y, ref), (shape, act, S)
        # no ids: the rows as they lie
        assert torch.equal(ops.linear_bf16(x[:M], w, None, act), ops.linear(x[:M].float(), w, None, act))


def test_linear_bf16_k12_takes_the_widening_route():
    """K = 12 is not a multiple of 8: the entry widens the rows and still equals the fp32 result (1 500 rows: two passes of
    the widening buffer, the second one partial, with blocks of 3 rows that straddle the pass boundary)."""
    M, N, K = 1500, 40, 12
    x, w, b = _int_operands(M, N, K, 12)
    ids = torch.randint(0, x.shape[0] // 3, (M // 3,), device=DEV, generator=_gen(3), dtype=torch.int32)
    with hip.knobs(**FORCE):
        y = ops.linear_bf16(x, w, b, hip.ACT_RELU, ids=ids, gather_s=3)
        y1 = ops.linear_bf16(x, w, b, hip.ACT_RELU)
    assert torch.equal(y, ops.linear(x.float()[_src_rows(ids, 3, M)], w, b, hip.ACT_RELU))
    assert torch.equal(y1, ops.linear(x.float(), w, b, hip.ACT_RELU))


# ------------------------------------------------------------------------------------------------ 2. primitive, fp32-grade
@pytest.mark.parametrize("act", [hip.ACT_NONE, hip.ACT_RELU, hip.ACT_TANH])
@pytest.mark.parametrize("shape", [(8200, 1000, 768), (130, 129, 40), (257, 384, 256)])
def test_linear_bf16_is_fp32_grade(shape, act):
    """The data of test_linear_modes_against_fp64 with x rounded to bf16 first; bars: that test's (fp32 kernel err0 <= 1e-6,
    the a16 kernel <= max(2e-7, 1.5 err0)), normwise against fp64 on x.float()."""
    M, N, K = shape
    g = _gen(M + N + K)
    x = (torch.randn(M, K, device=DEV, generator=g) * 3.0).to(BF16)
    w = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    b = torch.randn(N, device=DEV, generator=g) if act != hip.ACT_RELU else None
    prev = hip.set_gemm_mode(0)
    try:
        y0 = ops.linear(x.float(), w, b, act)
        with hip.knobs(**FORCE):
            y1 = ops.linear_bf16(x, w, b, act)
            hip.set_gemm_mode(2)  # the kernel ignores the mode: the same bits
            y2 = ops.linear_bf16(x, w, b, act)
    finally:
        hip.set_gemm_mode(prev)
    err0, err1 = _fp64_err(y0, x.float(), w, b, act), _fp64_err(y1, x.float(), w, b, act)
    print(f"linear_bf16 {shape} act {act}: fp32 kernel {err0:.3e}, a16 kernel {err1:.3e}")
    assert torch.isfinite(y1).all() and torch.equal(y1, y2)
    assert not torch.equal(y1, y0)  # (another summation: the a16 kernel ran, not the widening route)
    assert err0 <= 1e-6, (err0, err1)
    assert err1 <= max(2e-7, 1.5 * err0), f"the a16 kernel is not fp32-grade: {err0:.3e} {err1:.3e}"


def test_linear_bf16_handles_wide_dynamic_range():
    """The inputs of test_split_handles_wide_dynamic_range (x rounded to bf16, W columns scaled by 1e-12)."""
    g = _gen(5)
    M, N, K = 512, 256, 128
    x = torch.randn(M, K, device=DEV, generator=g)
    x[:, ::7] *= 1e18
    x[:, 1::7] *= 1e-18
    x[:, 2::7] = 0.0
    x = x.to(BF16)
    w = torch.randn(N, K, device=DEV, generator=g)
    w[:, ::5] *= 1e-12
    y0 = ops.linear(x.float(), w)
    with hip.knobs(**FORCE):
        y1 = ops.linear_bf16(x, w)
    e0, e1 = _fp64_err(y0, x.float(), w, None, 0), _fp64_err(y1, x.float(), w, None, 0)
    print(f"wide dynamic range: fp32 kernel {e0:.3e}, a16 kernel {e1:.3e}")
    assert e0 <= 1e-6 and e1 <= 1e-6, (e0, e1)


# ------------------------------------------------------------------------------------------------ 3. gather and dropout
@pytest.mark.parametrize("row_elems", [8, 24, 20 * 64, 6])  # 6: the scalar path (not a multiple of 8)
def test_gather_and_dropout_rows_bf16(row_elems):
    g = _gen(row_elems)
    table = (torch.randn(37, row_elems, device=DEV, generator=g) * 5).to(BF16)
    table[0] = 0
    ids = torch.randint(0, 37, (50,), device=DEV, generator=g, dtype=torch.int32)
    ids[:4] = torch.tensor([0, 5, 5, 0], dtype=torch.int32)
    got = ops.table_rows_f32(table, ids)
    assert got.dtype == torch.float32 and torch.equal(got, table.float()[ids.long()])
    p, seed = 0.3, 0x1234_5678_9ABC_DEF1
    word = torch.tensor([5], dtype=torch.int64, device=DEV)
    for w in (None, word):
        a = torch.empty(50, row_elems, device=DEV)
        hip.check(hip.lib().xnrs_dropout_rows_bf16(hip.ptr(table), hip.ptr(ids), hip.ptr(a), 50, row_elems, p, seed, hip.ptr(w),
                                                   hip.stream_ptr(DEV)), "xnrs_dropout_rows_bf16")
        ref = ops.dropout_rows(table.float(), ids, torch.empty(50, row_elems, device=DEV), p, seed, w)
        assert torch.equal(a, ref)
        assert 0.2 < (a == 0).float().mean().item() < 0.45  # (it did drop; the zero row adds 4 %)
    # p = 0: the widening gather; ids are required
    a = torch.empty(50, row_elems, device=DEV)
    assert hip.lib().xnrs_dropout_rows_bf16(hip.ptr(table), hip.ptr(ids), hip.ptr(a), 50, row_elems, 0.0, 1, None, hip.stream_ptr(DEV)) == 0
    assert torch.equal(a, got)
    assert hip.lib().xnrs_dropout_rows_bf16(hip.ptr(table), None, hip.ptr(a), 50, row_elems, p, 1, None, hip.stream_ptr(DEV)) == -1


# ------------------------------------------------------------------------------------------------ 4./5. the encoder
def _tower(c, seed=21):
    D, E = c["D"], c["E"]
    pooler = layers.AdditiveAttention(D, c["A"]) if c["pooler"] == "additive" else layers.MaskedMean()
    att = layers.MultiHeadAttention(c["h"], D) if c["att"] else None
    enc = news_encoding.TextEncoder(pooler=pooler, p_dropout=0.0, out_features=E, in_features=D, att=att, head=c["head"],
                                    bias=c["bias"])
    shapes = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    sd = synth.fill_state_dict(shapes, seed)
    enc.load_state_dict(sd)
    return enc.eval().to(DEV), sd


def _table(c, n_rows=40, seed=22):
    """(bf16 table, mask, ids (3, 7)) at the case's token shape: row 0 the empty slot, ids that repeat and include it."""
    rng = synth.rng_for(seed)
    tx, tm = synth.token_block(rng, 1, n_rows, c["S"], c["D"], min_len=3)
    tx, tm = tx[0], tm[0]
    tx[0], tm[0] = 0, 0
    ids = torch.from_numpy(rng.integers(0, n_rows, size=(3, 7)).astype("int64"))
    ids[0, 0], ids[2, 3] = 0, 0
    return tx.to(DEV).to(BF16), tm.to(DEV), ids.to(DEV)


WIDENING = [("news_nrms_300", {}), ("news_add_head_nobias", {}), ("news_add_head_nobias", dict(XNRS_ADDITIVE_FUSED="2")),
            ("news_mean_head", {}), ("news_nrms_300", dict(XNRS_NEWS_FUSED="2")), ("news_nrms_768", {})]


@pytest.mark.parametrize("name,knobs", WIDENING)
def test_encoder_widening_route_equals_the_fp32_call_bitwise(name, knobs):
    """XNRS_GEMM_A16=0: attention tower, attention-free additive tower (pipeline and one-launch kernel), mean pooling, a short
    title on news_fused -- forward_ids(bf16 table) == forward_ids(table.float()), y and hm, bit for bit; three news per pass
    so that the passes of the call do not line up with anything."""
    c = cases.ENCODERS[name]
    enc, _ = _tower(c)
    tb, tm, ids = _table(c)
    with torch.no_grad(), hip.knobs(XNRS_GEMM_A16="0", **FORCE, **knobs):
        y0, hm0 = enc.forward_ids(tb.float(), tm, ids)
        y1, hm1 = enc.forward_ids(tb, tm, ids)
        y2, hm2 = ops.text_encoder(tb, tm, enc, ids=ids.reshape(-1), chunk=3)
        y3, _ = ops.text_encoder(tb.float(), tm, enc, ids=ids.reshape(-1), chunk=3)
    assert torch.equal(y1, y0) and torch.equal(hm1, hm0)
    assert torch.equal(y2, y3) and torch.equal(y2.reshape(y0.shape), y0) and torch.equal(hm2.reshape(hm0.shape), hm0)


DIRECT = ["news_nrms_300", "news_nrms_768"]  # D = 300: refused by the kernel (300 % 8 = 4), widening; D = 768: the kernel


@pytest.mark.parametrize("name", DIRECT)
def test_encoder_direct_route_meets_the_bf16x3_bar_and_the_oracle(name):
    c = cases.ENCODERS[name]
    enc, sd = _tower(c)
    tb, tm, ids = _table(c)
    with torch.no_grad():
        with hip.knobs(**FORCE):
            y0, hm0 = enc.forward_ids(tb.float(), tm, ids)
            y1, hm1 = enc.forward_ids(tb, tm, ids)
        with hip.knobs(XNRS_GEMM_A16="0", **FORCE):
            yw, _ = enc.forward_ids(tb, tm, ids)
    assert torch.equal(hm1, hm0)
    H.assert_close(y1, y0, tol=1e-5, what=f"{name}: bf16 table, direct route vs the fp32 call", elementwise=True)
    xo, mo = tb.float().cpu()[ids.cpu()].double(), tm.cpu()[ids.cpu()].double()
    yo, hmo = O.text_encoder(xo, mo, {k: v.double() for k, v in sd.items()}, c["h"])
    H.assert_close(y1, yo, tol=H.RTOL, what=f"{name}: bf16 table vs the fp64 oracle on the widened inputs")
    assert torch.equal(hm1.cpu().double(), hmo)
    if c["D"] % 8 == 0:
        assert not torch.equal(y1, yw)  # the projection ran on the a16 kernel: another summation than the widening route's
    else:
        assert torch.equal(y1, yw)


@pytest.mark.parametrize("name", DIRECT)
def test_encoder_direct_route_is_batch_invariant(name):
    """The vectors of 3 ids computed alone == the same ids inside a call of 300.  XNRS_NEWS_FUSED=0: at S = 30 the fp32
    path itself sends a call of >= 192 short titles to the one-launch kernel and a call of 3 to the pipeline (the one
    dispatch that depends on the batch, encoder_fwd.hip) -- not the subject here."""
    c = cases.ENCODERS[name]
    enc, _ = _tower(c)
    tb, tm, _ = _table(c)
    ids = torch.randint(0, 40, (300,), device=DEV, generator=_gen(300))
    pick = torch.tensor([7, 150, 299], device=DEV)
    with torch.no_grad(), hip.knobs(XNRS_NEWS_FUSED="0", **FORCE):
        y_all, hm_all = ops.text_encoder(tb, tm, enc, ids=ids)
        y_3, hm_3 = ops.text_encoder(tb, tm, enc, ids=ids[pick])
    assert torch.equal(y_all[pick], y_3) and torch.equal(hm_all[pick], hm_3)


def _live_tile_case(S, D, h, n, dead_runs, seed):
    c = dict(D=D, E=32, A=64, h=h, S=S, att=True, pooler="additive", head=True, bias=True)
    enc, _ = _tower(c, seed)
    tb, tm, _ = _table(c, n_rows=24, seed=seed + 1)
    ids = torch.randint(1, 24, (n,), device=DEV, generator=_gen(seed), dtype=torch.int32)
    for lo, hi in dead_runs:
        ids[lo:hi] = 0
    return enc, tb, tm, ids


@pytest.mark.parametrize("S,D,h,n,dead_runs", [
    (16, 64, 4, 200, [(10, 50), (120, 150)]),  # 8 news per 128-row tile: runs of 40 and 30 empty news cover >= 3 whole tiles each
    (50, 768, 16, 64, [(5, 17), (30, 52)]),    # the shape at which the Q|K|V product itself walks the list (33 <= S <= 64)
])
def test_encoder_direct_route_honours_live_tiles(S, D, h, n, dead_runs):
    """A call above the live-tile threshold with whole all-masked row tiles beside live ones: == the same call with
    XNRS_GEMM_LIVE_TILES=0, bit for bit, also with the workspace poisoned (no skipped row is read)."""
    enc, tb, tm, ids = _live_tile_case(S, D, h, n, dead_runs, 40 + S)
    with torch.no_grad():
        with hip.knobs(XNRS_GEMM_LIVE_TILES="0", **FORCE):
            y0, hm0 = ops.text_encoder(tb, tm, enc, ids=ids)
        ws = hip.workspace(DEV, 1)
        with hip.knobs(XNRS_GEMM_LIVE_TILES="1", XNRS_GEMM_LIVE_TILES_MIN_ROWS="1024", XNRS_GEMM_LIVE_ROWS_MIN_ROWS="1024", **FORCE):
            ws.fill_(0xFF)
            y1, hm1 = ops.text_encoder(tb, tm, enc, ids=ids)
            ws.fill_(0xFF)
            y2, _ = ops.text_encoder(tb, tm, enc, ids=ids, chunk=27)  # pass boundaries inside the empty runs
        with hip.knobs(XNRS_GEMM_A16="0", **FORCE):
            yw, _ = ops.text_encoder(tb, tm, enc, ids=ids)
    assert torch.isfinite(y1).all()
    assert torch.equal(y1, y0) and torch.equal(hm1, hm0) and torch.equal(y2, y0)
    assert not torch.equal(y0, yw) and not (y0[ids.long() == 0] != y0[ids.long() == 0][0]).any()
    H.assert_close(y0, yw, tol=1e-5, what="direct vs widening route")


# ------------------------------------------------------------------------------------------------ 6. no whole-table copy
def test_no_call_converts_the_whole_table():
    """Table of 4 096 x 20 x 64 (10 MB in bf16, 21 MB in fp32), 16 ids: the peak allocation of each call above the level
    before it stays below the 21 MB of the fp32 copy that dev_f32(table) would make."""
    n_rows, S, D = 4096, 20, 64
    g = _gen(6)
    tb = torch.randn(n_rows, S, D, device=DEV, generator=g).to(BF16)
    tm = (torch.rand(n_rows, S, device=DEV, generator=g) > 0.2).float()
    tb[0], tm[0] = 0, 0
    store = NewsStore(tb, tm, list(range(n_rows - 1)))
    ids = torch.randint(0, n_rows, (2, 8), device=DEV, generator=g, dtype=torch.int32)
    base = dict(D=D, E=32, A=64, h=4, S=S, head=True, bias=True)
    nrms, _ = _tower(dict(base, att=True, pooler="additive"))
    addi, _ = _tower(dict(base, att=False, pooler="additive"))
    c = dict(NC.CASES["tiny"], S=S, D=D, H=5, C=3, n_users=30)
    npa = make_npa(Cfg(NC.model_cfg(c, "dot")))
    npa.load_state_dict(synth.fill_state_dict({k: tuple(v.shape) for k, v in npa.state_dict().items()}, 66))
    npa = npa.eval().to(DEV)
    uid = torch.tensor([3, 29], dtype=torch.int32, device=DEV)
    calls = {"nrms forward_ids": lambda: nrms.forward_ids(tb, tm, ids),
             "additive forward_ids": lambda: addi.forward_ids(tb, tm, ids),
             "NewsStore.gather": lambda: store.gather(ids),
             "NPA.forward_store": lambda: npa.forward_store(store, ids[:, :5], ids[:, 5:], uid)}
    bound = n_rows * S * D * 4
    with torch.no_grad():
        for what, fn in calls.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            out = fn()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - before
            assert peak < bound, f"{what}: {peak} bytes above the pre-call level (an fp32 copy of the table is {bound})"
            del out
    x, _ = store.gather(ids)
    assert torch.equal(x, tb.float()[ids.long()])


def test_load_to_device_keeps_or_converts_the_dtype(tmp_path):
    """File -> HBM: dtype=None keeps the file's dtype; torch.bfloat16 on an fp32 file converts chunk by chunk (chunks smaller
    than the table, the last one partial) to what astype gives; stats report the FILE's bytes."""
    from tests.test_bf16_store_host import _store
    s = _store(n=11, S=3, D=8)
    pf, pb = str(tmp_path / "f32"), str(tmp_path / "bf16")
    s.save(pf)
    s.astype(BF16).save(pb)
    st = {}
    a = NewsStore.load_to_device(pf, DEV, rows_per_chunk=4, dtype=BF16, stats=st)
    assert a.x.dtype == BF16 and a.x.is_cuda and torch.equal(a.x.cpu(), s.x.to(BF16))
    assert torch.equal(a.text("abstract_emb")[0].cpu(), s.texts["abstract_emb"][0].to(BF16)) and torch.equal(a.m.cpu(), s.m)
    assert st["bytes"] == 11 * 3 * 8 * 4 + 11 * 3 + 11 * 4 * 4 * 4 + 11 * 4
    b = NewsStore.load_to_device(pb, DEV, rows_per_chunk=4, stats=st)
    assert b.x.dtype == BF16 and torch.equal(b.x, a.x) and torch.equal(b.text("abstract_emb")[0], a.text("abstract_emb")[0])
    assert st["bytes"] == 11 * 3 * 8 * 2 + 11 * 3 + 11 * 4 * 4 * 2 + 11 * 4
    c = NewsStore.load_to_device(pf, DEV, rows_per_chunk=4)
    assert c.x.dtype == torch.float32 and torch.equal(c.x.cpu(), s.x)
    d = NewsStore.load_to_device(pb, DEV, rows_per_chunk=4, dtype=torch.float32)
    assert d.x.dtype == torch.float32 and torch.equal(d.x, a.x.float())


# ------------------------------------------------------------------------------------------------ 7. models
def _tiny(name, p=0.0):
    from tests.test_hip_input_dropout import tiny_model, tiny_store
    model, c = tiny_model(name, p)
    store, hist, cand = tiny_store(c, name == "naml_tiny")
    sb = store.astype(BF16)
    return model, sb, sb.astype(torch.float32), hist, cand


@pytest.mark.parametrize("name", ["nrms_tiny", "standard_tiny", "naml_tiny"])
def test_models_score_from_a_bf16_store(name):
    model, sb, sf, hist, cand = _tiny(name)
    model.eval()
    assert sb.x.dtype == BF16 and all(t.dtype == BF16 for t, _ in sb.texts.values())
    with torch.no_grad():
        r = model.forward_store(sb, hist, cand)
        ref = model.forward_store(sf, hist, cand)
        H.assert_close(r, ref, tol=H.RTOL, what=f"{name}: bf16 store vs its widened fp32 store")
        v, vm = model.encode_news_ids(sb, hist)
        v0, vm0 = model.encode_news_ids(sf, hist)
        H.assert_close(v, v0, tol=H.RTOL, what=f"{name}: news vectors")
        assert torch.equal(vm, vm0)
        with hip.knobs(**FORCE):  # the direct route wherever the towers have one
            H.assert_close(model.forward_store(sb, hist, cand), ref, tol=H.RTOL, what=f"{name}: direct route")


def test_evaluate_on_a_bf16_store():
    from tests.test_hip_data import model_for, setup
    _, sessions, store, beh = setup()
    c = cases.DATA
    model, _, _ = model_for(c)
    sb = store.to(DEV).astype(BF16)
    res = EV.evaluate(model, sb, beh.to(DEV), c["l_hist"], batch=4)
    ref = EV.evaluate(model, sb.astype(torch.float32), beh.to(DEV), c["l_hist"], batch=4)
    got, want = np.array([res[k] for k in EV.METRIC_NAMES]), np.array([ref[k] for k in EV.METRIC_NAMES])
    assert np.allclose(got, want, rtol=H.RTOL, atol=0), (got, want)


# ------------------------------------------------------------------------------------------------ 8. training
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_grad_step_from_a_bf16_store(p):
    """One grad step of NRMS through forward_store in train mode: the dense fp32 copies of the two stores are the same bits
    (p = 0: the widening gather; p > 0: the same keep mask), so loss and gradients agree far inside GTOL."""
    model, sb, sf, hist, cand = _tiny("nrms_tiny", p)
    model.train()
    w = torch.randn(hist.shape[0], cand.shape[1], 1, device=DEV, generator=_gen(8))
    out = {}
    for key, store in (("bf16", sb), ("fp32", sf)):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(1234)
        r = model.forward_store(store, hist, cand)
        loss = ((r - w) ** 2).mean()
        loss.backward()
        out[key] = (loss.item(), {n: q.grad.clone() for n, q in model.named_parameters() if q.grad is not None})
    (l1, g1), (l0, g0) = out["bf16"], out["fp32"]
    assert abs(l1 - l0) <= GTOL * abs(l0)
    gmax = max(v.abs().max().item() for v in g0.values())
    assert set(g1) == set(g0) and any("att" in n for n in g0)
    for n, ref in g0.items():
        scale = max(ref.abs().max().item(), 1e-3 * gmax)
        e = (g1[n].double() - ref.double()).abs().max().item() / scale
        assert e <= GTOL, f"{n}: {e:.3e}"


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals():
    c = cases.ENCODERS["news_nrms_tiny"]
    enc, _ = _tower(c)
    tb, tm, ids = _table(c)
    n, S, D, E = ids.numel(), c["S"], c["D"], c["E"]
    pool_kind, ap, pp, hp, keep = ops._encoder_params(enc.att, enc.pooler, enc.head)
    l = hip.lib()
    nbytes = l.xnrs_text_encoder_bf16_workspace_bytes(n, S, D, pp.hidden, E, 1, pool_kind, 1, 0)
    assert nbytes > l.xnrs_text_encoder_workspace_bytes(n, S, D, pp.hidden, E, 1, pool_kind, 1, 0)
    ws = hip.workspace(DEV, nbytes)
    y = torch.full((n, E), 7.0, device=DEV)
    hm = torch.full((n,), 7.0, device=DEV)
    rc = l.xnrs_text_encoder_fwd_bf16(hip.ptr(tb), hip.ptr(tm), None, n, S, D, hip.ref(ap), pool_kind, hip.ref(pp), hip.ref(hp),
                                      hip.ptr(y), hip.ptr(hm), 0, hip.ptr(ws), nbytes, hip.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == -1 and bool((y == 7.0).all()) and bool((hm == 7.0).all())  # XNRS_EINVAL, nothing written
    # dedup=True with active input dropout still raises, whatever the table's dtype
    model, sb, _, hist, cand = _tiny("nrms_tiny", 0.25)
    model.train()
    with pytest.raises(hip.XnrsHipError, match="dedup"):
        model.forward_store(sb, hist, cand, dedup=True)
