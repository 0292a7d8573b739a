"""Live rows of the dense encoder passes (XNRS_GEMM_LIVE_ROWS; encoder_fwd.hip "live rows").

Where a dense news-encoder pass walks the live row tiles, the Q projection and the fc1 product run over the list of the
pass's UNMASKED token rows only (mask != 0), gathered and scattered in place; K|V keep every row of the live tiles, since
a masked token stays a key and a value.  The Q rows and scores of masked tokens are never written -- and never read.
Nothing else may change: every comparison between the knob on and off (off = the live-tile path) is ``torch.equal``, the
scores meet the oracle at the usual 1e-4 bar, and non-binary mask values keep their dense meaning.  The default engages the
lists from 16 384 token rows per call; the tests lower both thresholds so that small batches take the path.

Which product takes the row list at which shape (one rule, encoder_fwd.hip): fc1 always; Q where the attention kernel of
the shape is the LDS-staged pair kernel, 33 <= S <= 64 (it reads no Q row of a masked query).  At S = 30 the head-per-wave
attention kernel reads every Q|K|V row, so the projection stays dense there and only fc1 walks the list."""
import numpy as np
import pytest
import torch

from oracle import xnrs_oracle as O
from tests import helpers as H
from xnrs_amd import hip, ops, synth
from xnrs_amd.models import make_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BM = 128  # tile height of the tile list (kernels.h LIVE_TILE_BM)
BASE = dict(XNRS_GEMM_LIVE_TILES="1", XNRS_GEMM_LIVE_TILES_MIN_ROWS="0", XNRS_GEMM_LIVE_ROWS_MIN_ROWS="0")
ON = dict(BASE, XNRS_GEMM_LIVE_ROWS="1")
OFF = dict(BASE, XNRS_GEMM_LIVE_ROWS="0")  # today's live-tile path


class Cfg(dict):
    __getattr__ = dict.__getitem__


def build(S, D=768, bias=False, seed=77, H_=12):
    c = dict(model="NRMS", E=256, bias=bias, h=16, D=D, H=H_, S=S)
    model = make_model(Cfg(synth.model_cfg(c)))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = synth.fill_state_dict(shapes, seed)
    model.load_state_dict(sd)
    return model.eval().to(DEV), sd


PATTERNS = ["prefix", "full", "all", "middle", "cand", "holes", "nonbinary"]


def batch(S, D=768, B=6, H_=12, C=3, seed=5, pattern="prefix"):
    """(hist, cand) CPU tensors.
    prefix: prefix masks of lengths 1..S (1 and S forced), trailing history slots empty; full: every token of every news
    unmasked; all: every history news empty; middle: empty news inside the histories; cand: prefix + some empty
    candidates; holes: zeros INSIDE the titles (x stays: those tokens are still keys); nonbinary: mask values 0.5 and 2.0
    on some unmasked tokens."""
    full = pattern == "full"
    b = synth.make_batch(seed, B, H_, C, S, D, min_len=S if full else 1, ragged_history=pattern in ("prefix", "cand", "holes", "nonbinary"))
    hx, hm = b["user_features"]["history"]["title_emb"]
    cx, cm = b["candidate_features"]["title_emb"]
    hx, hm, cx, cm = hx.clone(), hm.clone(), cx.clone(), cm.clone()
    if not full:  # prefix lengths 1 and S are always present (history slot 0 exists for every user)
        hm[0, 0, 1:] = 0
        hm[1, 0, :] = 1
        cm[0, 0, 1:] = 0
        cm[1, 0, :] = 1
    rng = np.random.default_rng(seed)
    if pattern == "all":
        hx.zero_()
        hm.zero_()
    if pattern == "middle":
        dead = torch.from_numpy(rng.random((B, H_)) < 0.6)
        dead[:, 0] = False
        dead[0, 3:9] = True  # a run long enough to hold whole tiles at S >= 50
        hx[dead] = 0
        hm[dead] = 0
    if pattern == "cand":
        cx[1::2, 1] = 0
        cm[1::2, 1] = 0
        cx[2] = 0
        cm[2] = 0
    if pattern == "holes":
        for m in (hm, cm):
            hole = torch.from_numpy(rng.random(tuple(m.shape)) < 0.3)
            m[hole] = 0  # also first tokens, also whole short titles now and then
    if pattern == "nonbinary":
        for m in (hm, cm):
            u = torch.from_numpy(rng.random(tuple(m.shape)))
            m[(u < 0.2) & (m != 0)] = 0.5
            m[(u > 0.8) & (m != 0)] = 2.0
    return (hx, hm), (cx, cm)


def to_dev(p):
    return tuple(t.to(DEV) for t in p)


def run(model, hist, cand, knobs):
    with hip.knobs(**knobs), torch.no_grad():
        r = model._forward(to_dev(hist), to_dev(cand))
        torch.cuda.synchronize()
    return r


def table_of(hist, cand):
    """The same batch as a news table + ids (row 0 = the empty slot, as NewsStore lays it out)."""
    hx, hm = hist
    cx, cm = cand
    B, H_, S, D = hx.shape
    C = cx.shape[1]
    x = torch.cat([torch.zeros(1, S, D), hx.reshape(B * H_, S, D), cx.reshape(B * C, S, D)])
    m = torch.cat([torch.zeros(1, S), hm.reshape(B * H_, S), cm.reshape(B * C, S)])
    hid = torch.arange(1, 1 + B * H_, dtype=torch.int32).reshape(B, H_)
    cid = torch.arange(1 + B * H_, 1 + B * H_ + B * C, dtype=torch.int32).reshape(B, C)
    hid = torch.where(hm.reshape(B, H_, S).ne(0).any(-1), hid, torch.zeros_like(hid))  # empty slots -> id 0
    return x.to(DEV), m.to(DEV), hid.to(DEV), cid.to(DEV)


def run_ids(model, hist, cand, knobs):
    tx, tm, hid, cid = table_of(hist, cand)
    with hip.knobs(**knobs), torch.no_grad():
        r = model.forward_ids(tx, tm, hid, cid)
        torch.cuda.synchronize()
    return r


_models = {}


def model_for(S, **kw):
    key = (S, tuple(sorted(kw.items())))
    if key not in _models:
        _models[key] = build(S, **kw)
    return _models[key]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("S", [50, 64, 33, 30])
def test_forward_equal_and_oracle(S, pattern):
    model, sd = model_for(S)
    hist, cand = batch(S, pattern=pattern, seed=11 + S)
    r1 = run(model, hist, cand, ON)
    r0 = run(model, hist, cand, OFF)
    assert torch.isfinite(r1).all()
    assert torch.equal(r1, r0)
    H.assert_close(r1, O.parent_forward(hist, cand, sd, 16), what=f"S={S} {pattern} vs oracle")
    i1 = run_ids(model, hist, cand, ON)
    i0 = run_ids(model, hist, cand, OFF)
    assert torch.equal(i1, i0)
    assert torch.equal(i1, r1)  # the id path takes the same kernels' bits


def test_biases_on():
    """bias=True: the skipped Q rows would have held the projection bias; nobody reads them."""
    model, sd = model_for(50, bias=True, seed=91)
    hist, cand = batch(50, pattern="middle", seed=3)
    r1 = run(model, hist, cand, ON)
    assert torch.equal(r1, run(model, hist, cand, OFF))
    assert torch.equal(run_ids(model, hist, cand, ON), r1)
    H.assert_close(r1, O.parent_forward(hist, cand, sd, 16), what="bias vs oracle")


def test_per_token_out_projection_order():
    """XNRS_FOLD_OUT=0: the out-projection runs per token row (dense, every O row is defined) and fc1 gathers the live
    rows of ITS output; the row lists change no bit there either."""
    model, sd = model_for(50)
    hist, cand = batch(50, pattern="holes", seed=8)
    r1 = run(model, hist, cand, dict(ON, XNRS_FOLD_OUT="0"))
    assert torch.isfinite(r1).all()
    assert torch.equal(r1, run(model, hist, cand, dict(OFF, XNRS_FOLD_OUT="0")))
    assert torch.equal(run_ids(model, hist, cand, dict(ON, XNRS_FOLD_OUT="0")), r1)
    H.assert_close(r1, O.parent_forward(hist, cand, sd, 16), what="per-token out-projection vs oracle")


def test_large_x_on_masked_tokens_and_masked_news():
    """The criterion is the mask, never x.  An all-masked news with x = 1e30 reaches nothing.  The masked tokens of a LIVE
    news stay keys and values -- only their Q and fc1 rows disappear: large finite x there changes the scores exactly as
    it does with the lists off, and as the oracle says."""
    model, sd = model_for(50)
    hist, cand = batch(50, pattern="middle", seed=21)
    hx, hm = hist
    dead = ~hm.ne(0).any(dim=2).squeeze(-1)  # (B, H)
    assert dead.any()
    big = hx.clone()
    big[dead] = 1e30
    r1 = run(model, (big, hm), cand, ON)
    assert torch.isfinite(r1).all()
    assert torch.equal(r1, run(model, (big, hm), cand, OFF))
    assert torch.equal(r1, run(model, hist, cand, ON))  # x of an all-masked news reaches nothing
    H.assert_close(r1, O.parent_forward(hist, cand, sd, 16), what="1e30 vs oracle")
    # masked tokens inside live news: still keys and values.  8.0 is large against the N(0, 1) tokens and leaves the fp32
    # rounding of the logits (which grows with |x|) well inside the oracle bar.
    keys = hx.clone()
    tok = (hm.squeeze(-1) == 0) & ~dead[:, :, None]
    assert tok.any()
    keys[tok] = keys[tok] + 8.0
    k1 = run(model, (keys, hm), cand, ON)
    assert torch.isfinite(k1).all()
    assert torch.equal(k1, run(model, (keys, hm), cand, OFF))
    assert torch.equal(run_ids(model, (keys, hm), cand, ON), k1)
    assert not torch.equal(k1, r1)
    H.assert_close(k1, O.parent_forward((keys, hm), cand, sd, 16), what="masked keys vs oracle")


def news_inputs(n, S, D, seed, dead_runs, holes=False):
    """n news (x:(n,S,D), m:(n,S,1)) with the news of `dead_runs` [(first, last+1), ...] empty."""
    rng = synth.rng_for(seed)
    x, m = synth.token_block(rng, 1, n, S, D, min_len=1)
    x, m = x[0].clone(), m[0].clone()
    if holes:
        m[torch.from_numpy(rng.random(tuple(m.shape)) < 0.25)] = 0
    for a, b in dead_runs:
        x[a:b] = 0
        m[a:b] = 0
    return x, m


def lists_host(m, S, chunk):
    """[(live tiles, all tiles, rows, live rows)] per pass, counted on the host from the same mask (mask != 0)."""
    on = m.reshape(-1, S).ne(0).cpu().numpy()
    alive = on.any(axis=1)
    n = alive.shape[0]
    out = []
    for c0 in range(0, n, chunk):
        nc = min(chunk, n - c0)
        rows = nc * S
        nt = (rows + BM - 1) // BM
        live = 0
        for t in range(nt):
            r0, r1 = t * BM, min((t + 1) * BM, rows) - 1
            live += bool(alive[c0 + r0 // S: c0 + r1 // S + 1].any())
        out.append((live, nt, rows, int(on[c0:c0 + nc].sum())))
    return out


ENC_CASES = [
    # S, n news, news per pass, empty runs, holes.  Every case: >= 3 passes, a short last pass, a pass of empty news only.
    (50, 41, 12, [(12, 24), (30, 33)], False),   # passes 12 | 12 (all empty) | 12 | 5
    (64, 27, 5, [(0, 3), (10, 15), (22, 24)], True),
    (33, 50, 8, [(8, 16), (17, 30), (44, 50)], True),   # the last (short) pass all empty too
    (30, 60, 13, [(0, 13), (30, 52)], False),    # fc1-only route
    (50, 30, 4, [(0, 30)], False),               # every news empty: every count 0, the Q and fc1 launches leave
]


@pytest.mark.parametrize("S,n,chunk,dead,holes", ENC_CASES)
def test_encoder_passes_engagement_and_poisoned_workspace(S, n, chunk, dead, holes):
    """The news encoder alone, dense rows and id gather, several passes.  (i) lists on == lists off, bit for bit; (ii) the
    same with the workspace filled with 0xFF bytes (NaN) before the call -- no unwritten Q row, O row or score is read;
    (iii) the launch timer's executed FLOPs of qkv_gemm and fc1_tanh_gemm are those of the live tiles (K|V) and the live
    rows (Q, fc1) counted on the host."""
    D, A = 768, 256
    model, _ = model_for(S)
    enc = model.news_encoder
    x, m = news_inputs(n, S, D, 100 + n + chunk, dead, holes)
    passes = lists_host(m, S, chunk)
    assert len(passes) >= 3 and passes[-1][2] < passes[0][2]
    assert any(p[3] == 0 for p in passes)
    if any(p[3] for p in passes):
        assert any(p[3] % BM for p in passes)  # a live-row count that is no multiple of the tile height
    xd, md = x.to(DEV), m.to(DEV)
    with torch.no_grad():
        with hip.knobs(**OFF):
            y0, hm0 = ops.text_encoder(xd, md, enc, chunk=chunk)
        ws = hip.workspace(DEV, 1)
        with hip.knobs(**ON):
            ws.fill_(0xFF)
            y1, hm1 = ops.text_encoder(xd, md, enc, chunk=chunk)
            assert hip.workspace(DEV, 1) is ws  # the call ran in the poisoned buffer
            # the same news through a table with ids (a permuted table, id 0 = the empty slot)
            perm = torch.randperm(n, generator=torch.Generator().manual_seed(n))
            tx = torch.cat([torch.zeros(1, S, D), x[perm]]).to(DEV)
            tm = torch.cat([torch.zeros(1, S, 1), m[perm]]).to(DEV)
            ids = (torch.argsort(perm) + 1).to(torch.int32)
            ids[~m.reshape(n, S).ne(0).any(dim=1)] = 0
            ws.fill_(0xFF)
            y2, hm2 = ops.text_encoder(tx, tm, enc, ids=ids.to(DEV), chunk=chunk)
            hip.profile_enable(0b1001)
            try:
                ops.text_encoder(xd, md, enc, chunk=chunk)
                torch.cuda.synchronize()
                prof = hip.profile_read()
            finally:
                hip.profile_enable(0)
        torch.cuda.synchronize()
    assert torch.isfinite(y1).all() and torch.isfinite(y2).all()
    assert torch.equal(y1, y0) and torch.equal(hm1, hm0)
    assert torch.equal(y2, y0) and torch.equal(hm2, hm0)
    tile_rows = sum(p[0] for p in passes) * BM
    rows = sum(p[2] for p in passes)
    live = sum(p[3] for p in passes)
    q_list = 33 <= S <= 64  # the attention kernel of the shape reads no Q row of a masked query (module docstring)
    qkv, fc1 = prof["qkv_gemm"][2], prof["fc1_tanh_gemm"][2]
    print(f"S={S} n={n} chunk={chunk}: live rows {live} of {rows}, live tiles {tile_rows // BM}; qkv flops {qkv:.6g} "
          f"(dense {2.0 * rows * 3 * D * D:.6g}), fc1 flops {fc1:.6g} (dense {2.0 * rows * A * D:.6g})")
    assert qkv == (2.0 * tile_rows * 2 * D * D + 2.0 * live * D * D if q_list else 2.0 * rows * 3 * D * D)
    assert fc1 == 2.0 * live * A * D
    assert fc1 < 2.0 * tile_rows * A * D or tile_rows == 0


def flops_of(x, m, enc, **knobs):
    with torch.no_grad(), hip.knobs(**knobs):
        hip.profile_enable(0b1001)
        try:
            ops.text_encoder(x.to(DEV), m.to(DEV), enc)
            torch.cuda.synchronize()
            prof = hip.profile_read()
        finally:
            hip.profile_enable(0)
    return prof["qkv_gemm"][2], prof["fc1_tanh_gemm"][2]


def test_default_threshold():
    """Defaults: a call of one impression's size stays on the dense launches (no list is built); a call of 16 384 token
    rows or more takes the lists (executed FLOPs of the live tiles / live rows); XNRS_GEMM_LIVE_ROWS=0 leaves that call
    on the live tiles, XNRS_GEMM_LIVE_TILES=0 on the dense launches."""
    S, D, A = 50, 768, 256
    model, _ = model_for(S)
    dflt = dict(XNRS_GEMM_LIVE_TILES=None, XNRS_GEMM_LIVE_TILES_MIN_ROWS=None, XNRS_GEMM_LIVE_ROWS=None,
                XNRS_GEMM_LIVE_ROWS_MIN_ROWS=None)
    n = 55
    x, m = news_inputs(n, S, D, 7, [(20, 45)])
    assert flops_of(x, m, model.news_encoder, **dflt) == (2.0 * n * S * 3 * D * D, 2.0 * n * S * A * D)
    n = 330  # 16 500 token rows
    x, m = news_inputs(n, S, D, 9, [(100, 250)])
    (tiles, _, rows, live), = lists_host(m, S, n)
    assert flops_of(x, m, model.news_encoder, **dflt) == (2.0 * tiles * BM * 2 * D * D + 2.0 * live * D * D, 2.0 * live * A * D)
    assert flops_of(x, m, model.news_encoder, **dict(dflt, XNRS_GEMM_LIVE_ROWS="0")) == (2.0 * tiles * BM * 3 * D * D,
                                                                                       2.0 * tiles * BM * A * D)
    assert flops_of(x, m, model.news_encoder, **dict(dflt, XNRS_GEMM_LIVE_TILES="0")) == (2.0 * rows * 3 * D * D, 2.0 * rows * A * D)


def test_hipgraph_replay_with_another_mask_pattern():
    """The launch sequence does not depend on the data: a captured step replayed after a different mask pattern was
    written into the same tensors equals the eager step on that batch."""
    S = 50
    model, _ = model_for(S)
    a_h, a_c = batch(S, pattern="prefix", seed=31)
    b_h, b_c = batch(S, pattern="holes", seed=32)
    with hip.knobs(**ON), torch.no_grad():
        ref_a = model._forward(to_dev(a_h), to_dev(a_c))
        ref_b = model._forward(to_dev(b_h), to_dev(b_c))
        static_h, static_c = to_dev(a_h), to_dev(a_c)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                model._forward(static_h, static_c)  # warm-up on the side stream (workspace allocation)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = model._forward(static_h, static_c)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref_a)
        for dst, src in zip(static_h + static_c, b_h + b_c):
            dst.copy_(src.to(DEV))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref_b)
    assert not torch.equal(ref_a, ref_b)
