"""Live row tiles of the dense encoder passes (XNRS_GEMM_LIVE_TILES; encoder_fwd.hip).

The Q|K|V projection and the fc1 product of an inference news-encoder call skip the 128-row tiles that hold only rows of
all-masked news.  Nothing else may change: every comparison between the knob on and off is ``torch.equal``, and the scores
meet the oracle at the usual 1e-4 bar.  The default engages the list from 16 384 token rows per call; the tests lower that
threshold (XNRS_GEMM_LIVE_TILES_MIN_ROWS=0) so that small batches take the path.

Which product takes the list at which shape (one rule, encoder_fwd.hip): fc1 always (the pooler leaves an all-masked news
before it reads a score); Q|K|V where the attention kernel of the shape leaves an all-masked news before it reads a row --
the LDS-staged pair kernel, 33 <= S <= 64.  At S = 30 the head-per-wave attention kernel reads every Q|K|V row, so the
projection stays dense there and only fc1 walks the list; the engagement test asserts exactly that."""
import numpy as np
import pytest
import torch

from oracle import xnrs_oracle as O
from tests import helpers as H
from xnrs_amd import hip, ops, synth
from xnrs_amd.models import make_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BM = 128  # tile height of the list (kernels.h LIVE_TILE_BM)
ON = dict(XNRS_GEMM_LIVE_TILES="1", XNRS_GEMM_LIVE_TILES_MIN_ROWS="0")
OFF = dict(XNRS_GEMM_LIVE_TILES="0")


class Cfg(dict):
    __getattr__ = dict.__getitem__


def build(S, D=768, bias=False, seed=77, H_=12):
    c = dict(model="NRMS", E=256, bias=bias, h=16, D=D, H=H_, S=S)
    model = make_model(Cfg(synth.model_cfg(c)))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = synth.fill_state_dict(shapes, seed)
    model.load_state_dict(sd)
    return model.eval().to(DEV), sd


def batch(S, D=768, B=6, H_=12, C=3, seed=5, pattern="ragged"):
    """(hist, cand) CPU tensors.  pattern: which news are empty (all-zero x and mask).
    ragged: trailing history slots; none; all: every history slot; middle: empty slots inside the histories;
    cand: ragged + some empty candidates."""
    b = synth.make_batch(seed, B, H_, C, S, D, min_len=3, ragged_history=pattern in ("ragged", "cand"))
    hx, hm = b["user_features"]["history"]["title_emb"]
    cx, cm = b["candidate_features"]["title_emb"]
    hx, hm, cx, cm = hx.clone(), hm.clone(), cx.clone(), cm.clone()
    if pattern == "all":
        hx.zero_()
        hm.zero_()
    if pattern == "middle":
        rng = np.random.default_rng(seed)
        dead = torch.from_numpy(rng.random((B, H_)) < 0.6)
        dead[:, 0] = False
        dead[0, 3:9] = True  # a run long enough to hold whole tiles at S >= 50
        hx[dead] = 0
        hm[dead] = 0
    if pattern == "cand":
        cx[1::2, 1] = 0
        cm[1::2, 1] = 0
        cx[0] = 0
        cm[0] = 0
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


@pytest.mark.parametrize("pattern", ["none", "all", "ragged", "middle", "cand"])
@pytest.mark.parametrize("S", [50, 64, 30])
def test_forward_equal_and_oracle(S, pattern):
    model, sd = build(S)
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
    """bias=True: the skipped Q|K|V rows would have held the projection bias; nobody reads them."""
    model, sd = build(50, bias=True, seed=91)
    hist, cand = batch(50, pattern="middle", seed=3)
    r1 = run(model, hist, cand, ON)
    assert torch.equal(r1, run(model, hist, cand, OFF))
    assert torch.equal(run_ids(model, hist, cand, ON), r1)
    H.assert_close(r1, O.parent_forward(hist, cand, sd, 16), what="bias vs oracle")


def test_large_x_on_masked_news_and_masked_keys():
    """The criterion is the mask, never x: an all-masked news with x = 1e30 is still skipped and still head(0); the masked
    tokens of a LIVE news stay keys (their x matters: changing it changes the scores, with the knob on as off)."""
    model, sd = build(50)
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
    # masked tokens inside live news: still keys
    keys = hx.clone()
    tok = (hm.squeeze(-1) == 0) & ~dead[:, :, None]  # masked tokens of live news
    assert tok.any()
    keys[tok] = keys[tok] + 1.0
    k1 = run(model, (keys, hm), cand, ON)
    assert torch.equal(k1, run(model, (keys, hm), cand, OFF))
    assert not torch.equal(k1, r1)
    H.assert_close(k1, O.parent_forward((keys, hm), cand, sd, 16), what="masked keys vs oracle")


def news_inputs(n, S, D, seed, dead_runs):
    """n news (x:(n,S,D), m:(n,S,1)) with the news of `dead_runs` [(first, last+1), ...] empty."""
    rng = synth.rng_for(seed)
    x, m = synth.token_block(rng, 1, n, S, D, min_len=2)
    x, m = x[0].clone(), m[0].clone()
    for a, b in dead_runs:
        x[a:b] = 0
        m[a:b] = 0
    return x, m


def live_tiles_host(m, S, chunk):
    """[(live tiles, all tiles, rows)] per pass, counted on the host from the same mask (mask != 0)."""
    alive = m.reshape(-1, S).ne(0).any(dim=1).cpu().numpy()
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
        out.append((live, nt, rows))
    return out


ENC_CASES = [
    # S, n news, chunk (0 = one pass), empty runs
    (50, 40, 0, [(5, 17), (20, 21), (30, 40)]),
    (50, 41, 7, [(3, 12), (13, 26), (33, 41)]),   # pass and tile boundaries inside empty runs
    (64, 24, 5, [(0, 9), (12, 20)]),
    (30, 60, 0, [(10, 31), (40, 60)]),
    (30, 60, 13, [(0, 25), (30, 52)]),
    (50, 30, 0, []),                              # no empty news: every tile live
    (50, 30, 4, [(0, 30)]),                       # every news empty: no tile live
]


@pytest.mark.parametrize("S,n,chunk,dead", ENC_CASES)
def test_encoder_passes_engagement_and_poisoned_workspace(S, n, chunk, dead):
    """The news encoder alone, dense rows and id gather, with a pass size that puts pass and tile boundaries inside empty
    runs.  (i) knob on == knob off, bit for bit; (ii) the same with the workspace filled with 0xFF bytes (NaN) before the
    call -- no skipped row is read; (iii) the launch timer's executed FLOPs of qkv_gemm and fc1_tanh_gemm are those of the
    live tiles counted on the host, strictly below the dense count whenever a tile is dead."""
    D, A = 768, 256
    model, _ = build(S)
    enc = model.news_encoder
    x, m = news_inputs(n, S, D, 100 + n + chunk, dead)
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
            # engagement: executed FLOPs from the launch timer
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
    passes = live_tiles_host(m, S, chunk or n)
    live_rows = sum(l for l, _, _ in passes) * BM
    rows = sum(r for _, _, r in passes)
    any_dead = any(l < t for l, t, _ in passes)
    qkv_list = 33 <= S <= 64  # the attention kernel of the shape skips all-masked news (module docstring)
    qkv, fc1 = prof["qkv_gemm"][2], prof["fc1_tanh_gemm"][2]
    print(f"S={S} n={n} chunk={chunk}: live tiles {live_rows // BM} of {sum(t for _, t, _ in passes)}; "
          f"qkv flops {qkv:.6g} (dense {2.0 * rows * 3 * D * D:.6g}), fc1 flops {fc1:.6g} (dense {2.0 * rows * A * D:.6g})")
    assert qkv == 2.0 * (live_rows if qkv_list else rows) * 3 * D * D
    assert fc1 == 2.0 * live_rows * A * D
    if any_dead:
        assert fc1 < 2.0 * rows * A * D
        if qkv_list:
            assert qkv < 2.0 * rows * 3 * D * D


def test_default_threshold_keeps_small_calls_dense():
    """Below XNRS_GEMM_LIVE_TILES_MIN_ROWS (default 16 384 token rows per call) no list is built: dense FLOPs."""
    S, D, A, n = 50, 768, 256, 40
    model, _ = build(S)
    x, m = news_inputs(n, S, D, 7, [(5, 30)])
    with torch.no_grad(), hip.knobs(XNRS_GEMM_LIVE_TILES="1", XNRS_GEMM_LIVE_TILES_MIN_ROWS=None):
        hip.profile_enable(0b1001)
        try:
            ops.text_encoder(x.to(DEV), m.to(DEV), model.news_encoder)
            torch.cuda.synchronize()
            prof = hip.profile_read()
        finally:
            hip.profile_enable(0)
    assert prof["qkv_gemm"][2] == 2.0 * n * S * 3 * D * D
    assert prof["fc1_tanh_gemm"][2] == 2.0 * n * S * A * D


def test_hipgraph_replay_with_another_empty_pattern():
    """The launch sequence does not depend on the data: a captured step replayed on a batch with a different empty
    pattern, written into the same tensors, equals the eager step on that batch."""
    S = 50
    model, _ = build(S)
    a_h, a_c = batch(S, pattern="ragged", seed=31)
    b_h, b_c = batch(S, pattern="middle", seed=32)
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
