"""Q and K|V of a dense live-row pass in one launch (XNRS_GEMM_QKV_ONE_LAUNCH; gemm_f32.hip gemm_qkv_one_launch_kernel,
DESIGN.md section 4.1 "One launch").

Where a dense encoder pass projects K|V over its live row tiles and Q over its live-row list (33 <= S <= 64, the
LDS-staged pair attention kernel) from dense rows, the two products go out as ONE grid: the K|V tiles first, the Q tiles
behind them (calls with ids keep the two launches, and must keep their bits).
Each section runs the body of the instantiation its own launch would run, so nothing may change: every comparison
between the knob on and off (off = the two launches) is ``torch.equal``, with the workspace poisoned before the call;
the launch counter says which route ran (the launch timer's executed FLOPs are the same on both and cannot tell).  The
default thresholds engage the lists from 16 384 token rows per call; the tests lower both to 0."""
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
BASE = dict(XNRS_GEMM_LIVE_TILES="1", XNRS_GEMM_LIVE_TILES_MIN_ROWS="0", XNRS_GEMM_LIVE_ROWS="1", XNRS_GEMM_LIVE_ROWS_MIN_ROWS="0")
ON = dict(BASE, XNRS_GEMM_QKV_ONE_LAUNCH="1")
OFF = dict(BASE, XNRS_GEMM_QKV_ONE_LAUNCH="0")   # two launches


class Cfg(dict):
    __getattr__ = dict.__getitem__


def build(S, D=768, bias=False, seed=77, H_=12):
    c = dict(model="NRMS", E=256, bias=bias, h=16, D=D, H=H_, S=S)
    model = make_model(Cfg(synth.model_cfg(c)))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = synth.fill_state_dict(shapes, seed)
    model.load_state_dict(sd)
    return model.eval().to(DEV), sd


_models = {}


def model_for(S, **kw):
    key = (S, tuple(sorted(kw.items())))
    if key not in _models:
        _models[key] = build(S, **kw)
    return _models[key]


def batch(S, D=768, B=6, H_=12, C=3, seed=5, holes=False):
    """(hist, cand) CPU tensors: prefix masks (lengths 1 and S forced), trailing history slots empty; holes: zeros inside
    the titles too."""
    b = synth.make_batch(seed, B, H_, C, S, D, min_len=1, ragged_history=True)
    hx, hm = b["user_features"]["history"]["title_emb"]
    cx, cm = b["candidate_features"]["title_emb"]
    hx, hm, cx, cm = hx.clone(), hm.clone(), cx.clone(), cm.clone()
    hm[0, 0, 1:] = 0
    hm[1, 0, :] = 1
    cm[0, 0, 1:] = 0
    cm[1, 0, :] = 1
    if holes:
        rng = np.random.default_rng(seed)
        for m in (hm, cm):
            m[torch.from_numpy(rng.random(tuple(m.shape)) < 0.3)] = 0
    return (hx, hm), (cx, cm)


def to_dev(p):
    return tuple(t.to(DEV) for t in p)


def launches(reset=True):
    return hip.lib().xnrs_qkv_launch_count(1 if reset else 0)


def news_inputs(n, S, D, chunk, seed):
    """n news (x:(n,S,D), m:(n,S,1)) in passes of `chunk`, by pass:
      0      prefix masks, an empty news in the middle, mask values 0.5 and 2.0 on some unmasked tokens
      1      empty news only: both device counts 0, every workgroup of the launch leaves
      2      every token of every news unmasked: the Q section at the size the grid was made for
      3 ...  prefix masks with holes inside the titles, an empty news in the middle of each
      last   short."""
    rng = synth.rng_for(seed)
    x, m = synth.token_block(rng, 1, n, S, D, min_len=1)
    x, m = x[0].clone(), m[0].clone()
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(tuple(m.shape), generator=g)
    m[:chunk][(u[:chunk] < 0.2) & (m[:chunk] != 0)] = 0.5
    m[:chunk][(u[:chunk] > 0.8) & (m[:chunk] != 0)] = 2.0
    m[0, 1:] = 0          # prefix length 1 ...
    m[chunk - 1, :] = 1   # ... and S
    x[chunk - 1] = torch.randn(S, D, generator=g)
    x[2] = 0
    m[2] = 0
    x[chunk:2 * chunk] = 0
    m[chunk:2 * chunk] = 0
    x[2 * chunk:3 * chunk] = torch.randn(chunk, S, D, generator=g)
    m[2 * chunk:3 * chunk] = 1
    hole = u < 0.25
    hole[:3 * chunk] = False
    m[hole] = 0
    for c0 in range(3 * chunk, n, chunk):
        if c0 + 1 < n:
            x[c0 + 1] = 0
            m[c0 + 1] = 0
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


def encode(x, m, enc, chunk, knobs, ids=None, timer=False):
    """One encoder call under `knobs` -> (y, hm, GEMM launches of the live-row Q|K|V branch, qkv_gemm executed FLOPs)."""
    with torch.no_grad(), hip.knobs(**knobs):
        for attempt in range(2):  # (the workspace only grows: a call that had to grow it runs again, in the poisoned buffer)
            ws = hip.workspace(DEV, 1)
            ws.fill_(0xFF)  # NaN everywhere: no unwritten Q row may be read
            launches()
            if timer:
                hip.profile_enable(0b1)
            try:
                y, hm = ops.text_encoder(x, m, enc, ids=ids, chunk=chunk)
                torch.cuda.synchronize()
                fl = hip.profile_read()["qkv_gemm"][2] if timer else None
            finally:
                if timer:
                    hip.profile_enable(0)
            if hip.workspace(DEV, 1) is ws:
                return y, hm, launches(), fl
    raise AssertionError("the call did not run in the poisoned workspace")


# S, n news, news per pass.  Every case: >= 4 passes, a short last pass, a pass of empty news only, an all-live pass.
ENC_CASES = [(50, 41, 12), (64, 27, 5), (33, 50, 8)]


@pytest.mark.parametrize("route", ["dense", "ids"])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("S,n,chunk", ENC_CASES)
def test_one_launch_equals_two_launches(S, n, chunk, bias, route):
    D = 768
    model, _ = model_for(S, bias=bias, seed=91 if bias else 77)
    enc = model.news_encoder
    x, m = news_inputs(n, S, D, chunk, 200 + n + chunk)
    passes = lists_host(m, S, chunk)
    assert len(passes) >= 4 and passes[-1][2] < passes[0][2]
    assert passes[1][0] == 0 and passes[1][3] == 0          # a pass of empty news only
    assert passes[2][3] == passes[2][2]                     # an all-live pass
    assert any(p[3] % BM and p[3] % 64 for p in passes)     # live-row counts that are no multiple of the Q tile height or its half
    assert (m != 0).any() and ((m != 0) & (m != 1)).any()   # non-binary values
    if route == "ids":  # a permuted table, id 0 = the empty slot
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(n))
        xd = torch.cat([torch.zeros(1, S, D), x[perm]]).to(DEV)
        md = torch.cat([torch.zeros(1, S, 1), m[perm]]).to(DEV)
        ids = (torch.argsort(perm) + 1).to(torch.int32)
        ids[~m.reshape(n, S).ne(0).any(dim=1)] = 0
        ids = ids.to(DEV)
    else:
        xd, md, ids = x.to(DEV), m.to(DEV), None
    y0, hm0, l0, _ = encode(xd, md, enc, chunk, OFF, ids)
    y1, hm1, l1, _ = encode(xd, md, enc, chunk, ON, ids)
    assert torch.isfinite(y0).all() and torch.isfinite(y1).all()
    assert torch.equal(y1, y0) and torch.equal(hm1, hm0)
    # dense rows: one launch per pass.  With ids the entry is not built (a gathered K|V section next to the Q body compiles
    # with a scratch reload in its K loop): those calls keep the two launches under either knob value
    per_pass = 1 if route == "dense" else 2
    assert (l0, l1) == (2 * len(passes), per_pass * len(passes))
    # the launch timer: the same executed FLOPs on both routes (the live tiles' K|V, the live rows' Q)
    f0 = encode(xd, md, enc, chunk, OFF, ids, timer=True)[3]
    y1t, hm1t, l1t, f1 = encode(xd, md, enc, chunk, ON, ids, timer=True)
    tile_rows = sum(p[0] for p in passes) * BM
    live = sum(p[3] for p in passes)
    print(f"S={S} n={n} chunk={chunk} bias={bias} {route}: launches {l0} / {l1}, qkv flops {f0:.6g} / {f1:.6g}")
    assert f0 == f1 == 2.0 * tile_rows * 2 * D * D + 2.0 * live * D * D
    assert l1t == per_pass * len(passes) and torch.equal(y1t, y0) and torch.equal(hm1t, hm0)


def test_short_sequences_keep_their_route():
    """S = 30: the head-per-wave attention kernel reads every Q|K|V row, the projection stays one dense launch over the live
    tiles; the live-row Q|K|V branch -- and with it the one-launch route -- does not engage."""
    S, n, chunk = 30, 60, 13
    model, _ = model_for(S)
    x, m = news_inputs(n, S, 768, chunk, 17)
    y0, hm0, l0, _ = encode(x.to(DEV), m.to(DEV), model.news_encoder, chunk, OFF)
    y1, hm1, l1, _ = encode(x.to(DEV), m.to(DEV), model.news_encoder, chunk, ON)
    assert (l0, l1) == (0, 0)
    assert torch.equal(y1, y0) and torch.equal(hm1, hm0)


def test_whole_model_against_the_oracle():
    S = 50
    model, sd = model_for(S)
    hist, cand = batch(S, seed=61, holes=True)
    with hip.knobs(**ON), torch.no_grad():
        launches()
        r1 = model._forward(to_dev(hist), to_dev(cand))
        torch.cuda.synchronize()
        n1 = launches()
    with hip.knobs(**OFF), torch.no_grad():
        r0 = model._forward(to_dev(hist), to_dev(cand))
        torch.cuda.synchronize()
        n0 = launches()
    assert n1 >= 1 and n0 == 2 * n1
    assert torch.isfinite(r1).all() and torch.equal(r1, r0)
    H.assert_close(r1, O.parent_forward(hist, cand, sd, 16), what="one launch vs oracle")


def test_hipgraph_replay_with_another_mask_pattern():
    """The grid is the worst case of both sections and the two counts stay on the device: a captured step replayed after a
    different mask pattern was written into the same tensors equals the eager step on that batch."""
    S = 50
    model, _ = model_for(S)
    a_h, a_c = batch(S, seed=31)
    b_h, b_c = batch(S, seed=32, holes=True)
    with hip.knobs(**ON), torch.no_grad():
        launches()
        ref_a = model._forward(to_dev(a_h), to_dev(a_c))
        assert launches() >= 1  # one launch per pass, the route under test
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
