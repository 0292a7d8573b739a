"""fc1 of the previous pass in the tail of the Q|K|V projection launch (XNRS_GEMM_FC1_IN_TAIL; gemm_f32.hip
gemm_qkv_fc1_launch_kernel, encoder_fwd.hip "fc1 in the tail").

Where a dense encoder call takes the one-launch projection and its pooler's fc1 walks the live-row list behind a folded
out-projection, the sequence per pass i becomes launch{K|V(i), Q(i), fc1(i-1)} -> pool(i-1) -> mha(i); the last pass keeps
an fc1 launch of its own.  The third section runs the body of the instantiation the stand-alone launch runs, so nothing
may change: every comparison between the knob on and off is ``torch.equal``, with the workspace poisoned before the call
and different data in every pass (a pool(i-1) placed behind mha(i) would read the O rows of the wrong pass).  The counter
says which route ran.  The default thresholds engage the lists from 16 384 token rows per call; the tests lower both to 0."""
import pytest
import torch

from oracle import xnrs_oracle as O
from tests import helpers as H
from tests import test_hip_qkv_one_launch as Q
from xnrs_amd import hip, ops

pytestmark = pytest.mark.gpu
DEV = Q.DEV
D, A = 768, 256
ON = dict(Q.BASE, XNRS_GEMM_QKV_ONE_LAUNCH="1", XNRS_GEMM_FC1_IN_TAIL="1")
OFF = dict(Q.BASE, XNRS_GEMM_QKV_ONE_LAUNCH="1", XNRS_GEMM_FC1_IN_TAIL="0")   # today's launches


def in_tail(reset=True):
    return hip.lib().xnrs_fc1_in_tail_count(1 if reset else 0)


def encode(x, m, enc, chunk, knobs, ids=None, timer=0):
    """One encoder call under `knobs` in a poisoned workspace -> (y, hm, fc1 products in a projection launch, GEMM launches of
    the live-row Q|K|V branch, qkv_gemm executed FLOPs or None)."""
    with torch.no_grad(), hip.knobs(**knobs):
        for attempt in range(2):  # (the workspace only grows: a call that had to grow it runs again, in the poisoned buffer)
            ws = hip.workspace(DEV, 1)
            ws.fill_(0xFF)  # NaN everywhere: no unwritten row may be read
            in_tail()
            Q.launches()
            if timer:
                hip.profile_enable(timer)
            try:
                y, hm = ops.text_encoder(x, m, enc, ids=ids, chunk=chunk)
                torch.cuda.synchronize()
                fl = hip.profile_read()["qkv_gemm"][2] if timer else None
            finally:
                if timer:
                    hip.profile_enable(0)
            if hip.workspace(DEV, 1) is ws:
                return y, hm, in_tail(), Q.launches(), fl
    raise AssertionError("the call did not run in the poisoned workspace")


def inputs(S, n, chunk):
    """Q.news_inputs: random rows, so every pass holds other data; masks with holes and non-binary values."""
    return Q.news_inputs(n, S, D, chunk, 300 + n + chunk)


# S, n news, news per pass: >= 4 passes, a pass of empty news only, an all-live pass, a short last pass (as test_hip_qkv_one_launch);
# then one pass (only the drain) and two full passes
CASES = Q.ENC_CASES + [(50, 12, 12), (50, 24, 12)]


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("S,n,chunk", CASES)
def test_knob_on_equals_knob_off(S, n, chunk, bias):
    model, _ = Q.model_for(S, bias=bias, seed=91 if bias else 77)
    enc = model.news_encoder
    if n > 2 * chunk:
        x, m = inputs(S, n, chunk)
        passes = Q.lists_host(m, S, chunk)
        assert len(passes) >= 4 and passes[-1][2] < passes[0][2]
        assert passes[1][0] == 0 and passes[1][3] == 0          # a pass of empty news only
        assert passes[2][3] == passes[2][2]                     # an all-live pass
    else:   # one or two full passes: prefix masks with holes and non-binary values, different rows in every pass
        x, m = Q.news_inputs(4 * chunk, S, D, chunk, 300 + n + chunk)
        keep = torch.cat([torch.arange(0, chunk), torch.arange(3 * chunk, 4 * chunk)])[:n]
        x, m = x[keep].clone(), m[keep].clone()
        passes = Q.lists_host(m, S, chunk)
        assert len(passes) == n // chunk and all(p[3] > 0 for p in passes)
    assert ((m != 0) & (m != 1)).any() and (m == 0).any()       # non-binary values, masked tokens
    xd, md = x.to(DEV), m.to(DEV)
    y0, hm0, t0, l0, _ = encode(xd, md, enc, chunk, OFF)
    y1, hm1, t1, l1, _ = encode(xd, md, enc, chunk, ON)
    print(f"S={S} n={n} chunk={chunk} bias={bias}: passes {len(passes)}, fc1 in the tail {t0} / {t1}, qkv launches {l0} / {l1}")
    assert torch.isfinite(y0).all() and torch.isfinite(y1).all()
    assert torch.equal(y1, y0) and torch.equal(hm1, hm0)
    assert (t0, t1) == (0, len(passes) - 1)
    assert (l0, l1) == (len(passes), len(passes))
    # stage 0 of the launch timer: the same executed FLOPs on both routes, the merged route taken under it
    _, _, t0f, _, f0 = encode(xd, md, enc, chunk, OFF, timer=0b1)
    y1f, hm1f, t1f, l1f, f1 = encode(xd, md, enc, chunk, ON, timer=0b1)
    tile_rows = sum(p[0] for p in passes) * Q.BM
    live = sum(p[3] for p in passes)
    assert f0 == f1 == 2.0 * tile_rows * 2 * D * D + 2.0 * live * D * D
    assert (t0f, t1f, l1f) == (0, len(passes) - 1, len(passes))
    assert torch.equal(y1f, y0) and torch.equal(hm1f, hm0)
    # ... and with stage 3 selected the call takes the separate launches
    y1t, hm1t, t1t, l1t, _ = encode(xd, md, enc, chunk, ON, timer=0b1001)
    assert t1t == 0 and l1t == len(passes)
    assert torch.equal(y1t, y0) and torch.equal(hm1t, hm0)


def test_ids_keep_their_route():
    S, n, chunk = 50, 41, 12
    model, _ = Q.model_for(S)
    x, m = inputs(S, n, chunk)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n))
    xd = torch.cat([torch.zeros(1, S, D), x[perm]]).to(DEV)
    md = torch.cat([torch.zeros(1, S, 1), m[perm]]).to(DEV)
    ids = (torch.argsort(perm) + 1).to(torch.int32)
    ids[~m.reshape(n, S).ne(0).any(dim=1)] = 0
    ids = ids.to(DEV)
    y0, hm0, t0, _, _ = encode(xd, md, model.news_encoder, chunk, OFF, ids)
    y1, hm1, t1, _, _ = encode(xd, md, model.news_encoder, chunk, ON, ids)
    assert (t0, t1) == (0, 0)
    assert torch.equal(y1, y0) and torch.equal(hm1, hm0)
    # the same news through ids and as dense rows: the same vectors (the dense call takes the merged route)
    y2, hm2, t2, _, _ = encode(x.to(DEV), m.to(DEV), model.news_encoder, chunk, ON)
    assert t2 == len(Q.lists_host(m, S, chunk)) - 1
    assert torch.equal(y2, y1) and torch.equal(hm2, hm1)


def test_whole_model_against_the_oracle():
    S = 50
    model, sd = Q.model_for(S)
    hist, cand = Q.batch(S, seed=61, holes=True)
    with hip.knobs(**ON), torch.no_grad():
        in_tail()
        r1 = model._forward(Q.to_dev(hist), Q.to_dev(cand))
        torch.cuda.synchronize()
        n1 = in_tail()
    with hip.knobs(**OFF), torch.no_grad():
        r0 = model._forward(Q.to_dev(hist), Q.to_dev(cand))
        torch.cuda.synchronize()
        n0 = in_tail()
    print(f"fc1 products in a projection launch: {n1} / {n0}")
    assert n0 == 0
    assert torch.isfinite(r1).all() and torch.equal(r1, r0)
    H.assert_close(r1, O.parent_forward(hist, cand, sd, 16), what="fc1 in the tail vs oracle")


def test_hipgraph_replay_with_another_mask_pattern():
    """The grid is the worst case of all three sections and the three counts stay on the device: a captured step -- and a
    captured encoder call of four passes -- replayed after a different mask pattern was written into the same tensors equals
    the eager run on that batch."""
    S, n, chunk = 50, 41, 12
    model, _ = Q.model_for(S)
    enc = model.news_encoder
    a_h, a_c = Q.batch(S, seed=31)
    b_h, b_c = Q.batch(S, seed=32, holes=True)
    xa, ma = Q.news_inputs(n, S, D, chunk, 401)
    xb, mb = Q.news_inputs(n, S, D, chunk, 402)
    mb = mb.roll(7, 0)   # another pattern per pass: the empty pass moves, the live counts of every pass change
    with hip.knobs(**ON), torch.no_grad():
        ref_a = model._forward(Q.to_dev(a_h), Q.to_dev(a_c))
        ref_b = model._forward(Q.to_dev(b_h), Q.to_dev(b_c))
        enc_a = ops.text_encoder(xa.to(DEV), ma.to(DEV), enc, chunk=chunk)
        enc_b = ops.text_encoder(xb.to(DEV), mb.to(DEV), enc, chunk=chunk)
        static_h, static_c = Q.to_dev(a_h), Q.to_dev(a_c)
        static_x, static_m = xa.to(DEV), ma.to(DEV)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):  # warm-up on the side stream (workspace allocation)
                model._forward(static_h, static_c)
                ops.text_encoder(static_x, static_m, enc, chunk=chunk)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        in_tail()
        with torch.cuda.graph(g):
            out = model._forward(static_h, static_c)
            y, hm = ops.text_encoder(static_x, static_m, enc, chunk=chunk)
        assert in_tail() == (n + chunk - 1) // chunk - 1   # the route under test was captured
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref_a)
        assert torch.equal(y, enc_a[0]) and torch.equal(hm, enc_a[1])
        for dst, src in zip(static_h + static_c + (static_x, static_m), b_h + b_c + (xb, mb)):
            dst.copy_(src.to(DEV))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref_b)
        assert torch.equal(y, enc_b[0]) and torch.equal(hm, enc_b[1])
    assert not torch.equal(ref_a, ref_b) and not torch.equal(enc_a[0], enc_b[0])
