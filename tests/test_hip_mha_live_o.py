"""Attention rows nobody reads are not stored (XNRS_MHA_LIVE_O; MhaCoreArgs::o_live_only, encoder_fwd.hip Route::o_live,
DESIGN.md section 4.2).

On the live-row route with the out-projection folded behind the pooling, O has two readers: fc1 walks the pass's live-row
list, and the pooler leaves an all-masked news behind its mask and then reads the rows with a non-zero weight only.  The
pair kernel therefore stores nothing for a masked query: not the zeros of an all-masked news or query tile, not the uniform
average of V of a masked query inside a partly live tile.  Nothing else may change: every comparison between the knob on
and off, and against the dense launches, is ``torch.equal`` with the workspace filled with NaN bytes before the call; the
counter says which route ran; a sentinel count over the whole workspace shows that the rows really stay unwritten.

Shapes: the smallest that reach mha_core_pair_kernel on the list route -- D = 64, 4 heads (d_k = 16), A = 32; S = 50 is the
tail-key variant (48 keys through the MFMAs + 2), S = 34 has three query tiles of which the last holds two rows.  41 news
in passes of 12: four passes, the second made of all-masked news only, the last one short.

Which knobs switch the route off: the route needs the folded out-projection, so XNRS_FOLD_OUT=0 (alone, or together with
XNRS_GEMM_FC1_IN_TAIL=0) keeps every write and the counter does not move.  XNRS_GEMM_FC1_IN_TAIL=0 alone only gives fc1
a launch of its own; it still walks the live-row list, so the route -- by its rule -- is taken there too."""
import pytest
import torch

from xnrs_amd import hip, ops
from xnrs_amd.models.blocks import AdditiveAttention, MultiHeadAttention, TextEncoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, HEADS, A, E = 64, 4, 32, 16
LISTS = dict(XNRS_GEMM_LIVE_TILES="1", XNRS_GEMM_LIVE_ROWS="1", XNRS_GEMM_LIVE_TILES_MIN_ROWS="0", XNRS_GEMM_LIVE_ROWS_MIN_ROWS="0")
ON = dict(LISTS, XNRS_MHA_LIVE_O="1")
OFF = dict(LISTS, XNRS_MHA_LIVE_O="0")    # the parent's route: every O row written
DENSE = dict(LISTS, XNRS_GEMM_LIVE_TILES="0")  # the dense launches: no list at all
N, CHUNK = 41, 12

_enc = {}


def encoder(bias=True):
    """TextEncoder(self-attention, additive pooler, head) at D = 64 / 4 heads / A = 32, seeded weights."""
    if bias not in _enc:
        torch.manual_seed(1234)
        enc = TextEncoder(pooler=AdditiveAttention(D, A), p_dropout=0.0, out_features=E, in_features=D, head=True,
                          att=MultiHeadAttention(HEADS, D), bias=bias)
        _enc[bias] = enc.eval().to(DEV)
    return _enc[bias]


_inputs = {}


def inputs(S, n=N, chunk=CHUNK):
    """(x:(n,S,D), m:(n,S,1)) on the CPU, other rows in every pass.  By pass of `chunk` = 12 news:
      0   prefix masks; news 1 fully live; news 2 with ONE live token, the last one (in the last query tile only); news 3
          all-masked between live ones; news 4 and 5 with non-binary values (0.5, 2.0)
      1   all-masked news only
      2   non-prefix masks (holes inside the titles, also first tokens); news 27 all-masked; news 28 fully live
      3   short: prefix masks, news 38 with the last token alone"""
    key = (S, n, chunk)
    if key in _inputs:
        return _inputs[key]
    g = torch.Generator().manual_seed(1000 + S + n)
    x = torch.randn(n, S, D, generator=g)
    length = torch.randint(1, S + 1, (n,), generator=g)
    m = (torch.arange(S)[None, :] < length[:, None]).float()
    m[1] = 1
    m[2] = 0
    m[2, S - 1] = 1
    m[3] = 0
    u = torch.rand(S, generator=g)
    m[4][(u < 0.4) & (m[4] != 0)] = 0.5
    m[5][(u > 0.5) & (m[5] != 0)] = 2.0
    m[4, 0], m[5, 0] = 0.5, 2.0
    m[chunk:2 * chunk] = 0
    holes = torch.rand(chunk, S, generator=g) < 0.35
    m[2 * chunk:3 * chunk][holes[: max(0, min(chunk, n - 2 * chunk))]] = 0
    if n > 2 * chunk + 4:
        m[2 * chunk + 3] = 0
        m[2 * chunk + 4] = 1
    if n > 3 * chunk + 2:
        m[3 * chunk + 2] = 0
        m[3 * chunk + 2, S - 1] = 1
    _inputs[key] = (x, m.reshape(n, S, 1))
    return _inputs[key]


def check_inputs(m, S, chunk=CHUNK):
    on = m.reshape(-1, S).ne(0)
    n = on.shape[0]
    assert not on[chunk:2 * chunk].any() and on[:chunk].any() and on[2 * chunk:3 * chunk].any()  # a pass of all-masked news only
    assert n % chunk and n > 3 * chunk                                   # several passes, a short last one
    assert on[1].all() and not on[3].any() and on[2].any() and on[4].any()
    assert on[2].sum() == 1 and on[2, S - 1]                             # one live token, in the last query tile only
    assert ((m != 0) & (m != 1)).any()                                   # non-binary values
    last_on = on.float().cumsum(1).argmax(1)                             # non-prefix: a masked token below a live one
    assert any((~on[j, : last_on[j]]).any() for j in range(2 * chunk, 3 * chunk))


def live_o(reset=True):
    return hip.lib().xnrs_mha_live_o_count(1 if reset else 0)


def table_of(x, m):
    """The same news through a permuted table with ids (row 0 = the empty slot)."""
    n, S = m.shape[0], m.shape[1]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n))
    tx = torch.cat([torch.zeros(1, S, D), x[perm]]).to(DEV)
    tm = torch.cat([torch.zeros(1, S, 1), m[perm]]).to(DEV)
    ids = (torch.argsort(perm) + 1).to(torch.int32)
    ids[~m.reshape(n, S).ne(0).any(dim=1)] = 0
    return tx, tm, ids.to(DEV)


def sentinels(ws):
    return int((ws[: ws.numel() // 4 * 4].view(torch.int32) == -1).sum().item())


def encode(x, m, enc, chunk, knobs, ids=None):
    """One encoder call under `knobs` in a workspace filled with 0xFF bytes (NaN; as int32: -1) -> (y, hm, attention launches
    that ran with o_live_only, floats of the whole workspace that still hold the fill)."""
    with torch.no_grad(), hip.knobs(**knobs):
        for attempt in range(2):  # (the workspace only grows: a call that had to grow it runs again, in the poisoned buffer)
            ws = hip.workspace(DEV, 1)
            ws.fill_(0xFF)
            live_o()
            y, hm = ops.text_encoder(x, m, enc, ids=ids, chunk=chunk)
            torch.cuda.synchronize()
            if hip.workspace(DEV, 1) is ws:
                return y, hm, live_o(), sentinels(ws)
    raise AssertionError("the call did not run in the poisoned workspace")


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("S", [50, 34])
def test_knob_on_equals_knob_off_and_dense(S, bias):
    enc = encoder(bias)
    x, m = inputs(S)
    check_inputs(m, S)
    passes = (N + CHUNK - 1) // CHUNK
    xd, md = x.to(DEV), m.to(DEV)
    yd, hmd, cd, _ = encode(xd, md, enc, CHUNK, DENSE)
    y0, hm0, c0, _ = encode(xd, md, enc, CHUNK, OFF)
    y1, hm1, c1, _ = encode(xd, md, enc, CHUNK, ON)
    print(f"S={S} bias={bias}: attention launches with o_live_only: dense {cd}, knob off {c0}, knob on {c1} ({passes} passes)")
    assert torch.isfinite(y1).all() and torch.isfinite(y0).all()
    assert (cd, c0, c1) == (0, 0, passes)       # one per pass exactly when the route is taken
    assert torch.equal(y1, y0) and torch.equal(hm1, hm0)
    assert torch.equal(y1, yd) and torch.equal(hm1, hmd)
    # the same news through ids into a table
    tx, tm, ids = table_of(x, m)
    yi0, hmi0, ci0, _ = encode(tx, tm, enc, CHUNK, OFF, ids)
    yi1, hmi1, ci1, _ = encode(tx, tm, enc, CHUNK, ON, ids)
    yid, hmid, _, _ = encode(tx, tm, enc, CHUNK, DENSE, ids)
    assert (ci0, ci1) == (0, passes)
    assert torch.equal(yi1, yi0) and torch.equal(hmi1, hmi0)
    assert torch.equal(yi1, yid) and torch.equal(hmi1, hmid)
    assert torch.equal(yi1, y1) and torch.equal(hmi1, hm1)


@pytest.mark.parametrize("extra,taken", [
    (dict(XNRS_GEMM_FC1_IN_TAIL="0", XNRS_FOLD_OUT="0"), False),
    (dict(XNRS_FOLD_OUT="0"), False),            # a dense reader of O (the out-projection GEMM): every write stays
    (dict(XNRS_GEMM_FC1_IN_TAIL="0"), True),     # fc1 in a launch of its own still walks the live-row list (module docstring)
    (dict(XNRS_GEMM_LIVE_ROWS="0"), False),      # the live-TILE fc1 without the row list reads masked rows of live tiles
    (dict(XNRS_MHA_SKIP_MASKED="0"), False),
])
def test_other_routes(extra, taken):
    S = 50
    enc = encoder()
    x, m = inputs(S)
    xd, md = x.to(DEV), m.to(DEV)
    y0, hm0, c0, _ = encode(xd, md, enc, CHUNK, dict(OFF, **extra))
    y1, hm1, c1, _ = encode(xd, md, enc, CHUNK, dict(ON, **extra))
    assert c0 == 0 and c1 == ((N + CHUNK - 1) // CHUNK if taken else 0)
    assert torch.isfinite(y1).all()
    assert torch.equal(y1, y0) and torch.equal(hm1, hm0)   # the parent's route under the same knobs


def test_multi_head_attention_alone_keeps_every_row():
    """MultiHeadAttention alone returns its rows to the caller: masked rows are computed and written, the counter stays."""
    S = 50
    enc = encoder()
    x, m = inputs(S)
    xd, md = x[:CHUNK].to(DEV), m[:CHUNK].to(DEV)
    with torch.no_grad(), hip.knobs(**OFF):
        o0 = ops.multi_head_attention(xd, md, enc.att)
    with torch.no_grad(), hip.knobs(**ON):
        live_o()
        o1 = ops.multi_head_attention(xd, md, enc.att)
        torch.cuda.synchronize()
        assert live_o() == 0
    assert torch.isfinite(o1).all() and torch.equal(o1, o0)


@pytest.mark.parametrize("S", [50, 34])
def test_masked_rows_stay_unwritten(S):
    """ONE pass (every O row of the call has a slot of its own in the workspace): with the knob on at least (rows with
    mask == 0) x D more floats of the workspace keep the fill than with it off -- no workspace offset needed."""
    enc = encoder()
    x, m = inputs(S)
    xd, md = x.to(DEV), m.to(DEV)
    y0, hm0, c0, s0 = encode(xd, md, enc, N, OFF)
    y1, hm1, c1, s1 = encode(xd, md, enc, N, ON)
    masked_rows = int((m.reshape(N, S) == 0).sum().item())
    print(f"S={S}: sentinel floats knob off {s0}, on {s1}, difference {s1 - s0}; masked rows x D = {masked_rows * D}")
    assert (c0, c1) == (0, 1)
    assert torch.equal(y1, y0) and torch.equal(hm1, hm0)
    assert masked_rows > 0 and s1 - s0 >= masked_rows * D


def test_hipgraph_capture_and_replay_equals_eager():
    S = 50
    enc = encoder()
    x, m = inputs(S)
    xd, md = x.to(DEV), m.to(DEV)
    with hip.knobs(**ON), torch.no_grad():
        ref = ops.text_encoder(xd, md, enc, chunk=CHUNK)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):  # warm-up on the side stream (workspace allocation)
                ops.text_encoder(xd, md, enc, chunk=CHUNK)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        live_o()
        with torch.cuda.graph(g):
            y, hm = ops.text_encoder(xd, md, enc, chunk=CHUNK)
        assert live_o() == (N + CHUNK - 1) // CHUNK   # the route under test was captured
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, ref[0]) and torch.equal(hm, ref[1])
