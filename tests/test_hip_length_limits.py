"""GPU: every sequence kernel at its declared length limit, against plain fp64 references.

The limits the library enforces: attention S <= 128 (eight 16-key tiles) and head width d_k <= 128 (eight feature blocks),
additive / mean pooling N <= 512, personalized attention L <= 4 096, CAUM pooling H <= 8 192; inside them the kernels
loop in rounds: 1 024 news per round of the row-list kernels, 256 rows per trip of the poolers, 64 tokens per ballot word.
The rest of the suite stays far below all of these (S <= 100, N <= 100, L = 13, H = 25, 300 news per pass), so a wrong second
trip, last key tile, last ballot word or carry between rounds passed it.  Here every loop takes its second (and last) trip.

Every batch has masks with holes, one all-masked sequence and one sequence whose only live token is the LAST one.
References: oracle/xnrs_oracle.py on .double() inputs and state, _ref_pa (tests/test_hip_npa.py) in fp64, a three-line fp64
softmax pool for CAUM.  Bars: the project's, no new number -- H.RTOL forward, GTOL gradients (2e-4 of max(own scale, 1e-3 of
the largest gradient)), H.fc2_bias_extra_bar on top for an additive pooler's fc2.bias, 2e-6 between two GPU paths that differ
in summation order only (tests/test_hip_random_shapes.py "exact switches").  Every case prints MARGIN = observed error / bar.

One past each limit the entry points refuse on the host, before the first launch (read per entry point: seq_encode and
xnrs_seq_encoder_bwd_rows, pa_check, pool_check, xnrs_text_encoder_fwd_compact / _unpadded).

Observed on an MI355X (error / bar, the largest of each group; three digits are printed, 0.000 is below 0.0005):
    attention core alone (six shapes)                 y 0.005   dx 0.003   dW 0.035
    TextEncoder S = 128                               y 0.001   dx 0.002   dW 0.002
    UserEncoder with attention, H = 128               y 0.002   a 0.000   dx 0.001   dW 0.013
    additive pooler, N = 255 .. 512                   y 0.001   a 0.001   dx 0.000   dW 0.017
    masked mean, N = 255 .. 512                       y 0.000   dx 0.000
    UserEncoder without attention, N = 255 .. 512     y 0.009   dx 0.004   dW 0.009 dense, 0.007 with the row list
    padding-free encoders, 64 < S <= 512, holes       y 0.002 against the oracle, 0.056 of the 2e-6 against the padded call
    2 100 news, S = 65 / S = 20                       y 0.001 / 0.002, 0.042 / 0.090 of the 2e-6 against the padded call
    personalized attention, L = 255 .. 4 096          y 0.003   dx 0.001   dq 0.005   dWx 0.012   head 0.001
    CAUM pooling, H = 63 .. 1 024                     u 0.014   a 0.003   dt2 0.002   dh_all 0.001   dw3 0.002   db3 0.346
Prefix masks at 64 < S <= 512: host-compacted, device-compacted and padded results are equal bit for bit, as the header of
xnrs_text_encoder_fwd_compact says.  No kernel computed a wrong result; one was not accurate enough:

db3 of the CAUM pooling is a sum that cancels analytically (a bias in front of a softmax) and with the op alone its bar, 1e-3 of
dw3, lies within a factor of two of what the fp32 rounding of the summed score gradients leaves.  The kernel used to sum the
rounded fp32 ds_j = a_j (da_j - sum a da): db3 sat between 0.016 and 0.776 of the bar in fifteen cases and at 1.443 in
[1024-8-300] (2.887e-4 of the scale against 2e-4).  caum_pool_bwd_kernel now subtracts the weighted mean c = sum a da / sum a,
taken in double, and sums each pair's share in double over the unrounded terms; db3 over the sixteen cases, error / bar:
H = 63: 0.127 0.346 0.074 0.030; H = 65: 0.153 0.097 0.045 0.088; H = 257: 0.102 0.035 0.149 0.013; H = 1 024: 0.063 0.116 0.168 0.015
(A, E = 8, 12 | 8, 300 | 70, 12 | 70, 300).  The bar is unchanged.

Mutations (scratch builds of the library, one change each, arithmetic only; not in the tree; made before the db3 change, so
[1024-8-300] failed in all of them and is not counted) and what this file then did:
    (a) mha_core_kernel treats keys >= 112 as padding: the four S >= 113 attention cases, the TextEncoder at S = 128 and
        the UserEncoder at H = 128 fail; (112, 1, 100), (24, 1, 128) and everything else pass
    (b) additive_pool_kernel leaves rows >= 256 out of its normaliser: all 7 additive and 14 UserEncoder cases with N >= 257
        and the 8 padding-free cases at S = 512 fail, the rest pass
    (c) compact_rows_kernel treats tokens >= 64 as masked (count and list loops alike): all 40 padding-free cases at S > 64,
        both 2 100-news cases at S = 65 and the non-binary case at S = 129 fail, the rest pass
    (d) compact_rows64_kernel does not add s_carry[0] to its offsets: the two 2 100-news cases at S = 20 fail, the rest pass
    (e) personalized_pool_kernel stops its denominator sum at 256 tokens: the five cases with L >= 257 (head and id table
        among them) fail, L = 255 and 256 pass
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import xnrs_oracle as O
from tests import helpers as H
from tests.test_hip_attention_dropout import f64, grad_excess
from tests.test_hip_grads import GTOL, load
from tests.test_hip_live_rows import OFF, ON
from tests.test_hip_npa import _ref_pa
from xnrs_amd import hip, ops, synth
from xnrs_amd.models.components import layers, news_encoding, user_encoding

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWITCH_TOL = 2e-6  # two GPU paths of the same arithmetic in another summation order (tests/test_hip_random_shapes.py)


# ------------------------------------------------------------------------------------------------ inputs
def limit_mask(rng, n, N, p_live=0.7):
    """[n, N] fp32 0/1, n >= 3: holes everywhere; sequence 0 has its first token masked and its last one live, sequence 1 is
    ALL-masked, the last sequence has ONE live token, the last one (index N - 1)."""
    assert n >= 3 and N >= 3
    m = (rng.random((n, N)) < p_live).astype(np.float32)
    m[0, 0], m[0, N // 2], m[0, N - 1] = 0, 0, 1
    m[1] = 0
    m[n - 1] = 0
    m[n - 1, N - 1] = 1
    return torch.from_numpy(m)


def normal(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def fc2_extra(osd, rows):
    """grad_excess's extra_bar: H.fc2_bias_extra_bar for the fc2.bias of an additive pooler (bare module or inside a tower)."""
    def extra(k, scale, gmax):
        if not k.endswith("fc2.bias"):
            return 0.0
        return H.fc2_bias_extra_bar(rows, osd[k[:-len("bias")] + "weight"].grad.abs().max().item(), scale, gmax)
    return extra


# ------------------------------------------------------------------------------------------------ 1. attention at S -> 128, d_k -> 128
# (S, h, d_k): the first KT = 8 shape (a 1-key tail) | KT = 8, full last tile | KT = 8, scalar loads | KT = 7 and seven feature
# blocks | FT = 8, the widest head | both limits at once
MHA_SHAPES = [(113, 2, 16), (128, 2, 16), (127, 3, 6), (112, 1, 100), (24, 1, 128), (128, 1, 128)]


@pytest.mark.parametrize("S,h,dk", MHA_SHAPES)
def test_attention_core_at_the_length_and_width_limits(S, h, dk):
    """layers.MultiHeadAttention alone (mha_core_kernel<KT, VEC>, mha_bwd dq + dkdv), eval mode: y, dx and the eight parameter
    gradients against the fp64 oracle; the no-grad forward (xnrs_mha_fwd) gives the same bits as the training forward."""
    D, n = h * dk, 3
    att, sd = load(layers.MultiHeadAttention(h, D), 301)
    rng = synth.rng_for(30000 + 131 * S + dk)
    x, m, w = normal(rng, n, S, D), limit_mask(rng, n, S).reshape(n, S, 1), normal(rng, n, S, D)
    xd = x.to(DEV).requires_grad_(True)
    y = att(xd, m.to(DEV))
    y.backward(w.to(DEV))
    with torch.no_grad():
        y_ng = att(x.to(DEV), m.to(DEV))
    osd = f64(sd)
    xo = x.double().requires_grad_(True)
    yo = O.multi_head_attention(xo, m.double(), osd, h)
    yo.backward(w.double())
    ey = H.assert_close(y, yo.detach(), H.RTOL, "y")
    ex = H.assert_close(xd.grad, xo.grad, GTOL, "dx")
    eg, cnt = grad_excess(att, osd)
    assert cnt == 8
    assert torch.equal(y_ng, y.detach())
    print(f"MARGIN mha ({S},{h},{dk}): y {ey / H.RTOL:.3f}  dx {ex / GTOL:.3f}  dW {eg:.3f}  (error / bar)")


def test_text_encoder_at_128_tokens():
    """TextEncoder (attention + additive pooler + head) at S = 128: inference forward, training forward, dx and all sixteen
    parameter gradients against the fp64 oracle."""
    S, h, D, A, E, n = 128, 2, 32, 16, 16, 4
    enc, sd = load(news_encoding.TextEncoder(pooler=layers.AdditiveAttention(D, A), p_dropout=0.0, out_features=E, in_features=D,
                                             att=layers.MultiHeadAttention(h, D)), 311)
    rng = synth.rng_for(31100)
    x, m, w = normal(rng, n, S, D), limit_mask(rng, n, S), normal(rng, n, E)
    xd = x.to(DEV).requires_grad_(True)
    y, hm = enc((xd.unsqueeze(0), m.to(DEV).reshape(1, n, S, 1)))
    (y[0] * w.to(DEV)).sum().backward()
    with torch.no_grad():
        y_inf, _ = enc((x.to(DEV).unsqueeze(0), m.to(DEV).reshape(1, n, S, 1)))
    osd = f64(sd)
    xo = x.double().requires_grad_(True)
    yo, hmo = O.text_encoder(xo.unsqueeze(0), m.double().reshape(1, n, S, 1), osd, h)
    (yo[0] * w.double()).sum().backward()
    ei = H.assert_close(y_inf, yo.detach(), H.RTOL, "news vectors, inference")
    ey = H.assert_close(y, yo.detach(), H.RTOL, "news vectors, training forward")
    assert torch.equal(hm.cpu().double(), hmo)
    ex = H.assert_close(xd.grad, xo.grad, GTOL, "dx")
    eg, cnt = grad_excess(enc, osd, fc2_extra(osd, n * S))
    assert cnt == 16
    print(f"MARGIN text encoder S=128: y {max(ei, ey) / H.RTOL:.3f}  dx {ex / GTOL:.3f}  dW {eg:.3f}  (error / bar)")


def test_user_encoder_with_attention_at_128_slots():
    """UserEncoder (attention over 128 history slots + additive pooler): inference forward with its pooling weights, training
    forward, dx and all twelve parameter gradients against the fp64 oracle."""
    N, h, E, A, n = 128, 2, 32, 16, 4
    enc, sd = load(user_encoding.UserEncoder(pooler=layers.AdditiveAttention(E, A), p_dropout=0.0, emb_dim=E,
                                             att=layers.MultiHeadAttention(h, E)), 313)
    rng = synth.rng_for(31300)
    x, m, w = normal(rng, n, N, E), limit_mask(rng, n, N).reshape(n, N, 1), normal(rng, n, E)
    xd = x.to(DEV).requires_grad_(True)
    y = enc((xd, m.to(DEV)))
    (y[:, 0] * w.to(DEV)).sum().backward()
    with torch.no_grad():
        y_inf, a_inf = enc((x.to(DEV), m.to(DEV)), None, return_weights=True)
    osd = f64(sd)
    xo = x.double().requires_grad_(True)
    yo, ao = O.user_encoder(xo, m.double(), osd, h, return_weights=True)
    (yo[:, 0] * w.double()).sum().backward()
    ei = H.assert_close(y_inf, yo.detach(), H.RTOL, "user vectors, inference")
    ea = H.assert_close(a_inf, ao.detach(), H.RTOL, "pooling weights")
    assert bool((a_inf.cpu()[m == 0] == 0).all())
    ey = H.assert_close(y, yo.detach(), H.RTOL, "user vectors, training forward")
    ex = H.assert_close(xd.grad, xo.grad, GTOL, "dx")
    eg, cnt = grad_excess(enc, osd, fc2_extra(osd, n * N))
    assert cnt == 12
    print(f"MARGIN user encoder H=128: y {max(ei, ey) / H.RTOL:.3f}  a {ea / H.RTOL:.3f}  dx {ex / GTOL:.3f}  dW {eg:.3f}  "
          "(error / bar)")


# ------------------------------------------------------------------------------------------------ 2. poolers at N -> 512
POOL_N = [255, 256, 257, 511, 512]
# (N, D, A): the 16-byte path of additive_pool_bwd_kernel<true>, the scalar path, and the shipped token width once
POOL_CASES = [(N, 64, 256) for N in POOL_N] + [(N, 20, 33) for N in POOL_N] + [(511, 768, 64)]


@functools.lru_cache(maxsize=None)
def pool_inputs(N, D):
    """x, mask [n, N, 1] and upstream gradient of the pooler cases, shared by the three tests of a shape."""
    n = 4
    rng = synth.rng_for(32000 + 7 * N + D)
    return n, normal(rng, n, N, D), limit_mask(rng, n, N).reshape(n, N, 1), normal(rng, n, 1, D)


@pytest.mark.parametrize("N,D,A", POOL_CASES)
def test_additive_pooler_up_to_512_rows(N, D, A):
    """layers.AdditiveAttention alone (additive_pool_kernel, additive_pool_bwd_kernel<VEC>): the `i += 256` loops take their
    second trip, the ballot walks up to eight 64-row words, s_idx holds up to 512 rows.  y, the weights a (exactly 0 on masked
    rows, their sum per sequence sum s / (sum s + 1e-8)), dx and the four parameter gradients against the fp64 oracle, and
    the inference forward's y and a."""
    n, x, m, w = pool_inputs(N, D)
    pool, sd = load(layers.AdditiveAttention(D, A), 321)
    xd = x.to(DEV).requires_grad_(True)
    y, a = pool(xd, m.to(DEV), return_weights=True)
    (y * w.to(DEV)).sum().backward()
    with torch.no_grad():
        y_inf, a_inf = pool(x.to(DEV), m.to(DEV), return_weights=True)
    osd = f64(sd)
    xo = x.double().requires_grad_(True)
    yo, ao = O.additive_attention(xo, m.double(), osd, return_weights=True)
    (yo * w.double()).sum().backward()
    ey = H.assert_close(y, yo.detach(), H.RTOL, "y")
    ea = H.assert_close(a, ao.detach(), H.RTOL, "a")
    assert bool((a.detach().cpu()[m == 0] == 0).all()), "a masked row has weight exactly 0"
    es = H.assert_close(a.detach().sum(1), ao.detach().sum(1), H.RTOL, "sum of the weights")
    sums = a.detach().sum(1).reshape(-1).cpu()
    assert sums[1] == 0 and abs(sums[-1] - 1) <= H.RTOL  # the all-masked sequence | the one-token sequence: s / (s + 1e-8)
    # (the inference call takes the fc2 dot in the fc1 GEMM's epilogue: other arithmetic than the training forward, the same bars)
    ey = max(ey, H.assert_close(y_inf, yo.detach(), H.RTOL, "y, inference"))
    ea = max(ea, H.assert_close(a_inf, ao.detach(), H.RTOL, "a, inference"))
    assert bool((a_inf.cpu()[m == 0] == 0).all())
    ex = H.assert_close(xd.grad, xo.grad, GTOL, "dx")
    eg, cnt = grad_excess(pool, osd, fc2_extra(osd, n * N))
    assert cnt == 4
    print(f"MARGIN additive N={N} D={D} A={A}: y {ey / H.RTOL:.3f}  a {max(ea, es) / H.RTOL:.3f}  dx {ex / GTOL:.3f}  dW {eg:.3f}  "
          "(error / bar)")


@pytest.mark.parametrize("N,D", sorted({(N, D) for N, D, _ in POOL_CASES}))
def test_masked_mean_up_to_512_rows(N, D):
    """layers.MaskedMean alone (mean_pool_kernel, mean_pool_bwd_kernel): y and dx against the fp64 oracle."""
    n, x, m, w = pool_inputs(N, D)
    xd = x.to(DEV).requires_grad_(True)
    y = layers.MaskedMean()(xd, m.to(DEV))
    (y * w.to(DEV)).sum().backward()
    with torch.no_grad():
        y_inf = layers.MaskedMean()(x.to(DEV), m.to(DEV))
    xo = x.double().requires_grad_(True)
    yo = O.masked_mean(xo, m.double())
    (yo * w.double()).sum().backward()
    ey = H.assert_close(y, yo.detach(), H.RTOL, "y")
    assert torch.equal(y_inf, y.detach())
    assert bool((y.detach()[1] == 0).all()), "an all-masked sequence has mean 0"
    ex = H.assert_close(xd.grad, xo.grad, GTOL, "dx")
    print(f"MARGIN mean N={N} D={D}: y {ey / H.RTOL:.3f}  dx {ex / GTOL:.3f}  (error / bar)")


@pytest.mark.parametrize("lists", ["dense", "lists"])
@pytest.mark.parametrize("N,D,A", POOL_CASES)
def test_user_encoder_without_attention_up_to_512_slots(N, D, A, lists, monkeypatch):
    """The StandardRec user tower (additive pooler + head, no attention) over up to 512 slots, dense and with the grad step's
    live-row list (built on the device where A is a multiple of 4: row_counts_kernel / row_lists_kernel walk eight ballot
    words; by torch bookkeeping otherwise): y, dx and the eight parameter gradients against the fp64 oracle."""
    from xnrs_amd import autograd as AG
    monkeypatch.setattr(AG, "LIVE_ROWS_MIN", 1)
    monkeypatch.setattr(AG, "LIVE_ROWS", lists != "dense")
    before = AG.STATS["live_row_forwards"]
    n, x, m, w = pool_inputs(N, D)
    enc, sd = load(user_encoding.UserEncoder(pooler=layers.AdditiveAttention(D, A), p_dropout=0.0, emb_dim=D, head=True,
                                             bias=True), 323)
    xd = x.to(DEV).requires_grad_(True)
    y = enc((xd, m.to(DEV)))
    (y * w.to(DEV)).sum().backward()
    assert (AG.STATS["live_row_forwards"] > before) == (lists != "dense")
    with torch.no_grad():
        y_inf = enc((x.to(DEV), m.to(DEV)))
    osd = f64(sd)
    xo = x.double().requires_grad_(True)
    yo = O.user_encoder(xo, m.double(), osd, None)
    (yo * w.double()).sum().backward()
    ey = H.assert_close(y, yo.detach(), H.RTOL, "user vectors")
    ei = H.assert_close(y_inf, yo.detach(), H.RTOL, "user vectors, inference")
    ex = H.assert_close(xd.grad, xo.grad, GTOL, "dx")
    eg, cnt = grad_excess(enc, osd, fc2_extra(osd, n * N))
    assert cnt == 8
    print(f"MARGIN user encoder (no attention) N={N} D={D} A={A} {lists}: y {max(ey, ei) / H.RTOL:.3f}  dx {ex / GTOL:.3f}  "
          f"dW {eg:.3f}  (error / bar)")


# ------------------------------------------------------------------------------------------------ 3. padding-free, 64 < S <= 512
LONG_S = [65, 128, 129, 200, 512]
PF_D, PF_A, PF_E = 16, 8, 12


def additive_encoder(head, seed=331):
    enc, sd = load(news_encoding.TextEncoder(pooler=layers.AdditiveAttention(PF_D, PF_A), p_dropout=0.0,
                                             out_features=PF_E if head else PF_D, in_features=PF_D, head=head, att=None), seed)
    return enc, sd


def three_paths(enc, x, m, ids, chunk):
    """(padded, host-compacted, device-compacted in one pass, device-compacted in passes of `chunk`) results on the GPU."""
    head = getattr(enc, "head", None)
    xd, md = x.to(DEV), m.to(DEV)
    idd = None if ids is None else ids.to(DEV)
    with torch.no_grad():
        pad = ops.text_encoder_forward(xd, md, None, enc.pooler, head, ids=idd)
        unp = ops.text_encoder_forward_unpadded(xd, md, None, enc.pooler, head, ids=idd)
        cmp0 = ops.text_encoder_forward_compact(xd, md, None, enc.pooler, head, ids=idd)
        cmpc = ops.text_encoder_forward_compact(xd, md, None, enc.pooler, head, ids=idd, chunk=chunk)
    torch.cuda.synchronize()
    return pad, unp, cmp0, cmpc


def oracle_news(x, m, ids, sd):
    xg, mg = (x, m) if ids is None else (x[ids.long()], m[ids.long()])
    n, S = mg.shape
    osd = {k: v.double() for k, v in sd.items()}
    y, hm = O.text_encoder(xg.double().unsqueeze(0), mg.double().reshape(1, n, S, 1), osd, None)
    return y[0], hm.reshape(-1)


@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("S", LONG_S)
def test_padding_free_encoders_are_bitwise_equal_to_the_padded_call_on_prefix_masks(S, head, with_ids):
    """The additive-only encoder beyond 64 tokens, prefix masks of lengths 0, 1, S and random ones: the host-compacted call
    and the device-compacted one (compact_rows_kernel, the S > 64 branch of launch_compact_rows; one pass and passes of 7
    news) equal the padded call BIT FOR BIT, as include/xnrs_hip.h promises, and all meet the fp64 oracle."""
    enc, sd = additive_encoder(head)
    rng = synth.rng_for(33000 + S)
    n_tab = 23
    x = normal(rng, n_tab, S, PF_D)
    lens = rng.integers(0, S + 1, size=(n_tab,))
    lens[:4] = (S, 0, 1, S - 1)
    m = torch.from_numpy((np.arange(S)[None, :] < lens[:, None]).astype(np.float32))
    ids = torch.from_numpy(rng.integers(0, n_tab, size=(31,)).astype(np.int32)) if with_ids else None
    if ids is not None:
        ids[:4] = torch.tensor([1, 0, 2, 1], dtype=torch.int32)
    pad, unp, cmp0, cmpc = three_paths(enc, x, m, ids, 7)
    yo, hmo = oracle_news(x, m, ids, sd)
    e = H.assert_close(pad[0], yo, H.RTOL, "padded vs oracle")
    assert torch.equal(pad[1].cpu().double(), hmo)
    for what, (y, hm) in (("host-compacted", unp), ("device-compacted", cmp0), ("device-compacted, passes of 7", cmpc)):
        assert torch.isfinite(y).all(), what
        assert torch.equal(hm, pad[1]), f"{what}: news mask"
        assert torch.equal(y, pad[0]), f"{what}: not bitwise equal to the padded call, {H.rel_err(y, pad[0]):.2e}"
    print(f"MARGIN padding-free prefix S={S} head={head} ids={with_ids}: y {e / H.RTOL:.3f}  (error / bar); the three paths bitwise")


@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("S", LONG_S)
def test_padding_free_encoders_match_the_oracle_on_masks_with_holes(S, head, with_ids):
    """The same with holes in the masks, an all-masked news and a news whose only live token is the last: every path against the
    fp64 oracle; against the padded call they differ by the normaliser's summation order at most (2e-6, the exact switches)."""
    enc, sd = additive_encoder(head)
    rng = synth.rng_for(33500 + S)
    n_tab = 23
    x, m = normal(rng, n_tab, S, PF_D), limit_mask(rng, n_tab, S, p_live=0.6)
    m[5] = 0
    ids = torch.from_numpy(rng.integers(0, n_tab, size=(31,)).astype(np.int32)) if with_ids else None
    if ids is not None:
        ids[:4] = torch.tensor([1, 0, n_tab - 1, 1], dtype=torch.int32)
    pad, unp, cmp0, cmpc = three_paths(enc, x, m, ids, 7)
    yo, hmo = oracle_news(x, m, ids, sd)
    worst, sw = 0.0, 0.0
    for what, (y, hm) in (("padded", pad), ("host-compacted", unp), ("device-compacted", cmp0), ("device-compacted, passes of 7", cmpc)):
        worst = max(worst, H.assert_close(y, yo, H.RTOL, f"{what} vs oracle"))
        assert torch.equal(hm.cpu().double(), hmo), f"{what}: news mask"
        sw = max(sw, H.assert_close(y, pad[0], SWITCH_TOL, f"{what} vs padded"))
    assert torch.equal(cmpc[0], cmp0[0])  # the passes change no bit
    print(f"MARGIN padding-free holes S={S} head={head} ids={with_ids}: y {worst / H.RTOL:.3f}  vs padded {sw / SWITCH_TOL:.3f}  "
          "(error / bar)")


def many_news(n, S, D, seed):
    """n news with holes, ~30 % of them empty, among them runs that straddle news 1 023 / 1 024 and 2 047 / 2 048."""
    rng = synth.rng_for(seed)
    x = normal(rng, n, S, D)
    m = limit_mask(rng, n, S, p_live=0.5)
    dead = torch.from_numpy(rng.random(n) < 0.27)
    dead[1020:1027] = True
    dead[2046:2050] = True
    dead[0] = dead[1023 + 5] = dead[n - 1] = False
    m[dead] = 0
    assert 0.25 < float((m.sum(1) == 0).float().mean()) < 0.35
    return x, m


@pytest.mark.parametrize("chunk", [2100, 1500])
def test_compact_rows_kernel_over_three_rounds_of_1024_news(chunk):
    """2 100 news of 65 tokens through the device-compacted encoder in ONE pass (rounds of 1 024, 1 024 and 52 news: two
    carries between rounds of compact_rows_kernel) and in passes of 1 500 (rounds 1 024 + 476, then 600): against the fp64
    oracle, the padded call (2e-6) and the host-compacted call."""
    n, S = 2100, 65
    enc, sd = additive_encoder(True, 335)
    x, m = many_news(n, S, PF_D, 33600)
    xd, md = x.to(DEV), m.to(DEV)
    with torch.no_grad():
        pad = ops.text_encoder_forward(xd, md, None, enc.pooler, enc.head)
        unp = ops.text_encoder_forward_unpadded(xd, md, None, enc.pooler, enc.head, news_per_pass=chunk)
        hip.workspace(DEV, 1).fill_(0xFF)
        cmp_ = ops.text_encoder_forward_compact(xd, md, None, enc.pooler, enc.head, chunk=chunk)
    yo, hmo = oracle_news(x, m, None, sd)
    worst, sw = 0.0, 0.0
    for what, (y, hm) in (("padded", pad), ("host-compacted", unp), ("device-compacted", cmp_)):
        assert torch.isfinite(y).all(), what
        worst = max(worst, H.assert_close(y, yo, H.RTOL, f"{what} vs oracle"))
        assert torch.equal(hm.cpu().double(), hmo), f"{what}: news mask"
        sw = max(sw, H.assert_close(y, pad[0], SWITCH_TOL, f"{what} vs padded"))
    assert torch.equal(cmp_[0], unp[0])  # the two compacted paths run the same kernels over the same lists
    print(f"MARGIN 2100 news S=65 chunk={chunk}: y {worst / H.RTOL:.3f}  vs padded {sw / SWITCH_TOL:.3f}  (error / bar)")


@pytest.mark.parametrize("tower", ["additive_only", "attention"])
def test_row_list_kernels_for_short_titles_over_three_rounds_of_1024_news(tower):
    """The same 2 100 news in one pass at S = 20 through compact_rows64_kernel (the device-compacted encoder) and
    dense_row_lists_kernel + list_live_tiles (the dense passes with their row lists on; row_lists.hip): lists on == lists off
    bit for bit with the workspace filled with 0xFF bytes first; the compacted call within 2e-6 of it; both meet the fp64 oracle."""
    n, S, h = 2100, 20, 2
    att = layers.MultiHeadAttention(h, PF_D) if tower == "attention" else None
    enc, sd = load(news_encoding.TextEncoder(pooler=layers.AdditiveAttention(PF_D, PF_A), p_dropout=0.0, out_features=PF_E,
                                             in_features=PF_D, att=att), 337)
    x, m = many_news(n, S, PF_D, 33700)
    xd, md = x.to(DEV), m.to(DEV).reshape(n, S, 1)
    with torch.no_grad(), hip.knobs(XNRS_NEWS_FUSED="0"):  # (the padded GEMM pipeline: the three paths share its kernels)
        with hip.knobs(**OFF):
            y0, hm0 = ops.text_encoder(xd, md, enc)
        ws = hip.workspace(DEV, 1)
        with hip.knobs(**ON):
            ws.fill_(0xFF)
            y1, hm1 = ops.text_encoder(xd, md, enc)
            assert hip.workspace(DEV, 1) is ws  # the call ran in the poisoned buffer
        ops.text_encoder_forward_compact(xd, md, att, enc.pooler, enc.head, chunk=n)  # (sizes the workspace)
        ws = hip.workspace(DEV, 1)
        ws.fill_(0xFF)
        y2, hm2 = ops.text_encoder_forward_compact(xd, md, att, enc.pooler, enc.head, chunk=n)
        assert hip.workspace(DEV, 1) is ws
    torch.cuda.synchronize()
    assert torch.isfinite(y1).all() and torch.isfinite(y2).all()
    assert torch.equal(y1, y0) and torch.equal(hm1, hm0)
    assert torch.equal(hm2, hm0)
    osd = {k: v.double() for k, v in sd.items()}
    yo, _ = O.text_encoder(x.double().unsqueeze(0), m.double().reshape(1, n, S, 1), osd, h if att is not None else None)
    e1 = H.assert_close(y1, yo[0], H.RTOL, "dense passes, lists on, vs oracle")
    e2 = H.assert_close(y2, yo[0], H.RTOL, "device-compacted vs oracle")
    sw = H.assert_close(y2, y0, SWITCH_TOL, "device-compacted vs dense")
    print(f"MARGIN 2100 news S=20 {tower}: y {max(e1, e2) / H.RTOL:.3f}  compacted vs dense {sw / SWITCH_TOL:.3f}  (error / bar)")


def test_nonbinary_mask_at_129_tokens_sets_the_status_word():
    """compact_rows_kernel's own non-binary check (a value in the third ballot word of a news): NaN outputs and
    XNRS_STATUS_NONBINARY_MASK, as test_nonbinary_mask_on_the_device_compacted_path_sets_the_status_word has it at S = 20."""
    S, n = 129, 9
    enc, _ = additive_encoder(True)
    rng = synth.rng_for(33800)
    x, m = normal(rng, n, S, PF_D).to(DEV), limit_mask(rng, n, S).to(DEV)
    hip.clear_status()
    with torch.no_grad():
        y_ok, _ = ops.text_encoder_forward_compact(x, m, None, enc.pooler, enc.head)
        assert torch.isfinite(y_ok).all()
        hip.check_status()
        bad = m.clone()
        bad[0, S - 1] = 0.5
        y_bad, hm_bad = ops.text_encoder_forward_compact(x, bad, None, enc.pooler, enc.head)
        assert torch.isnan(y_bad).all() and torch.isnan(hm_bad).all()
    with pytest.raises(hip.XnrsHipError, match="mask value other than 0 / 1"):
        hip.check_status()
    hip.check_status()


# ------------------------------------------------------------------------------------------------ 4. personalized attention at L -> 4 096
PA_L = [255, 256, 257, 1025, 4096]


def pa_case(L, with_head):
    D, A, E, n_q, per = 24, 40, 16, 2, 3
    n = n_q * per
    g = torch.Generator().manual_seed(34000 + L)
    torch.manual_seed(34000 + L)
    x = torch.randn(n, L, D, generator=g)
    m = limit_mask(synth.rng_for(34000 + L), n, L)
    q = torch.randn(n_q, A, generator=g) * 0.3
    q_idx = torch.div(torch.arange(n), per, rounding_mode="floor").to(torch.int32)
    x_fc = nn.Linear(D, A)
    head = nn.Sequential(nn.Linear(D, E), nn.ReLU(), nn.Linear(E, E)) if with_head else None
    dy = torch.randn(n, E if with_head else D, generator=g)
    return x, m, q, q_idx, x_fc, head, dy


@pytest.mark.parametrize("L,with_head", [(L, False) for L in PA_L] + [(1025, True)])
def test_personalized_attention_up_to_4096_tokens(L, with_head):
    """ops.personalized (personalized_pool_kernel / _bwd_kernel: every `i += PA_THREADS` loop beyond one trip, up to 32 KB of
    dynamic LDS), forward and backward against _ref_pa in fp64: y, hm, dx, dq, dWx, dbx and the head's gradients."""
    x, m, q, q_idx, x_fc, head, dy = pa_case(L, with_head)
    xd, qd = x.double().requires_grad_(True), q.double().requires_grad_(True)
    pd = [p.detach().double().requires_grad_(True) for p in x_fc.parameters()]
    hd = [p.detach().double().requires_grad_(True) for p in head.parameters()] if head is not None else []
    yr = _ref_pa(xd, m.double(), qd, q_idx, pd[0], pd[1], hd if hd else None)
    yr.backward(dy.double())
    x_fc = x_fc.to(DEV)
    head = head.to(DEV) if head is not None else None
    xg, qg = x.to(DEV).requires_grad_(True), q.to(DEV).requires_grad_(True)
    y, hm = ops.personalized(xg, m.to(DEV), None, qg, q_idx.to(DEV), x_fc, head)
    y.backward(dy.to(DEV))
    with torch.no_grad():
        y_inf, _ = ops.personalized(x.to(DEV), m.to(DEV), None, q.to(DEV), q_idx.to(DEV), x_fc, head)
    ey = H.assert_close(y, yr.detach(), H.RTOL, "y")
    assert torch.equal(y_inf, y.detach())
    assert torch.equal(hm.cpu(), (m.sum(1) > 0).float())
    if head is None:
        assert bool((y[1] == 0).all()), "an all-masked sequence pools to 0"
    ex = H.assert_close(xg.grad, xd.grad, GTOL, "dx")
    eq = H.assert_close(qg.grad, qd.grad, GTOL, "dq")
    ew = max(H.assert_close(got.grad, ref.grad, GTOL, k) for got, ref, k in zip(x_fc.parameters(), pd, ("dWx", "dbx")))
    eh = max([H.assert_close(got.grad, ref.grad, GTOL, "head") for got, ref in zip(head.parameters(), hd)]) if head is not None else 0.0
    print(f"MARGIN personalized L={L} head={with_head}: y {ey / H.RTOL:.3f}  dx {ex / GTOL:.3f}  dq {eq / GTOL:.3f}  "
          f"dWx {ew / GTOL:.3f}  head {eh / GTOL:.3f}  (error / bar)")


def test_personalized_attention_over_a_gathered_table_at_4096_tokens():
    """The id path (value and mask rows gathered from a table by news id) at L = 4 096, forward only: a gathered table has
    no dx."""
    L = 4096
    x, m, q, q_idx, x_fc, _, _ = pa_case(L, False)
    ids = torch.tensor([5, 1, 0, 3, 3, 2], dtype=torch.int32)
    with torch.no_grad():
        yr = _ref_pa(x.double()[ids.long()], m.double()[ids.long()], q.double(), q_idx, x_fc.weight.double(), x_fc.bias.double())
        y, hm = ops.personalized(x.to(DEV), m.to(DEV), ids.to(DEV), q.to(DEV), q_idx.to(DEV), x_fc.to(DEV), None)
    ey = H.assert_close(y, yr, H.RTOL, "y")
    assert torch.equal(hm.cpu(), (m[ids.long()].sum(1) > 0).float())
    print(f"MARGIN personalized ids L={L}: y {ey / H.RTOL:.3f}  (error / bar)")


# ------------------------------------------------------------------------------------------------ 5. CAUM pooling beyond one trip
@pytest.mark.parametrize("E", [12, 300])
@pytest.mark.parametrize("A", [8, 70])
@pytest.mark.parametrize("Hn", [63, 65, 257, 1024])
def test_caum_pooling_beyond_one_trip(Hn, A, E):
    """ops.caum_pool (caum_pool_fwd_kernel / _bwd_kernel: the `j += 64` and `j += 4` loops beyond one trip, the chunked
    dw3 / db3 sums) against an fp64 softmax pool: u, a, dt2, dh_all, dw3, db3.  db3 cancels analytically (a bias in front
    of a softmax); it gets what tests/test_hip_caum.py gives every parameter gradient: GTOL of max(its own scale, 1e-3 of
    the largest parameter gradient) -- with the op alone that is 1e-3 of dw3.  On an MI355X db3 sits between 0.013 and 0.346
    of that bar (module docstring: the kernel sums each pair's share in double; summed in fp32 it reached 1.443)."""
    P = 3
    g = torch.Generator().manual_seed(35000 + 7 * Hn + A + E)
    t2 = torch.tanh(torch.randn(P * Hn, A, generator=g))  # (the output of a tanh layer in the model)
    h_all = torch.randn(P * Hn, E, generator=g)
    w3 = torch.randn(1, A, generator=g) / A ** 0.5
    b3 = torch.randn(1, generator=g)
    du = torch.randn(P, E, generator=g)
    ref_in = [t.double().requires_grad_(True) for t in (t2, w3, b3, h_all)]
    s = (ref_in[0] @ ref_in[1].reshape(-1) + ref_in[2]).reshape(P, Hn)
    ar = torch.softmax(s, dim=-1)
    ur = (ar[..., None] * ref_in[3].reshape(P, Hn, E)).sum(1)
    ur.backward(du.double())
    got_in = [t.to(DEV).requires_grad_(True) for t in (t2, w3, b3, h_all)]
    u = ops.caum_pool(got_in[0], got_in[1], got_in[2], got_in[3], Hn)
    u.backward(du.to(DEV))
    with torch.no_grad():
        u_inf, a, _ = ops.caum_pool_forward(t2.to(DEV), w3.to(DEV), b3.to(DEV), h_all.to(DEV), Hn, keep=True)
    eu = H.assert_close(u, ur.detach(), H.RTOL, "u")
    assert torch.equal(u_inf, u.detach())
    ea = H.assert_close(a, ar.detach(), H.RTOL, "a")
    et = H.assert_close(got_in[0].grad, ref_in[0].grad, GTOL, "dt2")
    eh = H.assert_close(got_in[3].grad, ref_in[3].grad, GTOL, "dh_all")
    gmax = max(ref_in[1].grad.abs().max().item(), ref_in[2].grad.abs().max().item())
    ep = {}
    for k, got, ref in (("dw3", got_in[1].grad, ref_in[1].grad), ("db3", got_in[2].grad, ref_in[2].grad)):
        scale = max(ref.abs().max().item(), 1e-3 * gmax)
        ep[k] = (got.cpu().double() - ref).abs().max().item() / scale
    print(f"MARGIN caum pool H={Hn} A={A} E={E}: u {eu / H.RTOL:.3f}  a {ea / H.RTOL:.3f}  dt2 {et / GTOL:.3f}  dh_all {eh / GTOL:.3f}  "
          f"dw3 {ep['dw3'] / GTOL:.3f}  db3 {ep['db3'] / GTOL:.3f}  (error / bar)")
    for k, e in ep.items():
        assert e <= GTOL, f"{k}: {e:.3e} > {GTOL:.1e}"


# ------------------------------------------------------------------------------------------------ 6. one past each limit
def test_one_past_each_limit_is_refused_before_any_launch():
    """Attention at L = 129 (training forward and backward), the poolers at N = 513 (forward, training forward, backward),
    personalized attention at L = 4 097, CAUM pooling at H = 8 193 and the padding-free encoders at S = 513: XnrsHipError
    with XNRS_EUNSUPPORTED (-4) from the host-side checks, and an output buffer handed to the raw entry point stays as it was."""
    l, st = hip.lib(), hip.stream_ptr(DEV)
    code = "code -4"
    D, A, E = 8, 8, 8
    att, _ = load(layers.MultiHeadAttention(2, D), 361)
    pool, _ = load(layers.AdditiveAttention(D, A), 362)
    mean = layers.MaskedMean()
    x129 = torch.zeros(2, 129, D, device=DEV)
    x513 = torch.zeros(2, 513, D, device=DEV)
    m513 = torch.ones(2, 513, 1, device=DEV)
    with pytest.raises(hip.XnrsHipError, match=code):
        att(x129.clone().requires_grad_(True), None)  # training forward
    with torch.no_grad():
        with pytest.raises(hip.XnrsHipError, match=code):
            att(x129, None)
        with pytest.raises(hip.XnrsHipError, match=code):
            pool(x513, m513)
        with pytest.raises(hip.XnrsHipError, match=code):
            mean(x513, m513)
        with pytest.raises(hip.XnrsHipError, match=code):
            ops.text_encoder_forward_compact(x513, m513, None, pool, None)
        with pytest.raises(hip.XnrsHipError, match=code):
            ops.text_encoder_forward_unpadded(x513, m513, None, pool, None)
    with pytest.raises(hip.XnrsHipError, match=code):
        pool(x513.clone().requires_grad_(True), m513)  # training forward
    with pytest.raises(hip.XnrsHipError, match=code):
        mean(x513.clone().requires_grad_(True), m513)

    # the backward entry point, which autograd cannot reach with such a shape (its forward refuses first): raw calls
    ap, keep_a = hip.mha_params(att)
    pp, keep_p = hip.additive_params(pool)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)

    def bwd(x, att_p, pool_kind, pool_p):
        n, L, Dx = x.shape
        m = torch.ones(n, L, device=DEV)
        dy = torch.ones((n, L, Dx) if pool_kind == hip.POOL_NONE else (n, Dx), device=DEV)
        dx = torch.full((n, L, Dx), 7.0, device=DEV)
        rc = l.xnrs_seq_encoder_bwd(hip.ptr(x), hip.ptr(m), None, n, L, Dx, hip.ref(att_p), pool_kind, hip.ref(pool_p), None,
                                    hip.ptr(buf), buf.numel(), hip.ptr(dy), hip.ptr(dx), None, None, None, hip.ptr(buf),
                                    buf.numel(), st)
        torch.cuda.synchronize()
        assert bool((dx == 7.0).all()), "a refused call writes nothing"
        return rc

    assert bwd(x129, ap, hip.POOL_NONE, None) == -4
    assert bwd(x513, None, hip.POOL_ADDITIVE, pp) == -4
    assert bwd(x513, None, hip.POOL_MEAN, None) == -4
    # d_k = 132: the backward kernels hold eight 16-feature blocks (the inference forward takes any width)
    wide, _ = load(layers.MultiHeadAttention(1, 132), 363)
    wp, keep_w = hip.mha_params(wide)
    x_wide = torch.zeros(1, 4, 132, device=DEV)
    assert bwd(x_wide, wp, hip.POOL_NONE, None) == -4
    with pytest.raises(hip.XnrsHipError, match=code):
        wide(x_wide.clone().requires_grad_(True), None)  # ... so the training forward refuses it as well

    # personalized attention
    x_fc = nn.Linear(D, A).to(DEV)
    q, q_idx = torch.zeros(1, A, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    x4097 = torch.zeros(2, 4097, D, device=DEV)
    with torch.no_grad(), pytest.raises(hip.XnrsHipError, match=code):
        ops.personalized(x4097, None, None, q, q_idx, x_fc)
    with pytest.raises(hip.XnrsHipError, match=code):
        ops.personalized(x4097.clone().requires_grad_(True), None, None, q, q_idx, x_fc)
    from xnrs_amd import autograd as AG
    pa = AG.personalized_params(x_fc, q, q_idx, [])
    dx, dy = torch.full((2, 4097, D), 7.0, device=DEV), torch.ones(2, D, device=DEV)
    assert l.xnrs_personalized_bwd(hip.ptr(x4097), None, 2, 4097, D, hip.ref(pa), None, hip.ptr(buf), buf.numel(), hip.ptr(dy),
                                   hip.ptr(dx), None, None, None, 1, None, hip.ptr(buf), buf.numel(), st) == -4
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all())

    # CAUM pooling
    Hn = 8193
    t2, h_all, w3 = torch.zeros(Hn, A, device=DEV), torch.zeros(Hn, E, device=DEV), torch.zeros(1, A, device=DEV)
    with torch.no_grad(), pytest.raises(hip.XnrsHipError, match=code):
        ops.caum_pool(t2, w3, None, h_all, Hn)
    with pytest.raises(hip.XnrsHipError, match=code):
        ops.caum_pool(t2.clone().requires_grad_(True), w3, None, h_all, Hn)
    d_t2, a, du = torch.full((Hn, A), 7.0, device=DEV), torch.zeros(1, Hn, device=DEV), torch.ones(1, E, device=DEV)
    assert l.xnrs_caum_pool_bwd(hip.ptr(t2), hip.ptr(w3), hip.ptr(h_all), hip.ptr(a), hip.ptr(du), hip.ptr(d_t2), None, None, None,
                                1, Hn, A, E, hip.ptr(buf), buf.numel(), st) == -4
    torch.cuda.synchronize()
    assert bool((d_t2 == 7.0).all())
    msg = l.xnrs_error_string(-4).decode()
    for limit in ("S <= 128", "N <= 512", "d_k <= 128", "L <= 4096", "H <= 8192"):
        assert limit in msg, msg
