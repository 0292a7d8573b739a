"""GPU: train-mode attention (Dropout on the attention probabilities, layers.py:117,148) against the fp64 oracle under the
EXACT mask.  The generator of the kernels (kernels.h drop_uniform) is restated in numpy integer arithmetic in the oracle
(attention_keep_mask; tests/test_dropout_oracle.py), so every DROP=true kernel variant has a plain reference: forward,
input gradient and all parameter gradients, at the project's usual bars (H.RTOL forward, GTOL gradients).

Which instantiation a case reaches follows from mha_pick (mha_core.hip) / launch_mha_bwd (mha_bwd.hip); the rule is
restated in forward_pick / backward_pick below and test_case_table_reaches_every_dropout_variant holds the table to it.

    case (S, h, d_k) [knobs]          forward                          backward                     y      dx     dW
    (16, 4, 8)                        headwave<KT=1>                   fused<NFB=1>                 0.002  0.001  0.048
    (30, 2, 16)                       headwave<KT=2>                   fused<NFB=1>                 0.002  0.001  0.035
    (17, 2, 8)                        headwave<KT=2>                   fused<NFB=1>                 0.002  0.001  0.030
    (33, 2, 48)                       pair<KTM=2,NFB=3,TAIL>           fused<NFB=3>                 0.004  0.002  0.028
    (34, 3, 20)                       pair<KTM=2,NFB=2,TAIL>           fused<NFB=2>                 0.004  0.002  0.040
    (50, 2, 48)                       pair<KTM=3,NFB=3,TAIL>           fused<NFB=3>                 0.003  0.002  0.027
    (52, 2, 64)                       pair<KTM=3,NFB=4,TAIL>           fused<NFB=4>                 0.005  0.002  0.035
    (40, 2, 16)                       pair<KTM=3,NFB=1>                fused<NFB=1>                 0.002  0.001  0.034
    (48, 2, 4)                        pair<KTM=3,NFB=1>                fused<NFB=1>                 0.001  0.001  0.029
    (64, 2, 36)                       pair<KTM=4,NFB=3>                fused<NFB=3>                 0.003  0.002  0.036
    (53, 2, 64)                       pair<KTM=4,NFB=4>                fused<NFB=4>                 0.004  0.002  0.031
    (65, 2, 8)                        generic<KT=5,vec>                dq<KT=5,vec>+dkdv<vec>       0.001  0.001  0.039
    (100, 1, 16)                      generic<KT=7,vec>                dq<KT=7,vec>+dkdv<vec>       0.002  0.001  0.048
    (128, 1, 16)                      generic<KT=8,vec>                dq<KT=8,vec>+dkdv<vec>       0.002  0.002  0.083
    (120, 1, 6)                       generic<KT=8,scalar>             dq<KT=8,scalar>+dkdv<scalar> 0.002  0.002  0.084
    (24, 1, 128)                      generic<KT=2,vec>                dq<KT=2,vec>+dkdv<vec>       0.004  0.002  0.036
    (20, 1, 72)                       generic<KT=2,vec>                dq<KT=2,vec>+dkdv<vec>       0.004  0.002  0.031
    (9, 3, 6)                         generic<KT=1,scalar>             dq<KT=1,scalar>+dkdv<scalar> 0.002  0.001  0.036
    (50, 2, 18)                       generic<KT=4,scalar>             dq<KT=4,scalar>+dkdv<scalar> 0.002  0.001  0.027
    (50, 2, 48) XNRS_MHA_PAIR=0       lds<KT=4,NFB=3>                  fused<NFB=3>                 0.003  0.002  0.029
    (64, 2, 16) XNRS_MHA_PAIR=0       lds<KT=4,NFB=1>                  fused<NFB=1>                 0.002  0.001  0.038
    (40, 2, 16) XNRS_MHA_PAIR=0       lds<KT=3,NFB=1>                  fused<NFB=1>                 0.002  0.001  0.034
    (16, 2, 16) XNRS_MHA_LDS=1        lds<KT=1,NFB=1>                  fused<NFB=1>                 0.002  0.001  0.021
    (30, 2, 16) XNRS_MHA_LDS=1        lds<KT=2,NFB=1>                  fused<NFB=1>                 0.002  0.001  0.035
    (30, 2, 16) XNRS_MHA_HEADWAVE=0   generic<KT=2,vec>                fused<NFB=1>                 0.002  0.001  0.035
    (50, 2, 48) XNRS_MHA_BWD_FUSED=0  pair<KTM=3,NFB=3,TAIL>           dq<KT=4,vec>+dkdv<vec>       0.003  0.002  0.043

The last three columns: observed error / bar on an MI355X at p = 0.1 (y against H.RTOL, dx against GTOL, the worst parameter
gradient against its bar).  At p = 0.5, y/dx/dW: (50,2,48) 0.003/0.002/0.049, (30,2,16) 0.002/0.001/0.037, (64,2,36)
0.003/0.002/0.028, (65,2,8) 0.001/0.001/0.061, (9,3,6) 0.002/0.001/0.073.
Pooled encoders, y/dx/dW, the same in device, host and dense list mode to the digits shown: TextEncoder (50,2,48)
0.001/0.002/0.003, (33,4,16) 0.001/0.002/0.004; UserEncoder (50,2,48) 0.003/0.002/0.012, (33,4,16) 0.002/0.002/0.015 (dense;
0.014 with lists).  Two encodes with the merged product: y 0.001, dW 0.003.  Chunked forward: y 0.001 at h = 2 and h = 1.

With query and key swapped in ONE drop_uniform call (a scratch build, not in the tree) the file fails as it should: swapped in
mha_bwd_fused_kernel, all 36 cases whose backward is the fused kernel fail and the 11 others (dq + dkdv backward, forward only)
pass; swapped in the pair forward (mha_core_pair_kernel), all 31 cases that run or compare with a pair forward fail and the
16 others pass.  (Counted before the three rows at S = 128 / 120 and d_k = 128 joined the table: they run neither of the two
kernels and belong to the "others".)
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from oracle import xnrs_oracle as O
from tests import helpers as H
from tests.test_hip_grads import GTOL, load
from xnrs_amd import synth
from xnrs_amd.models.components import layers, news_encoding, user_encoding

gpu = pytest.mark.gpu
DEV = "cuda:0"
TORCH_SEED = 1234
WEIGHT_SEED = 61
N_SEQ = 4
GOLDEN64 = 0x9E3779B97F4A7C15


# ------------------------------------------------------------------------------------------------ the case table
def forward_pick(S, dk, knobs=None):
    """mha_pick + launch_mha_core (mha_core.hip) for the contiguous fp32 operands of these tests."""
    k = knobs or {}
    vec = dk % 4 == 0
    KT = (S + 15) // 16
    fast = vec and S <= 64 and dk <= 64 and k.get("XNRS_MHA_HEADWAVE", "1") != "0"
    use_lds = (k["XNRS_MHA_LDS"] != "0") if "XNRS_MHA_LDS" in k else KT >= 3
    rem = S & 15
    tail = S > 16 and 1 <= rem <= 4
    KTM = S >> 4 if tail else KT
    pair = fast and use_lds and k.get("XNRS_MHA_PAIR", "1") != "0" and (KTM in (2, 3) if tail else KTM in (3, 4))
    nfb = min((dk + 15) // 16, 4)
    if pair:
        return f"pair<KTM={KTM},NFB={nfb}{',TAIL' if tail else ''}>"
    if fast and use_lds:
        return f"lds<KT={min(KT, 4)},NFB={nfb}>"
    if fast:
        return f"headwave<KT={KT}>"
    return f"generic<KT={min(KT, 8)},{'vec' if vec else 'scalar'}>"


def backward_pick(S, dk, knobs=None):
    """launch_mha_bwd (mha_bwd.hip)."""
    k = knobs or {}
    vec = dk % 4 == 0
    if vec and S <= 64 and dk <= 64 and k.get("XNRS_MHA_BWD_FUSED", "1") != "0":
        return f"fused<NFB={min((dk + 15) // 16, 4)}>"
    v = "vec" if vec else "scalar"
    return f"dq<KT={min((S + 15) // 16, 8)},{v}>+dkdv<{v}>"


# (S, h, d_k, forward pick, backward pick)
DEFAULT_CASES = [
    (16, 4, 8, "headwave<KT=1>", "fused<NFB=1>"),
    (30, 2, 16, "headwave<KT=2>", "fused<NFB=1>"),
    (17, 2, 8, "headwave<KT=2>", "fused<NFB=1>"),  # a one-key tail with KTM = 1: not the pair kernel's
    (33, 2, 48, "pair<KTM=2,NFB=3,TAIL>", "fused<NFB=3>"),
    (34, 3, 20, "pair<KTM=2,NFB=2,TAIL>", "fused<NFB=2>"),
    (50, 2, 48, "pair<KTM=3,NFB=3,TAIL>", "fused<NFB=3>"),  # the shipped news shape's branch
    (52, 2, 64, "pair<KTM=3,NFB=4,TAIL>", "fused<NFB=4>"),
    (40, 2, 16, "pair<KTM=3,NFB=1>", "fused<NFB=1>"),
    (48, 2, 4, "pair<KTM=3,NFB=1>", "fused<NFB=1>"),
    (64, 2, 36, "pair<KTM=4,NFB=3>", "fused<NFB=3>"),
    (53, 2, 64, "pair<KTM=4,NFB=4>", "fused<NFB=4>"),
    (65, 2, 8, "generic<KT=5,vec>", "dq<KT=5,vec>+dkdv<vec>"),
    (100, 1, 16, "generic<KT=7,vec>", "dq<KT=7,vec>+dkdv<vec>"),
    (128, 1, 16, "generic<KT=8,vec>", "dq<KT=8,vec>+dkdv<vec>"),  # the longest sequence: eight full key tiles
    (120, 1, 6, "generic<KT=8,scalar>", "dq<KT=8,scalar>+dkdv<scalar>"),
    (24, 1, 128, "generic<KT=2,vec>", "dq<KT=2,vec>+dkdv<vec>"),  # the widest head: eight feature blocks
    (20, 1, 72, "generic<KT=2,vec>", "dq<KT=2,vec>+dkdv<vec>"),
    (9, 3, 6, "generic<KT=1,scalar>", "dq<KT=1,scalar>+dkdv<scalar>"),
    (50, 2, 18, "generic<KT=4,scalar>", "dq<KT=4,scalar>+dkdv<scalar>"),
]
# (S, h, d_k, knobs, forward pick, backward pick, forward vs the default pick: "bitwise" | relative bar | None)
# bitwise / 2e-6: what test_attention_core_pair_kernel_branches (tests/test_hip_grads.py) establishes in eval mode -- the pair kernel
# and the first-generation LDS-staged kernel share their arithmetic without a tail and differ by the VALU tail's summation order with one;
# dropout adds the same select and division to both.
KNOB_CASES = [
    (50, 2, 48, {"XNRS_MHA_PAIR": "0"}, "lds<KT=4,NFB=3>", "fused<NFB=3>", 2e-6),
    (64, 2, 16, {"XNRS_MHA_PAIR": "0"}, "lds<KT=4,NFB=1>", "fused<NFB=1>", "bitwise"),
    (40, 2, 16, {"XNRS_MHA_PAIR": "0"}, "lds<KT=3,NFB=1>", "fused<NFB=1>", "bitwise"),
    (16, 2, 16, {"XNRS_MHA_LDS": "1"}, "lds<KT=1,NFB=1>", "fused<NFB=1>", None),
    (30, 2, 16, {"XNRS_MHA_LDS": "1"}, "lds<KT=2,NFB=1>", "fused<NFB=1>", None),
    (30, 2, 16, {"XNRS_MHA_HEADWAVE": "0"}, "generic<KT=2,vec>", "fused<NFB=1>", None),
    (50, 2, 48, {"XNRS_MHA_BWD_FUSED": "0"}, "pair<KTM=3,NFB=3,TAIL>", "dq<KT=4,vec>+dkdv<vec>", "bitwise"),  # same forward
]
HALF_CASES = [(50, 2, 48), (30, 2, 16), (64, 2, 36), (65, 2, 8), (9, 3, 6)]  # p = 0.5: one per kernel family


def test_case_table_reaches_every_dropout_variant():
    """The picks written in the table are what the launchers' rules give, and together the cases reach every DROP=true
    forward variant (generic vector / scalar, head-per-wave KT 1 and 2, LDS-staged KT 1..4, the four pair kernels and
    each feature-block count NFB 1..4 among them) and every backward kernel (fused NFB 1..4, dq + dkdv vector and scalar)."""
    fw, bw = set(), set()
    for S, h, dk, f, b in DEFAULT_CASES:
        assert (forward_pick(S, dk), backward_pick(S, dk)) == (f, b), (S, h, dk)
        fw.add(f)
        bw.add(b)
    for S, h, dk, knobs, f, b, _ in KNOB_CASES:
        assert (forward_pick(S, dk, knobs), backward_pick(S, dk, knobs)) == (f, b), (S, h, dk, knobs)
        fw.add(f)
        bw.add(b)
    fam = lambda s: s.split("<")[0]  # noqa: E731
    assert {fam(f) for f in fw} == {"generic", "headwave", "lds", "pair"}
    assert {f for f in fw if f.startswith("headwave")} == {"headwave<KT=1>", "headwave<KT=2>"}
    assert {f.split(",")[0] for f in fw if f.startswith("lds")} == {f"lds<KT={k}" for k in (1, 2, 3, 4)}
    pairs = {f for f in fw if f.startswith("pair")}
    assert {(f.split(",")[0], "TAIL" in f) for f in pairs} == {("pair<KTM=2", True), ("pair<KTM=3", True), ("pair<KTM=3", False),
                                                              ("pair<KTM=4", False)}
    assert {f.split(",")[1].rstrip(">") for f in pairs} == {f"NFB={k}" for k in (1, 2, 3, 4)}
    assert any("vec" in f for f in fw if f.startswith("generic")) and any("scalar" in f for f in fw)
    assert {b for b in bw if b.startswith("fused")} == {f"fused<NFB={k}>" for k in (1, 2, 3, 4)}
    assert any(b.endswith("dkdv<vec>") for b in bw) and any(b.endswith("dkdv<scalar>") for b in bw)


# ------------------------------------------------------------------------------------------------ inputs and reference
def draw_seeds(torch_seed, count=1):
    """The next `count` attention-dropout seeds after torch.manual_seed(torch_seed), as ops._att_dropout draws them."""
    torch.manual_seed(torch_seed)
    return [int(torch.empty((), dtype=torch.int64).random_().item()) for _ in range(count)]


def block_mask(n, S):
    """[n, S] fp32: a sequence with holes, one with a ragged tail, one ALL-masked, the rest full."""
    m = np.ones((n, S), dtype=np.float32)
    m[0, 0] = m[0, S // 3] = 0
    m[1, S - max(1, S // 4):] = 0
    m[2] = 0
    return m


def f64(sd):
    return {k: v.double().requires_grad_(not k.endswith("dummy_param")) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def mha_reference(S, h, dk, p, seed):
    """fp64 oracle of the bare MultiHeadAttention under the restated mask of `seed`: inputs, y, dx and the state with its
    gradients; and the proof on the reference alone that the case is not vacuous (dropout moves y and dx by more than 100x
    their bars)."""
    D = h * dk
    shapes = {k: tuple(v.shape) for k, v in layers.MultiHeadAttention(h, D).state_dict().items()}
    sd = synth.fill_state_dict(shapes, WEIGHT_SEED)
    rng = synth.rng_for(6200 + 131 * S + dk)
    x = torch.from_numpy(rng.standard_normal((N_SEQ, S, D)).astype("float32"))
    m = torch.from_numpy(block_mask(N_SEQ, S)).reshape(N_SEQ, S, 1)
    dy = torch.from_numpy(rng.standard_normal((N_SEQ, S, D)).astype("float32"))
    keep = O.attention_keep_mask(seed, N_SEQ, h, S, p)
    osd = f64(sd)
    xo = x.double().requires_grad_(True)
    yo = O.multi_head_attention(xo, m.double(), osd, h, drop=(keep, p))
    yo.backward(dy.double())
    xe = x.double().requires_grad_(True)
    ye = O.multi_head_attention(xe, m.double(), f64(sd), h)
    ye.backward(dy.double())
    assert H.rel_err(ye.detach(), yo.detach()) > 100 * H.RTOL, "vacuous: dropout does not move y"
    assert H.rel_err(xe.grad, xo.grad) > 100 * GTOL, "vacuous: dropout does not move dx"
    return dict(x=x, m=m, dy=dy, y=yo.detach(), dx=xo.grad, osd=osd)


def grad_excess(module, osd, extra_bar=None):
    """check_param_grads (tests/test_hip_grads.py) that also returns the margin: asserts every parameter gradient within
    GTOL of max(|ref|, 1e-3 largest gradient), plus extra_bar(key, scale, gmax) where given, and returns the largest
    error / bar and the number of parameters checked."""
    gmax = max(v.grad.abs().max().item() for v in osd.values() if v.grad is not None)
    worst, n = 0.0, 0
    for k, prm in module.named_parameters():
        if k.endswith("dummy_param"):
            continue
        assert prm.grad is not None and osd[k].grad is not None, k
        ref = osd[k].grad
        scale = max(ref.abs().max().item(), 1e-3 * gmax)
        e = (prm.grad.cpu().double() - ref).abs().max().item() / scale
        bar = GTOL + (extra_bar(k, scale, gmax) if extra_bar else 0.0)
        assert e <= bar, f"{k}: {e:.3e} (bar {bar:.3e})"
        worst = max(worst, e / bar)
        n += 1
    return worst, n


def run_mha(S, h, dk, p, knobs=None, torch_seed=TORCH_SEED):
    """Train-mode forward + backward on the GPU, and the no-grad train-mode forward (the inference entry point xnrs_mha_fwd)
    under the same seed."""
    from xnrs_amd import hip
    ref = mha_reference(S, h, dk, p, draw_seeds(torch_seed)[0])
    att, _ = load(layers.MultiHeadAttention(h, h * dk), WEIGHT_SEED, train=True)
    att.dropout.p = p
    with hip.knobs(**knobs) if knobs else contextlib.nullcontext():
        torch.manual_seed(torch_seed)
        xd = ref["x"].to(DEV).requires_grad_(True)
        y = att(xd, ref["m"].to(DEV))
        y.backward(ref["dy"].to(DEV))
        with torch.no_grad():
            torch.manual_seed(torch_seed)
            y_ng = att(ref["x"].to(DEV), ref["m"].to(DEV))
    return att, y.detach(), xd.grad, y_ng


def check_mha(tag, ref, att, y, dx, y_ng):
    ey = H.assert_close(y, ref["y"], H.RTOL, f"{tag} y")
    ex = H.assert_close(dx, ref["dx"], GTOL, f"{tag} dx")
    eg, n = grad_excess(att, ref["osd"])
    assert n == 8
    assert torch.equal(y_ng, y), f"{tag}: the no-grad train-mode forward differs from the grad-mode forward"
    print(f"MARGIN {tag}: y {ey / H.RTOL:.3f}  dx {ex / GTOL:.3f}  dW {eg:.3f}  (error / bar)")


# ------------------------------------------------------------------------------------------------ every kernel variant
@gpu
@pytest.mark.parametrize("S,h,dk,fwd,bwd", DEFAULT_CASES)
def test_dropout_kernels_match_fp64_oracle(S, h, dk, fwd, bwd):
    """Dropout(0.1), the shipped value: y, dx and the eight parameter gradients of every default kernel pick against the
    fp64 oracle under the restated mask; masked queries keep their uniform rows and are dropped like the rest."""
    ref = mha_reference(S, h, dk, 0.1, draw_seeds(TORCH_SEED)[0])
    check_mha(f"({S},{h},{dk}) p=0.1 {fwd} | {bwd}", ref, *run_mha(S, h, dk, 0.1))


@gpu
@pytest.mark.parametrize("S,h,dk", HALF_CASES)
def test_dropout_one_half_matches_fp64_oracle(S, h, dk):
    """p = 0.5 (survivors scaled by exactly 2; every other probability gone) on one case per kernel family."""
    ref = mha_reference(S, h, dk, 0.5, draw_seeds(TORCH_SEED)[0])
    check_mha(f"({S},{h},{dk}) p=0.5 {forward_pick(S, dk)} | {backward_pick(S, dk)}", ref, *run_mha(S, h, dk, 0.5))


@gpu
@pytest.mark.parametrize("S,h,dk,knobs,fwd,bwd,same", KNOB_CASES)
def test_dropout_kernels_behind_knobs_match_fp64_oracle(S, h, dk, knobs, fwd, bwd, same):
    """The kernels only a development knob reaches (LDS-staged forward, generic forward on a small shape, the two-kernel
    backward on a shape the fused kernel serves), against the same reference; and against the default pick, bit for bit,
    where the two share their arithmetic."""
    ref = mha_reference(S, h, dk, 0.1, draw_seeds(TORCH_SEED)[0])
    att, y, dx, y_ng = run_mha(S, h, dk, 0.1, knobs)
    check_mha(f"({S},{h},{dk}) p=0.1 {knobs} {fwd} | {bwd}", ref, att, y, dx, y_ng)
    _, y0, dx0, _ = run_mha(S, h, dk, 0.1)
    print(f"   forward {'==' if torch.equal(y, y0) else '!='} default pick, dx {'==' if torch.equal(dx, dx0) else '!='} default pick")
    if same == "bitwise":
        assert torch.equal(y, y0)
    elif same is not None:
        H.assert_close(y, y0, same, "knob-forced forward vs the default pick")


# ------------------------------------------------------------------------------------------------ seed_dev
@gpu
@pytest.mark.parametrize("S,h,dk", [(50, 2, 48), (30, 2, 16), (9, 3, 6)])
def test_device_seed_word_is_added_in_forward_and_backward(S, h, dk):
    """ops.set_dropout_seed_word: with the device word holding k, forward AND backward equal the reference at seed + k
    (mod 2^64); after the word was incremented on the device, at seed + k + 1 -- the pair kernel + fused backward, the
    head-per-wave kernel, and the generic forward + two-kernel backward."""
    from xnrs_amd import ops
    k = 2 ** 62 + 5  # (seed + k wraps for half of all seeds)
    seed = draw_seeds(TORCH_SEED)[0]
    word = torch.tensor([k], dtype=torch.int64, device=DEV)
    ops.set_dropout_seed_word(word)
    try:
        for step in (0, 1):
            ref = mha_reference(S, h, dk, 0.1, (seed + k + step) % 2 ** 64)
            att, _ = load(layers.MultiHeadAttention(h, h * dk), WEIGHT_SEED, train=True)
            torch.manual_seed(TORCH_SEED)
            xd = ref["x"].to(DEV).requires_grad_(True)
            y = att(xd, ref["m"].to(DEV))
            y.backward(ref["dy"].to(DEV))
            H.assert_close(y, ref["y"], H.RTOL, f"y, word = k + {step}")
            H.assert_close(xd.grad, ref["dx"], GTOL, f"dx, word = k + {step}")
            assert grad_excess(att, ref["osd"])[1] == 8
            word.add_(1)
    finally:
        ops.set_dropout_seed_word(None)
    assert not torch.equal(mha_reference(S, h, dk, 0.1, (seed + k) % 2 ** 64)["y"],
                           mha_reference(S, h, dk, 0.1, (seed + k + 1) % 2 ** 64)["y"])


# ------------------------------------------------------------------------------------------------ pooled encoders
def fc2_bias_bar(osd, rows):
    """The extra bar of `pooler.fc2.bias` derived in test_random_bi_encoder_gradients_match_oracle (tests/test_hip_random_shapes.py):
    2e-4 of the scale plus 4 sqrt(rows) 2^-23 max|d fc2.weight| plus 1e-6 of the step's largest gradient."""
    def extra(k, scale, gmax):
        if not k.endswith("pooler.fc2.bias"):
            return 0.0
        gw = osd[k[:-len("bias")] + "weight"].grad.abs().max().item()
        return H.fc2_bias_extra_bar(rows, gw, scale, gmax)
    return extra


def pooled_inputs(n, S, D, Eo, seed):
    rng = synth.rng_for(seed)
    x = torch.from_numpy(rng.standard_normal((n, S, D)).astype("float32"))
    lens = rng.integers(1, S + 1, size=(n,))
    m = (np.arange(S)[None, :] < lens[:, None]).astype("float32")
    m *= (rng.random((n, S)) < 0.8)  # holes
    m[0] = 1
    m[1::3] = 0  # a third of the sequences all-masked
    w = torch.from_numpy(rng.standard_normal((n, Eo)).astype("float32"))
    return x, torch.from_numpy(m.astype("float32")), w


def list_mode(monkeypatch, lists):
    from xnrs_amd import autograd as AG
    monkeypatch.setattr(AG, "LIVE_ROWS_MIN", 1)
    monkeypatch.setattr(AG, "LIVE_ROWS", lists != "dense")
    monkeypatch.setattr(AG, "DEVICE_LISTS", lists == "device")
    return AG, dict(AG.STATS)


def assert_list_mode_ran(AG, before, lists, calls=1):
    d = {k: AG.STATS[k] - before[k] for k in before}
    if lists == "device":
        assert d["device_list_forwards"] == calls and d["live_row_forwards"] == calls, d
    elif lists == "host":
        assert d["device_list_forwards"] == 0 and d["live_row_forwards"] == calls, d
    else:
        assert d["device_list_forwards"] == 0 and d["live_row_forwards"] == 0, d


PAIR_SHAPES = [(50, 2, 48), (33, 4, 16)]  # pair<KTM=3,TAIL> (the shipped branch) and pair<KTM=2,TAIL>


@gpu
@pytest.mark.parametrize("lists", ["device", "host", "dense"])
@pytest.mark.parametrize("S,h,dk", PAIR_SHAPES)
def test_text_encoder_train_mode_matches_fp64_oracle(S, h, dk, lists, monkeypatch):
    """TextEncoder (attention + additive pooler + head) in train mode, 12 news of which a third are all-masked, through the
    row-list forms of the attention kernels (skip_dead forward; masked_do_is_zero / dead_seq_mode backward; the PADDED
    sequence index in the dropout counter while the projections run over compact rows): news vectors, input gradient and
    all sixteen parameter gradients (attention 8, pooler 4, head 4) against oracle text_encoder(..., drop=...) in fp64."""
    n, D, A, E, p = 12, h * dk, 48, 32, 0.1
    AG, before = list_mode(monkeypatch, lists)
    enc, sd = load(news_encoding.TextEncoder(pooler=layers.AdditiveAttention(D, A), p_dropout=0.0, out_features=E, in_features=D,
                                             att=layers.MultiHeadAttention(h, D)), 71, train=True)
    x, m, w = pooled_inputs(n, S, D, E, 7200 + S)
    seed = draw_seeds(TORCH_SEED)[0]
    torch.manual_seed(TORCH_SEED)
    xd = x.to(DEV).requires_grad_(True)
    y, hm = enc((xd.unsqueeze(0), m.to(DEV).reshape(1, n, S, 1)))
    (y[0] * w.to(DEV)).sum().backward()
    assert_list_mode_ran(AG, before, lists)
    osd = f64(sd)
    xo = x.double().requires_grad_(True)
    drop = (O.attention_keep_mask(seed, n, h, S, p), p)
    yo, hmo = O.text_encoder(xo.unsqueeze(0), m.double().reshape(1, n, S, 1), osd, h, drop=drop)
    (yo[0] * w.double()).sum().backward()
    xe = x.double().requires_grad_(True)
    ye, _ = O.text_encoder(xe.unsqueeze(0), m.double().reshape(1, n, S, 1), f64(sd), h)
    (ye[0] * w.double()).sum().backward()
    assert H.rel_err(ye.detach(), yo.detach()) > 100 * H.RTOL  # not vacuous: dropout moves the news vectors
    assert H.rel_err(xe.grad, xo.grad) > 100 * GTOL  # ... and the input gradient
    ey = H.assert_close(y, yo.detach(), H.RTOL, "news vectors")
    assert torch.equal(hm.cpu().double(), hmo)
    ex = H.assert_close(xd.grad, xo.grad, GTOL, "dx")
    eg, cnt = grad_excess(enc, osd, fc2_bias_bar(osd, n * S))
    assert cnt == 16
    print(f"MARGIN text encoder ({S},{h},{dk}) {lists}: y {ey / H.RTOL:.3f}  dx {ex / GTOL:.3f}  dW {eg:.3f}  (error / bar)")


@gpu
@pytest.mark.parametrize("lists", ["device", "host", "dense"])
@pytest.mark.parametrize("S,h,dk", PAIR_SHAPES)
def test_user_encoder_train_mode_matches_fp64_oracle(S, h, dk, lists, monkeypatch):
    """UserEncoder (attention over S history slots + additive pooler) in train mode, 12 users of which a third have no
    history at all, through the same three list modes: user vectors, input gradient and all parameter gradients against
    oracle user_encoder(..., drop=...) in fp64."""
    n, E, A, p = 12, h * dk, 48, 0.1
    AG, before = list_mode(monkeypatch, lists)
    enc, sd = load(user_encoding.UserEncoder(pooler=layers.AdditiveAttention(E, A), p_dropout=0.0, emb_dim=E,
                                             att=layers.MultiHeadAttention(h, E)), 73, train=True)
    x, m, w = pooled_inputs(n, S, E, E, 7400 + S)
    seed = draw_seeds(TORCH_SEED)[0]
    torch.manual_seed(TORCH_SEED)
    xd = x.to(DEV).requires_grad_(True)
    y = enc((xd, m.to(DEV).reshape(n, S, 1)))
    (y[:, 0] * w.to(DEV)).sum().backward()
    assert_list_mode_ran(AG, before, lists)
    osd = f64(sd)
    xo = x.double().requires_grad_(True)
    drop = (O.attention_keep_mask(seed, n, h, S, p), p)
    yo = O.user_encoder(xo, m.double().reshape(n, S, 1), osd, h, drop=drop)
    (yo[:, 0] * w.double()).sum().backward()
    xe = x.double().requires_grad_(True)
    ye = O.user_encoder(xe, m.double().reshape(n, S, 1), f64(sd), h)
    (ye[:, 0] * w.double()).sum().backward()
    assert H.rel_err(ye.detach(), yo.detach()) > 100 * H.RTOL  # not vacuous: dropout moves the user vectors
    assert H.rel_err(xe.grad, xo.grad) > 100 * GTOL  # ... and the input gradient
    ey = H.assert_close(y, yo.detach(), H.RTOL, "user vectors")
    ex = H.assert_close(xd.grad, xo.grad, GTOL, "dx")
    eg, cnt = grad_excess(enc, osd, fc2_bias_bar(osd, n * S))
    assert cnt == 12
    print(f"MARGIN user encoder ({S},{h},{dk}) {lists}: y {ey / H.RTOL:.3f}  dx {ex / GTOL:.3f}  dW {eg:.3f}  (error / bar)")


@gpu
@pytest.mark.parametrize("lists", ["device", "dense"])
def test_two_history_encodes_with_merged_weight_gradient_match_fp64_oracle(lists, monkeypatch):
    """The reference's train step encodes the history twice (training.py:406,409).  Here: one TextEncoder called twice on
    the same input in train mode, the loss over both outputs.  The second call reads the first one's Q|K|V image
    (qkv_shared) and draws the NEXT seed of the CPU generator; of the two backwards one defers its dQ|dK|dV and the other
    merges (XNRS_DQKV_DEFER / MERGE).  Reference: two fp64 oracle passes under the two restated masks, gradients summed."""
    S, h, dk, n, A, E, p = 50, 2, 48, 12, 48, 32, 0.1
    D = h * dk
    AG, before = list_mode(monkeypatch, lists)
    enc, sd = load(news_encoding.TextEncoder(pooler=layers.AdditiveAttention(D, A), p_dropout=0.0, out_features=E, in_features=D,
                                             att=layers.MultiHeadAttention(h, D)), 75, train=True)
    x, m, w1 = pooled_inputs(n, S, D, E, 7600)
    w2 = torch.from_numpy(synth.rng_for(7601).standard_normal((n, E)).astype("float32"))
    s1, s2 = draw_seeds(TORCH_SEED, 2)
    assert s1 != s2
    torch.manual_seed(TORCH_SEED)
    xd, md = x.to(DEV).unsqueeze(0), m.to(DEV).reshape(1, n, S, 1)  # (no input gradient: the merged product needs none asked for)
    ya, _ = enc((xd, md))
    yb, _ = enc((xd, md))
    ((ya[0] * w1.to(DEV)).sum() + (yb[0] * w2.to(DEV)).sum()).backward()
    d = {k: AG.STATS[k] - before[k] for k in before}
    assert (d["shared_qkv_forwards"], d["deferred_dqkv_backwards"], d["merged_dqkv_backwards"]) == (1, 1, 1), d
    assert d["device_list_forwards"] == (1 if lists == "device" else 0), d
    osd = f64(sd)
    xo, mo = x.double().unsqueeze(0), m.double().reshape(1, n, S, 1)
    y1, _ = O.text_encoder(xo, mo, osd, h, drop=(O.attention_keep_mask(s1, n, h, S, p), p))
    y2, _ = O.text_encoder(xo, mo, osd, h, drop=(O.attention_keep_mask(s2, n, h, S, p), p))
    ((y1[0] * w1.double()).sum() + (y2[0] * w2.double()).sum()).backward()
    assert H.rel_err(y2.detach(), y1.detach()) > 100 * H.RTOL  # the two encodes really differ
    e1 = H.assert_close(ya, y1.detach(), H.RTOL, "first encode")
    e2 = H.assert_close(yb, y2.detach(), H.RTOL, "second encode")
    eg, cnt = grad_excess(enc, osd, fc2_bias_bar(osd, 2 * n * S))
    assert cnt == 16
    print(f"MARGIN two encodes {lists}: y {max(e1, e2) / H.RTOL:.3f}  dW {eg:.3f}  (error / bar)")


# ------------------------------------------------------------------------------------------------ chunked inference forward
@gpu
@pytest.mark.parametrize("h,dk", [(2, 48), (1, 64)])
def test_chunked_inference_forward_with_dropout_on(h, dk):
    """ops.text_encoder_forward(..., chunk < n_news, dropout_p > 0) -- the no-grad train-mode forward over more news than one
    pass takes -- indexes the sequences of a pass from 0 and advances the seed by c0 * heads counter steps (encoder_fwd.hip),
    so sequence c0 + i draws what it draws in the unchunked call.  THIS reference follows the implementation rather than a
    contract: its mask is built per pass by that very rule (and tests/test_dropout_oracle.py shows the rule gives no two
    sequences of a call one stream).  The chunked call must also equal the unchunked one bit for bit."""
    from xnrs_amd import ops
    S, n, chunk, A, E, p = 50, 11, 4, 48, 32, 0.1
    D = h * dk
    enc, sd = load(news_encoding.TextEncoder(pooler=layers.AdditiveAttention(D, A), p_dropout=0.0, out_features=E, in_features=D,
                                             att=layers.MultiHeadAttention(h, D)), 77, train=True)
    x, m, _ = pooled_inputs(n, S, D, E, 7800)
    seed = draw_seeds(TORCH_SEED)[0]
    with torch.no_grad():
        y, hm = ops.text_encoder_forward(x.to(DEV), m.to(DEV), enc.att, enc.pooler, enc.head, chunk=chunk, dropout_p=p, seed=seed)
        y0, _ = ops.text_encoder_forward(x.to(DEV), m.to(DEV), enc.att, enc.pooler, enc.head, chunk=0, dropout_p=p, seed=seed)
    keep = np.concatenate([O.attention_keep_mask(seed + c0 * h * GOLDEN64, min(chunk, n - c0), h, S, p) for c0 in range(0, n, chunk)])
    streams = {keep[i, j].tobytes() for i in range(n) for j in range(h)}
    assert len(streams) == n * h  # no two (sequence, head) pairs of the call share a mask
    osd = {k: v.double() for k, v in sd.items()}
    yo, _ = O.text_encoder(x.double().unsqueeze(0), m.double().reshape(1, n, S, 1), osd, h, drop=(keep, p))
    ye, _ = O.text_encoder(x.double().unsqueeze(0), m.double().reshape(1, n, S, 1), osd, h)
    assert H.rel_err(ye, yo) > 100 * H.RTOL
    e = H.assert_close(y, yo[0], H.RTOL, "chunked train-mode forward")
    assert torch.equal(y, y0)
    print(f"MARGIN chunked forward h={h}: y {e / H.RTOL:.3f}  (error / bar)")
