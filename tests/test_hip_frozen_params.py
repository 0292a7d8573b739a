"""GPU: every hand-written backward with frozen parameters and partial gradients, against plain fp64 references.

Every backward entry point takes nullable outputs and branches on each of them (include/xnrs_hip.h; xnrs_seq_encoder_bwd_rows
alone: weight wanted -> product with the bias sum fused, bias only -> a stand-alone column sum, the folded pair's db' in place
or in the workspace, dWk|dWv as one product, dead_seq_mode 2 only while all three projection weights are wanted, ...), and
xnrs_amd/autograd.py adds its own (need and wanted per parameter, DEFER / MERGE of the two history encodes, the kept-back
gradient sets of a shared tower).  The rest of the suite runs two points of that space: everything trainable, and no
parameter gradient at all with dx (integrated gradients).  Here: requires_grad_(False) on named subsets of the parameters
("leave-one-out": that tensor alone frozen; "one-hot": that tensor alone trainable; the groups of groups() below), and
torch.autograd.grad(loss, inputs=subset) with everything requiring grad (the _wanted_inputs route; those cases spy on
autograd._wanted_inputs and assert that each backward node was told exactly the subset).

Every case asserts (1) each wanted gradient, dx where asked for and the forward value against the fp64 reference of the same
operation, computed ONCE with everything trainable: H.RTOL forward, GTOL = 2e-4 of max(own scale, 1e-3 of the largest
reference gradient of the all-trainable step) for gradients, H.fc2_bias_extra_bar on top for an additive pooler's fc2.bias
(for the CAUM pooling the floor is 1e-3 of the largest PARAMETER gradient, the bar of tests/test_hip_length_limits.py);
(2) every frozen tensor has .grad None -- after autograd.grad every tensor; (3) the reference gradient of every wanted tensor
is non-zero, with one exception by algebra: the key bias (a constant added to every score of a softmax row: its gradient is
zero in exact arithmetic; the case then checks that the kernel's sum is noise below the bar, which a column sum over
unwritten rows is not.  In fp64 the reference's key-bias gradient is 1.3e-17 (text), 2.1e-18 (D = 36), 1.5e-16 (attention
alone), 5.5e-17 (user tower), 5.9e-18 (two encodes): 6e-19 .. 1.3e-17 of the step's largest gradient, pure rounding; the
kernels' sum sits at 0.011 .. 0.023 of its bar, i.e. below 5e-9 of the largest gradient); (4) the same gradients equal the
all-trainable GPU run on the same inputs within 2e-5 of the same scale
(tests/test_hip_train_step.py::_close: two GPU runs that differ in summation order only); (5) hip.check_status() is clean.
Every case prints MARGIN = error / bar for (1) and (4).

References: oracle/xnrs_oracle.py on .double() state and inputs; _ref_pa (tests/test_hip_npa.py), _fp64
(tests/test_hip_scorers.py), _ref_gru (tests/test_hip_lstur.py); the fp64 softmax pool of tests/test_hip_length_limits.py and
the pair / bias-tanh formulas of include/xnrs_hip.h restated in fp64 for CAUM.

The two history encodes (section B), read against _SeqEncode.backward: qkv_all needs all six Q/K/V gradients in BOTH nodes (they
share their parameters, so both see the same answer); one of them frozen -> neither node defers or merges, STATS deltas
(shared_qkv_forwards, deferred, merged) = (1, 0, 0); only head or pooler tensors frozen -> (1, 1, 1).  The code agrees with
the expectation written into the cases.

The knob product of section A is run where a knob does something: the list modes {device, dense} for towers with an additive
pooler (the row lists ride on it: autograd._SeqEncode.forward; the others run "dense" only), XNRS_FOLD_TRAIN {1, 0} for towers
with attention AND an additive pooler (nothing is folded elsewhere; the others run "1" only), dx {no, yes} everywhere except
through forward_ids (a gathered table has no input gradient).  The D = 36 tower runs the group subsets only.

Read before anything ran (NULL handling of each entry point against the subsets here): xnrs_seq_encoder_bwd_rows,
xnrs_linear_bwd, embedding_linear_bwd, xnrs_dot_scoring*_bwd, xnrs_bilinear_scoring_bwd, xnrs_mlp_scoring_bwd,
xnrs_personalized_bwd, xnrs_gru_bwd, xnrs_caum_pair_bwd / _bias_tanh_bwd / _pool_bwd and their kernels: every nullable output
is tested before it is written, workspace stand-ins (dbf, dh, Delta, G) are sized by the plan whatever is asked for; the
unfused bias sum over "all rows" under dead_seq_mode 2 cannot occur (mode 2 exists in the fused attention backward only, which
needs d_k % 4 == 0, hence D % 4 == 0, hence the fused sum).  No bug found by reading the C side.

One bug found by the tests' own evidence (the first MARGIN table showed the grad(inputs=) cases BITWISE equal to the
all-trainable run, and mutation (b) failed none of them): autograd._wanted_inputs never took its per-parameter route under
torch.autograd.grad(loss, inputs=<parameters>).  torch._C._will_engine_execute_node answers False for the AccumulateGrad node
of a leaf that is not among the inputs but RAISES for one that is ("A leaf node was passed to _will_engine_execute_node but we
are currently running autograd.grad()"); the blanket `except RuntimeError` then answered "everything wanted", every weight
gradient was computed and torch threw the unwanted ones away -- right numbers, none of the promised savings, and for _Linear /
the scorers (whose inputs are asked about too) the same with grad(score, inputs=[tokens]).  Now autograd._engine_wants asks per
node and takes that refusal for what it means: a captured leaf is wanted.  The section D cases hold it with the spy.

Observed on an MI355X (error / bar, the largest of each group; 0.000 is below 0.0005; "run" = against the all-trainable GPU run,
bar 2e-5).  All 1 125 cases pass, the whole file in 6.6 s; no kernel computed a wrong gradient:
    group (cases)                                  y      dW     dx     run dW  run dx
    TextEncoder, 16 tensors (368)                  0.001  0.011  0.001  0.126   0.000
    TextEncoder D = 36, h = 6, groups only (152)   0.001  0.009  0.002  0.028   0.000
    MultiHeadAttention alone (52)                  0.002  0.028  0.001  0.138   0.000
    TextEncoder without attention (80)             0.003  0.005  0.001  0.010   0.000
    ... through forward_ids (40)                   0.001  0.007  -      0.042   -
    TextEncoder with MaskedMean (20)               0.001  0.001  0.000  0.005   0.000
    UserEncoder with attention (288)               0.001  0.061  0.001  0.176   0.000
    TextEncoder, autograd.grad(inputs=) (76)       0.001  0.011  0.001  0.112   0.000
    two history encodes (16)                       0.001  0.004  -      0.025   -
    NRMS step, requires_grad / grad(inputs=) (8)   0.008  0.008  -      0.005 / 0.005
    linear (12) y 0.007 grads 0.002 | dot (2) 0.002 0.001 | bilinear (2) 0.002 0.002 | mlp 0.001 0.001 | personalized (2) 0.002
    0.002 | gru (2) 0.001 0.001 | caum pair 0.001 0.001, bias tanh 0.002 0.002, pool 0.001 0.009; run <= 0.005 for all of them
    (linear, bilinear, mlp, personalized and gru: every subset also through grad(inputs=), inside the same figures)

Mutations (scratch builds of the library, one change each, every one only skips work or takes the other valid branch; not in
the tree) and what this file then did.  Every run_* here first fills the library's workspace with 0xFF bytes: without that,
(b) showed in 10 cases only -- the rows it leaves unwritten still held the zeros of an earlier call.
    (a) encoder_bwd.hip without the `else if (g_att && g_att->bo)` column sum of the out-projection: 38 cases fail -- only_bo
        and weights_frozen of every attention tower with the fold off or without a pooler (text, text36, user at fold 0; mha),
        (14 + 14), and the 10 loo_wo cases of text, user and mha (out.bias wanted, out.weight not; the unwritten gradient is
        torch.empty memory: in an earlier run one of the ten passed on the block of the previous run's out.bias gradient); the
        other 1 087 pass
    (b) lists_only without its `wq && wk && wv`: 42 cases fail -- text and user with device lists and no dx, either fold setting:
        loo_wq / loo_wk / loo_wv, only_bq / only_bk / only_bv, qkv_biases_only, qkv_weights_frozen, weights_frozen (a bias
        gradient summed over the unwritten rows of the all-masked sequence: NaN), and the two history encodes with wq, wk or wv
        frozen under device lists, and the grad(inputs=) cases weights_frozen, qkv_biases_only and qkv_weights_frozen under
        device lists without dx (none of them before the _wanted_inputs fix); the other 1 083 pass (dense list mode, dx asked
        for, d_k = 6: lists_only is false there)
    (c) folded path, db' always into the workspace: 220 cases fail -- every case with fc1.bias wanted of an attention + additive
        tower with the fold on (21 of 46 subsets per setting for text, 6 of 19 for text36, 16 of 36 for user, 24 of the
        grad(inputs=) tower cases, all 16 two-encode cases and all 8 step cases: their all-trainable control fails too, as the
        existing suite would); the other 905 pass
    (d) scorers.hip without the `if (dbias)` block: both bilinear cases fail, the other 1 123 pass
    (e) gru.hip without the stand-alone `else if (g && g->b_hh)` column sum: both GRU cases fail, the other 1 123 pass
    (f) autograd.py, qkv_all ignoring grads[:6]: the 12 two-encode cases with a frozen Q/K/V tensor fail (deltas (1, 1, 1)
        instead of (1, 0, 0)), the other 1 113 pass
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import xnrs_oracle as O
from tests import helpers as H
from tests.golden import cases
from tests.test_hip_attention_dropout import (TORCH_SEED, assert_list_mode_ran, draw_seeds, f64, fc2_bias_bar, list_mode,
                                              pooled_inputs)
from tests.test_hip_grads import GTOL, Cfg, load
from tests.test_hip_length_limits import limit_mask
from tests.test_hip_lstur import _ref_gru
from tests.test_hip_npa import _ref_pa
from tests.test_hip_scorers import _fp64
from xnrs_amd import hip, ops, synth
from xnrs_amd.models import make_model
from xnrs_amd.models.blocks import BilinScoring, FCScoring
from xnrs_amd.models.components import layers, news_encoding, user_encoding

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RUN_TOL = 2e-5  # two GPU runs of the same arithmetic in another summation order (tests/test_hip_train_step.py::_close)
ZERO_BY_ALGEBRA = ("k_linear.bias",)  # assertion (3) cannot hold for it: see the module docstring


# ------------------------------------------------------------------------------------------------ subset-aware checks
def subset_excess(tag, grads, ref, wanted, full=None, extra_bar=None, floor_keys=None):
    """The subset-aware twin of grad_excess (tests/test_hip_attention_dropout.py).  grads: name -> tensor | None of this run;
    ref: name -> fp64 gradient of the all-trainable reference step; full: name -> gradient of the all-trainable GPU run.
    Asserts (1)-(4) of the module docstring on the gradients and returns (worst error / bar vs fp64, worst vs the full run)."""
    gmax = max(ref[k].abs().max().item() for k in (floor_keys or ref))
    assert gmax > 0.0, f"{tag}: vacuous, every reference gradient is zero"
    worst, worst_run = 0.0, 0.0
    for k in ref:
        if k not in wanted:
            assert grads[k] is None, f"{tag}: {k} is frozen and has a gradient"
            continue
        assert grads[k] is not None, f"{tag}: {k} is wanted and has no gradient"
        own = ref[k].abs().max().item()
        if not k.endswith(ZERO_BY_ALGEBRA):
            assert own > 0.0, f"{tag}: vacuous, the reference gradient of {k} is zero"
        scale = max(own, 1e-3 * gmax)
        got = grads[k].detach().cpu().double()
        assert got.shape == ref[k].shape, (tag, k, got.shape, ref[k].shape)
        e = (got - ref[k]).abs().max().item() / scale
        bar = GTOL + (extra_bar(k, scale, gmax) if extra_bar else 0.0)
        assert e <= bar, f"{tag}: {k}: {e:.3e} of the scale (bar {bar:.3e})"
        worst = max(worst, e / bar)
        if full is not None:
            e4 = (got - full[k].detach().cpu().double()).abs().max().item() / scale
            assert e4 <= RUN_TOL, f"{tag}: {k}: {e4:.3e} of the scale away from the all-trainable GPU run (bar {RUN_TOL:.1e})"
            worst_run = max(worst_run, e4 / RUN_TOL)
    return worst, worst_run


def dx_excess(tag, dx, ref_dx, full_dx):
    e = H.assert_close(dx, ref_dx, GTOL, f"{tag}: dx")
    e4 = (dx - full_dx).abs().max().item() / ref_dx.abs().max().item()
    assert e4 <= RUN_TOL, f"{tag}: dx {e4:.3e} away from the all-trainable GPU run"
    return e / GTOL, e4 / RUN_TOL


def spy_wanted_inputs(monkeypatch):
    """-> the list that collects what autograd._wanted_inputs answers from here on, one [bool per input] per backward node: the
    proof that a torch.autograd.grad(inputs=...) case took the per-parameter route and not the compute-everything fall-back."""
    from xnrs_amd import autograd as AG
    seen, real = [], AG._wanted_inputs

    def spy(ctx, is_tensor, first):
        out = real(ctx, is_tensor, first)
        seen.append(list(out))
        return out
    monkeypatch.setattr(AG, "_wanted_inputs", spy)
    return seen


def poison_workspace():
    """0xFF bytes (NaN) into the library's scratch buffer before a run: a gradient summed over rows that this call did not write
    shows as NaN instead of passing on the zeros an earlier call left there (as tests/test_hip_length_limits.py does for the
    row-list kernels)."""
    hip.workspace(DEV, 1).fill_(0xFF)


def one_hot_and_leave_one_out(names):
    out = []
    for s in [frozenset([k]) for k in names] + [frozenset(names) - {k} for k in names]:
        if s and s not in out:
            out.append(s)
    return out


# ------------------------------------------------------------------------------------------------ A. the sequence encoder
N_SEQ, S_LEN, A_HID, E_OUT = 7, 17, 20, 12  # n % 4 != 0, S crosses the 16-row tile edge
TOWERS = {  # att: heads | None; pool: additive | mean | none; ids: through forward_ids
    "text": dict(kind="text", D=32, h=4, pool="additive"),        # attention + additive pooler + head: 16 tensors
    "text36": dict(kind="text", D=36, h=6, pool="additive"),      # d_k = 6: the scalar attention kernels
    "mha": dict(kind="mha", D=32, h=4, pool="none"),              # MultiHeadAttention alone (XNRS_POOL_NONE)
    "noatt": dict(kind="text", D=32, h=None, pool="additive"),
    "noatt_ids": dict(kind="text", D=32, h=None, pool="additive", ids=True),
    "mean": dict(kind="text", D=32, h=None, pool="mean"),
    "user": dict(kind="user", D=32, h=4, pool="additive"),
}
IDS = [3, 1, 0, 6, 6, 2, 5, 1, 4]  # rows of the 7-news table: repeats, the all-masked news twice, the one-token news
SHORT = {"wq": "q_linear.weight", "bq": "q_linear.bias", "wk": "k_linear.weight", "bk": "k_linear.bias", "wv": "v_linear.weight",
         "bv": "v_linear.bias", "wo": "out.weight", "bo": "out.bias", "w1": "pooler.fc1.weight", "b1": "pooler.fc1.bias",
         "w2": "pooler.fc2.weight", "b2": "pooler.fc2.bias", "h0w": "head.0.weight", "h0b": "head.0.bias", "h2w": "head.2.weight",
         "h2b": "head.2.bias"}
ATT, POOL, HEAD = list(SHORT)[:8], list(SHORT)[8:12], list(SHORT)[12:]
WEIGHTS = {"wq", "wk", "wv", "wo", "w1", "w2", "h0w", "h2w"}


def shorts_of(tower):
    c = TOWERS[tower]
    return (ATT if c["h"] else []) + (POOL if c["pool"] == "additive" else []) + (HEAD if c["kind"] == "text" else [])


def full_name(tower, short):
    return SHORT[short] if tower == "mha" or short not in ATT else "att." + SHORT[short]


def groups(tower):
    """The named group subsets (trainable tensors, short names), the rows of the list this tower has tensors for."""
    have = set(shorts_of(tower))
    table = [
        ("biases_frozen", have & WEIGHTS), ("weights_frozen", have - WEIGHTS), ("att_frozen", have - set(ATT)),
        ("pooler_frozen", have - set(POOL)), ("head_frozen", have - set(HEAD)), ("only_head", set(HEAD)),
        ("only_wo", {"wo"}), ("only_bo", {"bo"}), ("only_b1", {"b1"}), ("only_w1", {"w1"}),
        ("kv_wk_wv", {"wk", "wv"}), ("kv_wk_wv_bk", {"wk", "wv", "bk"}), ("kv_wk_wv_bk_bv", {"wk", "wv", "bk", "bv"}),
        ("kv_wk", {"wk"}), ("kv_wv_bv", {"wv", "bv"}),
        ("qkv_weights_only", {"wq", "wk", "wv"}), ("qkv_biases_only", {"bq", "bk", "bv"}),
        ("qkv_biases_frozen", have - {"bq", "bk", "bv"}), ("qkv_weights_frozen", have - {"wq", "wk", "wv"}),
    ]
    out, seen = [], []
    for name, s in table:
        s = frozenset(s)
        if s and s <= have and s != have and s not in seen:
            seen.append(s)
            out.append((name, s))
    return out


def subsets(tower, groups_only=False):
    """[(name, frozenset of short names)]: leave-one-out and one-hot of every tensor, then the groups that are neither."""
    names = shorts_of(tower)
    out = [] if groups_only else [(f"loo_{k}", frozenset(names) - {k}) for k in names] + [(f"only_{k}", frozenset([k])) for k in names]
    seen = [s for _, s in out]
    for name, s in groups(tower):
        if s not in seen:
            out.append((name, s))
    return [(n, s) for n, s in out if s]


@functools.lru_cache(maxsize=None)
def tower(name):
    c = TOWERS[name]
    D = c["D"]
    att = layers.MultiHeadAttention(c["h"], D) if c["h"] else None
    if c["kind"] == "mha":
        mod = att
    elif c["kind"] == "user":
        mod = user_encoding.UserEncoder(pooler=layers.AdditiveAttention(D, A_HID), p_dropout=0.0, emb_dim=D, att=att)
    else:
        pooler = layers.AdditiveAttention(D, A_HID) if c["pool"] == "additive" else layers.MaskedMean()
        mod = news_encoding.TextEncoder(pooler=pooler, p_dropout=0.0, out_features=E_OUT, in_features=D, att=att, bias=True)
    return load(mod, 401 + list(TOWERS).index(name))


def oracle_forward(name, x, m, osd):
    c = TOWERS[name]
    n, S = m.shape
    if c["kind"] == "mha":
        return O.multi_head_attention(x, m.reshape(n, S, 1), osd, c["h"])
    if c["kind"] == "user":
        return O.user_encoder(x, m.reshape(n, S, 1), osd, c["h"])[:, 0]
    return O.text_encoder(x.unsqueeze(0), m.reshape(1, n, S, 1), osd, c["h"])[0][0]


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs and the fp64 oracle step with EVERYTHING trainable (read-only): y, dx and every parameter gradient."""
    c = TOWERS[name]
    _, sd = tower(name)
    rng = synth.rng_for(41000 + list(TOWERS).index(name))
    x = torch.from_numpy(rng.standard_normal((N_SEQ, S_LEN, c["D"])).astype(np.float32))
    m = limit_mask(rng, N_SEQ, S_LEN)
    ids = torch.tensor(IDS, dtype=torch.int32) if c.get("ids") else None
    n = len(IDS) if ids is not None else N_SEQ
    osd = f64(sd)
    xo = x.double().requires_grad_(True)
    xg, mg = (xo, m.double()) if ids is None else (xo[ids.long()], m.double()[ids.long()])
    yo = oracle_forward(name, xg, mg, osd)
    w = torch.from_numpy(rng.standard_normal(tuple(yo.shape)).astype(np.float32))
    (yo * w.double()).sum().backward()
    ref = {k: v.grad for k, v in osd.items() if not k.endswith("dummy_param")}
    assert sorted(ref) == sorted(full_name(name, s) for s in shorts_of(name)), sorted(ref)
    return dict(x=x, m=m, ids=ids, w=w, y=yo.detach(), dx=xo.grad, ref=ref, osd=osd, rows=n * S_LEN)


def run_tower(name, trainable, want_dx, via_grad=False):
    """One forward + backward on the GPU with `trainable` (full parameter names) requiring grad -- or, via_grad, with everything
    requiring grad and torch.autograd.grad(loss, inputs=trainable).  -> (y, {name: grad | None}, dx | None)."""
    c = TOWERS[name]
    mod, _ = tower(name)
    ref = reference(name)
    params = {k: p for k, p in mod.named_parameters() if not k.endswith("dummy_param")}
    try:
        poison_workspace()
        for k, p in params.items():
            p.grad = None
            p.requires_grad_(via_grad or k in trainable)
        xd = ref["x"].to(DEV).requires_grad_(want_dx)
        md = ref["m"].to(DEV)
        if c["kind"] == "mha":
            y = mod(xd, md.reshape(N_SEQ, S_LEN, 1))
        elif c["kind"] == "user":
            y = mod((xd, md.reshape(N_SEQ, S_LEN, 1)))[:, 0]
        elif c.get("ids"):
            y = mod.forward_ids(xd, md, ref["ids"].to(DEV).reshape(1, -1))[0][0]
        else:
            y = mod((xd.unsqueeze(0), md.reshape(1, N_SEQ, S_LEN, 1)))[0][0]
        loss = (y * ref["w"].to(DEV)).sum()
        if via_grad:
            order = sorted(trainable)
            got = torch.autograd.grad(loss, [params[k] for k in order] + ([xd] if want_dx else []))
            assert all(p.grad is None for p in params.values()) and xd.grad is None, "autograd.grad left a .grad behind"
            grads = {k: None for k in params}
            grads.update(zip(order, got))
            dx = got[-1] if want_dx else None
        else:
            loss.backward()
            grads = {k: p.grad for k, p in params.items()}
            dx = xd.grad
        for p in params.values():
            p.grad = None
        return y.detach(), grads, dx
    finally:
        for p in params.values():
            p.requires_grad_(True)


_FULL_RUNS = {}


def tower_case(name, lists, fold, want_dx, sub_name, shorts, monkeypatch, via_grad=False):
    """One case of sections A / D: the subset run and (once per tower and knob setting) the all-trainable run, under the list
    mode and the fold knob; the five assertions of the module docstring."""
    c = TOWERS[name]
    ref = reference(name)
    trainable = {full_name(name, s) for s in shorts}
    listed = c["pool"] == "additive"  # (autograd._SeqEncode.forward: row lists ride on an additive pooler with a mask)
    AG, _ = list_mode(monkeypatch, lists)
    tag = f"{name} {lists} fold={fold} dx={int(want_dx)} {'grad(inputs=) ' if via_grad else ''}{sub_name}"
    hip.clear_status()
    with hip.knobs(XNRS_FOLD_TRAIN=fold):
        key = (name, lists, fold, want_dx)
        if key not in _FULL_RUNS:
            _FULL_RUNS[key] = run_tower(name, set(ref["ref"]), want_dx)
        before = dict(AG.STATS)
        seen = spy_wanted_inputs(monkeypatch) if via_grad else None
        y, grads, dx = run_tower(name, trainable, want_dx, via_grad)
        assert_list_mode_ran(AG, before, lists if listed else "dense")
    if via_grad:  # one node, and it was told exactly the subset (the order of autograd._att_tensors | _pool_tensors | _head_tensors)
        assert seen == [[k in shorts for k in shorts_of(name)]], f"{tag}: _wanted_inputs answered {seen}"
    y_full, g_full, dx_full = _FULL_RUNS[key]
    ey = H.assert_close(y, ref["y"], H.RTOL, f"{tag}: y")
    assert torch.equal(y, y_full), f"{tag}: the forward depends on what is frozen"
    eg, er = subset_excess(tag, grads, ref["ref"], trainable, g_full, fc2_bias_bar(ref["osd"], ref["rows"]))
    ex = exr = 0.0
    if want_dx:
        ex, exr = dx_excess(tag, dx, ref["dx"], dx_full)
    else:
        assert dx is None
    hip.check_status()
    print(f"MARGIN {tag}: y {ey / H.RTOL:.3f}  dW {eg:.3f}  dx {ex:.3f}  | vs all-trainable run: dW {er:.3f}  dx {exr:.3f}  (error / bar)")


def _a_cases():
    out = []
    for name, c in TOWERS.items():
        listed = c["pool"] == "additive"
        folds = ("1", "0") if (c["h"] and listed) else ("1",)
        for lists in (("device", "dense") if listed else ("dense",)):
            for fold in folds:
                for want_dx in ((False,) if c.get("ids") else (False, True)):  # (a gathered table has no input gradient)
                    for sub_name, shorts in subsets(name, groups_only=name == "text36"):
                        out.append(pytest.param(name, lists, fold, want_dx, sub_name, shorts,
                                                id=f"{name}-{lists}-fold{fold}-dx{int(want_dx)}-{sub_name}"))
    return out


def test_the_subset_list_is_the_named_one():
    """16 leave-one-out + 16 one-hot + the 14 groups that are neither for the full TextEncoder (only_wo / only_bo / only_b1 /
    only_w1 / kv_wk of the named list ARE one-hot rows); every tower's rows are non-empty proper subsets of its own tensors."""
    assert len(shorts_of("text")) == 16 and len(subsets("text")) == 16 + 16 + 14
    assert {n for n, _ in groups("text")} >= {"only_wo", "only_bo", "only_b1", "only_w1", "weights_frozen", "kv_wk_wv_bk"}
    assert [len(shorts_of(t)) for t in ("mha", "noatt", "mean", "user")] == [8, 8, 4, 12]
    for t in TOWERS:
        for _, s in subsets(t):
            assert s and s < set(shorts_of(t))


@pytest.mark.parametrize("name,lists,fold,want_dx,sub_name,shorts", _a_cases())
def test_sequence_encoder_backward_with_frozen_parameters(name, lists, fold, want_dx, sub_name, shorts, monkeypatch):
    """xnrs_seq_encoder_bwd_rows through requires_grad_(False): every tower, list mode, fold setting, with and without dx."""
    tower_case(name, lists, fold, want_dx, sub_name, shorts, monkeypatch)


# ------------------------------------------------------------------------------------------------ D (towers). autograd.grad(inputs=)
@pytest.mark.parametrize("want_dx", [False, True])
@pytest.mark.parametrize("lists", ["device", "dense"])
@pytest.mark.parametrize("sub_name,shorts", groups("text"), ids=[n for n, _ in groups("text")])
def test_sequence_encoder_backward_through_autograd_grad_inputs(sub_name, shorts, lists, want_dx, monkeypatch):
    """The _wanted_inputs route: every parameter requires grad, torch.autograd.grad(loss, inputs=subset) names what is computed;
    the group subsets on the full TextEncoder, fold on."""
    tower_case("text", lists, "1", want_dx, sub_name, shorts, monkeypatch, via_grad=True)


# ------------------------------------------------------------------------------------------------ B. the two history encodes
B_S, B_H, B_DK, B_N = 17, 2, 16, 7


@functools.lru_cache(maxsize=None)
def two_encode_case():
    D = B_H * B_DK
    enc, sd = load(news_encoding.TextEncoder(pooler=layers.AdditiveAttention(D, A_HID), p_dropout=0.0, out_features=E_OUT,
                                             in_features=D, att=layers.MultiHeadAttention(B_H, D)), 475, train=True)
    p = enc.att.dropout.p
    assert p == 0.1
    x, m, w1 = pooled_inputs(B_N, B_S, D, E_OUT, 47600)
    w2 = torch.from_numpy(synth.rng_for(47601).standard_normal((B_N, E_OUT)).astype("float32"))
    s1, s2 = draw_seeds(TORCH_SEED, 2)
    osd = f64(sd)
    xo, mo = x.double().unsqueeze(0), m.double().reshape(1, B_N, B_S, 1)
    y1, _ = O.text_encoder(xo, mo, osd, B_H, drop=(O.attention_keep_mask(s1, B_N, B_H, B_S, p), p))
    y2, _ = O.text_encoder(xo, mo, osd, B_H, drop=(O.attention_keep_mask(s2, B_N, B_H, B_S, p), p))
    ((y1[0] * w1.double()).sum() + (y2[0] * w2.double()).sum()).backward()
    assert H.rel_err(y2.detach(), y1.detach()) > 100 * H.RTOL  # the two encodes really differ
    ref = {k: v.grad for k, v in osd.items() if not k.endswith("dummy_param")}
    return dict(enc=enc, x=x, m=m, w1=w1, w2=w2, y1=y1.detach()[0], y2=y2.detach()[0], ref=ref, osd=osd)


def run_two_encodes(c, trainable, AG):
    enc = c["enc"]
    params = {k: p for k, p in enc.named_parameters() if not k.endswith("dummy_param")}
    try:
        poison_workspace()
        for k, p in params.items():
            p.grad = None
            p.requires_grad_(k in trainable)
        before = dict(AG.STATS)
        torch.manual_seed(TORCH_SEED)
        xd, md = c["x"].to(DEV).unsqueeze(0), c["m"].to(DEV).reshape(1, B_N, B_S, 1)  # (no input gradient: the merge needs none asked for)
        ya, _ = enc((xd, md))
        yb, _ = enc((xd, md))
        ((ya[0] * c["w1"].to(DEV)).sum() + (yb[0] * c["w2"].to(DEV)).sum()).backward()
        d = {k: AG.STATS[k] - before[k] for k in before}
        grads = {k: p.grad for k, p in params.items()}
        for p in params.values():
            p.grad = None
        return ya.detach()[0], yb.detach()[0], grads, d
    finally:
        for p in params.values():
            p.requires_grad_(True)


@pytest.mark.parametrize("lists", ["device", "dense"])
@pytest.mark.parametrize("frozen,deltas", [("wq", (1, 0, 0)), ("bq", (1, 0, 0)), ("wk", (1, 0, 0)), ("bk", (1, 0, 0)), ("wv", (1, 0, 0)),
                                           ("bv", (1, 0, 0)), ("head", (1, 1, 1)), ("pooler", (1, 1, 1))])
def test_two_history_encodes_with_a_frozen_tensor(frozen, deltas, lists, monkeypatch):
    """One TextEncoder in train mode (attention dropout 0.1) called twice on the same input, loss over both outputs; reference:
    two fp64 oracle passes under the two restated keep masks, gradients summed.  Control (everything trainable): the second
    forward shares the first one's Q|K|V image, one backward defers, one merges.  With one Q/K/V tensor frozen neither node
    defers or merges and every other gradient is complete; with only head or pooler tensors frozen the merge stays."""
    c = two_encode_case()
    AG, _ = list_mode(monkeypatch, lists)
    names = sorted(c["ref"])
    off = {"head": [k for k in names if k.startswith("head.")], "pooler": [k for k in names if k.startswith("pooler.")]}.get(
        frozen) or ["att." + SHORT[frozen]]
    trainable = set(names) - set(off)
    tag = f"two encodes {lists} {frozen} frozen"
    hip.clear_status()
    ya0, yb0, g0, d0 = run_two_encodes(c, set(names), AG)
    assert (d0["shared_qkv_forwards"], d0["deferred_dqkv_backwards"], d0["merged_dqkv_backwards"]) == (1, 1, 1), d0
    assert d0["device_list_forwards"] == (1 if lists == "device" else 0), d0
    extra = fc2_bias_bar(c["osd"], 2 * B_N * B_S)
    e0, _ = subset_excess(tag + " (control)", g0, c["ref"], set(names), None, extra)
    ya, yb, g, d = run_two_encodes(c, trainable, AG)
    assert (d["shared_qkv_forwards"], d["deferred_dqkv_backwards"], d["merged_dqkv_backwards"]) == deltas, d
    ey = max(H.assert_close(ya, c["y1"], H.RTOL, f"{tag}: first encode"), H.assert_close(yb, c["y2"], H.RTOL, f"{tag}: second encode"))
    assert torch.equal(ya, ya0) and torch.equal(yb, yb0)
    eg, er = subset_excess(tag, g, c["ref"], trainable, g0, extra)
    hip.check_status()
    print(f"MARGIN {tag}: y {ey / H.RTOL:.3f}  dW {eg:.3f} (control {e0:.3f})  | vs all-trainable run: dW {er:.3f}  (error / bar)")


# ------------------------------------------------------------------------------------------------ C. shared towers in a whole step
# (the seed: reference scores on both sides of the ReLU, -0.017 .. 0.033, none within 0.004 of it -- at seed 4300 every score is
# negative and every gradient of the step is exactly zero)
STEP = dict(model="NRMS", B=3, H=4, C=3, S=8, D=32, h=4, E=16, bias=True, seed=4303)
STEP_SUBSETS = {
    "news_tower_frozen": lambda k: k.startswith("user_encoder."),
    "user_tower_frozen": lambda k: k.startswith("news_encoder."),
    "only_biases": lambda k: k.endswith(".bias"),
    "only_news_head": lambda k: k.startswith("news_encoder.head."),
}


@functools.lru_cache(maxsize=None)
def step_case():
    c = STEP
    model, sd = load(make_model(Cfg(cases.model_cfg(c))), c["seed"] + 1)
    batch = cases.model_batch(c)
    osd = f64(sd)
    hist, cand = batch["user_features"]["history"]["title_emb"], batch["candidate_features"]["title_emb"]
    ro = O.parent_forward(tuple(t.double() for t in hist), tuple(t.double() for t in cand), osd, c["h"])
    rv = ro.detach()
    assert 0 < int((rv > 0).sum()) < rv.numel() and float(rv.abs().min()) > 100 * H.RTOL * float(rv.abs().max())
    torch.nn.functional.mse_loss(torch.relu(ro), batch["targets"].double()).backward()
    ref = {k: v.grad for k, v in osd.items() if not k.endswith("dummy_param")}
    assert len(ref) == 28 and all(v is not None for v in ref.values())  # news 16 + user 12: the tower is called twice per step
    rows = {"news_encoder": c["B"] * (c["H"] + c["C"]) * c["S"], "user_encoder": c["B"] * c["H"]}

    def extra(k, scale, gmax):  # H.fc2_bias_extra_bar with the token rows of the tower the pooler belongs to
        if not k.endswith("pooler.fc2.bias"):
            return 0.0
        return H.fc2_bias_extra_bar(rows[k.split(".")[0]], ref[k[:-len("bias")] + "weight"].abs().max().item(), scale, gmax)
    return dict(model=model, batch=batch, r=ro.detach(), ref=ref, extra=extra)


def step_wanted(trainable):
    """What _wanted_inputs must answer in the encoder nodes of the step: the user tower (12 tensors; every gradient passes
    through it) and, unless nothing of the news tower is asked for -- the engine then never runs its nodes --, the news tower
    twice (16 tensors)."""
    news = [("news_encoder." + full_name("text", k)) in trainable for k in shorts_of("text")]
    user = [("user_encoder." + full_name("user", k)) in trainable for k in shorts_of("user")]
    return sorted([user] + ([news, news] if any(news) else []))


def run_step(c, trainable, via_grad=False):
    model = c["model"]
    params = {k: p for k, p in model.named_parameters() if not k.endswith("dummy_param")}
    try:
        poison_workspace()
        for k, p in params.items():
            p.grad = None
            p.requires_grad_(via_grad or k in trainable)
        r = model(c["batch"])
        loss = torch.nn.functional.mse_loss(torch.relu(r), c["batch"]["targets"].to(DEV))
        if via_grad:
            order = sorted(trainable)
            got = torch.autograd.grad(loss, [params[k] for k in order])
            assert all(p.grad is None for p in params.values()), "autograd.grad left a .grad behind"
            grads = {k: None for k in params}
            grads.update(zip(order, got))
        else:
            loss.backward()
            grads = {k: p.grad for k, p in params.items()}
        for p in params.values():
            p.grad = None
        return r.detach(), grads
    finally:
        for p in params.values():
            p.requires_grad_(True)


@pytest.mark.parametrize("via_grad", [False, True], ids=["requires_grad", "grad_inputs"])
@pytest.mark.parametrize("subset", list(STEP_SUBSETS))
def test_whole_step_with_frozen_towers(subset, via_grad, monkeypatch):
    """A tiny NRMS (bias=True), loss mse(relu(model(batch)), targets), reference O.parent_forward in fp64.  The news tower is
    called for history and candidates, so its nodes keep gradient sets back (_sum_with_group): the frozen entries stay None
    through the merge, the wanted ones are complete.  Control: everything trainable.  Both through requires_grad_(False) and
    through torch.autograd.grad(loss, inputs=subset) (section D)."""
    c = step_case()
    names = set(c["ref"])
    trainable = {k for k in names if STEP_SUBSETS[subset](k)}
    assert trainable and trainable < names
    tag = f"step {subset} {'grad(inputs=)' if via_grad else 'requires_grad'}"
    hip.clear_status()
    r0, g0 = run_step(c, names)
    er0 = H.assert_close(r0, c["r"], H.RTOL, f"{tag}: scores (control)")
    e0, _ = subset_excess(tag + " (control)", g0, c["ref"], names, None, c["extra"])
    seen = spy_wanted_inputs(monkeypatch)
    r, g = run_step(c, trainable, via_grad)
    assert torch.equal(r, r0)
    if via_grad:  # (under requires_grad_(False) the engine executes every node it knows: the frozen ones are not in the graph)
        assert sorted(seen) == step_wanted(trainable), f"{tag}: _wanted_inputs answered {seen}"
    eg, er = subset_excess(tag, g, c["ref"], trainable, g0, c["extra"])
    hip.check_status()
    print(f"MARGIN {tag}: r {er0 / H.RTOL:.3f}  dW {eg:.3f} (control {e0:.3f})  | vs all-trainable run: dW {er:.3f}  (error / bar)")


# ------------------------------------------------------------------------------------------------ E. the other autograd functions
def run_op(leaves, call, dy, wanted, via_grad=False):
    """leaves: name -> persistent leaf tensor on the device (module parameters included); `wanted` require grad -- or, via_grad,
    all of them do and torch.autograd.grad(outputs, inputs=wanted) names what is computed."""
    try:
        poison_workspace()
        for k, t in leaves.items():
            t.grad = None
            t.requires_grad_(via_grad or k in wanted)
        y = call(leaves)
        ys, dys = (list(y), list(dy)) if isinstance(y, tuple) else ([y], [dy])
        if via_grad:
            order = [k for k in leaves if k in wanted]
            got = torch.autograd.grad(ys, [leaves[k] for k in order], [d.to(DEV) for d in dys])
            assert all(t.grad is None for t in leaves.values()), "autograd.grad left a .grad behind"
            grads = {k: None for k in leaves}
            grads.update(zip(order, got))
        else:
            torch.autograd.backward(ys, [d.to(DEV) for d in dys])
            grads = {k: t.grad for k, t in leaves.items()}
        for t in leaves.values():
            t.grad = None
        return [t.detach() for t in ys], grads
    finally:
        for t in leaves.values():
            t.requires_grad_(True)


def op_case(tag, leaves, call, dy, y_ref, ref, sets=None, floor_keys=None, monkeypatch=None):
    """One operator: the all-trainable run, then every output one-hot and leave-one-out (or `sets`), assertions (1)-(5).
    monkeypatch (the functions that ask _wanted_inputs: one node whose differentiable inputs are the leaves): every subset again
    through torch.autograd.grad(inputs=subset) with everything requiring grad, and the node was told exactly that many inputs."""
    names = list(leaves)
    y_ref = list(y_ref) if isinstance(y_ref, (tuple, list)) else [y_ref]
    hip.clear_status()
    y0, g0 = run_op(leaves, call, dy, set(names))
    worst = [0.0, 0.0, 0.0]
    for wanted in [frozenset(names)] + (sets or one_hot_and_leave_one_out(names)):
        t = f"{tag} {{{', '.join(k for k in names if k in wanted)}}}"
        y, g = run_op(leaves, call, dy, wanted)
        for a, b, b0 in zip(y, y_ref, y0):
            worst[0] = max(worst[0], H.assert_close(a, b, H.RTOL, f"{t}: y") / H.RTOL)
            assert torch.equal(a, b0), f"{t}: the forward depends on what is frozen"
        eg, er = subset_excess(t, g, ref, wanted, g0, None, floor_keys)
        worst[1], worst[2] = max(worst[1], eg), max(worst[2], er)
        if monkeypatch is not None:
            with monkeypatch.context() as mp:
                seen = spy_wanted_inputs(mp)
                _, g = run_op(leaves, call, dy, wanted, via_grad=True)
            assert len(seen) == 1 and sum(seen[0]) == len(wanted), f"{t}: _wanted_inputs answered {seen}"
            eg, er = subset_excess(t + " grad(inputs=)", g, ref, wanted, g0, None, floor_keys)
            worst[1], worst[2] = max(worst[1], eg), max(worst[2], er)
    hip.check_status()
    print(f"MARGIN {tag}: y {worst[0]:.3f}  grads {worst[1]:.3f}  | vs all-trainable run: {worst[2]:.3f}  (error / bar, the worst subset)")


def dev_leaf(t):
    return t.to(DEV).requires_grad_(True)


def gen(seed):
    return torch.Generator().manual_seed(seed)


ACTS = {"none": lambda t: t, "tanh": torch.tanh}


@pytest.mark.parametrize("mode", ["rows", "ids_dense", "ids_sparse"])
@pytest.mark.parametrize("K", [50, 64])
@pytest.mark.parametrize("act", list(ACTS))
def test_linear_backward_with_every_subset_of_its_outputs(act, K, mode, monkeypatch):
    """_Linear (xnrs_act_bwd + xnrs_linear_bwd / xnrs_embedding_linear_bwd / _sparse): the seven non-empty subsets of
    {dx or d_table, dw, db}; M = 7 rows, N = 70 columns (a wave and a tail)."""
    M, N, n_rows = 7, 70, 9
    g = gen(51000 + K)
    fn, code = ACTS[act], {"none": hip.ACT_NONE, "tanh": hip.ACT_TANH}[act]
    x = torch.randn(M if mode == "rows" else n_rows, K, generator=g)
    w, b, dy = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    ids = None if mode == "rows" else torch.tensor([8, 0, 3, 3, 5, 0, 7], dtype=torch.int32)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    yr = fn(torch.nn.functional.linear(xr if ids is None else xr[ids.long()], wr, br))
    yr.backward(dy.double())
    first = "x" if ids is None else "table"
    leaves = {first: dev_leaf(x), "w": dev_leaf(w), "b": dev_leaf(b)}
    idd = None if ids is None else ids.to(DEV)
    call = lambda L: ops.linear(L[first], L["w"], L["b"], code, ids=idd, table_grad="sparse" if mode == "ids_sparse" else "dense")  # noqa: E731
    names = list(leaves)
    sets = [frozenset(s) for s in ([names[0]], [names[1]], [names[2]], names[:2], names[1:], [names[0], names[2]])]
    op_case(f"linear {mode} act={act} K={K}", leaves, call, dy, yr.detach(), {first: xr.grad, "w": wr.grad, "b": br.grad}, sets,
            monkeypatch=monkeypatch)


@pytest.mark.parametrize("normalize", [False, True])
def test_dot_scoring_backward_with_one_output(normalize):
    """_DotScoring at B = 3, C = 5, E = 80: only du, only dc."""
    B, C, E = 3, 5, 80
    g = gen(52000)
    u, c, dr = torch.randn(B, 1, E, generator=g), torch.randn(B, C, E, generator=g), torch.randn(B, C, 1, generator=g)
    ur, cr = u.double().requires_grad_(True), c.double().requires_grad_(True)
    rr = O.dot_scoring(ur, cr, normalize)
    rr.backward(dr.double())
    leaves = {"u": dev_leaf(u), "c": dev_leaf(c)}
    op_case(f"dot scoring normalize={normalize}", leaves, lambda L: ops.dot_scoring(L["u"], L["c"], normalize), dr, rr.detach(),
            {"u": ur.grad, "c": cr.grad})


def scorer_case(tag, mod, kind, normalize, B, N, E, seed, monkeypatch):
    g = gen(seed)
    sd = {k: v.clone() for k, v in synth.fill_state_dict({k: tuple(v.shape) for k, v in mod.state_dict().items()}, seed).items()}
    mod.load_state_dict(sd)
    mod.to(DEV)
    u, c, ds = torch.randn(B, 1, E, generator=g), torch.randn(B, N, E, generator=g), torch.randn(B, N, 1, generator=g)
    s, du, dc, dp = _fp64(kind, sd, u, c, normalize, ds)
    leaves = {"u": dev_leaf(u), "c": dev_leaf(c)}
    leaves.update(dict(mod.named_parameters()))
    ref = {"u": du, "c": dc}
    ref.update(dp)
    op_case(tag, leaves, lambda L: mod(L["u"], L["c"]), ds, s.detach(), ref, monkeypatch=monkeypatch)


@pytest.mark.parametrize("normalize", [False, True])
def test_bilinear_scoring_backward_with_every_output_alone_and_left_out(normalize, monkeypatch):
    """_BilinScoring with a bias: du, dc, dw, db; only db wanted skips the whole `if (du || dc || dw)` block."""
    scorer_case(f"bilinear scoring normalize={normalize}", BilinScoring(80, normalize=normalize, bias=True), "bilin", normalize, 3, 5, 80,
                53000, monkeypatch)


def test_mlp_scoring_backward_with_every_output_alone_and_left_out(monkeypatch):
    """_MlpScoring: du, dc, dw1, db1, dw2, db2 (E = 80, H = 70)."""
    scorer_case("mlp scoring", FCScoring(80, hidden_dim=70, bias=True), "fc", False, 3, 5, 80, 54000, monkeypatch)


@pytest.mark.parametrize("with_ids", [False, True])
def test_personalized_backward_with_every_output_alone_and_left_out(with_ids, monkeypatch):
    """_Personalized with a head: dx, dq, dwx, dbx and the four head tensors (A = 70); over a gathered table there is no dx."""
    n_q, per, L, D, A, E = 2, 3, 13, 24, 70, 16
    n = n_q * per
    g = gen(55000)
    torch.manual_seed(55000)
    n_tab = 8 if with_ids else n
    x = torch.randn(n_tab, L, D, generator=g)
    m = limit_mask(synth.rng_for(55000), n_tab, L)
    ids = torch.tensor([5, 1, 0, 7, 7, 2], dtype=torch.int32) if with_ids else None
    q = torch.randn(n_q, A, generator=g) * 0.3
    q_idx = torch.div(torch.arange(n), per, rounding_mode="floor").to(torch.int32)
    x_fc = nn.Linear(D, A)
    head = nn.Sequential(nn.Linear(D, E), nn.ReLU(), nn.Linear(E, E))
    dy = torch.randn(n, E, generator=g)
    xr, qr = x.double().requires_grad_(True), q.double().requires_grad_(True)
    pr = [p.detach().double().requires_grad_(True) for p in list(x_fc.parameters()) + list(head.parameters())]
    xg, mg = (xr, m.double()) if ids is None else (xr[ids.long()], m.double()[ids.long()])
    yr = _ref_pa(xg, mg, qr, q_idx, pr[0], pr[1], pr[2:])
    yr.backward(dy.double())
    x_fc, head = x_fc.to(DEV), head.to(DEV)
    pnames = ["wx", "bx", "h0w", "h0b", "h2w", "h2b"]
    leaves = {} if with_ids else {"x": dev_leaf(x)}
    leaves["q"] = dev_leaf(q)
    leaves.update(zip(pnames, list(x_fc.parameters()) + list(head.parameters())))
    ref = {} if with_ids else {"x": xr.grad}
    ref["q"] = qr.grad
    ref.update(zip(pnames, [p.grad for p in pr]))
    xt, md, idd, qi = x.to(DEV), m.to(DEV), None if ids is None else ids.to(DEV), q_idx.to(DEV)
    call = lambda Lv: ops.personalized(Lv["x"] if "x" in Lv else xt, md, idd, Lv["q"], qi, x_fc, head)[0]  # noqa: E731
    op_case(f"personalized ids={with_ids}", leaves, call, dy, yr.detach(), ref, monkeypatch=monkeypatch)


@pytest.mark.parametrize("with_h0,Hd", [(True, 68), (False, 70)])
def test_gru_backward_with_every_output_alone_and_left_out(with_h0, Hd, monkeypatch):
    """_Gru: dx, dh0 and the four parameter tensors; with an initial state (Hd = 68: the 16-byte loads) and without (Hd = 70:
    the scalar loads; dh then lives in the workspace)."""
    B, T, N, E = 5, 7, 9, 12
    g = gen(56000 + Hd)
    torch.manual_seed(56000 + Hd)
    x = torch.randn(B, T, E, generator=g)
    m = (torch.rand(B, N, generator=g) > 0.4).float()
    m[0, :T] = 0
    m[B - 1, :T] = 1
    lens = m[:, :T].sum(1).long()
    h0 = torch.randn(B, Hd, generator=g) * 0.5 if with_h0 else None
    gru = nn.GRU(E, Hd, batch_first=True)
    dy = torch.randn(B, Hd, generator=g)
    pn = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"]
    xr = x.double().requires_grad_(True)
    hr = h0.double().requires_grad_(True) if with_h0 else None
    pr = [getattr(gru, k).detach().double().requires_grad_(True) for k in pn]
    yr = _ref_gru(xr, lens, hr, *pr)
    yr.backward(dy.double())
    gru = gru.to(DEV)
    leaves, ref = {"x": dev_leaf(x)}, {"x": xr.grad}
    if with_h0:
        leaves["h0"], ref["h0"] = dev_leaf(h0), hr.grad
    leaves.update({k: getattr(gru, k) for k in pn})
    ref.update({k: p.grad for k, p in zip(pn, pr)})
    md = m.to(DEV)[..., None]
    op_case(f"gru h0={with_h0} Hd={Hd}", leaves, lambda L: ops.gru(L["x"], md, L.get("h0"), gru), dy, yr.detach(), ref,
            monkeypatch=monkeypatch)


CAUM_B, CAUM_C, CAUM_H, CAUM_E, CAUM_A = 2, 3, 65, 12, 8


def test_caum_pair_backward_with_one_output():
    """_CaumPair (xnrs_caum_pair_bwd: d_hp / d_cp, each nullable) at H = 65 against the formulas of include/xnrs_hip.h in fp64."""
    B, C, Hn, E = CAUM_B, CAUM_C, CAUM_H, CAUM_E
    g = gen(57000)
    hp, cp = torch.randn(B * Hn, 4 * E, generator=g), torch.randn(B * C, 2 * E, generator=g)
    dy = (torch.randn(B * C * Hn, E, generator=g), torch.randn(B * C * Hn, E, generator=g))
    hr, cr = hp.double().requires_grad_(True), cp.double().requires_grad_(True)
    left, mid, right, zh = hr.reshape(B, Hn, 4 * E).split(E, dim=2)
    c3 = cr.reshape(B, C, 1, 2 * E)
    h_cnn = (torch.roll(left, 1, dims=1) + mid + torch.roll(right, -1, dims=1))[:, None] + c3[..., :E]
    z = zh[:, None] + c3[..., E:]
    yr = (h_cnn.reshape(-1, E), z.reshape(-1, E))
    torch.autograd.backward(list(yr), [d.double() for d in dy])
    leaves = {"hp": dev_leaf(hp), "cp": dev_leaf(cp)}
    op_case("caum pair", leaves, lambda L: ops.caum_pair(L["hp"], L["cp"], B, C, Hn), dy, [t.detach() for t in yr],
            {"hp": hr.grad, "cp": cr.grad})


def test_caum_bias_tanh_backward_with_one_output():
    """_CaumBiasTanh (xnrs_caum_bias_tanh_bwd: dcb nullable) at H = 65."""
    P, Hn, E = CAUM_B * CAUM_C, CAUM_H, CAUM_E
    g = gen(57100)
    pre, cb, dt = torch.randn(P * Hn, E, generator=g), torch.randn(P, E, generator=g), torch.randn(P * Hn, E, generator=g)
    pr, cr = pre.double().requires_grad_(True), cb.double().requires_grad_(True)
    tr = torch.tanh(pr.reshape(P, Hn, E) + cr[:, None]).reshape(P * Hn, E)
    tr.backward(dt.double())
    leaves = {"pre": dev_leaf(pre), "cb": dev_leaf(cb)}
    op_case("caum bias tanh", leaves, lambda L: ops.caum_bias_tanh(L["pre"], L["cb"], Hn), dt, tr.detach(), {"pre": pr.grad, "cb": cr.grad})


def test_caum_pool_backward_with_every_output_alone_and_left_out():
    """_CaumPool (xnrs_caum_pool_bwd: d_t2, d_h_all, d_w3, d_b3) at H = 65 against the fp64 softmax pool of
    tests/test_hip_length_limits.py, with its bar: GTOL of max(own scale, 1e-3 of the largest PARAMETER gradient) -- for db3,
    which cancels analytically (a bias in front of a softmax), that is 1e-3 of dw3."""
    P, Hn, A, E = CAUM_B * CAUM_C, CAUM_H, CAUM_A, CAUM_E
    g = gen(57200)
    t2 = torch.tanh(torch.randn(P * Hn, A, generator=g))
    h_all = torch.randn(P * Hn, E, generator=g)
    w3, b3, du = torch.randn(1, A, generator=g) / A ** 0.5, torch.randn(1, generator=g), torch.randn(P, E, generator=g)
    r = {k: t.double().requires_grad_(True) for k, t in (("t2", t2), ("w3", w3), ("b3", b3), ("h_all", h_all))}
    a = torch.softmax((r["t2"] @ r["w3"].reshape(-1) + r["b3"]).reshape(P, Hn), dim=-1)
    ur = (a[..., None] * r["h_all"].reshape(P, Hn, E)).sum(1)
    ur.backward(du.double())
    leaves = {k: dev_leaf(t) for k, t in (("t2", t2), ("w3", w3), ("b3", b3), ("h_all", h_all))}
    op_case("caum pool", leaves, lambda L: ops.caum_pool(L["t2"], L["w3"], L["b3"], L["h_all"], Hn), du, ur.detach(),
            {k: v.grad for k, v in r.items()}, floor_keys=("w3", "b3"))
