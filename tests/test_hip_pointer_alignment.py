"""GPU: every launcher's unaligned-pointer fallback, operand by operand.

include/xnrs_hip.h asks for contiguous device pointers and no more, so an operand 4 bytes (bf16: 2) off a 16-byte boundary is
a legal argument everywhere.  Almost every kernel family has a 16-byte vector instantiation and a scalar one (or a fused and
an unfused route) and a host predicate that picks from the widths AND the address bits.  The rest of the suite reaches the
scalar instantiations through odd widths only; here every width is a multiple of 4 (8 for bf16) -- the aligned call provably
takes the vector / fused route -- and the ADDRESSES are moved: tests/align_ref.py puts each operand at a chosen offset from a
16-byte boundary inside a buffer with 16 sentinel elements on either side.  Workspaces and saved blobs are never shifted: they
must be 256-byte aligned (the header's Conventions; xnrs_amd/hip.py::workspace checks its own).

Section 0 -- what was read before anything ran.  Launcher -> operands its vector code touches 8 / 16 bytes at a time -> what
its predicate tests -> where an ABI caller can reach it ("ws" = a region of the caller's workspace / saved blob only).

  launch_gemm_f32 `vec` (gemm_f32.hip)     A, W[s] rows (global / raw-buffer b128), lda, ldw, K or M, Nseg | all of them |
      every GEMM: xnrs_linear_fwd / _bwd, the encoders' x and weights.  bias, aux, rowdot_w, rowscale, C / ldc, colsum, slabs
      are read and written 4 bytes at a time (gemm_f32_body.h epilogue): nothing to test.
      ... but the RDOT / MDEV / LIVE instantiations exist in vector form only (launch_cfg returns an error without `vec`), so
      the route predicates in front of them must name every GEMM operand: fc1_rowdot_ok and device_counts_ok tested pool->w1
      but the product reads pool->w1_folded when the call folds  ->  ADDED (encoder_fwd.hip); xnrs_text_encoder_fwd_compact
      tested fc1 only, its Q and K|V products read x, wq, wk, wv  ->  ADDED (XNRS_EUNSUPPORTED, as the header promises; the
      Python mirror ops.compact_supported gained the same addresses: TextEncoder(unpadded=True) with flat parameters raised).
  gemm_dw_eligible (gemm_dw.hip)           A, W[0], colsum (f32x4 store), M, Nseg, lda, ldw | all | linear / encoder backward.
      Its row threshold (a contraction of >= 8192 rows, 64 x 64 outputs) is a constant that no knob lowers; XNRS_GEMM_DW=3
      sends a dense launch there: family linear_bwd_dw runs it at 8200 rows and moves dy and x (its A / W) off 16 bytes
  cs_copy, gemm_f32.hip:564                colsum_out in place only when 16-byte aligned, else colsum_final copies | db
  gemm_a16_ok / launch_gemm_split          bf16 rows (16-byte loads of 8), A / W of the split kernel, planes (ws) | x16 % 16,
      lda % 8, K % 8, the planes; the split kernel is entered behind launch_gemm_f32's `vec` only | xnrs_linear_fwd_bf16,
      xnrs_text_encoder_fwd_bf16, xnrs_linear_fwd in modes 1 / 2 (families linear_fwd_bf16, text_encoder_bf16, linear_fwd_split,
      each forced onto its small shape by XNRS_GEMM_SPLIT_MIN_TILES=0)
  gemm_qkv_one_launch_ok, gemm_fc1_in_tail_ok   A, W of each section | all (qkv_section_ok) | dense encoder passes; the lists
      they ride on also need device_counts_ok: x, wq, wk, wv, wo, w1 (+ w1_folded, added)
  mha_pick (mha_core.hip)                  q, k, V, out rows; ld, ldo, seq_stride, head_stride, d_k | q, k, out, ld, ldo, d_k
      ->  ADDED v, seq_stride % 4, head_stride % 4.  ws only: q | k | v are one workspace image, out a workspace region
      (qkv_shared: a saved blob) -- unreachable through the ABI today, the predicate is now right by itself.
  launch_mha_bwd `vec` / `fused`           q, k, v, d_o, o, dq, dk, dv, ld, lddo, ldd, ldo | all | ws only
  launch_additive_pool_bwd `vec`           x, dp, t, w2, dpre, dx, ldx, lddx, D, A | all | x, w2, dy (no head), dx
  additive_fused_ready                     x rows, w1 (raw buffer), y (f32x4), ldy | all | xnrs_text_encoder_fwd w/o attention
  news_fused_ready (news_fused.hip:745)    x, wq, wk, wv, wo, w1 (prep kernel f32x4), img, o_scratch (ws), p (f32x4 store)
      | all but p  ->  ADDED p, ldp (p is the caller's y without a head and with XNRS_FOLD_OUT=0); and news_fused_route asked
      about pool->w1 while prepare_weights hands the kernel pool->w1_folded  ->  ADDED: such a call FAILED (launch refused).
  tk_vec_ok (sweep.h: sweep_operands)      table / P, up rows through tk_load (sweep.h) / tl_load (table_loss.hip) | both, each on its own | top-k, rank,
      table loss.  Outputs, w, w1, bias: 4 bytes at a time.
  gru.hip:327                              w_hh, h0 (load_k4) | both, Hd % 4 | xnrs_gru_fwd*; the backward reads ws only
  gather.hip:49 / 105 / 183                table / x and out rows | both, row width | xnrs_gather_rows, _dropout_rows, *_bf16
  personalized.hip:434                     d_table (zero_fill f32x4) | d_table | xnrs_embedding_grad_sparse
  caum.hip, scorers.hip, infonce.hip, pool_score.hip   no 8 / 16-byte global access (grep, confirmed by reading): one
      "all shifted" case each below, through the models that run them and the raw dot / InfoNCE / CSR / long-attention calls.

What each case asserts: return code 0 and a clean status word; every output against the fp64 reference of the operation at
the project's bar (helpers.assert_close at RTOL with its elementwise part; gradients at the bars of the family's own file);
every output within RUN_TOL = 2e-5 of the aligned GPU run (the bar between two GPU routes of test_hip_frozen_params.py /
test_hip_train_step.py::_close); the same BITS as the aligned run where the two routes differ in load / store width only (the
gathers, dropout_rows_bf16, every top-k / rank / table-loss score, loss and lse; ids and ranks torch.equal); the guards
around every operand untouched.  No tolerance is new.  MARGIN lines print error / bar.

Route evidence: xnrs_qkv_launch_count / xnrs_fc1_in_tail_count / xnrs_mha_live_o_count (non-zero aligned, zero once an
operand the predicates name is shifted, unchanged otherwise) on the inference family text_encoder_lists -- the three routes
exist in inference only (make_route: live row tiles, and with them the one-launch projection, fc1 in the tail and live O, are
`!r.train`), so the seq_encoder_train* families have no such counter to assert; the launch timer's stage counts for the fused
news kernel (the timer counts one record per stage scope, not kernel launches: the extra colsum_final launch of the cs_copy
leg is inside the weight-gradient scope and cannot be told by it -- the mutation below is its evidence); XNRS_EUNSUPPORTED
with nothing written for the device-compacted encoder; autograd.STATS["device_list_forwards"] for the Python mirror.  Elsewhere: the table above and these value-only mutations,
each made in a scratch copy of the tree and never committed (failed cases of this file's 811; no "aligned" case failed in any):
  tk_load's scalar branch drops its fourth element           50: every top-k / rank / table-loss case with table / P or u shifted, the
                                                                 table-at-+4 test
  tl_load's scalar branch drops its fourth element           11: both table-loss families (table, up, all, the 8 / 12-byte cases), the
                                                                 table-at-+4 test
  gemm_f32_body.h row-major scalar A load x (1 + 2^-10)     215: every GEMM-fed family where a forward-layout A operand is shifted --
                                                                 linear_fwd_split x / w (the split kernel left for the fp32 one), the
                                                                 encoders, scorers, personalized, gru -- and every flat-parameter model
  gemm_f32_body.h k-major scalar A load x (1 + 2^-10)        55: the weight-gradient products: linear_bwd_dw dy / x (gemm_dw.hip left for
                                                                 the k-major kernel), linear_bwd, embedding_linear_bwd*, seq_encoder_train*,
                                                                 gru, personalized, the scorers, the models
  gather_rows_kernel<false> scales by 1 + 2^-10              10: gather_rows table / out / all / 8 / 12 (7), the three LSTUR models
  gather_rows_bf16_kernel<false> scales by 1 + 2^-10         22: gather_rows_bf16 and dropout_rows_bf16 (7 each), linear_fwd_bf16 and
                                                                 text_encoder_bf16 x 2 / 4 / 8 and all (gemm_a16_ok said no: widened)
  additive_pool_bwd_kernel<false> halves dpre                12: seq_encoder_train* w2 and all, both NRMS tests, LSTUR x3, CAUM
  the cs_copy leg (gemm_f32.hip:564) zeroes db[0]            32: every case that shifts a bias-gradient output of a one-slice product
  xnrs_embedding_grad_sparse's memset leg fills 0x40          4: embedding_linear_bwd_sparse d_table 4 / 8 / 12 and all
  gru.hip load_k4's scalar branch scales by 1 + 2^-10         8: gru w_hh, h0 (4 / 8 / 12) and all, the three LSTUR models
mha_core_kernel<KT, false> cannot be reached with d_k % 4 == 0 through the ABI (workspace operands only), so no mutation of it
can fail here; tests/test_hip_length_limits.py and the odd head widths of the attention tests run it.

Observed on an MI355X: the whole file 811 cases in 8.3 s (the slowest 0.8 s: the first launch of a process); every margin
against fp64 below 0.08 of its bar, against the aligned run below 0.02 of RUN_TOL except the two analytically zero
gradients of the training families (key bias 0.44, fc2 bias 0.48, both on the 1e-3 floor of their scale).

Not a case of its own: the *_rows training entry points with DEVICE counts refuse a misaligned operand by design
(device_counts_ok; the NRMS test shows the Python mirror choosing host lists instead), a shallow xnrs_topk_win does not exist
(the header: k <= 128 of xnrs_topk_deep*_win runs xnrs_topk's launches).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import xnrs_oracle as O
from tests import align_ref as AR
from tests import helpers as H
from tests import input_dropout_ref as R
from xnrs_amd import hip, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RUN_TOL = 2e-5   # two GPU routes of one computation (test_hip_frozen_params.py, test_hip_train_step.py::_close)
GRAD_TOL = 2e-4  # DESIGN.md's gradient bar: per tensor, of its own maximum (test_hip_linear_ops.py, test_hip_grads.py GTOL)
F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
EUNSUPPORTED = hip._CONSTANTS["EUNSUPPORTED"]
LISTS = dict(XNRS_GEMM_LIVE_TILES="1", XNRS_GEMM_LIVE_TILES_MIN_ROWS="0", XNRS_GEMM_LIVE_ROWS="1", XNRS_GEMM_LIVE_ROWS_MIN_ROWS="0",
             XNRS_GEMM_QKV_ONE_LAUNCH="1", XNRS_GEMM_FC1_IN_TAIL="1", XNRS_MHA_LIVE_O="1")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def stream():
    return hip.stream_ptr(torch.device(DEV))


def bits(t):
    return t.detach().contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()]).cpu()


def counters():
    l = hip.lib()
    return (l.xnrs_qkv_launch_count(1), l.xnrs_fc1_in_tail_count(1), l.xnrs_mha_live_o_count(1))


class Family:
    """One entry point at one shape: ins {name: host tensor} and outs {name: (shape, dtype)} are its pointer operands, call(o)
    launches it on the device tensors o[name] -> return code, ref {out: fp64 reference}.  bars {out: (tol, elementwise) or a
    callable(got, ref) -> error / bar}; bitwise: outputs with the bits of the aligned run; exact: integer outputs."""

    def __init__(self, ins, outs, call, ref, bars=None, bitwise=(), knobs=None, stages=False, route=None, run_floor=None, refuse=()):
        self.ins, self.outs, self.call, self.ref = {k: v for k, v in ins.items() if v is not None}, outs, call, ref
        self.bars, self.bitwise, self.knobs, self.stages, self.route = bars or {}, set(bitwise), knobs or {}, stages, route
        # {out: floor of the scale of the comparison with the aligned run}: test_hip_train_step.py::_close holds a gradient to
        # RUN_TOL of max(its own maximum, 1e-3 of the step's largest gradient) -- one that is analytically zero is rounding noise
        self.run_floor = run_floor or {}
        # operands whose shift the entry point answers with XNRS_EUNSUPPORTED by contract, before any launch, nothing written
        self.refuse = set(refuse)


def run_case(fam, shifts):
    """The call with operand k at shifts[k] bytes off a 16-byte boundary (others on one) -> ({out: tensor}, evidence)."""
    o = {k: AR.shifted(v, shifts.get(k, 0), device=DEV) for k, v in fam.ins.items()}
    for k, (shape, dtype) in fam.outs.items():
        o[k] = AR.shifted_empty(shape, shifts.get(k, 0), dtype, DEV)
    for k, t in o.items():
        assert t.data_ptr() % 16 == shifts.get(k, 0) and t.is_contiguous(), k
    word = hip.status_word(DEV)
    hip.clear_status()
    with hip.knobs(**fam.knobs):
        counters()
        if fam.stages:
            hip.profile_enable(hip.PROFILE_ALL)
        try:
            rc = fam.call(o)
            torch.cuda.synchronize()
            st = {k: v[1] for k, v in hip.profile_read().items()} if fam.stages else {}
        finally:
            if fam.stages:
                hip.profile_enable(0)
        ev = dict(rc=rc, counters=counters(), stages=st)
    assert int(word.item()) == 0, "status word"
    if set(shifts) & fam.refuse:
        assert rc == EUNSUPPORTED, f"return code {rc}, expected XNRS_EUNSUPPORTED for {sorted(shifts)}"
        for k in fam.outs:
            assert AR.unwritten(o[k]) == o[k].numel() and AR.guards_intact(o[k]), f"a refused call wrote {k}"
        return None, ev
    assert rc == 0, f"return code {rc}: {hip.lib().xnrs_error_string(rc).decode()}"
    for k, t in o.items():
        assert AR.guards_intact(t), f"the guard elements around {k} were written"
    return {k: o[k] for k in fam.outs}, ev


def margin(got, ref, bar, what):
    """error / bar of one output against its fp64 reference; non-finite reference entries must be met in kind."""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(got[~fin & ~torch.isnan(ref)], ref[~fin & ~torch.isnan(ref)]), what
    got, ref = torch.where(fin, got, torch.zeros_like(got)), torch.where(fin, ref, torch.zeros_like(ref))
    if callable(bar):
        return bar(got, ref)
    tol, elementwise = bar
    e = H.assert_close(got, ref, tol, what, elementwise=elementwise)
    return max(e / tol, H.elementwise_excess(got, ref, tol) if elementwise else 0.0)


def check_case(fam, name, case, got, base):
    for k in fam.outs:
        what = f"{name}[{case}] {k}"
        if fam.outs[k][1] in (I32, torch.int64):
            assert torch.equal(got[k], base[k]), f"{what}: differs from the aligned run"
            if k in fam.ref:
                assert torch.equal(got[k].cpu(), fam.ref[k]), what
            continue
        m = margin(got[k], fam.ref[k], fam.bars.get(k, (H.RTOL, True)), what)
        assert m <= 1.0, f"{what}: {m:.3f} of the bar"
        fin = torch.isfinite(base[k])
        assert torch.equal(bits(got[k][~fin]), bits(base[k][~fin])), what
        g0, b0 = torch.where(fin, got[k], 0.0).double(), torch.where(fin, base[k], 0.0).double()
        d = (g0 - b0).abs().max().item() / max(b0.abs().max().item(), fam.run_floor.get(k, 0.0), 1e-30)
        same = torch.equal(bits(got[k]), bits(base[k]))
        print(f"MARGIN {what}: {m:.3f} of the fp64 bar; vs aligned {d / RUN_TOL:.3f} of RUN_TOL, same bits: {same}")
        assert d <= RUN_TOL, f"{what}: {d:.3e} from the aligned run"
        if k in fam.bitwise:
            assert same, f"{what}: the two routes differ in load / store width only, the bits must not"


# ------------------------------------------------------------------------------------------------ families: GEMMs
def per_tensor(tol):
    return (tol, False)


def table_bar(n_ids):
    """d_table: the bound of test_hip_grads.py::test_embedding_table_gradient_vs_index_add (test_hip_linear_ops._table_close)"""
    def bar(got, ref):
        scale = max(ref.abs().max().item(), 1e-6)
        return (got - ref).abs().max().item() / (5e-6 * scale * max(1.0, (n_ids / ref.shape[0]) ** 0.5))
    return bar


def linear_operands(seed, M, K, N, n_tab=None):
    g = gen(seed)
    x = torch.randn(n_tab or M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    ids = torch.randint(0, n_tab, (M,), generator=g).to(I32) if n_tab else None
    dy = torch.randn(M, N, generator=g)
    return x, w, b, ids, dy


def fam_linear_fwd(gather):
    M, K, N = 130, 16, 24  # two row tiles, the second ragged; K % 4 == 0: raw buffer loads (dense) / 16-byte pointer loads (ids)
    x, w, b, ids, _ = linear_operands(11, M, K, N, 40 if gather else None)
    rows = x.double()[ids.long()] if gather else x.double()
    ref = dict(y=torch.tanh(F.linear(rows, w.double(), b.double())))

    def call(o):
        return hip.lib().xnrs_linear_fwd(hip.ptr(o["x"]), hip.ptr(o.get("ids")), 1 if gather else 0, hip.ptr(o["w"]), hip.ptr(o["bias"]),
                                         hip.ptr(o["y"]), M, N, K, hip.ACT_TANH, stream())
    return Family(dict(x=x, w=w, bias=b, ids=ids), dict(y=((M, N), F32)), call, ref)


def fam_linear_bwd():
    """dx, dw, db of nn.Linear; db through the product's own launch: in place when db is 16-byte aligned, else through
    colsum_final (gemm_f32.hip:564)."""
    M, K, N = 130, 16, 24
    x, w, _, _, dy = linear_operands(12, M, K, N)
    ref = dict(dx=dy.double() @ w.double(), dw=dy.double().T @ x.double(), db=dy.double().sum(0))

    def call(o):
        l = hip.lib()
        nws = l.xnrs_linear_bwd_workspace_bytes(M, N, K)
        ws = hip.workspace(DEV, nws)
        return l.xnrs_linear_bwd(hip.ptr(o["x"]), None, 0, hip.ptr(o["w"]), hip.ptr(o["dy"]), hip.ptr(o["dx"]), hip.ptr(o["dw"]),
                                 hip.ptr(o["db"]), M, N, K, hip.ptr(ws), nws, stream())
    return Family(dict(x=x, w=w, dy=dy), dict(dx=((M, K), F32), dw=((N, K), F32), db=((N,), F32)), call, ref,
                  bars={k: per_tensor(GRAD_TOL) for k in ("dx", "dw", "db")})


def fam_embedding_linear_bwd(sparse):
    """fc(embedder(ids)) backward; sparse: d_table through xnrs_embedding_grad_sparse, whose zero fill has a vector and a
    memset leg (personalized.hip:434)."""
    M, K, N, n_tab = 130, 16, 24, 40
    x, w, _, ids, dy = linear_operands(13, M, K, N, n_tab)
    d_rows = dy.double() @ w.double()
    ref = dict(d_table=torch.zeros(n_tab, K, dtype=torch.float64).index_add_(0, ids.long(), d_rows),
               dw=dy.double().T @ x.double()[ids.long()], db=dy.double().sum(0))

    def call(o):
        l = hip.lib()
        nws = l.xnrs_embedding_linear_bwd_workspace_bytes(M, N, K)
        ws = hip.workspace(DEV, nws)
        fn = l.xnrs_embedding_linear_bwd_sparse if sparse else l.xnrs_embedding_linear_bwd
        return fn(hip.ptr(o["table"]), hip.ptr(o["ids"]), hip.ptr(o["w"]), hip.ptr(o["dy"]), hip.ptr(o["d_table"]), hip.ptr(o["dw"]),
                  hip.ptr(o["db"]), M, N, K, n_tab, hip.ptr(ws), nws, stream())
    return Family(dict(table=x, ids=ids, w=w, dy=dy), dict(d_table=((n_tab, K), F32), dw=((N, K), F32), db=((N,), F32)), call, ref,
                  bars=dict(d_table=table_bar(M), dw=per_tensor(GRAD_TOL), db=per_tensor(GRAD_TOL)))


# ------------------------------------------------------------------------------------------------ families: row gathers
def fam_gather(kind):
    """xnrs_gather_rows / _bf16 / xnrs_dropout_rows_bf16: 7 rows of 600 elements (600 % 8 == 0) out of 12, a row twice."""
    n, n_tab, W, p, seed = 7, 12, 600, 0.3, R.SEEDS[0]
    g = gen(14)
    tab = torch.randn(n_tab, W, generator=g)
    tab[tab == 0] = 1
    ids = torch.tensor([3, 0, 11, 3, 7, 5, 1], dtype=I32)
    if kind != "f32":
        tab = tab.to(BF16)
    rows = tab.float()[ids.long()]
    ref = dict(out=torch.from_numpy(R.dropped(rows.numpy(), p, seed)) if kind == "drop_bf16" else rows)

    def call(o):
        l = hip.lib()
        a = (hip.ptr(o["table"]), hip.ptr(o["ids"]), hip.ptr(o["out"]), n, W)
        if kind == "f32":
            return l.xnrs_gather_rows(*a, stream())
        if kind == "bf16":
            return l.xnrs_gather_rows_bf16(*a, stream())
        return l.xnrs_dropout_rows_bf16(*a, p, seed % 2 ** 64, None, stream())

    def exact(got, ref):  # a gathered element is a copy, a kept one ONE fp32 multiply: the reference's bits
        return 0.0 if torch.equal(got, ref) else float("inf")
    return Family(dict(table=tab, ids=ids), dict(out=((n, W), F32)), call, ref, bars=dict(out=exact), bitwise=("out",))


# ------------------------------------------------------------------------------------------------ families: encoders
ATT = ("wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo")
ATT_KEYS = dict(wq="q_linear.weight", bq="q_linear.bias", wk="k_linear.weight", bk="k_linear.bias", wv="v_linear.weight",
                bv="v_linear.bias", wo="out.weight", bo="out.bias")
POOL = ("w1", "b1", "w2", "b2")
POOL_KEYS = dict(w1="fc1.weight", b1="fc1.bias", w2="fc2.weight", b2="fc2.bias")
HEAD = ("h0w", "h0b", "h2w", "h2b")
HEAD_KEYS = dict(h0w="0.weight", h0b="0.bias", h2w="2.weight", h2b="2.bias")


def weights(g, D, A=0, E=0, att=True):
    w = {}
    if att:
        for k in ("wq", "wk", "wv", "wo"):
            w[k] = torch.randn(D, D, generator=g) / D ** 0.5
        for k in ("bq", "bk", "bv", "bo"):
            w[k] = 0.1 * torch.randn(D, generator=g)
    if A:
        w.update(w1=torch.randn(A, D, generator=g) / D ** 0.5, b1=0.1 * torch.randn(A, generator=g),
                 w2=torch.randn(1, A, generator=g) / A ** 0.5, b2=0.1 * torch.randn(1, generator=g))
    if E:
        w.update(h0w=torch.randn(E, D, generator=g) / D ** 0.5, h0b=0.1 * torch.randn(E, generator=g),
                 h2w=torch.randn(E, E, generator=g) / E ** 0.5, h2b=0.1 * torch.randn(E, generator=g))
    return w


def oracle_sd(w):
    sd = {}
    for keys, prefix in ((ATT_KEYS, "att."), (POOL_KEYS, "pooler."), (HEAD_KEYS, "head.")):
        sd.update({prefix + v: w[k].double() for k, v in keys.items() if k in w})
    return sd


def att_struct(o, h):
    return hip.MhaParams(*[o[k].data_ptr() for k in ATT], h, 1, 0.0, 0)


def pool_struct(o, A):
    return hip.AdditiveParams(*[o[k].data_ptr() for k in POOL], A, o["w1f"].data_ptr() if "w1f" in o else None,
                              o["b1f"].data_ptr() if "b1f" in o else None)


def head_struct(o, E):
    return hip.HeadParams(*[o[k].data_ptr() for k in HEAD], E, hip.ACT_RELU, o["w0f"].data_ptr() if "w0f" in o else None,
                          o["b0v"].data_ptr() if "b0v" in o else None)


def prefix_mask(g, n, S):
    """(n, S) 0/1 prefix masks: row 0 one token, row 1 all of them, row 2 none (an empty slot), the rest random lengths"""
    lens = torch.randint(1, S + 1, (n,), generator=g)
    lens[0], lens[1] = 1, S
    if n > 2:
        lens[2] = 0
    return (torch.arange(S)[None, :] < lens[:, None]).float()


def fam_mha():
    """xnrs_mha_fwd: Q|K|V projection (x, wq, wk, wv vector-loaded), attention over the workspace image, out-projection."""
    B, S, D, h = 3, 40, 32, 4
    g = gen(15)
    x, m, w = torch.randn(B, S, D, generator=g), prefix_mask(g, B, S), weights(g, D)
    ref = dict(y=O.multi_head_attention(x.double(), m.double().unsqueeze(-1), {v: w[k].double() for k, v in ATT_KEYS.items()}, h))

    def call(o):
        l = hip.lib()
        p = att_struct(o, h)
        nws = l.xnrs_mha_workspace_bytes(B, S, D)
        ws = hip.workspace(DEV, nws)
        return l.xnrs_mha_fwd(hip.ptr(o["x"]), hip.ptr(o["m"]), hip.ref(p), hip.ptr(o["y"]), B, S, D, hip.ptr(ws), nws, stream())
    return Family(dict(x=x, m=m, **w), dict(y=((B, S, D), F32)), call, ref)


def fam_additive():
    B, N, D, A = 5, 12, 32, 16
    g = gen(16)
    x, m, w = torch.randn(B, N, D, generator=g), prefix_mask(g, B, N), weights(g, D, A, att=False)
    y, a = O.additive_attention(x.double(), m.double().unsqueeze(-1), {v: w[k].double() for k, v in POOL_KEYS.items()}, True)
    ref = dict(y=y.reshape(B, D), a_out=a.reshape(B, N))

    def call(o):
        l = hip.lib()
        p = pool_struct(o, A)
        nws = l.xnrs_additive_workspace_bytes(B, N, D, A)
        ws = hip.workspace(DEV, nws)
        return l.xnrs_additive_attention_fwd(hip.ptr(o["x"]), hip.ptr(o["m"]), hip.ref(p), hip.ptr(o["y"]), hip.ptr(o["a_out"]), B, N, D,
                                             hip.ptr(ws), nws, stream())
    return Family(dict(x=x, m=m, **w), dict(y=((B, D), F32), a_out=((B, N), F32)), call, ref)


def fam_masked_mean():
    B, N, D = 5, 12, 32
    g = gen(17)
    x, m = torch.randn(B, N, D, generator=g), prefix_mask(g, B, N)
    ref = dict(y=O.masked_mean(x.double(), m.double().unsqueeze(-1)).reshape(B, D))

    def call(o):
        return hip.lib().xnrs_masked_mean_fwd(hip.ptr(o["x"]), hip.ptr(o["m"]), hip.ptr(o["y"]), B, N, D, stream())
    return Family(dict(x=x, m=m), dict(y=((B, D), F32)), call, ref)


def fam_user_encoder():
    B, Hn, E, h, A = 4, 12, 32, 4, 16
    g = gen(18)
    x, m, w = torch.randn(B, Hn, E, generator=g), prefix_mask(g, B, Hn), weights(g, E, A)
    y, a = O.user_encoder(x.double(), m.double().unsqueeze(-1), oracle_sd(w), h, return_weights=True)
    ref = dict(y=y.reshape(B, E), a_out=a.reshape(B, Hn))

    def call(o):
        l = hip.lib()
        ap, pp = att_struct(o, h), pool_struct(o, A)
        nws = l.xnrs_user_encoder_workspace_bytes(B, Hn, E, A, 1, hip.POOL_ADDITIVE, 0)
        ws = hip.workspace(DEV, nws)
        return l.xnrs_user_encoder_fwd(hip.ptr(o["x"]), hip.ptr(o["m"]), B, Hn, E, hip.ref(ap), hip.POOL_ADDITIVE, hip.ref(pp), None,
                                       hip.ptr(o["y"]), hip.ptr(o["a_out"]), hip.ptr(ws), nws, stream())
    return Family(dict(x=x, m=m, **w), dict(y=((B, E), F32), a_out=((B, Hn), F32)), call, ref)


NF_NAMED = {"x", "wq", "wk", "wv", "wo", "w1"}        # news_fused_ready
COMPACT_REFUSES = {"x", "wq", "wk", "wv", "w1"}  # fc1_rowdot_ok + the device-counted Q and K|V products
LIST_NAMED = {"x", "wq", "wk", "wv", "wo", "w1"}      # device_counts_ok, in front of the one-launch / in-tail / live-O routes


def text_encoder_family(seed, n, S, D, h, A, E, knobs, folded=False, chunk=0, stages=False, route=None, entry="padded", refuse=()):
    """xnrs_text_encoder_fwd with attention, additive pooler and (E > 0) head.  folded: the caller's folded pairs
    (xnrs_fold_weights / xnrs_fold_head_weights, computed once on aligned operands) ride along as operands w1f, b1f, w0f, b0v."""
    g = gen(seed)
    x, m, w = torch.randn(n, S, D, generator=g), prefix_mask(g, n, S), weights(g, D, A, E)
    y, hm = O.text_encoder(x.double().unsqueeze(0), m.double().reshape(1, n, S, 1), oracle_sd(w), h)
    Eo = E or D
    ref = dict(y=y.reshape(n, Eo), hm=hm.reshape(n))
    ins = dict(x=x, m=m, **w)
    if folded:
        l = hip.lib()
        d = {k: v.to(DEV) for k, v in w.items()}
        ap, pp = att_struct(d, h), pool_struct(d, A)
        w1f, b1f = torch.empty(A, D, device=DEV), torch.empty(A, device=DEV)
        nws = l.xnrs_fold_weights_workspace_bytes(D, A)
        hip.check(l.xnrs_fold_weights(hip.ref(ap), hip.ref(pp), D, hip.ptr(w1f), hip.ptr(b1f), hip.ptr(hip.workspace(DEV, nws)), nws, stream()), "fold")
        ins.update(w1f=w1f.cpu(), b1f=b1f.cpu())
        if E:
            hp = head_struct(d, E)
            w0f, b0v = torch.empty(E, D, device=DEV), torch.empty(E, device=DEV)
            nws = l.xnrs_fold_head_weights_workspace_bytes(D, E)
            hip.check(l.xnrs_fold_head_weights(hip.ref(ap), hip.ref(hp), D, hip.ptr(w0f), hip.ptr(b0v), hip.ptr(hip.workspace(DEV, nws)), nws,
                                               stream()), "fold head")
            ins.update(w0f=w0f.cpu(), b0v=b0v.cpu())

    if entry == "unpadded":  # the host-compacted lists: the unmasked token rows and their CSR over the news (0/1 masks)
        del ins["m"]
        ins["rows"] = torch.nonzero(m.reshape(-1)).squeeze(1).to(I32)
        row_off = torch.cat([torch.zeros(1, dtype=torch.int64), m.sum(1).long().cumsum(0)]).to(DEV)
    if entry == "bf16":  # the rows as a bf16 TABLE of n + 3 rows read through ids; the reference is the widened table's
        g2 = gen(seed + 1000)
        tab = torch.randn(n + 3, S, D, generator=g2).to(BF16)
        ids = torch.randperm(n + 3, generator=g2)[:n].to(I32)
        tm = torch.zeros(n + 3, S)
        tm[ids.long()] = m
        y, hm = O.text_encoder(tab.float().double()[ids.long()].unsqueeze(0), m.double().reshape(1, n, S, 1), oracle_sd(w), h)
        ref = dict(y=y.reshape(n, Eo), hm=hm.reshape(n))
        ins.update(x=tab, m=tm, ids=ids)

    def call(o):
        l = hip.lib()
        ap, pp, hp = att_struct(o, h), pool_struct(o, A), head_struct(o, E) if E else None
        if entry == "compact":
            nws = l.xnrs_text_encoder_compact_workspace_bytes(n, S, D, A, Eo, 1, int(bool(E)), chunk)
            return l.xnrs_text_encoder_fwd_compact(hip.ptr(o["x"]), hip.ptr(o["m"]), None, n, S, D, hip.ref(ap), hip.ref(pp), hip.ref(hp), hip.ptr(o["y"]),
                                                   hip.ptr(o["hm"]), chunk, hip.ptr(hip.workspace(DEV, nws)), nws, stream())
        if entry == "unpadded":
            nv = o["rows"].numel()
            nws = l.xnrs_text_encoder_unpadded_workspace_bytes(n, nv, S, D, A, Eo, 1, int(bool(E)))
            return l.xnrs_text_encoder_fwd_unpadded(hip.ptr(o["x"]), None, n, S, D, hip.ptr(o["rows"]), hip.ptr(row_off), nv, hip.ref(ap), hip.ref(pp),
                                                    hip.ref(hp), hip.ptr(o["y"]), hip.ptr(o["hm"]), hip.ptr(hip.workspace(DEV, nws)), nws, stream())
        if entry == "bf16":
            nws = l.xnrs_text_encoder_bf16_workspace_bytes(n, S, D, A, Eo, 1, hip.POOL_ADDITIVE, int(bool(E)), chunk)
            return l.xnrs_text_encoder_fwd_bf16(hip.ptr(o["x"]), hip.ptr(o["m"]), hip.ptr(o["ids"]), n, S, D, hip.ref(ap), hip.POOL_ADDITIVE, hip.ref(pp),
                                                hip.ref(hp), hip.ptr(o["y"]), hip.ptr(o["hm"]), chunk, hip.ptr(hip.workspace(DEV, nws)), nws, stream())
        nws = l.xnrs_text_encoder_workspace_bytes(n, S, D, A, Eo, 1, hip.POOL_ADDITIVE, int(bool(E)), chunk)
        ws = hip.workspace(DEV, nws)
        return l.xnrs_text_encoder_fwd(hip.ptr(o["x"]), hip.ptr(o["m"]), None, n, S, D, hip.ref(ap), hip.POOL_ADDITIVE, hip.ref(pp), hip.ref(hp),
                                       hip.ptr(o["y"]), hip.ptr(o["hm"]), chunk, hip.ptr(ws), nws, stream())
    return Family(ins, dict(y=((n, Eo), F32), hm=((n,), F32)), call, ref, knobs=knobs, stages=stages, route=route, refuse=refuse)


def fused_route(named):
    """The fused news kernel serves the aligned call; the GEMM pipeline a call with a named operand off 16 bytes."""
    def route(shifts, ev, base_ev):
        fused = ev["stages"]["news_fused"] > 0
        assert base_ev["stages"]["news_fused"] > 0 and base_ev["stages"]["qkv_gemm"] == 0
        assert fused == (not (set(shifts) & named)), (sorted(shifts), ev["stages"])
        assert fused or ev["stages"]["qkv_gemm"] > 0
    return route


def lists_route(shifts, ev, base_ev):
    """(Q|K|V launches of the live-row branch, fc1 products in a projection launch, attention launches that store live O rows)"""
    assert all(c > 0 for c in base_ev["counters"]), base_ev["counters"]
    if set(shifts) & LIST_NAMED:
        assert ev["counters"] == (0, 0, 0), (sorted(shifts), ev["counters"])
    else:
        assert ev["counters"] == base_ev["counters"], (sorted(shifts), ev["counters"], base_ev["counters"])


GRADS = tuple("d" + k for k in ATT + POOL + HEAD)


def fam_seq_encoder_train(live):
    """xnrs_seq_encoder_fwd_train + _bwd (live: the _live pair over the unmasked token rows, host count): attention, additive
    pooler and head; x, mask, every parameter and dy in, y / a_out / hm, dx and every parameter gradient out.  The saved blob
    and the backward workspace stay aligned.  Gradients at the bar of tests/test_hip_grads.py::check_param_grads (GTOL of
    max(the tensor's own maximum, 1e-3 of the step's largest gradient); fc2.bias with helpers.fc2_bias_extra_bar on top)."""
    n, L, D, h, A, E = 6, 40, 32, 4, 16, 16
    g = gen(41 + (2 if live == "rows" else int(live)))
    x, m, w = torch.randn(n, L, D, generator=g), prefix_mask(g, n, L), weights(g, D, A, E)
    dy = torch.randn(n, E, generator=g)
    rows = torch.nonzero(m.reshape(-1)).squeeze(1).to(I32)
    xd = x.double().requires_grad_(True)
    sd = {k: v.requires_grad_(True) for k, v in oracle_sd(w).items()}
    m64 = m.double().reshape(n, L, 1)
    y64 = O.multi_head_attention(xd, m64, O._sub(sd, "att"), h)
    p64, a64 = O.additive_attention(y64, m64, O._sub(sd, "pooler"), return_weights=True)
    o64 = O._mlp_head(p64, O._sub(sd, "head")).reshape(n, E)
    (o64 * dy.double()).sum().backward()
    ref = dict(y=o64.detach(), a_out=a64.detach().reshape(n, L), hm=m.double().sum(1).clamp(0, 1), dx=xd.grad)
    for keys, prefix in ((ATT_KEYS, "att."), (POOL_KEYS, "pooler."), (HEAD_KEYS, "head.")):
        ref.update({"d" + k: sd[prefix + v].grad for k, v in keys.items()})
    gmax = max(ref[k].abs().max().item() for k in GRADS)

    def grad_bar(k):
        def bar(got, r):
            scale = max(r.abs().max().item(), 1e-3 * gmax)
            extra = H.fc2_bias_extra_bar(n * L, ref["dw2"].abs().max().item(), scale, gmax) if k == "db2" else 0.0
            return (got - r).abs().max().item() / ((GRAD_TOL + extra) * scale)
        return bar
    ins = dict(x=x, m=m, dy=dy, **w)
    if live:
        ins["live"] = rows
    if live == "rows":  # xnrs_row_lists with HOST counts: the live rows and the token rows of the non-empty sequences
        ins["kv"] = torch.nonzero(m.sum(1, keepdim=True).expand(n, L).reshape(-1)).squeeze(1).to(I32)
    outs = dict(y=((n, E), F32), a_out=((n, L), F32), hm=((n,), F32), dx=((n, L, D), F32))
    outs.update({"d" + k: (tuple(w[k].shape), F32) for k in ATT + POOL + HEAD})

    def call(o):
        l = hip.lib()
        ap, pp, hp = att_struct(o, h), pool_struct(o, A), head_struct(o, E)
        ga = hip.MhaGrads(*[o["d" + k].data_ptr() for k in ATT])
        gp = hip.AdditiveGrads(*[o["d" + k].data_ptr() for k in POOL])
        gh = hip.HeadGrads(*[o["d" + k].data_ptr() for k in HEAD])
        nsv = l.xnrs_seq_encoder_saved_bytes(n, L, D, A, E, h, hip.POOL_ADDITIVE, 1)
        saved = torch.empty(nsv, dtype=torch.uint8, device=DEV)
        nws = l.xnrs_seq_encoder_bwd_workspace_bytes(n, L, D, A, E, h, hip.POOL_ADDITIVE, 1)
        ws = hip.workspace(DEV, nws)
        assert saved.data_ptr() % hip.WORKSPACE_ALIGN == 0
        head = (hip.ptr(o["x"]), hip.ptr(o["m"]), None, n, L, D, hip.ref(ap), hip.POOL_ADDITIVE, hip.ref(pp), hip.ref(hp))
        lists = (hip.ptr(o["live"]), None, rows.numel()) if live else ()
        fwd = l.xnrs_seq_encoder_fwd_train_live if live else l.xnrs_seq_encoder_fwd_train
        bwd = l.xnrs_seq_encoder_bwd_live if live else l.xnrs_seq_encoder_bwd
        if live == "rows":
            rl = hip.RowLists(o["live"].data_ptr(), None, rows.numel(), o["kv"].data_ptr(), None, o["kv"].numel(), None, None, None, hip.DQKV_OWN)
            lists, fwd, bwd = (hip.ref(rl),), l.xnrs_seq_encoder_fwd_train_rows, l.xnrs_seq_encoder_bwd_rows
        rc = fwd(*head, hip.ptr(o["y"]), hip.ptr(o["a_out"]), hip.ptr(o["hm"]), hip.ptr(saved), nsv, *lists, stream())
        return rc or bwd(*head, hip.ptr(saved), nsv, hip.ptr(o["dy"]), hip.ptr(o["dx"]), hip.ref(ga), hip.ref(gp), hip.ref(gh), *lists,
                         hip.ptr(ws), nws, stream())
    bars = {k: grad_bar(k) for k in GRADS + ("dx",)}
    return Family(ins, outs, call, ref, bars=bars, run_floor={k: 1e-3 * gmax for k in GRADS + ("dx",)})


# ------------------------------------------------------------------------------------------------ families: scores over the table
def table_operands(seed, B, N, E, exact):
    """exact: small-integer operands -- every score is exact in fp32 and in fp64, ties are real ties, so the returned rows and
    ranks can be held to tests/topk_ref.py / rank_ref.py to the last place (the inner-product forms)."""
    g = gen(seed)
    if exact:
        return torch.randint(-3, 4, (N, E), generator=g).float(), torch.randint(-3, 4, (B, E), generator=g).float(), g
    return torch.randn(N, E, generator=g), torch.randn(B, E, generator=g) * (2.0 / E ** 0.5), g


def table_scores(kind, table, u, g, E, ins):
    """fp64 scores (B, N) of the form `kind` ('dot', 'bilinear', 'mlp'); adds the form's weight operands to ins (the MLP form
    reads P = xnrs_mlp_scoring_news_proj(table), given here as the operand `table`)."""
    if kind == "bilinear":
        w, b = torch.randn(1, E, E, generator=g) / E ** 0.5, torch.randn(1, generator=g)
        ins.update(w=w, bias=b)
        return u.double() @ w[0].double() @ table.double().T + b.double()
    if kind == "mlp":
        Hh = table.shape[1]
        w1, b1 = torch.randn(Hh, 2 * E, generator=g) / (2 * E) ** 0.5, 0.1 * torch.randn(Hh, generator=g)
        w2, b2 = torch.randn(1, Hh, generator=g) / Hh ** 0.5, 0.1 * torch.randn(1, generator=g)
        ins.update(w1=w1, b1=b1, w2=w2, b2=b2)
        q = u.double() @ w1[:, :E].double().T + b1.double()
        return torch.tanh(q[:, None, :] + table.double()[None]) @ w2[0].double() + b2.double()
    return u.double() @ table.double().T


def form_args(kind, o, N, E, B):
    """the leading arguments of xnrs_topk* / xnrs_rank* of the form `kind`, and the workspace's projection width"""
    if kind == "bilinear":
        return (hip.ptr(o["table"]), N, E, hip.ptr(o["u"]), B, hip.ptr(o["w"]), hip.ptr(o["bias"])), E
    if kind == "mlp":
        Hh = o["table"].shape[1]
        return (hip.ptr(o["table"]), N, E, Hh, hip.ptr(o["u"]), B, hip.ptr(o["w1"]), hip.ptr(o["b1"]), hip.ptr(o["w2"]), hip.ptr(o["b2"])), Hh
    return (hip.ptr(o["table"]), N, E, hip.ptr(o["u"]), B), 0


def window_excl(lo, hi, N):
    """a window as the exclusion list it is defined by: every row outside [lo, hi)"""
    return [[r for r in range(N) if not int(a) <= r < int(b)] for a, b in zip(lo, hi)]


def fam_topk(entry, kind="dot", k=10):
    """xnrs_topk / xnrs_topk_deep / xnrs_topk_deep_win and the bilinear / MLP forms at (B, N, E) = (130, 300, 40): two user tiles,
    three row chunks, the last ragged, a feature tail behind one 32-block.  vec_t and vec_u are independent: the four
    combinations occur as aligned, table+4, u+4, all.  The inner-product forms run on exact small-integer operands: rows and
    scores against tests/topk_ref.py; the other forms: the fp64 score of every returned row, and the rows of the aligned run."""
    from tests.topk_ref import topk_reference
    B, N, E = 130, 300, 40
    table, u, g = table_operands(19, B, N, 24 if kind == "mlp" else E, kind == "dot")
    if kind == "mlp":  # (table: P:(N, H = 24); u:(B, E))
        u = torch.randn(B, E, generator=g)
    ins = dict(table=table, u=u)
    s64 = table_scores(kind, table, u, g, E, ins)
    excl = None
    if entry == "deep_win":
        lo = torch.randint(0, N // 2, (B,), generator=g).to(I32)
        hi = (lo + torch.randint(0, N, (B,), generator=g)).to(I32)
        ins.update(win_lo=lo, win_hi=hi)
        excl = window_excl(lo, hi, N)
    ref = {}
    if kind == "dot":
        r, sc = topk_reference(s64.numpy(), k, excl)
        ref = dict(rows=torch.from_numpy(r), scores=torch.from_numpy(sc))
    out = {}

    def call(o):
        l = hip.lib()
        head, width = form_args(kind, o, N, E, B)
        tail = (-1, k, hip.ptr(o["rows"]), hip.ptr(o["scores"]))
        fn = {"plain": "xnrs_topk", "deep": "xnrs_topk_deep", "deep_win": "xnrs_topk_deep"}[entry] + {"dot": "", "bilinear": "_bilinear", "mlp": "_mlp"}[kind]
        nws = (l.xnrs_topk_workspace_bytes if entry == "plain" else l.xnrs_topk_deep_workspace_bytes)(B, N, width, k)
        ws = hip.workspace(DEV, nws)
        if entry == "deep_win":
            rc = getattr(l, fn + "_win")(*head, None, None, hip.ptr(o["win_lo"]), hip.ptr(o["win_hi"]), *tail, hip.ptr(ws), nws, stream())
        else:
            rc = getattr(l, fn)(*head, None, None, *tail, hip.ptr(ws), nws, stream())
        out["rows"] = o["rows"]
        return rc

    def at_rows(got, _):  # the fp64 score of every returned row (a user with a narrow window: row -1 / -inf in the tail)
        rows = out["rows"].cpu().long()
        want = torch.where(rows >= 0, s64.gather(1, rows.clamp(min=0)), torch.full_like(s64[:, :k], -float("inf")))
        fin = torch.isfinite(want)
        assert torch.equal(torch.isfinite(got), fin)
        got, want = torch.where(fin, got, 0.0), torch.where(fin, want, 0.0)
        H.assert_close(got, want, H.RTOL, f"top-k {kind} scores")
        return max(H.rel_err(got, want) / H.RTOL, H.elementwise_excess(got, want, H.RTOL))
    if kind != "dot":
        ref = dict(scores=torch.zeros(B, k, dtype=torch.float64))
    return Family(ins, dict(rows=((B, k), I32), scores=((B, k), F32)), call, ref, bars=dict(scores=at_rows) if kind != "dot" else {},
                  bitwise=("scores",))


def fam_rank(win, kind="dot"):
    """xnrs_rank / xnrs_rank_win and the bilinear / MLP forms; the inner-product forms on exact operands: ranks and scores
    against tests/rank_ref.py (a window: the exclusion list it is defined by)."""
    from tests.rank_ref import rank_reference
    B, N, E, T = 130, 300, 40, 2
    table, u, g = table_operands(20, B, N, 24 if kind == "mlp" else E, kind == "dot")
    if kind == "mlp":
        u = torch.randn(B, E, generator=g)
    tgt_rows = torch.randint(0, N, (B * T,), generator=g).to(I32)
    tgt_off = (torch.arange(B + 1) * T).to(torch.int64)
    ins = dict(table=table, u=u, tgt_rows=tgt_rows)
    s64 = table_scores(kind, table, u, g, E, ins)
    excl = None
    if win:
        lo = torch.randint(0, N // 2, (B,), generator=g).to(I32)
        ins.update(win_lo=lo, win_hi=(lo + torch.randint(0, N, (B,), generator=g)).to(I32))
        excl = window_excl(ins["win_lo"], ins["win_hi"], N)
    ref = dict(scores=s64.gather(1, tgt_rows.long().reshape(B, T)).reshape(-1))
    if kind == "dot":
        rk, sc = rank_reference(s64.numpy(), tgt_rows.reshape(B, T).tolist(), excl)
        ref = dict(ranks=torch.from_numpy(rk), scores=torch.from_numpy(sc))
    def call(o):
        l = hip.lib()
        off_d = tgt_off.to(DEV)
        head, width = form_args(kind, o, N, E, B)
        nws = l.xnrs_rank_workspace_bytes(B, width)
        ws = hip.workspace(DEV, nws)
        fn = "xnrs_rank" + {"dot": "", "bilinear": "_bilinear", "mlp": "_mlp"}[kind] + ("_win" if win else "")
        a = head + (hip.ptr(off_d), hip.ptr(o["tgt_rows"]), None, None)
        b = (-1, hip.ptr(o["ranks"]), hip.ptr(o["scores"]), hip.ptr(ws), nws, stream())
        return getattr(l, fn)(*a, hip.ptr(o["win_lo"]), hip.ptr(o["win_hi"]), *b) if win else getattr(l, fn)(*a, *b)
    return Family(ins, dict(ranks=((B * T,), I32), scores=((B * T,), F32)), call, ref, bitwise=("scores",))


def fam_table_loss(B, N, E, config):
    """xnrs_table_loss_fwd + _bwd on a problem of tests/test_hip_table_loss.py (its fp64 reference, computed once there):
    table, up and the upstream g in; scores, loss, lse, d_up, d_table out (the backward reads the forward's shifted outputs)."""
    from tests import test_hip_table_loss as TL
    from xnrs_amd import ops
    c = TL.case(B, N, E, config)
    T = c["tgt"][1].numel()
    r = c["ref"]
    ref = dict(scores=r["scores"], loss=r["loss"], lse=r["lse"], d_up=r["d_up"], d_table=r["d_table"])

    def call(o):
        l = hip.lib()
        _, _, _, _, (head, keep) = ops._table_loss_args(o["table"], o["up"], *c["tgt"], *c["excl_csr"], *c["win"], None)
        nws = l.xnrs_table_loss_workspace_bytes(B, N, E, 1)
        ws = hip.workspace(DEV, nws)
        o["loss"].zero_()  # (the entry point writes the positions of the CSR; ops.table_loss_forward starts from zeros / NaN)
        o["scores"].fill_(float("nan"))
        rc = l.xnrs_table_loss_fwd(*head, c["pad_row"], hip.ptr(o["scores"]), hip.ptr(o["loss"]), hip.ptr(o["lse"]), hip.ptr(ws), nws, stream())
        if rc:
            return rc
        return l.xnrs_table_loss_bwd(*head, c["pad_row"], hip.ptr(o["scores"]), hip.ptr(o["lse"]), hip.ptr(o["g"]), hip.ptr(o["d_up"]),
                                     hip.ptr(o["d_table"]), hip.ptr(ws), nws, stream())
    return Family(dict(table=c["table"].cpu(), up=c["up"].cpu(), g=c["g"].cpu()),
                  dict(scores=((T,), F32), loss=((T,), F32), lse=((B,), F32), d_up=((B, E), F32), d_table=((N, E), F32)), call, ref,
                  bitwise=("scores", "loss", "lse"))


# ------------------------------------------------------------------------------------------------ families without vector accesses
def fam_dot_scoring():
    """xnrs_dot_scoring_fwd, _bwd and _norm_bwd in one call (pool_score.hip, pool_bwd.hip: no 8 / 16-byte access)."""
    B, Cn, E = 5, 7, 32
    g = gen(21)
    u, c, dr = torch.randn(B, E, generator=g), torch.randn(B, Cn, E, generator=g), torch.randn(B, Cn, generator=g)
    ref = {}
    for norm in (False, True):
        ud, cd = u.double().requires_grad_(True), c.double().requires_grad_(True)
        un, cn = (ud / ud.norm(dim=1, keepdim=True), cd / cd.norm(dim=2, keepdim=True)) if norm else (ud, cd)
        r = torch.einsum("be,bce->bc", un, cn)
        r.backward(dr.double())
        s = "n" if norm else ""
        ref.update({"r" + s: r.detach(), "du" + s: ud.grad, "dc" + s: cd.grad})

    def call(o):
        l = hip.lib()
        a = (hip.ptr(o["u"]), hip.ptr(o["c"]))
        rcs = [l.xnrs_dot_scoring_fwd(*a, hip.ptr(o["r"]), B, Cn, E, 0, stream()), l.xnrs_dot_scoring_fwd(*a, hip.ptr(o["rn"]), B, Cn, E, 1, stream()),
               l.xnrs_dot_scoring_bwd(*a, hip.ptr(o["dr"]), hip.ptr(o["du"]), hip.ptr(o["dc"]), B, Cn, E, stream()),
               l.xnrs_dot_scoring_norm_bwd(*a, hip.ptr(o["dr"]), hip.ptr(o["dun"]), hip.ptr(o["dcn"]), B, Cn, E, stream())]
        return next((rc for rc in rcs if rc), 0)
    outs = dict(r=((B, Cn), F32), rn=((B, Cn), F32), du=((B, E), F32), dc=((B, Cn, E), F32), dun=((B, E), F32), dcn=((B, Cn, E), F32))
    return Family(dict(u=u, c=c, dr=dr), outs, call, ref, bars={k: (GRAD_TOL, True) for k in ("du", "dc", "dun", "dcn")})


def fam_score_csr():
    n_vec, E, B, n_cand = 40, 32, 6, 50
    g = gen(22)
    vecs, u = torch.randn(n_vec, E, generator=g), torch.randn(B, E, generator=g)
    rows, sess = torch.randint(0, n_vec, (n_cand,), generator=g).to(I32), torch.randint(0, B, (n_cand,), generator=g).to(I32)
    ref = dict(r=torch.relu((vecs.double()[rows.long()] * u.double()[sess.long()]).sum(1)))

    def call(o):
        return hip.lib().xnrs_score_csr(hip.ptr(o["vecs"]), hip.ptr(o["rows"]), hip.ptr(o["sess"]), hip.ptr(o["u"]), hip.ptr(o["r"]), n_cand, E, 1,
                                        stream())
    return Family(dict(vecs=vecs, rows=rows, sess=sess, u=u), dict(r=((n_cand,), F32)), call, ref)


def fam_infonce():
    B, E, temp = 9, 32, 0.08
    g = gen(23)
    emb, gout = torch.randn(B, E, generator=g), torch.tensor([0.7])
    labels = torch.tensor([0, 1, 0, 2, 1, 0, 2, 2, 3])
    ed = emb.double().requires_grad_(True)
    loss = O.contrastive_loss(ed, labels, temp)
    (loss * gout.double()).sum().backward()
    ref = dict(loss=loss.detach().reshape(1), demb=ed.grad)
    lab_d = labels.to(DEV)

    def call(o):
        l = hip.lib()
        nsv = l.xnrs_infonce_saved_bytes(B, E)
        saved = torch.empty(max(nsv, 1), dtype=torch.uint8, device=DEV)
        rc = l.xnrs_infonce_fwd(hip.ptr(o["emb"]), hip.ptr(lab_d), B, E, temp, hip.ptr(o["loss"]), hip.ptr(saved), nsv, stream())
        return rc or l.xnrs_infonce_bwd(hip.ptr(lab_d), B, E, temp, hip.ptr(saved), nsv, hip.ptr(o["gout"]), hip.ptr(o["demb"]), stream())
    return Family(dict(emb=emb, gout=gout), dict(loss=((1,), F32), demb=((B, E), F32)), call, ref, bars=dict(demb=(GRAD_TOL, True)))


def fam_attn_long():
    from tests.test_hip_caum import _ref_attention
    L, Nb, heads, dk = 154, 3, 2, 8  # past the short kernel's 128 keys: five key tiles, the last ragged
    E = heads * dk
    qkv = torch.randn(L, Nb, 3 * E, generator=gen(24))
    ref = dict(o=_ref_attention(qkv.double(), heads))

    def call(o):
        return hip.lib().xnrs_attn_long_fwd(hip.ptr(o["qkv"]), Nb * 3 * E, 3 * E, hip.ptr(o["o"]), Nb * E, E, L, Nb, E, heads, stream())
    return Family(dict(qkv=qkv), dict(o=((L, Nb, E), F32)), call, ref)



# ------------------------------------------------------------------------------------------------ families: more GEMM routes
def fam_linear_split():
    """xnrs_linear_fwd in mode 1 (bf16x3) with the split kernel forced onto the small shape (XNRS_GEMM_SPLIT_MIN_TILES=0, the
    knob of tests/test_hip_split_gemm.py): launch_gemm_f32 sends only a `vec` launch there, so a shifted x or w takes the fp32
    scalar kernel instead."""
    fam = fam_linear_fwd(False)
    inner = fam.call

    def call(o):
        prev = hip.set_gemm_mode(1)
        try:
            return inner(o)
        finally:
            hip.set_gemm_mode(prev)
    fam.call, fam.knobs = call, dict(XNRS_GEMM_SPLIT_MIN_TILES="0")
    return fam


def fam_linear_bf16():
    """xnrs_linear_fwd_bf16: bf16 rows on the bf16 matrix cores (gemm_a16_ok: K % 8 == 0, 16-byte aligned rows; forced onto the
    small shape by the same knob), else widened 1024 rows at a time and through xnrs_linear_fwd's route."""
    M, K, N = 130, 16, 24
    x, w, b, _, _ = linear_operands(25, M, K, N)
    x = x.to(BF16)
    ref = dict(y=torch.tanh(F.linear(x.float().double(), w.double(), b.double())))

    def call(o):
        l = hip.lib()
        nws = l.xnrs_linear_bf16_workspace_bytes(N, K)
        return l.xnrs_linear_fwd_bf16(hip.ptr(o["x"]), None, 0, hip.ptr(o["w"]), hip.ptr(o["bias"]), hip.ptr(o["y"]), M, N, K, hip.ACT_TANH,
                                      hip.ptr(hip.workspace(DEV, nws)), nws, stream())
    return Family(dict(x=x, w=w, bias=b), dict(y=((M, N), F32)), call, ref, knobs=dict(XNRS_GEMM_SPLIT_MIN_TILES="0"))


def fam_linear_bwd_dw():
    """dW through the register-transposing kernel of gemm_dw.hip: gemm_dw_eligible wants a contraction of >= 8192 rows (a
    constant, no knob lowers it) and 64 x 64 outputs, XNRS_GEMM_DW=3 sends a dense launch there.  A shifted dy or x (its A /
    W operands) falls back to the k-major kernel of launch_gemm_f32; db rides on the split-K reduction."""
    M, K, N = 8200, 64, 64
    x, w, _, _, dy = linear_operands(26, M, K, N)
    ref = dict(dx=dy.double() @ w.double(), dw=dy.double().T @ x.double(), db=dy.double().sum(0))

    def call(o):
        l = hip.lib()
        nws = l.xnrs_linear_bwd_workspace_bytes(M, N, K)
        return l.xnrs_linear_bwd(hip.ptr(o["x"]), None, 0, hip.ptr(o["w"]), hip.ptr(o["dy"]), hip.ptr(o["dx"]), hip.ptr(o["dw"]), hip.ptr(o["db"]),
                                 M, N, K, hip.ptr(hip.workspace(DEV, nws)), nws, stream())
    return Family(dict(x=x, w=w, dy=dy), dict(dx=((M, K), F32), dw=((N, K), F32), db=((N,), F32)), call, ref,
                  bars={k: per_tensor(GRAD_TOL) for k in ("dx", "dw", "db")}, knobs=dict(XNRS_GEMM_DW="3"))


# ------------------------------------------------------------------------------------------------ families: scorers
def scorer_operands(seed, B, N, E, Hh):
    g = gen(seed)
    return dict(u=torch.randn(B, E, generator=g), c=torch.randn(B, N, E, generator=g), ds=torch.randn(B, N, generator=g),
                w=torch.randn(1, E, E, generator=g) / E ** 0.5, bias=torch.randn(1, generator=g),
                w1=torch.randn(Hh, 2 * E, generator=g) / (2 * E) ** 0.5, b1=0.1 * torch.randn(Hh, generator=g),
                w2=torch.randn(1, Hh, generator=g) / Hh ** 0.5, b2=0.1 * torch.randn(1, generator=g))


def fam_bilinear_scoring():
    """xnrs_bilinear_scoring_fwd + _bwd (scorers.hip: no 8 / 16-byte access; the u W[0] product is a GEMM)."""
    B, N, E = 5, 7, 32
    t = scorer_operands(27, B, N, E, 8)
    d = {k: t[k].double().requires_grad_(True) for k in ("u", "c", "w", "bias")}
    s64 = torch.einsum("bi,ij,bnj->bn", d["u"], d["w"][0], d["c"]) + d["bias"]
    s64.backward(t["ds"].double())
    ref = dict(s=s64.detach(), du=d["u"].grad, dc=d["c"].grad, dw=d["w"].grad, dbias=d["bias"].grad)

    def call(o):
        l = hip.lib()
        nsv, nws = l.xnrs_bilinear_scoring_saved_bytes(B, E, 0), l.xnrs_bilinear_scoring_bwd_workspace_bytes(B, E, 0)
        saved = torch.empty(max(nsv, 1), dtype=torch.uint8, device=DEV)
        rc = l.xnrs_bilinear_scoring_fwd(hip.ptr(o["u"]), hip.ptr(o["c"]), hip.ptr(o["w"]), hip.ptr(o["bias"]), hip.ptr(o["s"]), B, N, E, 0,
                                         hip.ptr(saved), nsv, stream())
        return rc or l.xnrs_bilinear_scoring_bwd(hip.ptr(o["u"]), hip.ptr(o["c"]), hip.ptr(o["w"]), hip.ptr(saved), nsv, hip.ptr(o["ds"]), hip.ptr(o["du"]),
                                                 hip.ptr(o["dc"]), hip.ptr(o["dw"]), hip.ptr(o["dbias"]), B, N, E, 0, hip.ptr(hip.workspace(DEV, max(nws, 1))),
                                                 nws, stream())
    outs = dict(s=((B, N), F32), du=((B, E), F32), dc=((B, N, E), F32), dw=((1, E, E), F32), dbias=((1,), F32))
    return Family({k: t[k] for k in ("u", "c", "w", "bias", "ds")}, outs, call, ref, bars={k: (GRAD_TOL, True) for k in ("du", "dc", "dw", "dbias")})


def fam_mlp_scoring():
    B, N, E, Hh = 5, 7, 32, 24
    t = scorer_operands(28, B, N, E, Hh)
    d = {k: t[k].double().requires_grad_(True) for k in ("u", "c", "w1", "b1", "w2", "b2")}
    q = d["u"] @ d["w1"][:, :E].T + d["b1"]
    pr = d["c"] @ d["w1"][:, E:].T
    s64 = torch.tanh(q[:, None, :] + pr) @ d["w2"][0] + d["b2"]
    s64.backward(t["ds"].double())
    ref = dict(s=s64.detach(), du=d["u"].grad, dc=d["c"].grad, dw1=d["w1"].grad, db1=d["b1"].grad, dw2=d["w2"].grad, db2=d["b2"].grad)

    def call(o):
        l = hip.lib()
        nsv, nws = l.xnrs_mlp_scoring_saved_bytes(B, N, Hh), l.xnrs_mlp_scoring_bwd_workspace_bytes(B, N, Hh)
        saved = torch.empty(max(nsv, 1), dtype=torch.uint8, device=DEV)
        rc = l.xnrs_mlp_scoring_fwd(hip.ptr(o["u"]), hip.ptr(o["c"]), hip.ptr(o["w1"]), hip.ptr(o["b1"]), hip.ptr(o["w2"]), hip.ptr(o["b2"]), hip.ptr(o["s"]),
                                    B, N, E, Hh, hip.ptr(saved), nsv, stream())
        return rc or l.xnrs_mlp_scoring_bwd(hip.ptr(o["u"]), hip.ptr(o["c"]), hip.ptr(o["w1"]), hip.ptr(o["w2"]), hip.ptr(saved), nsv, hip.ptr(o["ds"]),
                                            hip.ptr(o["du"]), hip.ptr(o["dc"]), hip.ptr(o["dw1"]), hip.ptr(o["db1"]), hip.ptr(o["dw2"]), hip.ptr(o["db2"]),
                                            B, N, E, Hh, hip.ptr(hip.workspace(DEV, max(nws, 1))), nws, stream())
    outs = dict(s=((B, N), F32), du=((B, E), F32), dc=((B, N, E), F32), dw1=((Hh, 2 * E), F32), db1=((Hh,), F32), dw2=((1, Hh), F32), db2=((1,), F32))
    return Family({k: t[k] for k in ("u", "c", "w1", "b1", "w2", "b2", "ds")}, outs, call, ref,
                  bars={k: (GRAD_TOL, True) for k in ("du", "dc", "dw1", "db1", "dw2", "db2")})


def fam_score_csr_scorer(kind):
    """xnrs_score_csr_bilinear / _mlp: vecs (MLP: P = vecs . W1c^T, given) gathered by row, the user side projected by one GEMM"""
    n_vec, E, B, n_cand, Hh = 40, 32, 6, 50, 24
    t = scorer_operands(29, B, 1, E, Hh)
    g = gen(30)
    vecs = torch.randn(n_vec, E, generator=g)
    rows, sess = torch.randint(0, n_vec, (n_cand,), generator=g).to(I32), torch.randint(0, B, (n_cand,), generator=g).to(I32)
    u64 = t["u"].double()[sess.long()]
    if kind == "bilinear":
        ins = dict(vecs=vecs, rows=rows, sess=sess, u=t["u"], w=t["w"], bias=t["bias"])
        ref = dict(r=torch.relu(((u64 @ t["w"][0].double()) * vecs.double()[rows.long()]).sum(1) + t["bias"].double()))
    else:
        P = (vecs @ t["w1"][:, E:].T).contiguous()
        ins = dict(P=P, rows=rows, sess=sess, u=t["u"], w1=t["w1"], b1=t["b1"], w2=t["w2"], b2=t["b2"])
        q = u64 @ t["w1"][:, :E].double().T + t["b1"].double()
        ref = dict(r=torch.relu(torch.tanh(q + P.double()[rows.long()]) @ t["w2"][0].double() + t["b2"].double()))

    def call(o):
        l = hip.lib()
        nws = l.xnrs_score_csr_scorer_workspace_bytes(B, E if kind == "bilinear" else Hh)
        ws = hip.workspace(DEV, nws)
        if kind == "bilinear":
            return l.xnrs_score_csr_bilinear(hip.ptr(o["vecs"]), hip.ptr(o["rows"]), hip.ptr(o["sess"]), hip.ptr(o["u"]), B, hip.ptr(o["w"]), hip.ptr(o["bias"]),
                                             hip.ptr(o["r"]), n_cand, E, 1, hip.ptr(ws), nws, stream())
        return l.xnrs_score_csr_mlp(hip.ptr(o["P"]), hip.ptr(o["rows"]), hip.ptr(o["sess"]), hip.ptr(o["u"]), B, hip.ptr(o["w1"]), hip.ptr(o["b1"]),
                                    hip.ptr(o["w2"]), hip.ptr(o["b2"]), hip.ptr(o["r"]), n_cand, E, Hh, 1, hip.ptr(ws), nws, stream())
    return Family(ins, dict(r=((n_cand,), F32)), call, ref)


# ------------------------------------------------------------------------------------------------ families: NPA, LSTUR, CAUM kernels
def fam_personalized():
    """xnrs_personalized_fwd (y_inf), _fwd_train and _bwd with a head: x, mask, x_fc, the query rows, q_idx, the head, dy in;
    y, a_out, hm, dx, dwx, dbx, dq and the head's gradients out (personalized.hip: its GEMMs are launch_gemm_f32's)."""
    from tests.test_hip_npa import _ref_pa
    n_q, per, L, D, A, E = 3, 4, 8, 24, 40, 12
    n = n_q * per
    g = gen(31)
    x, m = torch.randn(n, L, D, generator=g), prefix_mask(g, n, L)
    w = dict(wx=torch.randn(A, D, generator=g) / D ** 0.5, bx=0.1 * torch.randn(A, generator=g), q=0.3 * torch.randn(n_q, A, generator=g))
    w.update({k: v for k, v in weights(g, D, 0, E, att=False).items()})
    q_idx = torch.div(torch.arange(n), per, rounding_mode="floor").to(I32)
    dy = torch.randn(n, E, generator=g)
    d = {k: v.double().requires_grad_(True) for k, v in dict(x=x, **w).items()}
    y64 = _ref_pa(d["x"], m.double(), d["q"], q_idx, d["wx"], d["bx"], [d[k] for k in HEAD])
    y64.backward(dy.double())
    t64 = torch.tanh(x.double() @ w["wx"].double().T + w["bx"].double())
    e64 = torch.exp((t64 * w["q"].double()[q_idx.long()][:, None, :]).sum(-1)) * m.double()
    ref = dict(y=y64.detach(), y_inf=y64.detach(), a_out=e64 / (e64.sum(1, keepdim=True) + 1e-8), hm=m.double().sum(1).clamp(0, 1), dx=d["x"].grad,
               dwx=d["wx"].grad, dbx=d["bx"].grad, dq=d["q"].grad, **{"d" + k: d[k].grad for k in HEAD})
    PP = hip.STRUCTS["xnrs_personalized_params"]

    def call(o):
        l = hip.lib()
        pp, hp = PP(o["wx"].data_ptr(), o["bx"].data_ptr(), o["q"].data_ptr(), o["q_idx"].data_ptr(), A, 0, n_q), head_struct(o, E)
        gh = hip.HeadGrads(*[o["d" + k].data_ptr() for k in HEAD])
        nsv, nws = l.xnrs_personalized_saved_bytes(n, L, D, A, E, 1), l.xnrs_personalized_bwd_workspace_bytes(n, L, D, A, E, 1)
        saved = torch.empty(max(nsv, 1), dtype=torch.uint8, device=DEV)
        head = (hip.ptr(o["x"]), hip.ptr(o["m"]), None, n, L, D, hip.ref(pp), hip.ref(hp))
        rc = l.xnrs_personalized_fwd(*head, hip.ptr(o["y_inf"]), None, None, hip.ptr(hip.workspace(DEV, nsv)), nsv, stream())
        rc = rc or l.xnrs_personalized_fwd_train(*head, hip.ptr(o["y"]), hip.ptr(o["a_out"]), hip.ptr(o["hm"]), hip.ptr(saved), nsv, stream())
        return rc or l.xnrs_personalized_bwd(hip.ptr(o["x"]), None, n, L, D, hip.ref(pp), hip.ref(hp), hip.ptr(saved), nsv, hip.ptr(o["dy"]), hip.ptr(o["dx"]),
                                             hip.ptr(o["dwx"]), hip.ptr(o["dbx"]), hip.ptr(o["dq"]), n_q, hip.ref(gh), hip.ptr(hip.workspace(DEV, nws)), nws,
                                             stream())
    outs = dict(y=((n, E), F32), y_inf=((n, E), F32), a_out=((n, L), F32), hm=((n,), F32), dx=((n, L, D), F32), dwx=((A, D), F32), dbx=((A,), F32),
                dq=((n_q, A), F32))
    outs.update({"d" + k: (tuple(w[k].shape), F32) for k in HEAD})
    grads = ("dx", "dwx", "dbx", "dq") + tuple("d" + k for k in HEAD)
    return Family(dict(x=x, m=m, q_idx=q_idx, dy=dy, **w), outs, call, ref, bars={k: (GRAD_TOL, True) for k in grads})


def fam_gru():
    """xnrs_gru_fwd (y_inf), _fwd_train and _bwd: x, mask, h0, the four parameters and dy in; y, dx, dh0 and the parameter
    gradients out.  gru.hip:327 names w_hh and h0 (load_k4); Hd = 40: two column tiles, a multiple of 4."""
    from tests.test_hip_lstur import _ref_gru
    B, T, N, E, Hd = 9, 5, 6, 16, 40
    g = gen(32)
    x = torch.randn(B, T, E, generator=g)
    m = (torch.rand(B, N, generator=g) > 0.4).float()
    m[0, :T], m[B - 1, :T] = 0, 1
    lens = m[:, :T].sum(1).long()
    w = dict(h0=0.5 * torch.randn(B, Hd, generator=g), w_ih=torch.randn(3 * Hd, E, generator=g) / E ** 0.5,
             w_hh=torch.randn(3 * Hd, Hd, generator=g) / Hd ** 0.5, b_ih=0.1 * torch.randn(3 * Hd, generator=g), b_hh=0.1 * torch.randn(3 * Hd, generator=g))
    dy = torch.randn(B, Hd, generator=g)
    d = {k: v.double().requires_grad_(True) for k, v in dict(x=x, **w).items()}
    y64 = _ref_gru(d["x"], lens, d["h0"], d["w_ih"], d["w_hh"], d["b_ih"], d["b_hh"])
    y64.backward(dy.double())
    ref = dict(y=y64.detach(), y_inf=y64.detach(), dx=d["x"].grad, **{"d" + k: d[k].grad for k in w})
    GP, GG = hip.STRUCTS["xnrs_gru_params"], hip.STRUCTS["xnrs_gru_grads"]

    def call(o):
        l = hip.lib()
        gp = GP(o["w_ih"].data_ptr(), o["w_hh"].data_ptr(), o["b_ih"].data_ptr(), o["b_hh"].data_ptr(), Hd)
        gg = GG(o["dw_ih"].data_ptr(), o["dw_hh"].data_ptr(), o["db_ih"].data_ptr(), o["db_hh"].data_ptr())
        nw, nsv, nws = l.xnrs_gru_workspace_bytes(B, T, E, Hd), l.xnrs_gru_saved_bytes(B, T, E, Hd), l.xnrs_gru_bwd_workspace_bytes(B, T, E, Hd)
        saved = torch.empty(max(nsv, 1), dtype=torch.uint8, device=DEV)
        rc = l.xnrs_gru_fwd(hip.ptr(o["x"]), hip.ptr(o["m"]), N, hip.ptr(o["h0"]), hip.ref(gp), hip.ptr(o["y_inf"]), B, T, E, hip.ptr(hip.workspace(DEV, nw)), nw,
                            stream())
        rc = rc or l.xnrs_gru_fwd_train(hip.ptr(o["x"]), hip.ptr(o["m"]), N, hip.ptr(o["h0"]), hip.ref(gp), hip.ptr(o["y"]), B, T, E, hip.ptr(saved), nsv, stream())
        return rc or l.xnrs_gru_bwd(hip.ptr(o["x"]), hip.ref(gp), hip.ptr(saved), nsv, hip.ptr(o["dy"]), hip.ptr(o["dx"]), hip.ptr(o["dh0"]), hip.ref(gg), B, T, E,
                                    hip.ptr(hip.workspace(DEV, nws)), nws, stream())
    outs = dict(y=((B, Hd), F32), y_inf=((B, Hd), F32), dx=((B, T, E), F32), **{"d" + k: (tuple(v.shape), F32) for k, v in w.items()})
    return Family(dict(x=x, m=m, dy=dy, **w), outs, call, ref, bars={k: (GRAD_TOL, True) for k in ("dx",) + tuple("d" + k for k in w)},
                  )


def fam_attn_long_bwd():
    from tests.test_hip_caum import _ref_attention
    L, Nb, heads, dk = 154, 3, 2, 8
    E = heads * dk
    g = gen(33)
    qkv, d_o = torch.randn(L, Nb, 3 * E, generator=g), torch.randn(L, Nb, E, generator=g)
    qd = qkv.double().requires_grad_(True)
    o64 = _ref_attention(qd, heads)
    o64.backward(d_o.double())

    def call(o):
        l = hip.lib()
        nsv, nws = l.xnrs_attn_long_saved_bytes(L, Nb, E, heads), l.xnrs_attn_long_workspace_bytes(L, Nb, E, heads)
        saved = torch.empty(max(nsv, 1), dtype=torch.uint8, device=DEV)
        rc = l.xnrs_attn_long_fwd_train(hip.ptr(o["qkv"]), Nb * 3 * E, 3 * E, hip.ptr(o["o"]), Nb * E, E, L, Nb, E, heads, hip.ptr(saved), nsv, stream())
        return rc or l.xnrs_attn_long_bwd(hip.ptr(o["qkv"]), Nb * 3 * E, 3 * E, hip.ptr(o["o"]), hip.ptr(o["d_o"]), Nb * E, E, hip.ptr(saved), nsv, hip.ptr(o["dqkv"]),
                                          L, Nb, E, heads, hip.ptr(hip.workspace(DEV, max(nws, 1))), nws, stream())
    return Family(dict(qkv=qkv, d_o=d_o), dict(o=((L, Nb, E), F32), dqkv=((L, Nb, 3 * E), F32)), call, dict(o=o64.detach(), dqkv=qd.grad),
                  bars=dict(dqkv=(GRAD_TOL, True)))


def fam_caum():
    """xnrs_caum_pair_fwd / _bwd, xnrs_caum_bias_tanh_fwd / _bwd and xnrs_caum_pool_fwd / _bwd in one call, each against fp64
    autograd of the formula the header states (caum.hip: no 8 / 16-byte access)."""
    B, Cn, Hn, E, A = 3, 2, 5, 16, 12
    P = B * Cn
    g = gen(34)
    t = dict(hp=torch.randn(B * Hn, 4 * E, generator=g), cp=torch.randn(P, 2 * E, generator=g), d_hcnn=torch.randn(P * Hn, E, generator=g),
             d_z=torch.randn(P * Hn, E, generator=g), pre=torch.randn(P * Hn, E, generator=g), cb=torch.randn(P, E, generator=g),
             dt=torch.randn(P * Hn, E, generator=g), t2=torch.randn(P * Hn, A, generator=g), w3=torch.randn(A, generator=g) / A ** 0.5,
             b3=torch.randn(1, generator=g), h_all=torch.randn(P * Hn, E, generator=g), du=torch.randn(P, E, generator=g))
    d = {k: v.double().requires_grad_(True) for k, v in t.items()}
    hp4 = d["hp"].reshape(B, Hn, 4, E)
    cpr = d["cp"].reshape(B, Cn, 1, 2, E)
    hc = (torch.roll(hp4[:, :, 0], 1, 1) + hp4[:, :, 1] + torch.roll(hp4[:, :, 2], -1, 1))[:, None] + cpr[:, :, :, 0]
    z = hp4[:, None, :, 3] + cpr[:, :, :, 1]
    ((hc.reshape(P * Hn, E) * d["d_hcnn"].detach()).sum() + (z.reshape(P * Hn, E) * d["d_z"].detach()).sum()).backward()
    tt = torch.tanh(d["pre"].reshape(P, Hn, E) + d["cb"][:, None, :]).reshape(P * Hn, E)
    (tt * d["dt"].detach()).sum().backward()
    sc = (d["t2"] @ d["w3"] + d["b3"]).reshape(P, Hn)
    a = torch.softmax(sc, dim=1)
    uu = (a[..., None] * d["h_all"].reshape(P, Hn, E)).sum(1)
    (uu * d["du"].detach()).sum().backward()
    gw = max(d["w3"].grad.abs().max().item(), 1e-30)
    ref = dict(h_cnn=hc.detach().reshape(P * Hn, E), z=z.detach().reshape(P * Hn, E), d_hp=d["hp"].grad, d_cp=d["cp"].grad, t=tt.detach(),
               dpre=d["pre"].grad, dcb=d["cb"].grad, u=uu.detach(), a_out=a.detach(), d_t2=d["t2"].grad, d_w3=d["w3"].grad, d_b3=d["b3"].grad,
               d_hall=d["h_all"].grad)

    def call(o):
        l = hip.lib()
        nws = l.xnrs_caum_pool_bwd_workspace_bytes(P, Hn, A)
        rcs = [l.xnrs_caum_pair_fwd(hip.ptr(o["hp"]), hip.ptr(o["cp"]), 2 * E, hip.ptr(o["h_cnn"]), hip.ptr(o["z"]), B, Cn, Hn, E, stream()),
               l.xnrs_caum_pair_bwd(hip.ptr(o["d_hcnn"]), hip.ptr(o["d_z"]), hip.ptr(o["d_hp"]), hip.ptr(o["d_cp"]), 2 * E, B, Cn, Hn, E, stream()),
               l.xnrs_caum_bias_tanh_fwd(hip.ptr(o["pre"]), hip.ptr(o["cb"]), E, hip.ptr(o["t"]), P, Hn, E, stream()),
               l.xnrs_caum_bias_tanh_bwd(hip.ptr(o["t"]), hip.ptr(o["dt"]), hip.ptr(o["dpre"]), hip.ptr(o["dcb"]), P, Hn, E, stream()),
               l.xnrs_caum_pool_fwd(hip.ptr(o["t2"]), hip.ptr(o["w3"]), hip.ptr(o["b3"]), hip.ptr(o["h_all"]), hip.ptr(o["u"]), hip.ptr(o["a_out"]), P, Hn, A, E,
                                    stream()),
               l.xnrs_caum_pool_bwd(hip.ptr(o["t2"]), hip.ptr(o["w3"]), hip.ptr(o["h_all"]), hip.ptr(o["a_out"]), hip.ptr(o["du"]), hip.ptr(o["d_t2"]),
                                    hip.ptr(o["d_w3"]), hip.ptr(o["d_b3"]), hip.ptr(o["d_hall"]), P, Hn, A, E, hip.ptr(hip.workspace(DEV, max(nws, 1))), nws,
                                    stream())]
        return next((rc for rc in rcs if rc), 0)

    def b3_bar(got, r):  # analytically zero (a bias in front of a softmax): rounding noise on the scale of d_w3, as the header says
        return (got - r).abs().max().item() / (GRAD_TOL * gw)
    outs = {k: (tuple(v.shape), F32) for k, v in ref.items()}
    bars = {k: (GRAD_TOL, True) for k in ("d_hp", "d_cp", "dpre", "dcb", "d_t2", "d_w3", "d_hall")}
    bars["d_b3"] = b3_bar
    return Family(t, outs, call, ref, bars=bars, run_floor=dict(d_b3=gw))


# ------------------------------------------------------------------------------------------------ the matrix
#: family -> (builder, the (input, output) pair that also takes the 8- and 12-byte shifts; None: "all shifted" only)
FAMILIES = {
    "linear_fwd": (lambda: fam_linear_fwd(False), ("x", "y")),
    "linear_fwd_ids": (lambda: fam_linear_fwd(True), ("w", "y")),
    "linear_bwd": (fam_linear_bwd, ("dy", "db")),
    "embedding_linear_bwd": (lambda: fam_embedding_linear_bwd(False), ("table", "dw")),
    "embedding_linear_bwd_sparse": (lambda: fam_embedding_linear_bwd(True), ("dy", "d_table")),
    "gather_rows": (lambda: fam_gather("f32"), ("table", "out")),
    "gather_rows_bf16": (lambda: fam_gather("bf16"), ("table", "out")),
    "dropout_rows_bf16": (lambda: fam_gather("drop_bf16"), ("table", "out")),
    "mha_fwd": (fam_mha, ("x", "y")),
    "additive_attention_fwd": (fam_additive, ("w1", "a_out")),
    "masked_mean_fwd": (fam_masked_mean, ("x", "y")),
    "user_encoder_fwd": (fam_user_encoder, ("wo", "y")),
    # one fused launch (S <= 32; XNRS_NEWS_FUSED=2: whenever eligible)
    "text_encoder_fused": (lambda: text_encoder_family(31, 11, 30, 64, 4, 256, 32, dict(XNRS_NEWS_FUSED="2"), stages=True,
                                                       route=fused_route(NF_NAMED)), ("x", "y")),
    # ... given the caller's folded fc1 pair: the kernel's fc1 image is built from w1f
    "text_encoder_fused_folded": (lambda: text_encoder_family(32, 11, 30, 64, 4, 256, 32, dict(XNRS_NEWS_FUSED="2"), folded=True, stages=True,
                                                              route=fused_route(NF_NAMED | {"w1f"})), ("w1f", "y")),
    # ... without a head and with the per-token out-projection: the kernel stores the pooled vectors straight into y
    "text_encoder_fused_y": (lambda: text_encoder_family(33, 11, 30, 64, 4, 256, 0, dict(XNRS_NEWS_FUSED="2", XNRS_FOLD_OUT="0"), stages=True,
                                                         route=fused_route(NF_NAMED | {"y"})), ("wq", "y")),
    # the GEMM pipeline (fc2 dots in the fc1 epilogue) with every folded pointer given
    "text_encoder_gemm_folded": (lambda: text_encoder_family(34, 11, 30, 64, 4, 32, 32, dict(XNRS_NEWS_FUSED="0"), folded=True), ("w1f", "y")),
    # two passes over the live-row lists: Q|K|V in one launch, fc1 in the tail, live O rows (33 <= S <= 64, thresholds at 0)
    "text_encoder_lists": (lambda: text_encoder_family(35, 24, 40, 64, 4, 32, 32, dict(LISTS, XNRS_NEWS_FUSED="0"), chunk=12,
                                                       route=lists_route), ("x", "y")),
    "seq_encoder_train": (lambda: fam_seq_encoder_train(False), ("dy", "dx")),
    "seq_encoder_train_live": (lambda: fam_seq_encoder_train(True), ("x", "dwq")),
    "seq_encoder_train_rows": (lambda: fam_seq_encoder_train("rows"), ("w1", "dw1")),
    # the padding-free entry points: host-compacted lists; device-compacted (refuses what its device-counted products cannot
    # load: XNRS_EUNSUPPORTED, nothing written); a bf16 table (direct route forced onto the small shape / widening route)
    "text_encoder_unpadded": (lambda: text_encoder_family(36, 24, 40, 64, 4, 32, 32, dict(XNRS_NEWS_FUSED="0"), entry="unpadded"), ("x", "y")),
    "text_encoder_compact": (lambda: text_encoder_family(35, 24, 40, 64, 4, 32, 32, dict(XNRS_NEWS_FUSED="0"), chunk=12, entry="compact",
                                                         refuse=COMPACT_REFUSES), ("wo", "y")),
    "text_encoder_bf16": (lambda: text_encoder_family(37, 24, 40, 64, 4, 32, 32, dict(XNRS_NEWS_FUSED="0", XNRS_GEMM_SPLIT_MIN_TILES="0"),
                                                      entry="bf16"), ("x", "y")),
    "linear_fwd_split": (fam_linear_split, ("x", "y")),
    "linear_fwd_bf16": (fam_linear_bf16, ("x", "y")),
    "linear_bwd_dw": (fam_linear_bwd_dw, ("dy", "dw")),
    "bilinear_scoring": (fam_bilinear_scoring, ("w", "du")),
    "mlp_scoring": (fam_mlp_scoring, ("w1", "dc")),
    "score_csr_bilinear": (lambda: fam_score_csr_scorer("bilinear"), ("vecs", "r")),
    "score_csr_mlp": (lambda: fam_score_csr_scorer("mlp"), ("P", "r")),
    "personalized": (fam_personalized, ("q", "dq")),
    "gru": (fam_gru, ("h0", "dh0")),
    "topk": (lambda: fam_topk("plain"), ("table", "scores")),
    "topk_deep": (lambda: fam_topk("deep", k=200), ("u", "scores")),
    "topk_deep_win": (lambda: fam_topk("deep_win"), ("u", "rows")),
    "topk_bilinear": (lambda: fam_topk("plain", "bilinear"), ("table", "scores")),
    "topk_mlp": (lambda: fam_topk("plain", "mlp"), ("table", "scores")),
    "rank": (lambda: fam_rank(False), ("table", "scores")),
    "rank_win": (lambda: fam_rank(True), ("u", "ranks")),
    "rank_bilinear": (lambda: fam_rank(False, "bilinear"), ("u", "scores")),
    "rank_mlp_win": (lambda: fam_rank(True, "mlp"), ("table", "ranks")),
    "table_loss_130_300_40": (lambda: fam_table_loss(130, 300, 40, "messy"), ("table", "d_up")),
    "table_loss_129_1153_272": (lambda: fam_table_loss(129, 1153, 272, "plain"), ("up", "d_table")),  # two feature passes in the backward
    "dot_scoring": (fam_dot_scoring, None),
    "score_csr": (fam_score_csr, None),
    "infonce": (fam_infonce, None),
    "attn_long_fwd": (fam_attn_long, None),
    "attn_long_bwd": (fam_attn_long_bwd, None),
    "caum": (fam_caum, None),
}
#: family -> its pointer operands, in call order (checked against the builder; written out so that collection builds nothing)
OPERANDS = {
    "linear_fwd": "x w bias y", "linear_fwd_ids": "x ids w bias y", "linear_bwd": "x w dy dx dw db",
    "embedding_linear_bwd": "table ids w dy d_table dw db", "embedding_linear_bwd_sparse": "table ids w dy d_table dw db",
    "gather_rows": "table ids out", "gather_rows_bf16": "table ids out", "dropout_rows_bf16": "table ids out",
    "mha_fwd": "x m " + " ".join(ATT) + " y", "additive_attention_fwd": "x m " + " ".join(POOL) + " y a_out", "masked_mean_fwd": "x m y",
    "user_encoder_fwd": "x m " + " ".join(ATT + POOL) + " y a_out",
    "text_encoder_fused": "x m " + " ".join(ATT + POOL + HEAD) + " y hm",
    "text_encoder_fused_folded": "x m " + " ".join(ATT + POOL + HEAD) + " w1f b1f w0f b0v y hm",
    "text_encoder_fused_y": "x m " + " ".join(ATT + POOL) + " y hm",
    "text_encoder_gemm_folded": "x m " + " ".join(ATT + POOL + HEAD) + " w1f b1f w0f b0v y hm",
    "text_encoder_lists": "x m " + " ".join(ATT + POOL + HEAD) + " y hm",
    "seq_encoder_train": "x m dy " + " ".join(ATT + POOL + HEAD) + " y a_out hm dx " + " ".join(GRADS),
    "seq_encoder_train_live": "x m dy live " + " ".join(ATT + POOL + HEAD) + " y a_out hm dx " + " ".join(GRADS),
    "seq_encoder_train_rows": "x m dy live kv " + " ".join(ATT + POOL + HEAD) + " y a_out hm dx " + " ".join(GRADS),
    "text_encoder_unpadded": "x rows " + " ".join(ATT + POOL + HEAD) + " y hm",
    "text_encoder_compact": "x m " + " ".join(ATT + POOL + HEAD) + " y hm",
    "text_encoder_bf16": "x m ids " + " ".join(ATT + POOL + HEAD) + " y hm",
    "linear_fwd_split": "x w bias y", "linear_fwd_bf16": "x w bias y", "linear_bwd_dw": "x w dy dx dw db",
    "bilinear_scoring": "u c w bias ds s du dc dw dbias", "mlp_scoring": "u c w1 b1 w2 b2 ds s du dc dw1 db1 dw2 db2",
    "score_csr_bilinear": "vecs rows sess u w bias r", "score_csr_mlp": "P rows sess u w1 b1 w2 b2 r",
    "personalized": "x m q_idx dy wx bx q " + " ".join(HEAD) + " y y_inf a_out hm dx dwx dbx dq " + " ".join("d" + k for k in HEAD),
    "gru": "x m dy h0 w_ih w_hh b_ih b_hh y y_inf dx dh0 dw_ih dw_hh db_ih db_hh",
    "topk": "table u rows scores", "topk_deep": "table u rows scores", "topk_deep_win": "table u win_lo win_hi rows scores",
    "topk_bilinear": "table u w bias rows scores", "topk_mlp": "table u w1 b1 w2 b2 rows scores",
    "rank": "table u tgt_rows ranks scores", "rank_win": "table u tgt_rows win_lo win_hi ranks scores",
    "rank_bilinear": "table u w bias tgt_rows ranks scores", "rank_mlp_win": "table u w1 b1 w2 b2 tgt_rows win_lo win_hi ranks scores",
    "table_loss_130_300_40": "table up g scores loss lse d_up d_table", "table_loss_129_1153_272": "table up g scores loss lse d_up d_table",
    "dot_scoring": "u c dr r rn du dc dun dcn", "score_csr": "vecs rows sess u r", "infonce": "emb gout loss demb", "attn_long_fwd": "qkv o",
    "attn_long_bwd": "qkv d_o o dqkv",
    "caum": "hp cp d_hcnn d_z pre cb dt t2 w3 b3 h_all du h_cnn z d_hp d_cp t dpre dcb u a_out d_t2 d_w3 d_b3 d_hall",
}
BF16_OPERANDS = {("gather_rows_bf16", "table"), ("dropout_rows_bf16", "table"), ("linear_fwd_bf16", "x"), ("text_encoder_bf16", "x")}


def case_shifts(name, case):
    ops_ = OPERANDS[name].split()
    step = lambda k, i: ((2, 4, 8) if (name, k) in BF16_OPERANDS else (4, 8, 12))[i]  # noqa: E731
    if case == "aligned":
        return {}
    if case == "all":
        return {k: step(k, 0) for k in ops_}
    k, nbytes = case.split("+")
    assert k in ops_ and int(nbytes) in ((2, 4, 8) if (name, k) in BF16_OPERANDS else (4, 8, 12))
    return {k: int(nbytes)}


def all_cases():
    out = []
    for name, (_, pair) in FAMILIES.items():
        cases_ = ["aligned"]
        if pair is not None:
            for k in OPERANDS[name].split():
                cases_.append(f"{k}+{2 if (name, k) in BF16_OPERANDS else 4}")
        cases_.append("all")
        for k in pair or ():
            cases_ += [f"{k}+{s}" for s in ((4, 8) if (name, k) in BF16_OPERANDS else (8, 12))]
        out += [(name, c) for c in cases_]
    return out


@functools.lru_cache(maxsize=None)
def family(name):
    fam = FAMILIES[name][0]()
    assert sorted(OPERANDS[name].split()) == sorted(list(fam.ins) + list(fam.outs)), name
    return fam


@functools.lru_cache(maxsize=None)
def aligned(name):
    """(a): every operand on a 16-byte boundary -- run once per family, what every other case is compared with"""
    return run_case(family(name), {})


@pytest.mark.parametrize("name,case", all_cases(), ids=lambda v: v)
def test_operand_off_a_16_byte_boundary(name, case):
    fam = family(name)
    base, base_ev = aligned(name)
    shifts = case_shifts(name, case)
    got, ev = run_case(fam, shifts) if shifts else (base, base_ev)
    if got is None:  # (refused by contract: run_case has checked the code and that nothing was written)
        return
    check_case(fam, name, case, got, base)
    if fam.route is not None:
        fam.route(shifts, ev, base_ev)


def test_the_matrix_covers_every_operand_of_every_family():
    """(b) each pointer operand on its own, (c) all at once, (d) 8 and 12 bytes (bf16: 4 and 8) for one input and one output"""
    have = all_cases()
    for name, (_, pair) in FAMILIES.items():
        cs = {c for n, c in have if n == name}
        assert {"aligned", "all"} <= cs
        if pair is None:
            continue
        for k in OPERANDS[name].split():
            assert any(c.startswith(k + "+") for c in cs), (name, k)
        assert pair[0] in OPERANDS[name].split() and pair[1] in OPERANDS[name].split()
        assert sum(c.startswith(pair[0] + "+") for c in cs) == 3 and sum(c.startswith(pair[1] + "+") for c in cs) == 3


# ------------------------------------------------------------------------------------------------ through Python
def _f64(t):
    return t.double() if t.is_floating_point() else t


def _f64_batch(b):
    if isinstance(b, dict):
        return {k: _f64_batch(v) for k, v in b.items()}
    if isinstance(b, (tuple, list)):
        return tuple(_f64_batch(v) for v in b)
    return _f64(b.cpu()) if isinstance(b, torch.Tensor) else b


NRMS = dict(model="NRMS", B=8, H=12, C=3, S=50, D=64, h=4, E=32, bias=False, seed=4501, min_len=3)


@pytest.mark.parametrize("nbytes", [4, 12])
def test_nrms_grad_step_with_flat_misaligned_parameters(nbytes, monkeypatch):
    """A tiny NRMS (S = 50, D = 64, 4 heads) whose parameters are views at +4 (+12) bytes into ONE flat buffer -- what a
    flattened-parameter wrapper gives behind dummy_param:(1,) -- does forward, loss (MSE + InfoNCE) and backward: loss,
    scores and every parameter gradient within RUN_TOL of the same model with ordinary parameters, and at the bars of
    tests/test_hip_grads.py against the fp64 oracle.  The Python mirror of device_counts_ok says no for it and yes for the
    aligned model (STATS["device_list_forwards"]), and the library never contradicts it (a yes the library refuses raises)."""
    from tests.golden import cases
    from tests.test_hip_grads import check_param_grads
    from tests.test_hip_train_step import _close, _nrms, _step
    from xnrs_amd import autograd as AG
    monkeypatch.setattr(AG, "LIVE_ROWS_MIN", 1)
    plain, flat_model = _nrms(NRMS, 0.0), _nrms(NRMS, 0.0)
    sd = {k: v.detach().cpu() for k, v in plain.state_dict().items()}
    flat = AR.misalign_parameters(flat_model, nbytes)
    assert all(p.data_ptr() % 16 == nbytes for p in flat_model.parameters()) and all(p.data_ptr() % 16 == 0 for p in plain.parameters())
    batch = synth.batch_to(cases.model_batch(NRMS), DEV)
    labels = torch.tensor([0, 1, 0, 2, 1, 0, 2, 2], device=DEV)
    n0 = AG.STATS["device_list_forwards"]
    l0, g0 = _step(plain, batch, labels)
    with torch.no_grad():
        r0 = plain(batch)
    n1 = AG.STATS["device_list_forwards"]
    l1, g1 = _step(flat_model, batch, labels)
    with torch.no_grad():
        r1 = flat_model(batch)
    n2 = AG.STATS["device_list_forwards"]
    hip.check_status()
    assert n1 - n0 >= 2 and n2 == n1, "device-built row lists: for the aligned model only"
    assert AR.flat_guards_intact(flat)
    assert abs(l1.item() - l0.item()) <= RUN_TOL * abs(l0.item()) and H.rel_err(r1, r0) <= RUN_TOL
    _close(g1, g0, RUN_TOL)
    # the fp64 oracle of the step (tests/test_hip_grads.py: loss 1e-5, scores RTOL, gradients GTOL)
    osd = {k: v.double().requires_grad_(not k.endswith("dummy_param")) for k, v in sd.items()}
    b64 = _f64_batch(cases.model_batch(NRMS))
    lo, _, _ = O.train_step_loss(b64, osd, NRMS["h"], labels.cpu(), 0.08, 0.1)
    lo.backward()
    ro = O.parent_forward(b64["user_features"]["history"]["title_emb"], b64["candidate_features"]["title_emb"], osd, NRMS["h"])
    H.assert_close(l1.reshape(1), lo.detach().reshape(1), 1e-5, "loss")
    e = H.assert_close(r1, ro.detach(), H.RTOL, "scores")
    assert check_param_grads(flat_model, osd) >= 20
    print(f"MARGIN nrms flat +{nbytes}: scores {e / H.RTOL:.3f}; loss vs aligned {abs(l1.item() - l0.item()) / abs(l0.item()) / RUN_TOL:.3f} of RUN_TOL")


def test_inference_encode_with_flat_misaligned_parameters_with_and_without_folded_weights(monkeypatch):
    """The news encoder of that model in inference: padded and padding-free (TextEncoder.unpadded: the device-compacted entry
    point for the aligned model, the host-compacted one for the flat model -- it used to raise), with hip.py's cached folded
    pairs (keyed by data_ptr) and with XNRS_FOLD_CACHE off.  Against the aligned model at RUN_TOL and the fp64 oracle."""
    from tests.golden import cases
    from tests.test_hip_train_step import _nrms
    plain, flat_model = _nrms(NRMS, 0.0).eval(), _nrms(NRMS, 0.0).eval()
    sd = {k[len("news_encoder."):]: v.detach().cpu().double() for k, v in plain.state_dict().items() if k.startswith("news_encoder.")}
    flat = AR.misalign_parameters(flat_model, 4)
    hx, hm = cases.model_batch(NRMS)["user_features"]["history"]["title_emb"]
    yo, hmo = O.text_encoder(hx.double(), hm.double(), sd, NRMS["h"])
    x, m = hx.to(DEV), hm.to(DEV)
    for unpadded in (False, True):
        for cache in (True, False):
            monkeypatch.setattr(hip, "FOLD_CACHE", cache)
            hip.invalidate_fold_cache()
            outs = []
            for model in (plain, flat_model):
                enc = model.news_encoder
                enc.unpadded = unpadded
                with torch.no_grad():
                    outs.append(enc((x, m)))
                    outs.append(enc((x, m)))  # (the second call: the cached pair)
            hip.check_status()
            (y0, h0), (y0b, _), (y1, h1), (y1b, _) = outs
            assert torch.equal(y0, y0b) and torch.equal(y1, y1b) and torch.equal(h0, h1) and torch.equal(h1.cpu().double(), hmo)
            e = H.assert_close(y1, yo, H.RTOL, f"news vectors unpadded={unpadded} cache={cache}")
            d = H.rel_err(y1, y0)
            print(f"MARGIN flat encode unpadded={unpadded} cache={cache}: {e / H.RTOL:.3f} of the fp64 bar, vs aligned {d / RUN_TOL:.3f} of RUN_TOL")
            assert d <= RUN_TOL
    assert AR.flat_guards_intact(flat)


def _flat(model):
    model._align_flat = AR.misalign_parameters(model, 4)
    assert all(p.data_ptr() % 16 == 4 for p in model.parameters())
    return model


@pytest.mark.parametrize("which", ["lstur", "lstur_bilin", "lstur_fc", "npa_dot", "npa_bilin", "npa_fc", "caum"])
def test_other_models_grad_step_with_flat_misaligned_parameters(which, monkeypatch):
    """LSTUR (GRU w_hh / h0, the bilinear and MLP scorers), NPA (the personalized query table, its sparse table gradient)
    and CAUM (long attention, the candidate-aware kernels) with every parameter at +4 bytes in one flat buffer: the grad step
    of the family's own test against the reference's golden vectors at that file's bars, and against the same model with
    ordinary parameters at RUN_TOL."""
    import torch.nn.functional as F_
    if which.startswith("lstur"):
        from tests import test_hip_lstur as T
        from tests.golden import lstur_cases as Cs
        name = {"lstur": "tiny/embedding_ini", "lstur_bilin": "tiny/bilin", "lstur_fc": "tiny/fc"}[which]
        assert name in Cs.CASES
        args, make = (name,), lambda: T._model(Cs.CASES[name]).train()  # noqa: E731
    elif which.startswith("npa"):
        from tests import test_hip_npa as T
        from tests.golden import npa_cases as Cs
        scoring = which.split("_")[1]
        args, make = ("tiny", scoring), lambda: T._model(Cs.CASES["tiny"], scoring).train()  # noqa: E731
    else:
        from tests import test_hip_caum as T
        from tests.golden import caum_cases as Cs
        args, make = ("tiny",), lambda: Cs.fix_dropouts(T._model(Cs.CASES["tiny"]), Cs.CASES["tiny"])  # noqa: E731
    c = Cs.CASES[args[0]]

    def step(model):
        batch = synth.batch_to(Cs.batch(c), DEV)
        model.zero_grad(set_to_none=True)
        preds = torch.relu(model(batch))
        loss = F_.mse_loss(preds, batch["targets"])
        loss.backward()
        return loss.detach(), preds.detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    l0, p0, g0 = step(make())
    flat_model = _flat(make())
    l1, p1, g1 = step(flat_model)
    hip.check_status()
    assert AR.flat_guards_intact(flat_model._align_flat)
    assert abs(l1.item() - l0.item()) <= RUN_TOL * abs(l0.item()) and H.rel_err(p1, p0) <= RUN_TOL
    from tests.test_hip_train_step import _close
    _close(g1, g0, RUN_TOL)
    # the family's own golden test on the flat model
    real = T._model
    monkeypatch.setattr(T, "_model", lambda *a: _flat(real(*a)))
    T.test_grad_step_equals_the_reference(*args)


# ------------------------------------------------------------------------------------------------ a news table inside a larger buffer
def test_news_table_viewed_at_4_bytes_inside_a_larger_buffer():
    """ops.topk_dot / topk_deep_dot / rank_dot / table_loss (with backward) on a table that is a view at +4 bytes into a larger
    buffer, `up` shifted too: ids and ranks equal, scores, loss and lse bit-equal to the aligned table's, the gradients (aligned
    tensors of their own) within RUN_TOL and at the fp64 bar."""
    from tests import test_hip_table_loss as TL
    from xnrs_amd import ops
    c = TL.case(130, 300, 40, "messy")
    big = torch.full((4 * 300 * 40,), float("nan"), device=DEV)
    off = 300 * 40 + ((4 - (big.data_ptr() + 300 * 40 * 4)) % 16) // 4
    tab = big[off:off + 300 * 40].view(300, 40)
    tab.copy_(c["table"])
    up = AR.shifted(c["up"], 4)
    assert tab.data_ptr() % 16 == 4 and up.data_ptr() % 16 == 4 and hip.dev_f32(tab, "t").data_ptr() == tab.data_ptr()
    for fn, k in ((ops.topk_dot, 10), (ops.topk_deep_dot, 200)):
        r0, s0 = fn(c["table"], c["up"], k, *c["excl_csr"], c["pad_row"])
        r1, s1 = fn(tab, up, k, *c["excl_csr"], c["pad_row"])
        assert torch.equal(r0, r1) and torch.equal(bits(s0), bits(s1))
    q0 = ops.rank_dot(c["table"], c["up"], *c["tgt"], *c["excl_csr"], c["pad_row"], win_lo=c["win"][0], win_hi=c["win"][1])
    q1 = ops.rank_dot(tab, up, *c["tgt"], *c["excl_csr"], c["pad_row"], win_lo=c["win"][0], win_hi=c["win"][1])
    assert torch.equal(q0[0], q1[0]) and torch.equal(bits(q0[1]), bits(q1[1]))
    res = []
    for t, u in ((c["table"].clone(), c["up"].clone()), (tab, up)):
        t, u = t.requires_grad_(True), u.requires_grad_(True)
        loss, scores, lse = ops.table_loss(t, u, *c["tgt"], *c["excl_csr"], c["pad_row"], *c["win"])
        (loss * c["g"]).sum().backward()
        res.append((loss.detach(), scores.detach(), lse.detach(), u.grad, t.grad))
    assert res[1][4].data_ptr() % 16 == 0  # (table.grad is a tensor of its own)
    for a, b in zip(res[0][:3], res[1][:3]):
        assert torch.equal(bits(a), bits(b))
    for i, k in ((3, "d_up"), (4, "d_table")):
        assert H.rel_err(res[1][i], res[0][i]) <= RUN_TOL
        TL.check(res[1][i], c["ref"][k], f"table at +4 {k}")
    assert torch.isnan(big[:off]).all() and torch.isnan(big[off + 300 * 40:]).all()
    # BilinScoring.table_loss: v = u W[0] through ops.linear, the bias for the score bits; the scorer's parameters flat at +4 too
    from tests.table_loss_ref import table_loss_ref
    from xnrs_amd.models.blocks import BilinScoring
    torch.manual_seed(5)
    sc0, sc1 = BilinScoring(40).to(DEV), BilinScoring(40).to(DEV)
    sc1.load_state_dict(sc0.state_dict())
    AR.misalign_parameters(sc1, 4)
    assert sc1.bilin.weight.data_ptr() % 16 == 4
    out = []
    for scorer, t, u in ((sc0, c["table"], c["up"]), (sc1, tab, up)):
        u = u.detach().clone().requires_grad_(True) if scorer is sc0 else AR.shifted(u.detach(), 4).requires_grad_(True)
        loss, scores, lse = scorer.table_loss(t.detach(), u, *c["tgt"], *c["excl_csr"], c["pad_row"], *c["win"])
        (loss * c["g"]).sum().backward()
        out.append((loss.detach(), scores.detach(), u.grad, scorer.bilin.weight.grad))
    v64 = c["up"].double().cpu() @ sc0.bilin.weight[0].detach().double().cpu()
    r = table_loss_ref(c["table"], v64, *c["tgt"], *c["excl_csr"], c["pad_row"], *c["win"], sc0.bilin.bias.detach(), c["g"])
    TL.check(out[1][0], r["loss"], "BilinScoring.table_loss at +4 loss")
    for a, b in zip(out[0], out[1]):
        fin = torch.isfinite(a)
        assert torch.equal(fin, torch.isfinite(b)) and H.rel_err(torch.where(fin, b, 0.0), torch.where(fin, a, 0.0)) <= RUN_TOL


def test_workspace_base_is_checked():
    """include/xnrs_hip.h: a workspace must be 256-byte aligned; the one place that hands them out says so."""
    ws = hip.workspace(DEV, 1000)
    assert ws.data_ptr() % hip.WORKSPACE_ALIGN == 0 and hip.WORKSPACE_ALIGN == 256
