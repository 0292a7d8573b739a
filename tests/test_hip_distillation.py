"""GPU: losses.distillation_loss over synth.click_world(n_news=90, n_sess=40) -- an fc-scorer teacher and an NPA teacher, each
into a dot student and a bilinear student: the loss against the KL computed in fp64 on the CPU from the returned lists, the
teacher's own scores of them and the student's table and user vectors; the gradients of the student's user tower against
that reference's; the student as its own teacher; reuse of lists; windows and history; evaluation.list_recall."""
import functools

import pytest
import torch

from tests import helpers as H
from tests import test_hip_table_loss_model as TLM
from xnrs_amd import evaluation as EV
from xnrs_amd import losses, synth
from xnrs_amd.data import DeviceBatcher

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# TAU: the towers are untrained, so at temperature 1 both distributions over a pool are nearly uniform and the KL is 1e-4 of the
# cross-entropy it is the difference of -- below the fp32 rounding of that cross-entropy when held to RTOL of ITSELF.  At 0.05 the
# logits are 20 times larger and the KL is a sizeable part of the cross-entropy: the comparison with the fp64 KL is then
# well-conditioned.  The nearly-uniform regime is what test_the_student_as_its_own_teacher_has_no_kl holds to the cross-entropy.
L_HIST, POOL, TAU = 5, 16, 0.05
N_NEWS, N_SESS = 90, 40
SESS = [4, 0, 2, 23, 11, 7, 39, 3, 5, 31]
COMBOS = [(t, s) for t in ("fc", "npa") for s in ("dot", "bilin")]


@functools.lru_cache(maxsize=None)
def world():
    store, beh = synth.click_world(n_news=N_NEWS, n_sess=N_SESS)
    store, beh = store.to(DEV), beh.to(DEV)
    beh.user_index = torch.arange(len(beh), device=DEV) % 7
    return store, beh


@functools.lru_cache(maxsize=None)
def model(kind):
    """'dot' / 'bilin' / 'fc': a small StandardRec with that scorer; 'npa': a tiny NPA over the same token shapes"""
    if kind == "npa":
        return H.npa_and_nrms(DEV)[0]
    from tests.test_hip_scorers import _eval_model
    m = _eval_model(kind)
    if kind == "bilin":
        with torch.no_grad():
            m.rec_model.bilin.weight.mul_(4.0)
    return m


def teacher_scores(teacher, rows, sess=SESS):
    """the teacher's own raw scores of the listed rows, by the public hooks: score_csr over its table / score_impressions"""
    store, beh = world()
    s = torch.tensor(sess, device=DEV)
    hist = DeviceBatcher(beh, L_HIST, store.pad_row).eval_batch(s)[0]
    with torch.no_grad():
        if getattr(teacher, "user_dependent_news", False):
            b, k = rows.shape
            csess = torch.arange(b, device=DEV, dtype=torch.int32).repeat_interleave(k)
            crows = torch.where(rows >= 0, rows, torch.full_like(rows, store.pad_row)).reshape(-1)
            return teacher.score_impressions(store, hist, crows, csess, beh.user_index[s], relu=False).reshape(b, k)
        vecs, hm = EV.encode_news_table(teacher, store)
        u = teacher.encode_user(vecs[hist.long()], hm[hist.long()])
        return EV._raw_scores(teacher.rec_model, teacher.rec_model.prepare_csr(vecs), u, rows)


def reference_kl(student, vecs, u, rows, t, pad_row, tau):
    """fp64 on the CPU: KL(softmax(t / tau) || softmax(s / tau)) per session over the filled slots, s the student's scores of
    the listed rows -> (kl:(B,), cross-entropy:(B,), d kl.mean / d u, d kl.mean / d W or None)"""
    sc = student.rec_model
    rows = rows.cpu().long()
    B = rows.shape[0]
    up = u.detach().double().cpu().reshape(B, -1).requires_grad_(True)
    v, W, bias = up, None, 0.0
    if hasattr(sc, "bilin"):
        W = sc.bilin.weight.detach().double().cpu().requires_grad_(True)
        v, bias = up @ W[0], sc.bilin.bias.detach().double().cpu()
    table = vecs.detach().double().cpu()
    filled = (rows >= 0) & (rows < table.shape[0]) & (rows != pad_row)
    assert filled.any(dim=1).all()
    s = (table[rows.clamp(0, table.shape[0] - 1)] * v[:, None, :]).sum(-1) + bias
    logp = torch.log_softmax((s / tau).masked_fill(~filled, float("-inf")), dim=1).masked_fill(~filled, 0.0)
    w = torch.softmax((t.double().cpu() / tau).masked_fill(~filled, float("-inf")), dim=1)
    xent = -(w * logp).sum(dim=1)
    kl = xent + (w * torch.where(w > 0, w.log(), torch.zeros_like(w))).sum(dim=1)
    g = torch.autograd.grad(kl.mean(), [up] + ([W] if W is not None else []))
    return kl.detach(), xent.detach(), g[0], (g[1] if W is not None else None)


@pytest.mark.parametrize("teacher_kind,student_kind", COMBOS)
def test_loss_and_user_tower_gradients_match_the_fp64_kl(teacher_kind, student_kind):
    store, beh = world()
    student, teacher = model(student_kind), model(teacher_kind)
    vecs, hm = EV.encode_news_table(student, store)  # a detached pair: the user tower and the scorer train
    student.zero_grad(set_to_none=True)
    loss, rows = losses.distillation_loss(student, teacher, (vecs, hm), beh, SESS, L_HIST, pool=POOL, temperature=TAU,
                                          store=store, return_lists=True)
    assert rows.shape == (len(SESS), POOL) and rows.dtype == torch.int32 and (rows >= 0).all()
    loss.backward()
    got_g = TLM.grads_of(student)
    _, u, _, _, _, pad_row = losses._encode_sessions(student, (vecs, hm), beh, SESS, L_HIST, True, None, store, None, "test")
    kl, xent, d_u, d_W = reference_kl(student, vecs, u, rows, teacher_scores(teacher, rows), pad_row, TAU)
    what = f"{teacher_kind} -> {student_kind}"
    e = H.rel_err(loss.detach().reshape(1), kl.mean().reshape(1))
    print(f"MARGIN {what} loss: {e / H.RTOL:.3f} of the bar (KL {kl.mean().item():.4e}, cross-entropy {xent.mean().item():.4e})")
    assert kl.mean().item() > 0
    H.assert_close(loss.detach().reshape(1), kl.mean().reshape(1), what=f"{what} loss")
    each = losses.distillation_loss(student, teacher, (vecs, hm), beh, SESS, L_HIST, pool=POOL, temperature=TAU, store=store,
                                    reduction="none")
    H.assert_close(each.detach(), kl, what=f"{what} loss per session")
    params = {k: p for k, p in student.named_parameters() if k.startswith("user_encoder.")}
    want = torch.autograd.grad(u, list(params.values()), grad_outputs=d_u.float().to(DEV).reshape(u.shape), allow_unused=True)
    want_g = {k: g for k, g in zip(params, want) if g is not None}
    if d_W is not None:
        want_g["rec_model.bilin.weight"] = d_W.float().to(DEV)
    assert any(k.startswith("user_encoder.") for k in got_g)
    TLM.compare(student, got_g, want_g, what)


@pytest.mark.parametrize("student_kind", ["dot", "bilin"])
def test_the_student_as_its_own_teacher_has_no_kl(student_kind):
    store, beh = world()
    student = model(student_kind)
    with torch.no_grad():
        kl, rows = losses.distillation_loss(student, student, store, beh, SESS, L_HIST, pool=POOL, reduction="none",
                                            return_lists=True)
        vecs, u, _, _, _, pad_row = losses._encode_sessions(student, store, beh, SESS, L_HIST, True, None, None, None, "test")
    _, xent, _, _ = reference_kl(student, vecs, u, rows, teacher_scores(student, rows), pad_row, 1.0)
    e = (kl.cpu().double().abs() / xent).max().item()
    print(f"MARGIN own teacher {student_kind}: |KL| / cross-entropy {e / H.RTOL:.3f} of the bar")
    assert e <= H.RTOL


@pytest.mark.parametrize("teacher_kind,student_kind", [("fc", "dot"), ("npa", "bilin")])
def test_given_lists_reproduce_the_mined_call_and_serve_the_ranking_loss(teacher_kind, student_kind):
    store, beh = world()
    student, teacher = model(student_kind), model(teacher_kind)
    student.zero_grad(set_to_none=True)
    mined, rows = losses.distillation_loss(student, teacher, store, beh, SESS, L_HIST, pool=POOL, temperature=TAU, return_lists=True)
    mined.backward()
    g_mined = TLM.grads_of(student)
    given = losses.distillation_loss(student, teacher, store, beh, SESS, L_HIST, temperature=TAU, rows=rows.clone())
    given.backward()
    g_given = TLM.grads_of(student)
    assert torch.equal(given.detach(), mined.detach()) and set(g_mined) == set(g_given)
    assert any(k.startswith("news_encoder.") for k in g_mined)  # a NewsStore: the table is encoded under autograd
    for k in g_mined:
        assert torch.equal(g_mined[k], g_given[k]), k
    # the teacher's table encoded once and handed in: the same loss
    if teacher_kind == "fc":
        table = EV.encode_news_table(teacher, store)
        again = losses.distillation_loss(student, teacher, store, beh, SESS, L_HIST, temperature=TAU, rows=rows, teacher_table=table)
        assert torch.equal(again.detach(), mined.detach())
    # the same lists as the negatives of the ranking loss in the same step
    rank = losses.mined_negatives_loss(student, store, beh, SESS, L_HIST, neg_rows=rows)
    assert torch.isfinite(rank) and rank.item() > 0


def test_windows_and_history_are_honoured_and_clicks_stay():
    store, beh = world()
    student, teacher = model("dot"), model("fc")
    lo = torch.arange(N_SESS, dtype=torch.int32, device=DEV) % 20
    hi = lo + 30
    hi[SESS[1]] = lo[SESS[1]]  # an empty window: no filled slot, no NaN, no share in the mean
    sess = torch.tensor(SESS, device=DEV)
    ho, hv = beh.hist_off.tolist(), beh.hist_val.tolist()
    with torch.no_grad():
        loss, rows = losses.distillation_loss(student, teacher, store, beh, SESS, L_HIST, pool=POOL, windows=(lo, hi),
                                              reduction="none", return_lists=True)
        mean = losses.distillation_loss(student, teacher, store, beh, SESS, L_HIST, windows=(lo, hi), rows=rows)
    assert torch.isfinite(loss).all() and loss[1].item() == 0 and (rows[1] == -1).all()
    assert mean.item() == pytest.approx(loss.sum().item() / (len(SESS) - 1), rel=1e-5)
    listed = rows >= 0
    assert listed[[0] + list(range(2, len(SESS)))].any(dim=1).all()
    assert ((rows >= lo[sess][:, None]) & (rows < hi[sess][:, None]))[listed].all()
    for i, s in enumerate(SESS):
        got = set(rows[i][listed[i]].tolist())
        assert not got & set(hv[ho[s]:ho[s + 1]]) and store.pad_row not in got, s
    # a pool longer than the table lists every eligible row: the session's click is among them unless its history holds it
    with torch.no_grad():
        rows = losses.distillation_loss(student, teacher, store, beh, SESS, L_HIST, pool=128, return_lists=True)[1]
        free = losses.distillation_loss(student, teacher, store, beh, SESS, L_HIST, pool=128, exclude_history=False,
                                        return_lists=True)[1]
    po, pv = beh.pos_off.tolist(), beh.pos_val.tolist()
    seen = 0
    for i, s in enumerate(SESS):
        hist, got = set(hv[ho[s]:ho[s + 1]]), set(rows[i].tolist())
        assert not got & hist and got | hist >= set(range(store.n_rows)) - {store.pad_row}
        clicks = set(pv[po[s]:po[s + 1]]) - hist - {store.pad_row}
        assert clicks <= got
        seen += len(clicks)
        assert set(free[i].tolist()) >= set(range(store.n_rows)) - {store.pad_row}
    assert seen > 0


def test_list_recall_against_a_loop():
    store, beh = world()
    student, teacher = model("dot"), model("fc")
    pool_rows = EV.recommend(student, store, beh, L_HIST, k=24)[0]
    top = EV.recommend(teacher, store, beh, L_HIST, k=10)[0].clone()
    top[3, 4:] = -1
    top[7] = -1
    got = EV.list_recall(pool_rows, top)
    assert got.shape == (N_SESS,) and got.dtype == torch.float32 and got.device == pool_rows.device
    for i in range(N_SESS):
        want = [r for r in top[i].tolist() if r >= 0]
        have = set(pool_rows[i].tolist())
        assert got[i].item() == pytest.approx(sum(r in have for r in want) / max(len(want), 1), abs=1e-6), i
    assert got[7].item() == 0 and 0 < got.mean().item() < 1
