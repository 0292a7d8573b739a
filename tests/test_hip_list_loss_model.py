"""GPU: losses.mined_negatives_loss on a tiny NRMS and a tiny StandardRec, with the dot and the bilinear scorer, over
synth.click_world(n_news=60, n_sess=24): the loss against the fp64 reference of the definition (tests/list_loss_ref.py) fed
with the model's own user vectors, table and mined lists; the lists against topk_deep under the merged exclusions; every
parameter gradient against the composed route (ops.embedding_rows + the scorer + torch's logsumexp on the same lists); the
order n_negatives = 4 <= 16 <= full_table_loss; windows; given lists."""
import functools

import pytest
import torch

from tests import helpers as H
from tests import test_hip_table_loss_model as TLM
from tests.list_loss_ref import list_loss_ref
from xnrs_amd import losses, ops, synth
from xnrs_amd.models import make_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L_HIST = 5
N_NEWS, N_SESS = 60, 24
COMBOS = [("NRMS", "dot"), ("NRMS", "bilin"), ("standard", "dot"), ("standard", "bilin")]
SESS = [4, 0, 2, 23, 11, 7, 19, 3, 5]


@functools.lru_cache(maxsize=None)
def build(kind, scoring):
    torch.manual_seed(3)
    store, beh = synth.click_world(n_news=N_NEWS, n_sess=N_SESS, S=6, D=32)
    store, beh = store.to(DEV), beh.to(DEV)
    beh.pos_val[2] = store.pad_row  # a click without an answer: it must not count in the mean
    cfg = TLM.Cfg(synth.model_cfg(dict(model=kind, E=32, bias=True, h=4, D=32, H=L_HIST, S=6)))
    cfg["scoring"] = scoring
    model = make_model(cfg).to(DEV).eval()  # (no dropout: the two sides encode the users in separate calls)
    if scoring == "bilin":
        with torch.no_grad():
            model.rec_model.bilin.weight.mul_(4.0)
    return model, store, beh


def operands(model, store, beh, sess=SESS, windows=None):
    """what the loss sees behind the shared path: table, user vectors, history and click CSRs, the sessions' windows"""
    return losses._encode_sessions(model, store, beh, sess, L_HIST, True, windows, None, None, "test")


def reference(model, vecs, u, tgt, rows, pad_row):
    sc = model.rec_model
    up, bias = u.detach().double().cpu().reshape(len(rows), -1), None
    if hasattr(sc, "bilin"):
        up, bias = up @ sc.bilin.weight[0].detach().double().cpu(), sc.bilin.bias.detach()
    r = list_loss_ref(vecs.detach(), up, tgt[0], tgt[1], rows, pad_row, bias)
    return r, r["loss"].sum() / max(int(r["valid"].sum()), 1)


def composed_loss(model, vecs, u, tgt, rows, pad_row):
    """the route a user composes from the parent's operators: gather the listed rows and the click into a (B, L + 1, E) copy,
    score it with the scorer's forward, logsumexp in torch"""
    B, L = rows.shape
    n_rows, E = vecs.shape
    click = tgt[1].reshape(B, 1)  # (one click per session in this world)
    idx = torch.cat((click, rows), dim=1)
    valid = (idx >= 0) & (idx < n_rows) & (idx != pad_row)
    valid[:, 1:] &= rows != click
    c = ops.embedding_rows(idx.clamp(0, n_rows - 1).reshape(-1).contiguous(), vecs).reshape(B, L + 1, E)
    sc = model.rec_model
    s = (ops.bilinear_scoring(u.reshape(B, 1, E), c, sc) if hasattr(sc, "bilin") else ops.dot_scoring(u.reshape(B, 1, E), c))
    s = s.reshape(B, L + 1).masked_fill(~valid, float("-inf"))
    has = valid[:, 0] & valid[:, 1:].any(dim=1)
    loss = torch.logsumexp(s[has], dim=1) - s[has][:, 0]
    return loss.sum() / valid[:, 0].sum()


@pytest.mark.parametrize("kind,scoring", COMBOS)
def test_loss_and_lists_match_the_reference_and_topk_deep(kind, scoring):
    model, store, beh = build(kind, scoring)
    with torch.no_grad():
        got, rows = losses.mined_negatives_loss(model, store, beh, SESS, L_HIST, n_negatives=8, return_negatives=True)
        vecs, u, hist, tgt, _, pad_row = operands(model, store, beh)
    assert rows.shape == (len(SESS), 8) and rows.dtype == torch.int32
    r, want = reference(model, vecs, u, tgt, rows, pad_row)
    assert int(r["valid"].sum()) == len(SESS) - 1 and r["filled"].all()
    e = H.rel_err(got.reshape(1), want.reshape(1))
    print(f"MARGIN {kind} {scoring} loss: {e / H.RTOL:.3f} of the bar")
    H.assert_close(got.reshape(1), want.reshape(1), what="loss")
    # the lists: topk_deep under the merged exclusions, as recommend() would call it
    excl = losses.merged_exclusions(hist, tgt)
    with torch.no_grad():
        want_rows = model.rec_model.topk_deep(vecs, u, 8, excl[0], excl[1], pad_row)[0]
    assert torch.equal(rows, want_rows)
    ho, hr, to, tr = hist[0].tolist(), hist[1].tolist(), tgt[0].tolist(), tgt[1].tolist()
    for b, l in enumerate(rows.tolist()):
        banned = set(hr[ho[b]:ho[b + 1]]) | set(tr[to[b]:to[b + 1]]) | {pad_row}
        assert len(set(l)) == 8 and not set(l) & banned and all(0 <= x < store.n_rows for x in l), b
    each = losses.mined_negatives_loss(model, store, beh, SESS, L_HIST, n_negatives=8, reduction="none")
    assert each.shape == (len(SESS),) and (each[2] == 0).all()  # session 2 is the third of SESS: its click is the pad row


@pytest.mark.parametrize("kind,scoring", COMBOS)
def test_parameter_gradients_match_the_composed_route(kind, scoring):
    model, store, beh = build(kind, scoring)
    model.zero_grad(set_to_none=True)
    got, rows = losses.mined_negatives_loss(model, store, beh, SESS, L_HIST, n_negatives=8, return_negatives=True)
    got.backward()
    got_g = TLM.grads_of(model)
    vecs, u, _, tgt, _, pad_row = operands(model, store, beh)
    want = composed_loss(model, vecs, u, tgt, rows, pad_row)
    want.backward()
    want_g = TLM.grads_of(model)
    H.assert_close(got.detach().reshape(1), want.detach().reshape(1), what="loss")
    assert any(k.startswith("news_encoder.") for k in got_g) and any(k.startswith("user_encoder.") for k in got_g)
    TLM.compare(model, got_g, want_g, f"{kind} {scoring}")


@pytest.mark.parametrize("kind,scoring", COMBOS)
def test_more_negatives_never_lower_the_loss_and_all_of_them_give_the_full_table_loss(kind, scoring):
    model, store, beh = build(kind, scoring)
    with torch.no_grad():
        l4, l16, lall = (losses.mined_negatives_loss(model, store, beh, SESS, L_HIST, n_negatives=k, reduction="none")
                         for k in (4, 16, 64))
        full = losses.full_table_loss(model, store, beh, SESS, L_HIST, reduction="none")
    # the prefix property of topk_deep: the list of 16 starts with the list of 4, so only terms are added under the log
    assert (l4 <= l16 + 1e-6).all() and (l16 <= full + 1e-6).all()
    assert (l4 < l16).any()
    e = H.assert_close(lall, full, what="every eligible row listed")
    print(f"MARGIN {kind} {scoring} n_negatives >= n_news vs full_table_loss: {e / H.RTOL:.3f} of the bar")


@pytest.mark.parametrize("kind,scoring", COMBOS[:1] + COMBOS[3:])
def test_windows_restrict_the_mined_rows_and_given_lists_reproduce_the_mined_call(kind, scoring):
    model, store, beh = build(kind, scoring)
    n = store.n_rows
    lo = torch.arange(N_SESS, dtype=torch.int32, device=DEV) % 20
    hi = lo + 30
    with torch.no_grad():
        loss, rows = losses.mined_negatives_loss(model, store, beh, SESS, L_HIST, n_negatives=8, windows=(lo, hi),
                                                 return_negatives=True)
    sess = torch.tensor(SESS, device=DEV)
    listed = rows >= 0
    assert listed.any() and (rows[listed] < n).all()
    assert ((rows >= lo[sess][:, None]) & (rows < hi[sess][:, None]))[listed].all()
    # given lists: the mining is skipped, the same bits
    mined = losses.mined_negatives_loss(model, store, beh, SESS, L_HIST, n_negatives=8, return_negatives=True)
    model.zero_grad(set_to_none=True)
    mined[0].backward()
    g_mined = TLM.grads_of(model)
    given = losses.mined_negatives_loss(model, store, beh, SESS, L_HIST, neg_rows=mined[1].clone())
    given.backward()
    g_given = TLM.grads_of(model)
    assert torch.equal(given.detach(), mined[0].detach()) and set(g_mined) == set(g_given)
    for k in g_mined:
        assert torch.equal(g_mined[k], g_given[k]), k


@pytest.mark.parametrize("kind,scoring", COMBOS[:1] + COMBOS[3:])
def test_a_session_with_an_empty_window_between_sessions_that_click_the_same_news(kind, scoring):
    """Sessions 13, 14 and 15 click the same news.  Session 14 gets an empty window, so it mines fillers only and has no
    negatives: it contributes 0, and in the table gradient its click lies between the clicks of 13 and 15 -- the gradients of
    every tower still meet the composed route."""
    model, store, beh = build(kind, scoring)
    sess = [13, 14, 15, 4, 6, 0]
    assert len({int(beh.pos_val[s]) for s in sess[:3]}) == 1
    lo = torch.zeros(N_SESS, dtype=torch.int32, device=DEV)
    hi = torch.full((N_SESS,), store.n_rows, dtype=torch.int32, device=DEV)
    hi[14] = 0
    model.zero_grad(set_to_none=True)
    got, rows = losses.mined_negatives_loss(model, store, beh, sess, L_HIST, n_negatives=8, windows=(lo, hi), return_negatives=True)
    assert (rows[1] == -1).all() and (rows[[0, 2, 3, 4, 5]] >= 0).all()
    got.backward()
    got_g = TLM.grads_of(model)
    vecs, u, _, tgt, _, pad_row = operands(model, store, beh, sess)
    want = composed_loss(model, vecs, u, tgt, rows, pad_row)
    want.backward()
    want_g = TLM.grads_of(model)
    H.assert_close(got.detach().reshape(1), want.detach().reshape(1), what="loss")
    TLM.compare(model, got_g, want_g, f"empty window {kind} {scoring}")
    each = losses.mined_negatives_loss(model, store, beh, sess, L_HIST, n_negatives=8, windows=(lo, hi), reduction="none")
    assert each[1].item() == 0 and (each[[0, 2]] > 0).all()
