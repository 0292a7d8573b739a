"""GPU: losses.full_table_loss on a tiny NRMS and a tiny bilinear-scorer model against the same loss assembled in torch on the
device -- the model's own encoded table and encode_user through the project's autograd encoders, a dense u @ table.T and a
masked logsumexp -- the loss value and every parameter gradient, with a detached table and with the table under autograd."""
import pytest
import torch

from tests import helpers as H
from tests.table_loss_ref import negatives_mask
from xnrs_amd import evaluation as EV
from xnrs_amd import losses, synth
from xnrs_amd.data import DeviceBatcher
from xnrs_amd.models import make_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L_HIST = 5


class Cfg(dict):
    __getattr__ = dict.__getitem__


def build(scoring):
    torch.manual_seed(3)
    store, beh = synth.click_world(n_news=300, n_sess=6, S=6, D=32)
    store, beh = store.to(DEV), beh.to(DEV)
    beh.pos_val[2] = store.pad_row  # a click without an answer: it must not count in the mean
    cfg = Cfg(synth.model_cfg(dict(model="NRMS", E=32, bias=True, h=4, D=32, H=L_HIST, S=6)))
    cfg["scoring"] = scoring
    model = make_model(cfg).to(DEV).eval()  # (no attention dropout: the two sides encode the users in separate calls)
    if scoring == "bilin":
        with torch.no_grad():
            model.rec_model.bilin.weight.mul_(4.0)
    return model, store, beh


def torch_loss(model, store, beh, sess, table, windows):
    """the definition in torch ops on the device; table = (vecs, hm), with or without a graph behind vecs"""
    vecs, hm = table
    sess_t = torch.tensor(sess, device=DEV)
    hist = DeviceBatcher(beh, L_HIST, store.pad_row).eval_batch(sess_t)[0]
    u = model.encode_user(vecs[hist.long()], hm[hist.long()]).reshape(len(sess), -1)
    sc = model.rec_model
    # the scores and everything behind them in fp64: the only fp32 arithmetic the two sides do not share is what is under test
    if hasattr(sc, "bilin"):
        s = (u.double() @ sc.bilin.weight[0].double()) @ vecs.double().T + sc.bilin.bias.double()
    else:
        s = u.double() @ vecs.double().T
    print(f"max|s| = {s.abs().max().item():.2f}")
    tgt = EV._session_csr(beh.pos_off, beh.pos_val, sess_t, None)
    excl = EV._history_csr(beh, sess_t, None)
    win = (None, None) if windows is None else (windows[0][sess_t], windows[1][sess_t])
    neg = negatives_mask(len(sess), vecs.shape[0], tgt[0], tgt[1], excl[0], excl[1], store.pad_row, *win).to(DEV)
    lse = torch.logsumexp(s.masked_fill(~neg, float("-inf")), dim=1)
    off, rows = tgt[0].tolist(), tgt[1].tolist()
    terms = []
    for b in range(len(sess)):
        for t in rows[off[b]:off[b + 1]]:
            if 0 <= t < vecs.shape[0] and t != store.pad_row:
                terms.append(torch.logaddexp(s[b, t], lse[b]) - s[b, t])
    return torch.stack(terms).sum() / len(terms), len(terms)


def grads_of(model):
    g = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    return g


def compare(model, got, want, what):
    """every gradient at the project's bar, a tensor's scale being max(its own, 1e-3 of the step's largest gradient): one that
    is analytically zero (the key bias of an attention) is rounding noise on both sides (tests/helpers.py assert_grads_close)"""
    bias = "rec_model.bilin.bias"  # cancels in the loss: torch's sum of rounding noise on one side, no gradient on the other
    assert bias not in got or (got[bias] == 0).all()
    want = {k: v for k, v in want.items() if k != bias}
    got = {k: v for k, v in got.items() if k != bias}
    assert set(got) == set(want) and got, what
    gmax = max(v.abs().max().item() for v in want.values())
    assert gmax > 0
    over = []
    for k in want:
        scale = max(want[k].abs().max().item(), 1e-3 * gmax)
        e = (got[k].double() - want[k].double()).abs().max().item() / scale
        print(f"MARGIN {what} {k}: {e / H.RTOL:.3f} of the bar")
        if not e <= H.RTOL:
            over.append(f"{k}: {e:.3e}")
    assert not over, f"{what}: {over}"


@pytest.mark.parametrize("scoring", ["dot", "bilin"])
@pytest.mark.parametrize("detached", [True, False])
def test_full_table_loss_matches_the_torch_assembly(scoring, detached):
    model, store, beh = build(scoring)
    sess = [4, 0, 2, 5, 1, 3]
    n = store.n_rows
    windows = None
    if detached:  # with row windows, indexed by session id: the second half, the whole table, an empty one, ...
        windows = (torch.tensor([n // 2, 0, 0, 7, 100, 0], dtype=torch.int32, device=DEV),
                   torch.tensor([n, n, n, 7, 260, n - 40], dtype=torch.int32, device=DEV))
    if detached:
        table = EV.encode_news_table(model, store)
    else:
        y, m = model.encode_news_ids(store, torch.arange(n, dtype=torch.int32, device=DEV).reshape(1, -1))
        table = (y[0], m[0])
    want, n_valid = torch_loss(model, store, beh, sess, table, windows)
    want.backward()
    want_g = grads_of(model)
    if detached:
        got = losses.full_table_loss(model, table, beh, sess, L_HIST, windows=windows, store=store)
    else:
        got = losses.full_table_loss(model, store, beh, sess, L_HIST)
    got.backward()
    got_g = grads_of(model)
    assert n_valid == 5  # six sessions with one click each, one of them the pad row
    e = H.rel_err(got.reshape(1), want.detach().reshape(1))
    print(f"MARGIN {scoring} detached={detached} loss: {e / H.RTOL:.3f} of the bar")
    H.assert_close(got.reshape(1), want.detach().reshape(1), what="loss")
    news = [k for k in want_g if k.startswith("news_encoder.")]
    assert (not news) if detached else news, "the news encoder trains exactly when the table is under autograd"
    compare(model, got_g, want_g, f"{scoring} detached={detached}")
    total = losses.full_table_loss(model, table if detached else store, beh, sess, L_HIST, windows=windows, reduction="sum",
                                   store=store)
    each = losses.full_table_loss(model, table if detached else store, beh, sess, L_HIST, windows=windows, reduction="none",
                                  store=store)
    assert each.shape == (6,) and (each[2] == 0).all()  # session 2 is the third of `sess`: its click is the pad row
    H.assert_close(total.reshape(1), (got * n_valid).detach().reshape(1), what="sum = mean * valid clicks")
