"""NPA (xnrs/models/full_models/npa.py:8-95) and layers.PersonalizedAttention (xnrs/models/components/layers.py:72-102) on
the HIP path.  Same constructor signatures, submodule registration order and state_dict keys as the reference, so that under
the same torch.manual_seed every parameter starts at the reference's value.

Deliberately NOT exported from xnrs_amd.models.components.*: install() mirrors those modules into the reference's import
paths, and the reference's own NPA would then pick up this GPU-only pooler.  The model is opt-in there:
install(hip_models=("NPA",)).

Per step: the two q_fc projections of the user embedding as ONE gathered GEMM (their weights stacked, N = 2 x 128), one
personalized encoder call per news block with the news head fused behind it (history and candidates may share one call
through q_idx), one for the user tower, then the model's scorer.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch
import torch.nn as nn

from .. import hip, ops

HIDDEN = 128  # npa.py:18,29: hidden_features=128 of both poolers


class PersonalizedAttention(nn.Module):
    """layers.PersonalizedAttention: x_fc Linear(in, hidden), q_fc Linear(query, hidden); a_i = exp(q_fc(q) . tanh(x_fc x_i))
    * m_i / (sum + 1e-8), p = sum_i a_i x_i.  q:(B,1,Dq), x:(B,N,D), m:(B,N,1) -> (B,1,D)."""

    def __init__(self, in_features, hidden_features, query_features):
        super().__init__()
        self.x_fc = nn.Linear(in_features, hidden_features)
        self.q_fc = nn.Linear(query_features, hidden_features)

    def forward(self, q: torch.Tensor, x: torch.Tensor, m: torch.Tensor = None):
        b, n, d = x.shape
        qp = ops.linear(q.reshape(b, -1), self.q_fc.weight, self.q_fc.bias)
        y, _ = ops.personalized(x, None if m is None else m.reshape(b, n), None, qp, _index_rows(b, 1, x.device), self.x_fc)
        return y.reshape(b, 1, d)


_IDX: Dict[Tuple, torch.Tensor] = {}
_IDX_MAX = 256


def _index_rows(n_rows: int, per: int, device) -> torch.Tensor:
    """int32 [n_rows * per]: s // per (the query row of every sequence when each user owns `per` consecutive ones), every
    value in [0, n_rows).  Cached per shape, but only entries built outside a hipGraph capture (a tensor created during a
    capture holds its values only once the graph has replayed), and never evicted (a captured graph may read a cached
    entry); past _IDX_MAX shapes the index is built per call."""
    key = (n_rows, per, str(device))
    t = _IDX.get(key)
    if t is None:
        t = torch.div(torch.arange(n_rows * per, device=device, dtype=torch.int32), per, rounding_mode="floor")
        if len(_IDX) < _IDX_MAX and not torch.cuda.is_current_stream_capturing():
            _IDX[key] = t
    return t


def _checked_uids(uid: torch.Tensor, n_rows: int) -> torch.Tensor:
    """uid as int32 clamped into the user table (no host read): the gathered GEMM never reads outside the table, and an id
    that had to be clamped sets hip.STATUS_QUERY_RANGE in the device status word (hip.check_status raises at the next sync).
    (The word is created outside a hipGraph capture only: a capture records its zero fill without running it.)"""
    flat = uid.reshape(-1).to(torch.int32)
    ok = flat.clamp(0, n_rows - 1)
    if flat.numel() and flat.is_cuda and (not torch.cuda.is_current_stream_capturing()
                                          or torch.device(flat.device).index in hip._status):
        bad = (ok != flat).any().to(torch.int32) * hip.STATUS_QUERY_RANGE
        hip.status_word(flat.device).bitwise_or_(bad.reshape(1))
    return ok


class NPA(nn.Module):
    """npa.py:8-95.  forward(batch) on the reference's batch dict; forward_store(store, hist_ids, cand_ids, uid) with the
    news given as rows of a device-resident NewsStore (tokens gathered inside the first GEMM's load)."""

    #: evaluate() encodes news per impression batch for this model: its news vectors depend on the user
    user_dependent_news = True

    def __init__(self, cfg, rec_model):
        super().__init__()
        self.user_embedder = nn.Embedding(num_embeddings=cfg.n_users + 1, embedding_dim=cfg.user_emb_dim)
        self.title_pooler = PersonalizedAttention(in_features=cfg.d_backbone, hidden_features=HIDDEN,
                                                  query_features=cfg.user_emb_dim)
        self.dropout = nn.Dropout(p=cfg.p_dropout)
        self.news_head = nn.Sequential(nn.Linear(cfg.d_backbone, cfg.title_emb_dim), nn.ReLU(),
                                       nn.Linear(cfg.title_emb_dim, cfg.title_emb_dim))
        self.user_encoder = PersonalizedAttention(in_features=cfg.title_emb_dim, hidden_features=HIDDEN,
                                                  query_features=cfg.user_emb_dim)
        self.rec_model = rec_model

    # ---- pieces
    def queries(self, uid: torch.Tensor) -> torch.Tensor:
        """(B, 2A): [title_pooler.q_fc | user_encoder.q_fc] of user_embedder(uid) as ONE gathered GEMM (one backward, one
        table gradient of the cost of the batch)."""
        tq, uq = self.title_pooler.q_fc, self.user_encoder.q_fc
        w = torch.cat([tq.weight, uq.weight], 0)
        b = None if tq.bias is None or uq.bias is None else torch.cat([tq.bias, uq.bias], 0)
        if (tq.bias is None) != (uq.bias is None):
            raise hip.XnrsHipError("NPA: the two q_fc layers must both have a bias or both have none")
        if not uid.is_cuda:
            raise hip.XnrsHipError("NPA: user indices must live on the HIP device")
        return ops.embedding_linear_table(_checked_uids(uid, self.user_embedder.num_embeddings), self.user_embedder.weight, w, b)

    def encode_news(self, x, m, ids, q, q_idx):
        """Personalized title pooling + news head: -> (vectors (n, E), hm (n,))."""
        return ops.personalized(x, m, ids, q, q_idx, self.title_pooler.x_fc, self.news_head)

    def encode_user(self, h, hm, q):
        """user_encoder over the news vectors h:(B, nh, E) with mask hm:(B, nh) -> (B, E)."""
        b = h.shape[0]
        u, _ = ops.personalized(h, hm, None, q, _index_rows(b, 1, h.device), self.user_encoder.x_fc)
        return u

    def _device(self):
        return self.user_embedder.weight.device

    # ---- reference API
    def _forward(self, hist_title_features: tuple, cand_title_features: tuple, uid: torch.Tensor):
        dev = self._device()
        h, hm = (t.to(dev) for t in hist_title_features)
        c, cm = (t.to(dev) for t in cand_title_features)
        Q = self.queries(uid.to(dev))
        qt, qu = Q[:, :HIDDEN], Q[:, HIDDEN:]
        b, nh, s, d = h.shape
        hv, hmask = self.encode_news(self.dropout(h.reshape(b * nh, s, d)), hm.reshape(b * nh, s), None, qt,
                                     _index_rows(b, nh, dev))
        e = hv.shape[1]
        u = self.encode_user(hv.reshape(b, nh, e), hmask.reshape(b, nh), qu)
        b, nc, s, d = c.shape
        cv, _ = self.encode_news(self.dropout(c.reshape(b * nc, s, d)), cm.reshape(b * nc, s), None, qt, _index_rows(b, nc, dev))
        return self.rec_model(u.reshape(b, 1, e), cv.reshape(b, nc, e))

    def forward(self, batch: dict):
        return self._forward(hist_title_features=batch['user_features']['history']['title_emb'],
                             cand_title_features=batch['candidate_features']['title_emb'],
                             uid=batch['user_features']['other']['user_index'])

    # ---- device data path
    def _id_path_rows(self, store, ids):
        """(x, m, ids) of an id-path encoder call: the token table, its mask and the rows -- or, with input dropout active
        (train mode, p_dropout > 0), the dense dropped rows of `ids`, their mask rows and None: the personalized encoder
        takes dense rows as it is, and a gathered row cannot be dropped out inside its load."""
        tx, tm = store.text('title_emb')
        if self.training and self.dropout.p > 0:
            xd, md = ops.id_path_dropout(tx, tm, ids, self.dropout.p)
            return xd, md.reshape(ids.numel(), -1), None
        return tx, tm, ids

    def forward_store(self, store, hist_ids: torch.Tensor, cand_ids: torch.Tensor, uid: torch.Tensor):
        """forward() with the news as rows of a NewsStore (hist_ids:(B,nh), cand_ids:(B,nc), uid:(B,) or (B,1)); history and
        candidates go through ONE encoder call."""
        Q = self.queries(uid)
        dev = self._device()
        (b, nh), nc = hist_ids.shape, cand_ids.shape[1]
        ids = torch.cat([hist_ids.reshape(-1), cand_ids.reshape(-1)]).to(torch.int32)
        q_idx = torch.cat([_index_rows(b, nh, dev), _index_rows(b, nc, dev)])
        tx, tm, ids = self._id_path_rows(store, ids)
        y, hm = self.encode_news(tx, tm, ids, Q[:, :HIDDEN], q_idx)
        e = y.shape[1]
        u = self.encode_user(y[:b * nh].reshape(b, nh, e), hm[:b * nh].reshape(b, nh), Q[:, HIDDEN:])
        return self.rec_model(u.reshape(b, 1, e), y[b * nh:].reshape(b, nc, e))

    def score_impressions(self, store, hist_rows: torch.Tensor, cand_rows: torch.Tensor, cand_sess: torch.Tensor,
                          uid: torch.Tensor, relu: bool = True) -> torch.Tensor:
        """Evaluation hook (xnrs_amd.evaluation.evaluate): a batch of impressions with CSR candidate lists.  The history is
        encoded with q_idx = s / l_hist, the candidates with q_idx = their impression; then the user tower and the model's
        scorer (prepare_csr on the batch's candidate vectors, score_csr).  -> r:(n_cand,)."""
        Q = self.queries(uid)
        dev = self._device()
        b, nh = hist_rows.shape
        n = cand_rows.numel()
        ids = torch.cat([hist_rows.reshape(-1), cand_rows.reshape(-1)]).to(torch.int32)
        q_idx = torch.cat([_index_rows(b, nh, dev), cand_sess.to(torch.int32)])
        tx, tm, ids = self._id_path_rows(store, ids)
        y, hm = self.encode_news(tx, tm, ids, Q[:, :HIDDEN], q_idx)
        e = y.shape[1]
        u = self.encode_user(y[:b * nh].reshape(b, nh, e), hm[:b * nh].reshape(b, nh), Q[:, HIDDEN:])
        table = self.rec_model.prepare_csr(y[b * nh:])
        rows = torch.arange(n, device=dev, dtype=torch.int32)
        return self.rec_model.score_csr(table, rows, cand_sess.to(torch.int32), u, relu=relu)


def make_npa(cfg):
    """make_model.py:15-56 for cfg.model == 'NPA': the scorer first, then the model (the reference's order)."""
    from .assemblies import _scorer
    if cfg.model != 'NPA':
        raise ValueError(f'make_npa: cfg.model is {cfg.model!r}')
    return NPA(cfg, _scorer(cfg))
