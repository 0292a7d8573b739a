"""LSTUR (xnrs/models/full_models/lstur.py:9-159) on the HIP path: the news encoder of assemblies.LSTURNewsEncoder and the
user tower -- a one-layer GRU over the first st_hist_len history vectors, seeded with ('ini') or concatenated to ('con') a
long-term user vector (a user-table row, or the masked mean of the whole history through a head).  Same constructor
signatures, submodule registration order and state_dict keys as the reference; the parameters live in a real nn.GRU /
nn.Embedding, so under the same torch.manual_seed every parameter starts at the reference's value.

Deliberately NOT exported from xnrs_amd.models.components.*; the model is opt-in like NPA: install(hip_models=("LSTUR",)).

Per step: the news encoder over history and candidates, the long-term vector (one row gather, or the mean-pooling user
encoder), the GRU (ops.gru: one input-projection GEMM + the recurrence kernels of csrc/gru.hip), the model's scorer.  The
history lengths are counted on the device (the reference's .cpu() at lstur.py:141 is not reproduced); a user with an empty
short-term history keeps the initial state instead of raising in pack_padded_sequence.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import hip, ops
from .assemblies import LSTURNewsEncoder
from .blocks import MaskedMean, UserEncoder
from .npa import _checked_uids

LONG_TERM = ("mean", "embedding")
COMBINE = ("ini", "con", "lt_only")


class LSTURUserEncoder(nn.Module):
    """lstur.py:83-159.  forward((h:(B,N,E), hm:(B,N,1)), user_ids:(B,1)) -> (B,1,E)."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        long_term_emb_dim = cfg.total_emb_dim
        if cfg.long_short_term_method == 'con':
            long_term_emb_dim //= 2
        if cfg.long_term_method == 'embedding':
            self.long_term_encoder = nn.Embedding(num_embeddings=cfg.n_users + 1, embedding_dim=long_term_emb_dim, padding_idx=0)
        elif cfg.long_term_method == 'mean':
            # (the head of user_encoding.UserEncoder maps emb_dim -> emb_dim; out_dim is accepted and ignored, lstur.py:101-109)
            self.long_term_encoder = UserEncoder(pooler=MaskedMean(), att=None, head=True, emb_dim=cfg.total_emb_dim,
                                                 out_dim=long_term_emb_dim, p_dropout=cfg.p_dropout, bias=cfg.bias)
        else:
            raise ValueError(f'long_term_method must be in [mean, embedding], got {cfg.long_term_method}')
        self.dropout = nn.Dropout(p=cfg.p_user_dropout)
        self.gru = nn.GRU(cfg.total_emb_dim, long_term_emb_dim, batch_first=True)

    def _device(self):
        return self.gru.weight_ih_l0.device

    def long_term(self, h: torch.Tensor, hm: torch.Tensor, user_ids: Optional[torch.Tensor]) -> torch.Tensor:
        """u_lt:(B, long-term width) after the user dropout (lstur.py:130-135)."""
        if self.cfg.long_term_method == 'mean':
            u_lt = self.long_term_encoder((h, hm)).squeeze(1)
        else:
            if user_ids is None:
                raise hip.XnrsHipError("LSTUR (long_term_method 'embedding'): the user index of every row is required")
            if not user_ids.is_cuda:
                raise hip.XnrsHipError("LSTUR: user indices must live on the HIP device")
            table = self.long_term_encoder
            u_lt = ops.embedding_rows(_checked_uids(user_ids, table.num_embeddings), table.weight, table.padding_idx)
        return self.dropout(u_lt)

    def forward(self, history_features, user_ids: Optional[torch.Tensor] = None):
        cfg = self.cfg
        how = cfg.long_short_term_method
        if how not in COMBINE:
            raise ValueError(f'invalid value for long_short_term_method, got {how}')
        dev = self._device()
        if dev.type != "cuda":
            raise hip.XnrsHipError(f"LSTUR: the module is on {dev}; xnrs_amd runs on a HIP device only (there is no CPU fallback)")
        h, hm = (t.to(dev) for t in history_features)
        if how == 'con' and cfg.long_term_method == 'mean':
            hd, e = self.gru.hidden_size, cfg.total_emb_dim
            raise hip.XnrsHipError(
                f"LSTUR (long_term_method 'mean', long_short_term_method 'con'): the user vector would have {hd + e} columns "
                f"(GRU state {hd} + long-term vector {e}: the mean encoder's head maps emb_dim -> emb_dim, not -> out_dim) "
                f"against news vectors of {e}; the reference fails the same way at scoring (lstur.py:99-109,151-154)")
        u_lt = self.long_term(h, hm, None if user_ids is None else user_ids.to(dev))
        if how == 'lt_only':
            return u_lt.unsqueeze(1)
        st = cfg.st_hist_len
        # the first st slots of every history; the GRU reads the first sum(hm[:, :st]) of them (lstur.py:139-145)
        u_st = ops.gru(h[:, :st], hm, u_lt if how == 'ini' else None, self.gru)
        if how == 'ini':
            return u_st.unsqueeze(1)
        return torch.cat((u_st, u_lt), dim=1).unsqueeze(1)  # (concatenation: data movement only)


class LSTUR(nn.Module):
    """lstur.py:9-79.  forward(batch) on the reference's batch dict; forward_store(store, hist_ids, cand_ids, uid) with the
    news given as rows of a device-resident NewsStore."""

    @property
    def uses_user_index(self) -> bool:
        """evaluate() hands encode_user the user index of every session when the long-term vector is a row of the user table."""
        return self.cfg.long_term_method == 'embedding'

    def __init__(self, cfg, rec_model):
        super().__init__()
        self.news_encoder = LSTURNewsEncoder(cfg)
        self.user_encoder = LSTURUserEncoder(cfg)
        self.rec_model = rec_model
        self.cfg = cfg

    def _subcats(self, batch):
        if 'subcategory_index' in self.cfg.catg_features:
            return (batch['user_features']['history']['subcategory_index'], batch['candidate_features']['subcategory_index'])
        return None, None

    def _forward(self, user_ids, hist_title_features, cand_title_features, hist_cat_idxs, cand_cat_idxs,
                 hist_subcat_idxs=None, cand_subcat_idxs=None, return_embeddings: bool = False):
        h, hm = self.news_encoder(title_features=hist_title_features, cat_idxs=hist_cat_idxs, subcat_idxs=hist_subcat_idxs)
        c, _ = self.news_encoder(title_features=cand_title_features, cat_idxs=cand_cat_idxs, subcat_idxs=cand_subcat_idxs)
        u = self.user_encoder((h, hm), user_ids)
        r = self.rec_model(u, c)
        return (r, u, c) if return_embeddings else r

    def forward(self, batch: dict, return_embeddings: bool = False):
        hs, cs = self._subcats(batch)
        return self._forward(user_ids=batch['user_features']['other']['user_index'],
                             hist_title_features=batch['user_features']['history']['title_emb'],
                             cand_title_features=batch['candidate_features']['title_emb'],
                             hist_cat_idxs=batch['user_features']['history']['category_index'],
                             cand_cat_idxs=batch['candidate_features']['category_index'],
                             hist_subcat_idxs=hs, cand_subcat_idxs=cs, return_embeddings=return_embeddings)

    def get_user_embeddings(self, batch: dict) -> torch.Tensor:
        """lstur.py:65-79 -> (B, E)."""
        hs, _ = self._subcats(batch)
        h, hm = self.news_encoder(title_features=batch['user_features']['history']['title_emb'],
                                  cat_idxs=batch['user_features']['history']['category_index'], subcat_idxs=hs)
        return self.user_encoder((h, hm), batch['user_features']['other']['user_index']).squeeze(1)

    # ---- device data path (the hooks of xnrs_amd.evaluation.evaluate: the news vectors do not depend on the user, so the
    # news table is encoded once per epoch)
    def encode_news_ids(self, store, ids: torch.Tensor, dedup: bool = False):
        return self.news_encoder.forward_ids(store, ids, dedup=dedup)

    def encode_user(self, h: torch.Tensor, hm: torch.Tensor, uid: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self.user_encoder((h, hm), None if uid is None else uid.reshape(-1, 1))

    def forward_store(self, store, hist_ids: torch.Tensor, cand_ids: torch.Tensor, uid: Optional[torch.Tensor] = None,
                      return_embeddings: bool = False):
        """forward() with the batch given as table rows of a NewsStore (hist_ids:(B,nh), cand_ids:(B,nc), uid:(B,) or (B,1))."""
        h, hm = self.encode_news_ids(store, hist_ids)
        c, _ = self.encode_news_ids(store, cand_ids)
        u = self.encode_user(h, hm, uid)
        r = self.rec_model(u, c)
        return (r, u, c) if return_embeddings else r


def make_lstur(cfg):
    """make_model.py:15-56 for cfg.model == 'LSTUR': the scorer first, then the model (the reference's order)."""
    from .assemblies import _scorer
    if cfg.model != 'LSTUR':
        raise ValueError(f'make_lstur: cfg.model is {cfg.model!r}')
    return LSTUR(cfg, _scorer(cfg))
