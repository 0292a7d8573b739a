"""CAUM (xnrs/models/full_models/caum.py:11-172) on the HIP path: the one model whose user vector depends on the candidate.
Same constructor signatures, submodule registration order and state_dict keys as the reference; the parameters live in real
nn.Linear / nn.Embedding / nn.MultiheadAttention modules that are never called, so under the same torch.manual_seed every
parameter starts at the reference's value.

Per step: the news encoder over history and candidates (multi-head self-attention + additive pooling + head, concatenated
with the category encoders), the candidate-aware user tower (ops.caum_user: two small projections, the pair broadcast,
long attention, the dense candidate attention and its pooling -- csrc/caum.hip), the per-candidate scorer.

Attention geometry (reproduced, not fixed): caum.py:52-54 builds nn.MultiheadAttention WITHOUT batch_first and caum.py:91-92
calls it on a (B*n_c, n_h, d) view, so the attended sequence is the batch x candidate axis and the "batch" is the history
slot.  One impression's scores therefore depend on the other impressions of the batch, and evaluate() cannot encode users
once per epoch for this model.

Not routed by make_model / install(): the public routes are xnrs_amd.models.CAUM and make_caum(cfg).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import hip, ops
from .blocks import AdditiveAttention, DotScoring, MultiHeadAttention, TextEncoder


class DenseAttention(nn.Module):
    """layers.py:159-175: Linear(in, h1) - tanh - Linear(h1, h2) - tanh - Linear(h2, 1).  A parameter holder here: CAUM's
    tower splits `linear` into its h_all and candidate halves (ops.caum_user); forward() serves a plain (..., in) input."""

    def __init__(self, input_dim: int, hidden_dim1: int, hidden_dim2: int):
        super().__init__()
        self.linear = nn.Linear(input_dim, hidden_dim1)
        self.tanh1 = nn.Tanh()
        self.linear2 = nn.Linear(hidden_dim1, hidden_dim2)
        self.tanh2 = nn.Tanh()
        self.linear3 = nn.Linear(hidden_dim2, 1)

    def forward(self, x: torch.Tensor):
        t = ops.linear(x, self.linear.weight, self.linear.bias, hip.ACT_TANH)
        t = ops.linear(t, self.linear2.weight, self.linear2.bias, hip.ACT_TANH)
        return ops.linear(t, self.linear3.weight, self.linear3.bias)


class CategoryEncoder(nn.Module):
    """news_encoding.py:63-91: embedding -> Linear(Ec, Ec) -> relu, as one row-gathered GEMM with the relu in its epilogue.
    `activation`: torch.relu (the reference's default) or None."""

    def __init__(self, n_categories: int, embedding_dim: int, head: bool = True, activation=torch.relu):
        super().__init__()
        if activation is not None and activation is not torch.relu:
            raise NotImplementedError(f"CategoryEncoder activation {activation!r}: the HIP path implements torch.relu and None")
        self.embedding = nn.Embedding(num_embeddings=n_categories + 1, embedding_dim=embedding_dim)
        if head:
            self.linear = nn.Linear(in_features=embedding_dim, out_features=embedding_dim)
        if activation is not None:
            self.activation = activation

    def forward(self, x: torch.Tensor):
        dev = self.embedding.weight.device
        if dev.type != "cuda":
            raise hip.XnrsHipError(f"CategoryEncoder: the module is on {dev}; xnrs_amd runs on a HIP device only")
        if not hasattr(self, 'linear'):
            raise NotImplementedError("CategoryEncoder(head=False) has no HIP implementation (CAUM builds it with head=True)")
        act = hip.ACT_RELU if hasattr(self, 'activation') else hip.ACT_NONE
        return ops.embedding_linear(x.to(dev), self.embedding, self.linear, act)


class CAUMScoring(DotScoring):
    """scoring.py:26-38: u:(B,N,D) candidate-aware user vectors, c:(B,N,D) -> (B,N,1), r[b,i] = u[b,i] . c[b,i] (the diagonal
    of DotScoring's product; `normalize` as in DotScoring)."""

    def forward(self, u: torch.Tensor, c: torch.Tensor):
        return ops.diag_scoring(u, c, self.normalize)

    # no once-per-epoch news table: CAUM's user vector depends on the candidates (and, through the attention axis, on the
    # batch), so evaluation.evaluate() raises NotImplementedError for this scorer before it encodes anything
    prepare_csr = None
    score_csr = None
    topk = None
    topk_sample = None
    rank = None
    table_loss = None
    list_loss = None
    list_xent = None


class CAUMNewsEncoder(nn.Module):
    """caum.py:114-172: TextEncoder(multi-head self-attention, additive pooler with hidden = title_emb_dim, head) (+)
    CategoryEncoder of the category [(+) of the sub-category when cfg.catg_features lists it]."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        title_pooler = AdditiveAttention(in_features=cfg.d_backbone, hidden_features=cfg.title_emb_dim)
        title_att = MultiHeadAttention(n_heads=cfg.n_heads, d_model=cfg.d_backbone)
        self.title_encoder = TextEncoder(pooler=title_pooler, att=title_att, p_dropout=cfg.p_dropout,
                                         out_features=cfg.title_emb_dim, in_features=cfg.d_backbone, head=True, bias=cfg.bias)
        self.cat_embedder = CategoryEncoder(n_categories=cfg.n_categories, embedding_dim=cfg.cat_emb_dim)
        if 'subcategory_index' in cfg.catg_features:
            self.subcat_embedder = CategoryEncoder(n_categories=cfg.n_subcategories, embedding_dim=cfg.cat_emb_dim)

    def _concat(self, emb, cat_idxs, subcat_idxs):
        parts = [emb, self.cat_embedder(cat_idxs)]
        if subcat_idxs is not None:
            assert hasattr(self, 'subcat_embedder')
            parts.append(self.subcat_embedder(subcat_idxs))
        return torch.cat(parts, dim=2)  # (concatenation: data movement only)

    def _forward(self, title_emb, cat_idxs: torch.Tensor, subcat_idxs: Optional[torch.Tensor]):
        emb, m = self.title_encoder(title_emb)
        return self._concat(emb, cat_idxs, subcat_idxs), m

    def forward(self, news_features: dict):
        return self._forward(title_emb=news_features['title_emb'], cat_idxs=news_features['category_index'],
                             subcat_idxs=news_features.get('subcategory_index'))

    def forward_ids(self, store, ids: torch.Tensor, dedup: bool = False):
        """forward() by table rows `ids:(B,N)` of a NewsStore: tokens gathered in the first GEMM's load, the category
        columns looked up by the same rows."""
        emb, m = self.title_encoder.forward_ids(*store.text('title_emb'), ids, dedup=dedup)
        rows = ids.long()
        sub = store.column('subcategory_index')[rows] if hasattr(self, 'subcat_embedder') else None
        return self._concat(emb, store.column('category_index')[rows], sub), m


class CAUMUserEncoder(nn.Module):
    """caum.py:31-111.  forward((h:(B,H,E), hm), (c:(B,C,E), cm)) -> u:(B,C,E), one user vector per candidate; the masks are
    accepted and ignored exactly like the reference (no stage of the tower is masked).

    The self-attention runs along the batch x candidate axis (nn.MultiheadAttention without batch_first on a (B*C, H, E)
    view, caum.py:52-54,91-92): reproduced, so a row's output depends on the batch it is in."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        e = cfg.total_emb_dim
        self.dropout1 = nn.Dropout(p=cfg.p_dropout)
        self.dropout2 = nn.Dropout(p=cfg.p_dropout)
        self.dropout3 = nn.Dropout(p=cfg.p_dropout)
        self.linear1 = nn.Linear(in_features=e * 4, out_features=e)
        self.linear2 = nn.Linear(in_features=e * 2, out_features=e)
        self.linear3 = nn.Linear(in_features=e + e, out_features=e)
        self.dense_att = DenseAttention(input_dim=e * 2, hidden_dim1=e, hidden_dim2=e // 2)
        self.multihead_attention = nn.MultiheadAttention(embed_dim=e, num_heads=cfg.n_heads)

    def forward(self, history_features, cand_features):
        dev = self.linear1.weight.device
        if dev.type != "cuda":
            raise hip.XnrsHipError(f"CAUM: the module is on {dev}; xnrs_amd runs on a HIP device only (there is no CPU fallback)")
        h, c = history_features[0], cand_features[0]
        return ops.caum_user(h.to(dev), c.to(dev), self)


class CAUM(nn.Module):
    """caum.py:11-28.  forward(batch) on the reference's batch dict -> r:(B,C,1) [, u:(B,C,E), c:(B,C,E)];
    forward_store(store, hist_ids, cand_ids) with the news given as rows of a device-resident NewsStore.

    Its self-attention attends along the batch x candidate axis (see CAUMUserEncoder): scores depend on the batch
    composition, as in the reference."""

    def __init__(self, cfg, rec_model: nn.Module):
        super().__init__()
        self.cfg = cfg
        self.news_encoder = CAUMNewsEncoder(cfg)
        self.user_encoder = CAUMUserEncoder(cfg)
        self.rec_model = rec_model

    def _score(self, h, hm, c, cm, return_embeddings):
        u = self.user_encoder((h, hm), (c, cm))
        r = self.rec_model(u, c)  # (the scorer reads the candidate vectors BEFORE the tower's dropout1)
        return (r, u, c) if return_embeddings else r

    def forward(self, batch: dict, return_embeddings: bool = False):
        h, hm = self.news_encoder(batch['user_features']['history'])
        c, cm = self.news_encoder(batch['candidate_features'])
        return self._score(h, hm, c, cm, return_embeddings)

    def forward_store(self, store, hist_ids: torch.Tensor, cand_ids: torch.Tensor, return_embeddings: bool = False):
        h, hm = self.news_encoder.forward_ids(store, hist_ids)
        c, cm = self.news_encoder.forward_ids(store, cand_ids)
        return self._score(h, hm, c, cm, return_embeddings)

    def encode_news_ids(self, store, ids: torch.Tensor, dedup: bool = False):
        return self.news_encoder.forward_ids(store, ids, dedup=dedup)

    def encode_user(self, *args, **kwargs):
        raise NotImplementedError("CAUM has no candidate-independent user vector: evaluate() cannot encode users once per "
                                  "epoch (and the attention axis makes scores depend on the batch); score with forward_store")


def make_caum(cfg):
    """make_model.py:15-56 for cfg.model == 'CAUM': the scorer first, then the model (the reference's order)."""
    from .assemblies import _scorer
    if cfg.model != 'CAUM':
        raise ValueError(f'make_caum: cfg.model is {cfg.model!r}')
    scorer = CAUMScoring() if cfg.scoring == 'CAUMScoring' else _scorer(cfg)
    return CAUM(cfg, scorer)
