"""Loss kernels next to the hot path: the in-batch InfoNCE "theme" contrastive loss of
ContrastiveRankingTrainer._compute_contrastive_loss (xnrs/training.py:433-472) as ONE fused HIP forward +
ONE fused backward instead of a Python loop over the batch rows; and the full-table softmax ranking loss -- the reference's
ranking_loss (xnrs/utils.py:117-131) with every eligible news of the table as a negative -- over the sweep of
recommend() / rank_clicked(), without a (sessions, n_rows) score matrix (table_ranking_loss, full_table_loss); and the same
loss over per-session row lists, the hardest negatives mined by topk_deep per step or any list the caller brings, without a
copy of the listed rows (listed_ranking_loss, mined_negatives_loss)."""
from __future__ import annotations

import torch

from . import hip


class _InfoNCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, labels, temperature):
        emb = hip.dev_f32(emb, "embeddings")
        B, E = emb.shape
        labels = labels.to(device=emb.device, dtype=torch.int64).contiguous()
        l = hip.lib()
        nsaved = l.xnrs_infonce_saved_bytes(B, E)
        saved = torch.empty(nsaved, dtype=torch.uint8, device=emb.device)
        loss = torch.empty((), dtype=torch.float32, device=emb.device)
        hip.check(l.xnrs_infonce_fwd(hip.ptr(emb), hip.ptr(labels), B, E, float(temperature), hip.ptr(loss), hip.ptr(saved),
                                     nsaved, hip.stream_ptr(emb.device)), "xnrs_infonce_fwd")
        ctx.save_for_backward(labels, saved)
        ctx.shape, ctx.temperature, ctx.nsaved = (B, E), float(temperature), nsaved
        return loss

    @staticmethod
    def backward(ctx, g):
        labels, saved = ctx.saved_tensors
        B, E = ctx.shape
        g = hip.dev_f32(g.reshape(1), "upstream gradient")
        demb = torch.empty((B, E), dtype=torch.float32, device=saved.device)
        hip.check(hip.lib().xnrs_infonce_bwd(hip.ptr(labels), B, E, ctx.temperature, hip.ptr(saved), ctx.nsaved, hip.ptr(g),
                                             hip.ptr(demb), hip.stream_ptr(saved.device)), "xnrs_infonce_bwd")
        return demb, None, None


def contrastive_loss(embeddings: torch.Tensor, labels: torch.Tensor, temperature: float) -> torch.Tensor:
    """Drop-in for ContrastiveRankingTrainer._compute_contrastive_loss(embeddings:(B,E)|(B,1,E), labels:(B,)).
    (The `if embeddings.dim() > 2: view(B, -1)` of training.py:442-443 is kept for NAML's (B,1,E).)"""
    if embeddings.dim() > 2:
        embeddings = embeddings.reshape(embeddings.size(0), -1)
    return _InfoNCE.apply(embeddings, labels, temperature)


def _table_loss_scorer(scorer, who: str):
    fn = getattr(scorer, "table_loss", None)
    if fn is None:
        raise NotImplementedError(f"{who}: the scorer {type(scorer).__name__} has no full-table loss over a news table "
                                  "(table_loss); training it with a plain dot product would train another model")
    return fn


def reduce_table_loss(loss: torch.Tensor, scores: torch.Tensor, reduction: str) -> torch.Tensor:
    """'none': the loss per query; 'sum'; 'mean': the sum over the number of queries that have an answer (scores not NaN),
    counted on the device, 0 when there are none."""
    if reduction == "none":
        return loss
    if reduction == "sum":
        return loss.sum()
    if reduction == "mean":
        n = (~torch.isnan(scores)).sum()
        return loss.sum() / n.clamp(min=1).to(loss.dtype)
    raise ValueError(f"reduction {reduction!r}: 'mean', 'sum' or 'none'")


def table_ranking_loss(scorer, table: torch.Tensor, u: torch.Tensor, tgt_off: torch.Tensor, tgt_rows: torch.Tensor,
                       excl_off=None, excl_rows=None, pad_row: int = -1, win_lo=None, win_hi=None,
                       reduction: str = "mean") -> torch.Tensor:
    """ranking_loss(p, n) = -log(e^p / (e^p + sum e^n)) of every (user, target row) of the CSR tgt_off / tgt_rows with ALL
    eligible rows of `table` as the negatives n (include/xnrs_hip.h: xnrs_table_loss_fwd): the rows rank() counts -- not
    pad_row, not on the user's exclusion list, inside the user's window -- minus every target of the user.  `scorer`: a
    DotScoring or BilinScoring (scorer.table_loss); differentiable in `table`, `u` and the scorer's weight.  A query without
    an answer (a target outside the table, the pad row) and a user without negatives contribute 0."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"reduction {reduction!r}: 'mean', 'sum' or 'none'")
    fn = _table_loss_scorer(scorer, "table_ranking_loss()")
    loss, scores, _ = fn(table, u, tgt_off, tgt_rows, excl_off, excl_rows, pad_row, win_lo=win_lo, win_hi=win_hi)
    return reduce_table_loss(loss, scores, reduction)


def _refuse_before_encoding(model, behaviors, reduction: str, who: str, scorer_of, loss_name: str):
    """What full_table_loss() and mined_negatives_loss() refuse before anything is encoded -> (scorer, user index or None).
    scorer_of(scorer, who) raises for a scorer without the loss; loss_name words the normalize=True refusal."""
    if getattr(model, "user_dependent_news", False):
        raise NotImplementedError(f"{who}: the news vectors of {type(model).__name__} depend on the user, so no table of "
                                  "news vectors exists to rank")
    scorer = getattr(model, "rec_model", None)
    scorer_of(scorer, who)
    if getattr(scorer, "normalize", False):
        raise NotImplementedError(f"{who}: {type(scorer).__name__}(normalize=True) has no {loss_name}")
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"reduction {reduction!r}: 'mean', 'sum' or 'none'")
    uidx = None
    if getattr(model, "uses_user_index", False):
        uidx = getattr(behaviors, "user_index", None)
        if uidx is None:
            raise ValueError(f"{who}: {type(model).__name__} needs the user index of every session (sessions without "
                             "'user_index': Behaviors.from_sessions keeps it when every session carries it)")
    return scorer, uidx


def _encode_sessions(model, store_or_table, behaviors, sessions, l_hist: int, exclude_history: bool, windows, store, uidx,
                     who: str):
    """The shared path of both losses from the table to the user vectors, with autograd on -> (vecs, u, hist_csr, tgt_csr,
    (win_lo, win_hi), pad_row): the table is encoded (a NewsStore) or taken as given (a pair with store=), the sessions' last
    `l_hist` history rows are gathered from it, model.encode_user gives u; hist_csr is the exclusion CSR of the sessions'
    FULL histories ((None, None) without `exclude_history`), tgt_csr their clicked rows, the windows those of the sessions."""
    from . import evaluation as EV
    if isinstance(store_or_table, (tuple, list)):
        vecs, hm = store_or_table
        if store is None:
            raise ValueError(f"{who}: a pre-encoded table comes with store= (its pad row and the history batcher's)")
    else:
        store = store_or_table
        ids = torch.arange(store.n_rows, dtype=torch.int32, device=store.x.device).reshape(1, -1)
        y, m = model.encode_news_ids(store, ids)  # (encode_news_table without its no_grad)
        vecs, hm = y[0], m[0]
    dev = vecs.device
    windows = EV._session_windows(windows, behaviors, dev, who)
    sess = torch.as_tensor(sessions, dtype=torch.int64, device=dev)
    hist = EV.DeviceBatcher(behaviors, l_hist, store.pad_row).eval_batch(sess)[0]
    h = _gather_rows(vecs, hist)
    m = hm[hist.long()]
    u = model.encode_user(h, m) if uidx is None else model.encode_user(h, m, uidx.to(dev)[sess])
    excl = EV._history_csr(behaviors, sess, None) if exclude_history else (None, None)
    tgt = EV._session_csr(behaviors.pos_off, behaviors.pos_val, sess, None)
    win = (None, None) if windows is None else (windows[0][sess].contiguous(), windows[1][sess].contiguous())
    return vecs, u, excl, tgt, win, store.pad_row


def full_table_loss(model, store_or_table, behaviors, sessions, l_hist: int, exclude_history: bool = True, windows=None,
                    reduction: str = "mean", store=None) -> torch.Tensor:
    """The full-table ranking loss of one batch of sessions, on the path of recommend() / rank_clicked() with autograd on:
    the sessions' last `l_hist` history rows are gathered from the table of news vectors, model.encode_user gives the user
    vectors, every clicked news of a session (pos_off / pos_val) is a query, the session's FULL history is excluded
    (`exclude_history`) and `windows` = (lo, hi) indexed by session id restrict the negatives as in rank_clicked().

    store_or_table: a NewsStore -- the table is encoded here, under autograd, so the news encoder trains too -- or a pair
    (vecs:(n_rows,E), hm:(n_rows,1)) as encode_news_table returns it, together with `store` (its pad row): a detached pair
    trains the user tower (and the scorer) only.  reduction 'mean' divides by the number of clicks that have an answer.
    A scorer without table_loss (FCScoring), a model whose news vectors depend on the user (NPA) and CAUM raise
    NotImplementedError before anything is encoded."""
    who = "full_table_loss()"
    scorer, uidx = _refuse_before_encoding(model, behaviors, reduction, who, _table_loss_scorer, "full-table loss")
    vecs, u, excl, tgt, win, pad_row = _encode_sessions(model, store_or_table, behaviors, sessions, l_hist, exclude_history,
                                                        windows, store, uidx, who)
    return table_ranking_loss(scorer, vecs, u, tgt[0], tgt[1], excl[0], excl[1], pad_row, win[0], win[1], reduction)


def _list_loss_scorer(scorer, who: str):
    fn = getattr(scorer, "list_loss", None)
    if fn is None:
        raise NotImplementedError(f"{who}: the scorer {type(scorer).__name__} has no ranking loss over listed rows of a news "
                                  "table (list_loss); training it with a plain dot product would train another model")
    return fn


def listed_ranking_loss(scorer, table: torch.Tensor, u: torch.Tensor, tgt_off: torch.Tensor, tgt_rows: torch.Tensor,
                        neg_rows: torch.Tensor, pad_row: int = -1, reduction: str = "mean") -> torch.Tensor:
    """ranking_loss(p, n) of every (user, target row) of the CSR tgt_off / tgt_rows with the rows the user LISTS in
    neg_rows:(B, L) int32 as the negatives n (include/xnrs_hip.h: xnrs_list_loss_fwd): a slot counts when its row is inside
    the table, not pad_row and no target of the user; -1 fillers and everything else are empty slots; a row listed twice
    counts twice.  `scorer`: a DotScoring or BilinScoring (scorer.list_loss); differentiable in `table`, `u` and the scorer's
    weight, without a copy of the listed rows.  Reduction as table_ranking_loss."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"reduction {reduction!r}: 'mean', 'sum' or 'none'")
    fn = _list_loss_scorer(scorer, "listed_ranking_loss()")
    loss, scores = fn(table, u, tgt_off, tgt_rows, neg_rows, pad_row)[:2]
    return reduce_table_loss(loss, scores, reduction)


def merged_exclusions(hist_csr, tgt_csr):
    """Per session its history list followed by its clicked rows, as one exclusion CSR (off int64, rows int32): what the
    mining step may not return.  hist_csr: (off, rows) or (None, None); both CSRs start at offset 0.  Device arithmetic
    only; the lists stay unsorted and may hold duplicates, which the exclusion lists of xnrs_topk* allow."""
    to, tr = tgt_csr
    ho, hr = hist_csr
    if ho is None:
        return to, tr
    nh, nt = hr.numel(), tr.numel()
    dev = tr.device
    rows = torch.empty((nh + nt,), dtype=torch.int32, device=dev)
    # history entry k of session b moves behind the clicks of the sessions before b, click k behind the histories up to b
    shift_h = torch.repeat_interleave(to[:-1], ho[1:] - ho[:-1], output_size=nh)
    shift_t = torch.repeat_interleave(ho[1:], to[1:] - to[:-1], output_size=nt)
    rows[torch.arange(nh, device=dev) + shift_h] = hr.to(torch.int32)
    rows[torch.arange(nt, device=dev) + shift_t] = tr.to(torch.int32)
    return ho + to, rows


def _check_neg_rows(neg_rows, n_sessions: int, who: str):
    if not isinstance(neg_rows, torch.Tensor) or neg_rows.dtype != torch.int32 or neg_rows.dim() != 2 \
            or neg_rows.shape[0] != n_sessions:
        raise ValueError(f"{who}: neg_rows is a ({n_sessions}, L) int32 tensor, one list of table rows per session; got "
                         f"{tuple(getattr(neg_rows, 'shape', ()))} {getattr(neg_rows, 'dtype', type(neg_rows))}")


def _check_sampling(temperature, seed, who: str):
    """temperature / seed of a loss whose negatives are drawn: a finite temperature above 0 comes with an integer seed."""
    import math
    if temperature is None:
        if seed is not None:
            raise ValueError(f"{who}: seed = {seed!r} without a temperature: the hardest negatives are not drawn")
        return
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not math.isfinite(temperature) or temperature <= 0:
        raise ValueError(f"{who}: temperature = {temperature!r}: a finite number above 0, or None for the hardest negatives")
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"{who}: seed = {seed!r}: drawn negatives need an integer seed; vary it per step")


def mine_and_rank(scorer, vecs, u, hist_csr, tgt_csr, pad_row: int, n_negatives: int, win=(None, None), reduction: str = "mean",
                  neg_rows=None, return_negatives: bool = False, temperature=None, seed=None, user_keys=None):
    """The part of mined_negatives_loss() behind the user vectors: without `neg_rows` the scorer's topk_deep lists, under
    no_grad and on detached operands, the n_negatives rows each user scores highest outside the merged exclusions (history
    and clicks) and inside the window; then the listed loss over those rows, under autograd.  With a `temperature` the lists
    are DRAWN instead (scorer.topk_sample: P(row first) ~ exp(score / temperature), without replacement) under the same
    exclusions and windows, from `seed` and the (B,) int64 `user_keys` (None: the user's index)."""
    if neg_rows is None:
        _check_sampling(temperature, seed, "mine_and_rank()")
        excl = merged_exclusions(hist_csr, tgt_csr)
        with torch.no_grad():
            kw = {} if win[0] is None else dict(win_lo=win[0], win_hi=win[1])
            if temperature is None:
                neg_rows = scorer.topk_deep(vecs.detach(), u.detach(), int(n_negatives), excl[0], excl[1], pad_row, **kw)[0]
            else:
                neg_rows = scorer.topk_sample(vecs.detach(), u.detach(), int(n_negatives), float(temperature), seed, user_keys,
                                              excl[0], excl[1], pad_row, **kw)[0]
    loss = listed_ranking_loss(scorer, vecs, u, tgt_csr[0], tgt_csr[1], neg_rows, pad_row, reduction)
    return (loss, neg_rows) if return_negatives else loss


def mined_negatives_loss(model, store_or_table, behaviors, sessions, l_hist: int, n_negatives: int = 128,
                         exclude_history: bool = True, windows=None, reduction: str = "mean", store=None, neg_rows=None,
                         return_negatives: bool = False, temperature=None, seed=None):
    """The ranking loss of one batch of sessions against the `n_negatives` HARDEST negatives of each -- the news of the whole
    table the session's user scores highest, mined per step -- instead of against the whole table: the path of
    full_table_loss() up to the user vectors (same arguments, same refusals, raised before anything is encoded), then
    scorer.topk_deep under no_grad over the detached table and user vectors, excluding the pad row, the session's clicked
    rows and (`exclude_history`) its full history, inside the session's window (`windows`); then the scorer's list_loss over
    the mined rows under autograd (xnrs_list_loss_fwd / _bwd: no copy of the listed rows).  The lists have the prefix
    property of topk_deep, so the loss does not decrease with n_negatives and meets full_table_loss() when every eligible
    row is listed.  1 <= n_negatives <= 1024, else ValueError.

    neg_rows: a (len(sessions), L) int32 tensor of table rows on the table's device skips the mining: stale lists reused
    over several steps, random sampled negatives.  A slot whose row is outside the table, the pad row or a click of its
    session is ignored (-1 is the filler).  return_negatives=True returns (loss, rows) with the lists that were used.

    temperature: the hardest rows are where the false negatives live; with a finite temperature > 0 the n_negatives rows are
    DRAWN instead, without replacement, P(row first) ~ exp(score / temperature) (scorer.topk_sample: Gumbel top-k inside the
    same sweep, the same exclusions and windows; the draws are keyed by the session ids).  `seed` (an integer) is then
    required, and the caller varies it per step -- the same seed draws the same lists.  The listed loss behind the lists is
    the same call.  temperature=None (the default) is the mining above, bit for bit."""
    who = "mined_negatives_loss()"
    scorer, uidx = _refuse_before_encoding(model, behaviors, reduction, who, _list_loss_scorer, "ranking loss over listed rows")
    n_sessions = int(torch.as_tensor(sessions).numel())
    if neg_rows is not None:
        _check_neg_rows(neg_rows, n_sessions, who)
    else:
        _check_sampling(temperature, seed, who)
        if temperature is not None and getattr(scorer, "topk_sample", None) is None:
            raise NotImplementedError(f"{who}: the scorer {type(scorer).__name__} has no topk_sample to draw negatives with")
        if isinstance(n_negatives, bool) or int(n_negatives) != n_negatives or not 1 <= int(n_negatives) <= 1024:
            raise ValueError(f"{who}: n_negatives = {n_negatives!r}: an integer in [1, 1024], the list lengths of topk_deep")
        if getattr(scorer, "topk_deep", None) is None:
            raise NotImplementedError(f"{who}: the scorer {type(scorer).__name__} has no topk_deep to mine negatives with")
    vecs, u, excl, tgt, win, pad_row = _encode_sessions(model, store_or_table, behaviors, sessions, l_hist, exclude_history,
                                                        windows, store, uidx, who)
    if neg_rows is None and temperature is not None:
        keys = torch.as_tensor(sessions, dtype=torch.int64, device=vecs.device).reshape(-1).contiguous()
        return mine_and_rank(scorer, vecs, u, excl, tgt, pad_row, n_negatives, win, reduction, None, return_negatives,
                             temperature, seed, keys)
    return mine_and_rank(scorer, vecs, u, excl, tgt, pad_row, n_negatives, win, reduction, neg_rows, return_negatives)


def _list_xent_scorer(scorer, who: str):
    fn = getattr(scorer, "list_xent", None)
    if fn is None:
        raise NotImplementedError(f"{who}: the scorer {type(scorer).__name__} has no soft-target loss over listed rows of a "
                                  "news table (list_xent); training it with a plain dot product would train another model")
    return fn


def listed_soft_target_loss(scorer, table: torch.Tensor, u: torch.Tensor, rows: torch.Tensor, weights: torch.Tensor,
                            pad_row: int = -1, reduction: str = "mean") -> torch.Tensor:
    """The listwise loss against SOFT targets: per user the cross-entropy between the weights:(B, L) float32 a caller gives
    the rows:(B, L) int32 the user lists and the softmax of the user's scores over the same slots (include/xnrs_hip.h:
    xnrs_list_xent_fwd) -- sum over the filled slots of w (lse - s).  Teacher scores through a softmax give distillation,
    graded labels ListNet.  A slot counts when its row is inside the table and not pad_row; -1 fillers and everything else
    are empty slots whose weight is ignored; a row listed twice is two slots.  `scorer`: a DotScoring or BilinScoring
    (scorer.list_xent); differentiable in `table`, `u` and the scorer's weight, without a copy of the listed rows.
    reduction 'mean' divides by the number of users with a filled slot, counted on the device (at least 1); 'sum'; 'none':
    the loss per user."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"reduction {reduction!r}: 'mean', 'sum' or 'none'")
    fn = _list_xent_scorer(scorer, "listed_soft_target_loss()")
    loss, lse = fn(table, u, rows, weights, pad_row)[:2]
    return _reduce_per_user(loss, lse, reduction)


def _reduce_per_user(loss: torch.Tensor, lse: torch.Tensor, reduction: str) -> torch.Tensor:
    if reduction == "none":
        return loss
    if reduction == "sum":
        return loss.sum()
    return loss.sum() / torch.isfinite(lse).sum().clamp(min=1).to(loss.dtype)


def _teacher_kind(teacher, who: str) -> str:
    """'table': a teacher that ranks a table of news vectors with its own user vector; 'impressions': one whose news vectors
    depend on the user and that scores listed impressions (NPA).  Anything else (CAUM) is refused."""
    if getattr(teacher, "user_dependent_news", False):
        if callable(getattr(teacher, "score_impressions", None)):
            return "impressions"
    else:
        scorer = getattr(teacher, "rec_model", None)
        if callable(getattr(scorer, "prepare_csr", None)) and callable(getattr(scorer, "score_csr", None)):
            return "table"
    raise NotImplementedError(f"{who}: the teacher {type(teacher).__name__} neither scores listed rows of a news table with a "
                              "user vector of its own (prepare_csr / score_csr of a dot, bilinear or fc scorer) nor has "
                              "score_impressions over news vectors that depend on the user")


def _teacher_scores(teacher, kind: str, store, behaviors, sess, l_hist: int, rows: torch.Tensor, teacher_table, t_uidx):
    """(B, L) raw scores the teacher gives the listed rows of each session, under no_grad; the score of an empty place (-1)
    means nothing."""
    from . import evaluation as EV
    B, L = rows.shape
    dev = rows.device
    hist = EV.DeviceBatcher(behaviors, l_hist, store.pad_row).eval_batch(sess)[0]
    csess = torch.arange(B, device=dev, dtype=torch.int32).repeat_interleave(L)
    spare = store.pad_row if store.pad_row >= 0 else 0  # what stands in for an empty place
    crows = torch.where(rows >= 0, rows, torch.full_like(rows, spare)).reshape(-1)
    if kind == "impressions":
        return teacher.score_impressions(store, hist, crows, csess, t_uidx.to(dev)[sess], relu=False).reshape(B, L)
    vecs, hm = EV.encode_news_table(teacher, store) if teacher_table is None else teacher_table
    h, m = vecs[hist.long()], hm[hist.long()]
    u = teacher.encode_user(h, m) if t_uidx is None else teacher.encode_user(h, m, t_uidx.to(dev)[sess])
    scorer = teacher.rec_model
    return scorer.score_csr(scorer.prepare_csr(vecs), crows, csess, u, relu=False).reshape(B, L)


def soft_targets(teacher_scores: torch.Tensor, filled: torch.Tensor, temperature: float = 1.0):
    """softmax(teacher_scores / temperature) over the filled slots -> (weights:(B, L) float32 with 0 in the empty slots and
    all zeros for a session without a filled slot, entropy:(B,) of those weights); no NaN."""
    z = (teacher_scores.float() / temperature).masked_fill(~filled, float("-inf"))
    z = z - z.max(dim=1, keepdim=True).values.clamp(min=torch.finfo(torch.float32).min)  # (-inf - -inf never happens)
    e = torch.where(filled, z.exp(), torch.zeros_like(z))
    w = e / e.sum(dim=1, keepdim=True).clamp(min=torch.finfo(torch.float32).tiny)
    entropy = -(w * torch.where(w > 0, w.log(), torch.zeros_like(w))).sum(dim=1)
    return w.contiguous(), entropy


def distillation_loss(student, teacher, store_or_table, behaviors, sessions, l_hist: int, pool: int = 128,
                      temperature: float = 1.0, exclude_history: bool = True, windows=None, reduction: str = "mean", store=None,
                      rows=None, teacher_table=None, return_lists: bool = False):
    """Distil a re-ranker into its candidate generator: per session KL(teacher || student) between the two models' softmax
    distributions over the `pool` rows the STUDENT lists for the session, so that the student's pool comes to hold what the
    teacher would put on top.  The path is that of mined_negatives_loss() up to the user vectors (same arguments, the
    student's refusals raised before anything is encoded); then

      the pool    : without `rows`, the student's topk_deep(pool) under no_grad over the detached table and user vectors,
                    excluding the pad row and (`exclude_history`) the session's full history, inside its window (`windows`).
                    The session's clicks are NOT excluded: they are what both models should rank high.  1 <= pool <= 1024.
      the teacher : scores exactly those rows under no_grad.  A teacher that ranks a table (a dot, bilinear or fc scorer:
                    prepare_csr / score_csr) encodes its own user vector from the same history batch and scores the rows of
                    ITS table -- encoded here, or given as teacher_table=(vecs, hm) as encode_news_table returns it: a
                    teacher is normally frozen, so encode its table ONCE and pass it to every step.  A teacher whose news
                    vectors depend on the user (NPA: user_dependent_news and score_impressions) scores the rows as the second
                    stage of recommend(generator=...) does; it needs a NewsStore and behaviors.user_index.
      the targets : softmax(teacher scores / temperature) over the filled slots, 0 in the empty ones.
      the loss    : the scorer's list_xent (xnrs_list_xent_fwd / _bwd: no copy of the listed rows) with the student's user
                    vector divided by `temperature` (its logits are its scores / temperature; a bias cancels), minus the
                    targets' entropy, which is constant in the student: KL per session, >= 0 up to rounding.

    reduction 'mean' divides by the number of sessions with a filled slot.  rows: a (len(sessions), L) int32 tensor of table
    rows skips the mining; return_lists=True returns (loss, rows) with the lists that were used -- one mining pass then
    serves this loss and mined_negatives_loss(neg_rows=...) in the same step (the mining is what such a step costs most).
    Raised before anything is encoded: everything mined_negatives_loss() refuses for the student; a temperature that is not
    a finite number above 0; a pool outside [1, 1024]; a teacher of neither kind (CAUM: no user vector of its own and no
    score_impressions)."""
    import math
    who = "distillation_loss()"
    scorer, uidx = _refuse_before_encoding(student, behaviors, reduction, who, _list_xent_scorer, "soft-target loss over listed rows")
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not math.isfinite(temperature) or temperature <= 0:
        raise ValueError(f"{who}: temperature = {temperature!r}: a finite number above 0")
    n_sessions = int(torch.as_tensor(sessions).numel())
    if rows is not None:
        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or rows.dim() != 2 or rows.shape[0] != n_sessions:
            raise ValueError(f"{who}: rows is a ({n_sessions}, L) int32 tensor, one list of table rows per session; got "
                             f"{tuple(getattr(rows, 'shape', ()))} {getattr(rows, 'dtype', type(rows))}")
    else:
        if isinstance(pool, bool) or int(pool) != pool or not 1 <= int(pool) <= 1024:
            raise ValueError(f"{who}: pool = {pool!r}: an integer in [1, 1024], the list lengths of topk_deep")
        if getattr(scorer, "topk_deep", None) is None:
            raise NotImplementedError(f"{who}: the scorer {type(scorer).__name__} has no topk_deep to list a pool with")
    kind = _teacher_kind(teacher, who)
    the_store = store if isinstance(store_or_table, (tuple, list)) else store_or_table
    if the_store is None:
        raise ValueError(f"{who}: a pre-encoded table comes with store= (its pad row and the history batcher's)")
    t_uidx = None
    if kind == "impressions" or getattr(teacher, "uses_user_index", False):
        t_uidx = getattr(behaviors, "user_index", None)
        if t_uidx is None:
            raise ValueError(f"{who}: the teacher {type(teacher).__name__} needs the user index of every session (sessions "
                             "without 'user_index': Behaviors.from_sessions keeps it when every session carries it)")
    vecs, u, excl, _, win, pad_row = _encode_sessions(student, store_or_table, behaviors, sessions, l_hist, exclude_history,
                                                      windows, store, uidx, who)
    dev = vecs.device
    sess = torch.as_tensor(sessions, dtype=torch.int64, device=dev).reshape(-1)
    with torch.no_grad():
        if rows is None:
            kw = {} if win[0] is None else dict(win_lo=win[0], win_hi=win[1])
            rows = scorer.topk_deep(vecs.detach(), u.detach(), int(pool), excl[0], excl[1], pad_row, **kw)[0]
        filled = (rows >= 0) & (rows < vecs.shape[0]) & (rows != pad_row)
        t = _teacher_scores(teacher, kind, the_store, behaviors, sess, l_hist, rows, teacher_table, t_uidx)
        weights, entropy = soft_targets(t, filled, float(temperature))
    xent, lse = _list_xent_scorer(scorer, who)(vecs, u * (1.0 / float(temperature)), rows, weights, pad_row)[:2]
    loss = _reduce_per_user(xent - entropy, lse, reduction)
    return (loss, rows) if return_lists else loss


def _gather_rows(vecs: torch.Tensor, hist: torch.Tensor) -> torch.Tensor:
    """vecs[hist]: through the project's row gather when the table carries a gradient (its backward scatters on the HIP
    path), a plain index otherwise."""
    if vecs.requires_grad and torch.is_grad_enabled():
        from . import ops
        return ops.embedding_rows(hist.reshape(-1), vecs).reshape(tuple(hist.shape) + (vecs.shape[1],))
    return vecs[hist.long()]
