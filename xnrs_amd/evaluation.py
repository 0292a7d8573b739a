"""Evaluation path on the device: the reference's test loop runs batch_size 1 and
re-encodes every candidate of every impression (xnrs/training.py:61-67,194-243); here every news is
encoded ONCE per epoch, impressions are scored as CSR candidate lists against those vectors, and the
per-impression metrics of xnrs/evaluation/metrics.py are computed by a HIP kernel."""
from __future__ import annotations

from typing import Dict

import torch

from . import hip
from .data import Behaviors, DeviceBatcher, NewsStore

METRIC_NAMES = ("ndcg@5", "ndcg@10", "rr", "ctr@1", "ctr@10", "auc", "acc", "rec", "prec")


def _dist_rank_world(distributed):
    """(rank, world, on) of the evaluation job: `distributed` None = the default process group when one with more than one
    rank exists, False = this process alone, True = the default group (must be initialised)."""
    import torch.distributed as dist
    if distributed is False or not (dist.is_available() and dist.is_initialized()):
        if distributed is True:
            raise RuntimeError("evaluate(distributed=True) needs an initialised torch.distributed process group")
        return 0, 1, False
    world = dist.get_world_size()
    return dist.get_rank(), world, world > 1


def sharded_mean(local_sums: torch.Tensor, n_total: int, on: bool) -> torch.Tensor:
    """Sum of the per-rank metric sums (ONE all-reduce, fp64) over the global number of impressions."""
    if on:
        import torch.distributed as dist
        dist.all_reduce(local_sums, op=dist.ReduceOp.SUM)
    return local_sums / max(int(n_total), 1)


@torch.no_grad()
def encode_news_table(model, store: NewsStore, rows_per_call: int = 0, rows=None):
    """All rows of the store through the model's news tower -> (vecs:(n_rows,E), hm:(n_rows,1)).  Row 0 (the
    empty slot) gets the tower's output for an all-padded news (head-bias leak, SURVEY.md finding 4).

    Works for every model on the path through its `encode_news_ids(store, ids)` hook (ParentRec: one TextEncoder over
    the title table; NAML: title + abstract tables and the two category columns, naml.py:76-107).  `rows_per_call`
    bounds the rows handed to one hook call (0 = all at once; the C ABI chunks its own workspace either way)."""
    r0, r1 = (0, store.n_rows) if rows is None else rows  # (rows: the slice of the table this rank encodes)
    n = r1 - r0
    step = max(n, 1) if rows_per_call <= 0 else int(rows_per_call)
    ys, hms = [], []
    for lo in range(r0, max(r1, r0 + 1), step):
        ids = torch.arange(lo, max(min(lo + step, r1), lo), dtype=torch.int32, device=store.x.device).reshape(1, -1)
        y, hm = model.encode_news_ids(store, ids)
        ys.append(y[0])
        hms.append(hm[0])
    return (ys[0], hms[0]) if len(ys) == 1 else (torch.cat(ys), torch.cat(hms))


def score_csr(vecs: torch.Tensor, cand_rows: torch.Tensor, cand_sess: torch.Tensor, u: torch.Tensor, relu: bool = True):
    vecs = hip.dev_f32(vecs, "news vectors")
    u = hip.dev_f32(u, "user vectors").reshape(-1, vecs.shape[1])
    r = torch.empty((cand_rows.numel(),), dtype=torch.float32, device=vecs.device)
    hip.check(hip.lib().xnrs_score_csr(hip.ptr(vecs), hip.ptr(cand_rows), hip.ptr(cand_sess), hip.ptr(u), hip.ptr(r),
                                       cand_rows.numel(), vecs.shape[1], int(relu), hip.stream_ptr(vecs.device)), "xnrs_score_csr")
    return r


def rank_metrics(scores: torch.Tensor, targets: torch.Tensor, cand_off: torch.Tensor):
    """-> (B, 9) tensor in METRIC_NAMES order (xnrs/evaluation/metrics.py:9-64 per impression)."""
    B = cand_off.numel() - 1
    out = torch.empty((B, len(METRIC_NAMES)), dtype=torch.float32, device=scores.device)
    hip.check(hip.lib().xnrs_rank_metrics(hip.ptr(hip.dev_f32(scores, "scores")), hip.ptr(hip.dev_f32(targets, "targets")),
                                          hip.ptr(cand_off), hip.ptr(out), B, hip.stream_ptr(scores.device)), "xnrs_rank_metrics")
    return out


def encode_news_table_sharded(model, store: NewsStore, rank: int, world: int):
    """Every rank encodes a contiguous slice of the table (the 6.6 TFLOP of a MIND-large corpus divide by the world size) and
    ONE all-gather hands every rank all vectors: rows padded to the largest slice, [vector | news mask] side by side."""
    import torch.distributed as dist
    from .distributed import shard_range
    lo, hi = shard_range(store.n_rows, rank, world)
    y, hm = encode_news_table(model, store, rows=(lo, hi)) if hi > lo else (None, None)
    sizes = [shard_range(store.n_rows, r, world) for r in range(world)]
    mx = max(b - a for a, b in sizes)
    dev = store.x.device
    E = model.encode_news_ids(store, torch.zeros((1, 1), dtype=torch.int32, device=dev))[0].shape[-1] if y is None else y.shape[-1]
    mine = torch.zeros((mx, E + 1), dtype=torch.float32, device=dev)
    if y is not None:
        mine[:hi - lo, :E] = y
        mine[:hi - lo, E:] = hm.reshape(-1, 1)
    out = torch.empty((world * mx, E + 1), dtype=torch.float32, device=dev)
    dist.all_gather_into_tensor(out, mine)
    both = torch.cat([out[r * mx:r * mx + (b - a)] for r, (a, b) in enumerate(sizes)])
    return both[:, :E].contiguous(), both[:, E:].contiguous()


def _evaluate_per_batch(model, store: NewsStore, behaviors: Behaviors, l_hist: int, batch: int, distributed) -> Dict[str, float]:
    """evaluate() for a model whose news vectors depend on the user (NPA: its title pooler's query is the user's embedding),
    so no table of news vectors exists: every impression batch encodes its own history and CSR candidates through the
    model's hook score_impressions(store, hist_rows, cand_rows, cand_sess, uid), then rank_metrics.  Under a process group
    every rank scores a contiguous block of the sessions (distributed.shard_range) and one fp64 all-reduce adds the sums.
    Runs under evaluate()'s torch.no_grad()."""
    uidx = getattr(behaviors, "user_index", None)
    if uidx is None:
        raise ValueError(f"evaluate(): {type(model).__name__} needs the user index of every session (sessions without "
                         "'user_index': Behaviors.from_sessions keeps it when every session carries it)")
    rank, world, on = _dist_rank_world(distributed)
    n = len(behaviors)
    s_lo, s_hi = 0, n
    if on:
        from .distributed import shard_range
        s_lo, s_hi = shard_range(n, rank, world)
    batcher = DeviceBatcher(behaviors, l_hist, store.pad_row)
    dev = behaviors.hist_off.device
    uidx = uidx.to(dev)
    sums = torch.zeros(len(METRIC_NAMES), dtype=torch.float64, device=dev)
    for lo in range(s_lo, s_hi, batch):
        sess = torch.arange(lo, min(lo + batch, s_hi), device=dev)
        hist, off, rows, csess, targets = batcher.eval_batch(sess)
        r = model.score_impressions(store, hist, rows, csess, uidx[sess], relu=True)
        sums += rank_metrics(r, targets, off).double().sum(0)
    mean = sharded_mean(sums, n, on)
    out = {k: float(v) for k, v in zip(METRIC_NAMES, mean.tolist())}
    hip.check_status(dev)
    return out


@torch.no_grad()
def evaluate(model, store: NewsStore, behaviors: Behaviors, l_hist: int, batch: int = 4096, distributed=None) -> Dict[str, float]:
    """Mean of the per-impression metrics over all sessions (training.py:245-303 aggregates the same way).

    With a torch.distributed process group of more than one rank (`distributed` None / True) the epoch is rank-sharded: the
    news table is encoded in slices (one all-gather of the vectors), every rank scores a contiguous block of the sessions
    (distributed.shard_range) and ONE fp64 all-reduce adds the metric sums -- every rank returns the same dict, equal to the
    single-process result up to the order of that final sum.  (The reference's test loop is one process, batch size 1:
    training.py:194-243.)

    Impressions are scored by the model's own scorer (`model.rec_model`) through its two evaluation hooks: prepare_csr(vecs)
    once per epoch over the (all-gathered) news table, score_csr(table, rows, sess, u, relu) per batch.  A scorer without
    them raises NotImplementedError."""
    scorer = getattr(model, "rec_model", None)
    prepare, score = getattr(scorer, "prepare_csr", None), getattr(scorer, "score_csr", None)
    if prepare is None or score is None:
        raise NotImplementedError(f"evaluate(): the scorer {type(scorer).__name__} has no CSR scoring path (prepare_csr / "
                                  "score_csr); scoring it with a plain dot product would report another model's metrics")
    if getattr(model, "user_dependent_news", False):
        return _evaluate_per_batch(model, store, behaviors, l_hist, batch, distributed)
    rank, world, on = _dist_rank_world(distributed)
    if on:
        from .distributed import shard_range
        vecs, hm = encode_news_table_sharded(model, store, rank, world)
        s_lo, s_hi = shard_range(len(behaviors), rank, world)
    else:
        vecs, hm = encode_news_table(model, store)
        s_lo, s_hi = 0, len(behaviors)
    table = prepare(vecs)  # once per epoch: the scorer's news-side work (identity for the plain dot product)
    batcher = DeviceBatcher(behaviors, l_hist, store.pad_row)
    dev = vecs.device
    uidx = None
    if getattr(model, "uses_user_index", False):  # (LSTUR: the user tower reads a row of its long-term table per session)
        uidx = getattr(behaviors, "user_index", None)
        if uidx is None:
            raise ValueError(f"evaluate(): {type(model).__name__} needs the user index of every session (sessions without "
                             "'user_index': Behaviors.from_sessions keeps it when every session carries it)")
        uidx = uidx.to(dev)
    sums = torch.zeros(len(METRIC_NAMES), dtype=torch.float64, device=dev)
    n = len(behaviors)
    for lo in range(s_lo, s_hi, batch):
        sess = torch.arange(lo, min(lo + batch, s_hi), device=dev)
        hist, off, rows, csess, targets = batcher.eval_batch(sess)
        h = vecs[hist.long()]            # (B, l_hist, E) row gather of pre-encoded vectors (data movement only)
        m = hm[hist.long()]
        u = model.encode_user(h, m) if uidx is None else model.encode_user(h, m, uidx[sess])
        r = score(table, rows, csess, u, relu=True)
        sums += rank_metrics(r, targets, off).double().sum(0)
    mean = sharded_mean(sums, n, on)
    out = {k: float(v) for k, v in zip(METRIC_NAMES, mean.tolist())}
    hip.check_status(dev)  # (the read above was the epoch's sync point: what the sync-free encoders could not raise, raises here)
    return out


def _session_csr(off: torch.Tensor, val: torch.Tensor, sess: torch.Tensor, first):
    """(off:(B+1) int64 absolute into rows, rows int32): the lists of the sessions out of the CSR (off, val).  A contiguous
    run of sessions from session `first` on (an int) is a slice of `off` over the whole `val` (no copy); any other selection
    (`first` None) gathers its lists."""
    if first is not None:
        return off[first:first + sess.numel() + 1], val
    start, n = off[sess], off[sess + 1] - off[sess]
    new_off = torch.zeros(sess.numel() + 1, dtype=torch.int64, device=off.device)
    torch.cumsum(n, 0, out=new_off[1:])
    idx = torch.arange(int(new_off[-1]), device=off.device) + torch.repeat_interleave(start - new_off[:-1], n)
    return new_off, val[idx]


def _history_csr(behaviors: Behaviors, sess: torch.Tensor, first):
    """The FULL histories of the sessions as an exclusion CSR (_session_csr of hist_off / hist_val)."""
    return _session_csr(behaviors.hist_off, behaviors.hist_val, sess, first)


TOPK_MAX_K, TOPK_DEEP_MAX_K = hip._CONSTANTS["TOPK_MAX_K"], hip._CONSTANTS["TOPK_DEEP_MAX_K"]  # include/xnrs_hip.h


def _takes_windows(fn) -> bool:
    """Whether a scorer's topk_deep / rank accepts the row windows as the keywords win_lo, win_hi."""
    import inspect
    try:
        params = inspect.signature(fn).parameters
    except (TypeError, ValueError):
        return False
    return ("win_lo" in params and "win_hi" in params) or any(p.kind is p.VAR_KEYWORD for p in params.values())


def _session_windows(windows, behaviors: Behaviors, dev, who: str):
    """`windows` = (lo, hi), integer tensors with one row bound per session of `behaviors` (indexed by session id, like
    user_index) -> the pair as int32 on `dev`; None stays None."""
    if windows is None:
        return None
    try:
        lo, hi = windows
    except (TypeError, ValueError):
        raise ValueError(f"{who}: windows is a pair (lo, hi) of integer tensors, one entry per session") from None
    out = []
    for t in (lo, hi):
        t = torch.as_tensor(t)
        if t.dim() != 1 or t.numel() != len(behaviors) or t.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8,
                                                                          torch.uint8):
            raise ValueError(f"{who}: windows holds two integer tensors of length len(behaviors) = {len(behaviors)}, indexed by "
                             f"session id; got {tuple(t.shape)} {t.dtype}")
        out.append(t.to(device=dev, dtype=torch.int32).contiguous())
    return tuple(out)


def row_windows(row_time: torch.Tensor, session_time: torch.Tensor, horizon=None):
    """The rows of a time-ordered news table a session at time t may see -> (lo, hi) int32 on row_time's device, the
    `windows` of recommend / rank_clicked / evaluate_full_ranking: hi = the first row with row_time > t (published after
    the impression), lo = the first row with row_time >= t - horizon (older than the horizon; 0 when `horizon` is None).
    row_time:(n_rows,) must be non-decreasing over the table's rows -- a row_time that decreases anywhere raises ValueError
    (one check, one host read, per call: build the windows once, outside any batch loop); the caller orders the table."""
    row_time = torch.as_tensor(row_time)
    if row_time.dim() != 1:
        raise ValueError(f"row_windows(): row_time is 1-D, one time per table row; got {tuple(row_time.shape)}")
    if row_time.numel() > 1 and bool((row_time[1:] < row_time[:-1]).any()):
        raise ValueError("row_windows(): row_time decreases somewhere; a row window needs the table ordered by time")
    row_time = row_time.contiguous()
    t = torch.as_tensor(session_time).to(device=row_time.device, dtype=row_time.dtype).reshape(-1)
    hi = torch.searchsorted(row_time, t, right=True)
    lo = torch.zeros_like(hi) if horizon is None else torch.searchsorted(row_time, t - horizon, right=False)
    return lo.to(torch.int32), hi.to(torch.int32)


def _recommending_model_parts(model, behaviors: Behaviors, k: int, windowed: bool = False, fn: str = "recommend",
                              method: str = "topk"):
    """(prepare_csr, the scorer's `method` call for this k, user index or None) of a model that can rank the table on its own,
    or the refusal under the name `fn` of the public function called -- before anything is encoded.  method "topk" becomes topk_deep beyond k = 128;
    windowed: the call carries row windows, which go through topk_deep too."""
    scorer = getattr(model, "rec_model", None)
    prepare, topk = getattr(scorer, "prepare_csr", None), getattr(scorer, method, None)
    if prepare is None or topk is None:
        raise NotImplementedError(f"{fn}(): the scorer {type(scorer).__name__} has no {method} path over a news table "
                                  f"(prepare_csr / {method}); ranking it with a plain dot product would recommend another "
                                  "model's news")
    if getattr(model, "user_dependent_news", False):
        raise NotImplementedError(f"{fn}(): the news vectors of {type(model).__name__} depend on the user, so no table of "
                                  "news vectors exists to rank; recommend() re-ranks the list of a candidate generator for it "
                                  "-- recommend(model, ..., generator=a model that ranks the table, pool=...)")
    if method == "topk" and (k > TOPK_MAX_K or windowed):
        method, topk = "topk_deep", getattr(scorer, "topk_deep", None)
        if topk is None and not windowed:
            raise NotImplementedError(f"{fn}(): the scorer {type(scorer).__name__} has no topk_deep, so it lists at most "
                                      f"k = {TOPK_MAX_K} news per session, not {k}")
    if windowed and (topk is None or not _takes_windows(topk)):
        raise NotImplementedError(f"{fn}(windows=...): the {method} of the scorer {type(scorer).__name__} takes no "
                                  "row windows (win_lo, win_hi)")
    uidx = None
    if getattr(model, "uses_user_index", False):
        uidx = getattr(behaviors, "user_index", None)
        if uidx is None:
            raise ValueError(f"{fn}(): {type(model).__name__} needs the user index of every session (sessions without "
                             "'user_index': Behaviors.from_sessions keeps it when every session carries it)")
    return prepare, topk, uidx


def _table_topk_batches(model, parts, store: NewsStore, behaviors: Behaviors, l_hist: int, k: int, sessions, batch: int,
                        exclude_history: bool, windows=None, vecs_out=None, sample=None):
    """The table of `model` encoded once, then per batch of sessions (lo, sess, hist rows, top-k rows, top-k scores).
    windows: (lo, hi) int32 per session id on the device, gathered with the batch's sessions, or None.  vecs_out: a list that
    receives the encoded news vectors before the first batch (what a second stage over the same table reads), or None.
    sample = (temperature, seed): parts holds the scorer's topk_sample, called with the session ids as the user keys, and a
    batch is (lo, sess, hist rows, sampled rows, their raw scores, their perturbed keys)."""
    prepare, topk, uidx = parts
    vecs, hm = encode_news_table(model, store)
    if vecs_out is not None:
        vecs_out.append(vecs)
    table = prepare(vecs)
    batcher = DeviceBatcher(behaviors, l_hist, store.pad_row)
    dev = vecs.device
    if uidx is not None:
        uidx = uidx.to(dev)
    every = sessions is None
    sessions = torch.arange(len(behaviors), device=dev) if every else torch.as_tensor(sessions, dtype=torch.int64, device=dev)
    for lo in range(0, sessions.numel(), batch):
        sess = sessions[lo:lo + batch]
        hist = batcher.eval_batch(sess)[0]
        h = vecs[hist.long()]
        m = hm[hist.long()]
        u = model.encode_user(h, m) if uidx is None else model.encode_user(h, m, uidx[sess])
        excl = _history_csr(behaviors, sess, lo if every else None) if exclude_history else (None, None)
        noise = () if sample is None else (sample[0], sample[1], sess.contiguous())
        kw = {} if windows is None else dict(win_lo=windows[0][sess], win_hi=windows[1][sess])
        out = tuple(topk(table, u, k, *noise, excl[0], excl[1], store.pad_row, **kw))
        if sample is not None:
            out = (out[0], _raw_scores(model.rec_model, table, u, out[0]), out[1])
        yield (lo, sess, hist) + out


def _raw_scores(scorer, table: torch.Tensor, u: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """The scorer's raw scores (score_csr, no ReLU) of the listed rows:(b, k) int32 of each user, -inf on the empty places (-1)."""
    b, k = rows.shape
    ok = rows >= 0
    sess = torch.arange(b, device=rows.device, dtype=torch.int32).repeat_interleave(k)
    r = scorer.score_csr(table, torch.where(ok, rows, torch.zeros_like(rows)).reshape(-1), sess, u, relu=False).reshape(b, k)
    return torch.where(ok, r, torch.full_like(r, float("-inf")))


def _rerank(rows: torch.Tensor, r: torch.Tensor, k: int):
    """Per session the k best of the scored candidates rows:(b, pool) int32 (-1: no candidate), r:(b, pool), in the order of
    xnrs_topk: higher score first, equal scores (-0 == +0) lower table row first, a NaN never, fillers -1 / -inf behind.
    Two stable device sorts over at most 1024 entries per session: by row, then by score descending."""
    ok = (rows >= 0) & ~torch.isnan(r)
    score = torch.where(ok, r + 0.0, torch.full_like(r, float("-inf")))  # (-0 + 0 == +0: the sort sees one zero)
    by_row = torch.where(ok, rows, torch.full_like(rows, torch.iinfo(torch.int32).max)).argsort(dim=1, stable=True)
    by_score = score.gather(1, by_row).argsort(dim=1, descending=True, stable=True)
    idx = by_row.gather(1, by_score)[:, :k]
    ok = ok.gather(1, idx)
    return (torch.where(ok, rows.gather(1, idx), torch.full_like(idx, -1, dtype=torch.int32)),
            torch.where(ok, r.gather(1, idx), torch.full_like(score[:, :k], float("-inf"))))


def _pool_arg(who: str, k: int, pool) -> int:
    """The list length a re-ranker or a second stage picks k from: k <= pool <= 1024, by default min(1024, max(8 k, 128))."""
    pool = min(TOPK_DEEP_MAX_K, max(8 * k, TOPK_MAX_K)) if pool is None else int(pool)
    if not k <= pool <= TOPK_DEEP_MAX_K:
        raise ValueError(f"{who}: pool = {pool} must lie in [k, {TOPK_DEEP_MAX_K}], k = {k}")
    return pool


def _pool_batches(model, generator, parts, uidx, store, behaviors, l_hist, n_list, pool, sessions, batch, exclude_history, windows,
                  vecs_out=None):
    """Per batch of sessions (lo, sess, rows:(b,n_list), scores:(b,n_list)), best first: the scorer's own list over its table
    (generator None), or the generator's `pool` best as `model` re-scored them (two stages), in the order of recommend()."""
    if generator is None:
        for lo, sess, _, rows, scores in _table_topk_batches(model, parts, store, behaviors, l_hist, n_list, sessions, batch,
                                                             exclude_history, windows, vecs_out=vecs_out):
            yield lo, sess, rows, scores
    else:
        for lo, sess, cand, r in _two_stage_batches(model, generator, parts, uidx, store, behaviors, l_hist, pool, sessions, batch,
                                                    exclude_history, windows):
            yield (lo, sess) + _rerank(cand, r, n_list)


def _fill_lists(behaviors: Behaviors, sessions, k: int, batch: int, dtypes, batches):
    """One (n, k) tensor per dtype on the device, filled from `batches` = (lo, one (b, k) tensor per dtype) in turn; then the
    status of the device is checked."""
    n = len(behaviors) if sessions is None else len(sessions)
    dev = behaviors.hist_off.device
    outs = tuple(torch.empty((n, k), dtype=t, device=dev) for t in dtypes)
    for lo, *got in batches:
        for out, g in zip(outs, got):
            out[lo:lo + batch] = g
    hip.check_status(dev)
    return outs


_ROWS_SCORES = (torch.int32, torch.float32)


@torch.no_grad()
def recommend(model, store: NewsStore, behaviors: Behaviors, l_hist: int, k: int, sessions=None, batch: int = 4096,
              exclude_history: bool = True, generator=None, pool=None, windows=None):
    """For every session the k news of the WHOLE table its user scores highest -> (rows:(n,k) int32, scores:(n,k) fp32) on the
    device, best first (include/xnrs_hip.h: xnrs_topk -- higher raw score first, equal scores lower row first, no ReLU; with
    fewer than k eligible news the tail is row -1 / score -inf).  k <= 128 runs the scorer's topk, 129 <= k <= 1024 its
    topk_deep (xnrs_topk_deep: the same order and bits, longer lists); a larger k raises ValueError.

    Once per call the news table is encoded (encode_news_table) and handed to the scorer (prepare_csr); per batch of sessions
    the user tower runs over the last `l_hist` clicks as DeviceBatcher builds them (encode_user, as evaluate) and the scorer's
    topk(table, u, k, ...) ranks the table without a (sessions, n_rows) score matrix.  store.pad_row is never recommended;
    with `exclude_history` neither is any news of the session's FULL history (hist_off / hist_val, not only the last l_hist).
    `sessions`: session indices (None = all); row i of the result is session sessions[i].

    Two stages (`generator`): for a `model` whose news vectors depend on the user (NPA: user_dependent_news and the hook
    score_impressions) no table exists to rank.  `generator` -- any model recommend() accepts on its own -- then lists `pool`
    news per session over ITS table (k <= pool <= 1024, default min(1024, max(8 k, 128)); exclusions and the pad row apply
    there), `model` scores exactly those through score_impressions(store, hist, rows, sess, user_index[sess], relu=False),
    and the k best of its scores are returned in the order above with the scores of `model`.  A place the generator could
    not fill is encoded as the pad row and its score thrown away, so no list length is read on the host.  The selection
    among at most 1024 scores per session is two device sorts, not a kernel of its own.  behaviors.user_index is required.

    `windows` = (lo, hi), integer tensors indexed by session id (see row_windows): session i sees the table rows
    [lo[i], hi[i]) only -- with a table ordered by publication time, the news that existed at the session's time and was still
    fresh.  The result is that of per-session exclusion lists holding every other row, without the lists and without scoring
    those rows (xnrs_topk_deep_win; every k goes through the scorer's topk_deep, the same bits).  With a `generator` the
    windows apply to the generator's list, the only place rows are chosen.  None: the scorer is called exactly as before.

    One process, one device: rank-sharded recommendation is out of scope.  A scorer without topk / prepare_csr, a model
    whose news vectors depend on the user (NPA) without `generator`, and CAUM (no candidate-independent user vector, no
    score_impressions) raise NotImplementedError."""
    k = int(k)
    if k > TOPK_DEEP_MAX_K:
        raise ValueError(f"recommend(): k = {k} is above the longest list of the top-k kernels, {TOPK_DEEP_MAX_K}")
    if generator is None:
        if pool is not None:
            raise ValueError("recommend(): `pool` is the list length of a `generator`; there is none")
        parts, uidx = _recommending_model_parts(model, behaviors, k, windows is not None), None
    else:
        pool, parts, uidx = _two_stage_parts(model, generator, behaviors, k, pool, windows is not None)
    windows = _session_windows(windows, behaviors, behaviors.hist_off.device, "recommend()")
    return _fill_lists(behaviors, sessions, k, batch, _ROWS_SCORES,
                       ((lo, r, s) for lo, _, r, s in _pool_batches(model, generator, parts, uidx, store, behaviors, l_hist, k, pool,
                                                                   sessions, batch, exclude_history, windows)))


@torch.no_grad()
def recommend_sampled(model, store: NewsStore, behaviors: Behaviors, l_hist: int, k: int, temperature: float, seed: int,
                      sessions=None, batch: int = 4096, exclude_history: bool = True, windows=None, return_keys: bool = False,
                      generator=None):
    """recommend() as a stochastic ranking policy: for every session a list of k news DRAWN from the whole table instead of
    the k best -- a sample without replacement from the Plackett-Luce distribution P(news first) ~ exp(score / temperature),
    continued over the rest (include/xnrs_hip.h: xnrs_topk_sample_win; Gumbel top-k inside the top-k sweep, no (sessions,
    n_rows) matrix) -> (rows:(n,k) int32, scores:(n,k) fp32[, keys:(n,k) fp32]) on the device, in the order drawn.  One
    temperature trades accuracy against exposure: towards 0 the lists tend to recommend()'s, a large one spreads exposure
    over the catalogue (diversity_metrics measures coverage and the Gini of exposure of either).

    The draw of a (session, news) pair is a pure function of (seed, SESSION ID, table row): a session's list does not depend
    on `batch`, on which other sessions are asked for or on the run; vary `seed` to draw again.  Encoding, eligibility
    (store.pad_row, `exclude_history`), `sessions` and `windows` are those of recommend().

    `scores` are the model's RAW scores of the returned rows, from the scorer's score_csr(..., relu=False), -inf on the empty
    places (-1) of a session with fewer than k eligible news.  They agree with recommend()'s scores of the same rows to
    rounding, NOT bit for bit: score_csr sums a row's products in another order than the sweep's score tile.
    return_keys=True adds the perturbed keys score / temperature + g the lists are ordered by.

    Refused before anything is encoded: temperature not finite or <= 0 and k > 1024 (ValueError); a scorer without
    topk_sample / prepare_csr / score_csr, a model whose news vectors depend on the user (NPA), CAUM, and `generator` --
    sampling behind a candidate generator is not implemented (NotImplementedError)."""
    import math
    k = int(k)
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not math.isfinite(temperature) or temperature <= 0:
        raise ValueError(f"recommend_sampled(): temperature = {temperature!r}: a finite number above 0")
    if k > TOPK_DEEP_MAX_K:
        raise ValueError(f"recommend_sampled(): k = {k} is above the longest list of the top-k kernels, {TOPK_DEEP_MAX_K}")
    if generator is not None:
        raise NotImplementedError("recommend_sampled(generator=...): sampling behind a candidate generator is not implemented")
    scorer = getattr(model, "rec_model", None)
    if getattr(scorer, "score_csr", None) is None:
        raise NotImplementedError(f"recommend_sampled(): the scorer {type(scorer).__name__} has no score_csr for the raw scores "
                                  "of the sampled rows")
    from .models.caum import CAUM
    if isinstance(model, CAUM):
        raise NotImplementedError("recommend_sampled(): CAUM has no candidate-independent user vector to rank a table with")
    parts = _recommending_model_parts(model, behaviors, k, windows is not None, "recommend_sampled", "topk_sample")
    windows = _session_windows(windows, behaviors, behaviors.hist_off.device, "recommend_sampled()")
    out = _fill_lists(behaviors, sessions, k, batch, _ROWS_SCORES + (torch.float32,),
                      ((lo, r, s, g) for lo, _, _, r, s, g in
                       _table_topk_batches(model, parts, store, behaviors, l_hist, k, sessions, batch, exclude_history, windows,
                                           sample=(float(temperature), int(seed)))))
    return out if return_keys else out[:2]


def _two_stage_parts(model, generator, behaviors: Behaviors, k: int, pool, windowed: bool):
    """(pool, the generator's _recommending_model_parts for it, user index) of recommend(generator=...), or the refusal --
    before anything is encoded."""
    if not getattr(model, "user_dependent_news", False) or getattr(model, "score_impressions", None) is None:
        raise NotImplementedError(f"recommend(generator=...): {type(model).__name__} has no score_impressions over news vectors "
                                  "that depend on the user; a model that ranks the table is called without a generator")
    pool = _pool_arg("recommend()", k, pool)
    parts = _recommending_model_parts(generator, behaviors, pool, windowed)
    uidx = getattr(behaviors, "user_index", None)
    if uidx is None:
        raise ValueError(f"recommend(): {type(model).__name__} needs the user index of every session (sessions without "
                         "'user_index': Behaviors.from_sessions keeps it when every session carries it)")
    return pool, parts, uidx


def _two_stage_batches(model, generator, parts, uidx, store: NewsStore, behaviors: Behaviors, l_hist: int, pool: int, sessions,
                       batch: int, exclude_history: bool, windows):
    """Per batch of sessions (lo, sess, cand:(b,pool) int32, r:(b,pool)): the generator's list over its table and the scores
    `model` gives exactly those news (score_impressions, no ReLU); the score of an empty place (-1) means nothing."""
    dev = behaviors.hist_off.device
    uidx = uidx.to(dev)
    spare = store.pad_row if store.pad_row >= 0 else 0  # what stands in for a place the generator left empty
    for lo, sess, hist, cand, _ in _table_topk_batches(generator, parts, store, behaviors, l_hist, pool, sessions, batch,
                                                       exclude_history, windows):
        b = sess.numel()
        csess = torch.arange(b, device=dev, dtype=torch.int32).repeat_interleave(pool)
        crows = torch.where(cand >= 0, cand, torch.full_like(cand, spare)).reshape(-1)
        r = model.score_impressions(store, hist, crows, csess, uidx[sess], relu=False)
        yield lo, sess, cand, r.reshape(b, pool)


def _ranking_model_parts(model, behaviors: Behaviors, who: str, windowed: bool = False):
    """(prepare_csr, rank, user index or None) of a model whose clicked news can be ranked within the table, or the refusal
    -- before anything is encoded.  windowed: the call carries row windows."""
    scorer = getattr(model, "rec_model", None)
    prepare, rank = getattr(scorer, "prepare_csr", None), getattr(scorer, "rank", None)
    if prepare is None or rank is None:
        raise NotImplementedError(f"{who}: the scorer {type(scorer).__name__} has no ranking path over a news table "
                                  "(prepare_csr / rank); ranking it with a plain dot product would evaluate another model")
    if getattr(model, "user_dependent_news", False):
        raise NotImplementedError(f"{who}: the news vectors of {type(model).__name__} depend on the user, so no table of "
                                  "news vectors exists to rank")
    if windowed and not _takes_windows(rank):
        raise NotImplementedError(f"{who}: the rank of the scorer {type(scorer).__name__} takes no row windows (win_lo, win_hi)")
    uidx = None
    if getattr(model, "uses_user_index", False):
        uidx = getattr(behaviors, "user_index", None)
        if uidx is None:
            raise ValueError(f"{who}: {type(model).__name__} needs the user index of every session (sessions without "
                             "'user_index': Behaviors.from_sessions keeps it when every session carries it)")
    return prepare, rank, uidx


@torch.no_grad()
def rank_clicked(model, store: NewsStore, behaviors: Behaviors, l_hist: int, sessions=None, batch: int = 4096,
                 exclude_history: bool = True, windows=None):
    """Where every clicked news ranks among ALL news of the table for its session's user -> (query_session int64, query_row
    int32, rank int32, score fp32) on the device, one entry per (session, clicked news) in session order (pos_off / pos_val;
    a session without a click gives no query).

    rank = the number of eligible news that come before the clicked one in the order of recommend() (include/xnrs_hip.h:
    xnrs_rank -- higher raw score first, equal scores lower row first, no ReLU), so rank < k exactly when recommend(k) lists
    the news, at position rank.  Eligible: every news but store.pad_row and, with `exclude_history`, the session's FULL
    history; the clicked news itself is ranked even when it is in that history.  rank -1 / score NaN: the clicked news is
    the pad row, or its score is NaN.

    Once per call the news table is encoded (encode_news_table) and handed to the scorer (prepare_csr); per batch of sessions
    the user tower runs as in recommend() and the scorer's rank(table, u, ...) sweeps the table without a (sessions, n_rows)
    score matrix.  `sessions`: session indices (None = all; a range of step 1 is taken as a slice, without gathering).
    `windows` = (lo, hi) indexed by session id, as recommend(): only the rows [lo[i], hi[i]) compete with session i's clicked
    news (xnrs_rank_win); a clicked news outside its session's window is ranked all the same.  Refusals as recommend()."""
    prepare, rank_fn, uidx = _ranking_model_parts(model, behaviors, "rank_clicked()", windows is not None)
    windows = _session_windows(windows, behaviors, behaviors.hist_off.device, "rank_clicked()")
    vecs, hm = encode_news_table(model, store)
    table = prepare(vecs)
    batcher = DeviceBatcher(behaviors, l_hist, store.pad_row)
    dev = vecs.device
    if uidx is not None:
        uidx = uidx.to(dev)
    first = None  # the first session of a contiguous run
    if sessions is None:
        sessions = range(len(behaviors))
    if isinstance(sessions, range) and sessions.step == 1:
        first = sessions.start
        sessions = torch.arange(sessions.start, max(sessions.stop, sessions.start), device=dev)
    else:
        sessions = torch.as_tensor(sessions, dtype=torch.int64, device=dev)
    pos_off, pos_val = behaviors.pos_off, behaviors.pos_val
    n_pos = pos_off[sessions + 1] - pos_off[sessions]
    q_sess = torch.repeat_interleave(sessions, n_pos)
    if first is not None:  # one pair of outputs indexed like pos_val; every batch writes its own span
        ranks = torch.full((pos_val.numel(),), -1, dtype=torch.int32, device=dev)
        scores = torch.full((pos_val.numel(),), float("nan"), dtype=torch.float32, device=dev)
    parts = []
    for lo in range(0, sessions.numel(), batch):
        sess = sessions[lo:lo + batch]
        hist = batcher.eval_batch(sess)[0]
        h = vecs[hist.long()]
        m = hm[hist.long()]
        u = model.encode_user(h, m) if uidx is None else model.encode_user(h, m, uidx[sess])
        at = None if first is None else first + lo
        excl = _history_csr(behaviors, sess, at) if exclude_history else (None, None)
        tgt = _session_csr(pos_off, pos_val, sess, at)
        win = {}
        if windows is not None:  # the batch's sessions: a slice of a contiguous run, a gather otherwise
            win = {"win_lo": windows[0][sess] if at is None else windows[0][at:at + sess.numel()],
                   "win_hi": windows[1][sess] if at is None else windows[1][at:at + sess.numel()]}
        if first is not None:
            rank_fn(table, u, tgt[0], tgt[1], excl[0], excl[1], store.pad_row, out=(ranks, scores), **win)
        else:
            parts.append((tgt[1],) + tuple(rank_fn(table, u, tgt[0], tgt[1], excl[0], excl[1], store.pad_row, **win)))
    hip.check_status(dev)
    if first is not None:
        a, b = (int(v) for v in pos_off[[first, first + sessions.numel()]].tolist())
        return q_sess, pos_val[a:b], ranks[a:b], scores[a:b]
    if not parts:
        return (q_sess, pos_val[:0], torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.float32, device=dev))
    return (q_sess,) + tuple(torch.cat([p[i] for p in parts]) for i in range(3))


def full_ranking_sums(rank: torch.Tensor, ks) -> torch.Tensor:
    """fp64 sums over the queries with rank >= 0: [n_queries, hit@k for k in ks, ndcg@k for k in ks, reciprocal rank, rank].
    Post-processing of an integer vector (ranks are 0-based: the best news has rank 0)."""
    r = rank[rank >= 0].double()
    out = [torch.tensor(float(r.numel()), dtype=torch.float64, device=rank.device)]
    out += [(r < k).double().sum() for k in ks]
    out += [torch.where(r < k, 1.0 / torch.log2(2.0 + r), torch.zeros_like(r)).sum() for k in ks]  # one relevant item: DCG / 1
    out += [(1.0 / (1.0 + r)).sum(), r.sum()]
    return torch.stack(out)


def full_ranking_metrics(sums: torch.Tensor, ks) -> Dict[str, float]:
    """The dict of evaluate_full_ranking out of full_ranking_sums (added over the ranks of a job)."""
    v = sums.tolist()
    n, nk = v[0], len(ks)
    d = max(n, 1.0)
    out = {f"hit@{k}": v[1 + i] / d for i, k in enumerate(ks)}
    out.update({f"ndcg@{k}": v[1 + nk + i] / d for i, k in enumerate(ks)})
    out.update({"mrr": v[1 + 2 * nk] / d, "mean_rank": v[2 + 2 * nk] / d, "n_queries": int(n)})
    return out


@torch.no_grad()
def evaluate_full_ranking(model, store: NewsStore, behaviors: Behaviors, l_hist: int, ks=(5, 10, 100), sessions=None,
                          batch: int = 4096, exclude_history: bool = True, distributed: bool = False, windows=None) -> Dict[str, float]:
    """Full-corpus ranking metrics of the clicked news (rank_clicked): hit@k (= recall@k: one relevant news per query),
    ndcg@k (1 / log2(2 + rank) when rank < k), mrr (1 / (1 + rank)), mean_rank (0-based) and n_queries, averaged in fp64
    over the queries with rank >= 0.

    `distributed=True` (opt-in, never automatic: every rank of the default process group must then make this call) shards
    the sessions over the ranks (distributed.shard_range); every rank encodes the whole table, and ONE fp64 all-reduce adds
    the sums and the count, so every rank returns the same dict, equal to the single-process one up to the order of that
    final sum.  `windows` as rank_clicked(): indexed by session id, so they are sharded with the sessions."""
    _ranking_model_parts(model, behaviors, "evaluate_full_ranking()", windows is not None)
    ks = tuple(int(k) for k in ks)
    on = False
    if distributed:
        rank, world, on = _dist_rank_world(True)
    if on:
        from .distributed import shard_range
        n = len(behaviors) if sessions is None else len(sessions)
        lo, hi = shard_range(n, rank, world)
        if sessions is None:
            sessions = range(lo, hi)
        else:
            sessions = sessions[lo:hi]
    _, _, ranks, _ = rank_clicked(model, store, behaviors, l_hist, sessions, batch, exclude_history, windows)
    sums = full_ranking_sums(ranks, ks)
    if on:
        import torch.distributed as dist
        dist.all_reduce(sums, op=dist.ReduceOp.SUM)
    return full_ranking_metrics(sums, ks)


# ---------------------------------------------------------------------------------------------- diverse recommendations
DIVERSITY_MAX_K = TOPK_MAX_K  # the longest list of xnrs_list_diversity


def _rerank_args(who: str, k: int, lam, pool, rel: str, other: str, keep_pool: bool = False):
    """(k, lam, pool) of a re-ranking call checked against include/xnrs_hip.h: xnrs_mmr_rerank / xnrs_calibrated_rerank, or the
    ValueError; lam None (no re-ranking) passes, with pool None unless a generator lists the pool (keep_pool).  other: what
    lam = 0 ranks by alone."""
    from .ops import MMR_REL
    k = int(k)
    if k < 1 or k > TOPK_DEEP_MAX_K:
        raise ValueError(f"{who}: k = {k} must lie in [1, {TOPK_DEEP_MAX_K}], the longest list of the top-k kernels")
    if lam is None:
        if pool is not None and not keep_pool:
            raise ValueError(f"{who}: `pool` is the list that is re-ranked; without `lam` nothing is re-ranked")
        return k, None, pool
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:  # (NaN too)
        raise ValueError(f"{who}: lam = {lam} must lie in [0, 1] (1: relevance alone, 0: {other} alone)")
    if rel not in MMR_REL:
        raise ValueError(f"{who}: rel is one of {sorted(MMR_REL)}, got {rel!r}")
    return k, lam, _pool_arg(who, k, pool)


def _diverse_batches(model, parts, store, behaviors, l_hist, k, lam, pool, rel, sessions, batch, exclude_history, windows):
    """Per batch of sessions (lo, sess, rows:(b,k), scores:(b,k), vecs, inv): the lists of recommend(k) (lam None) or the MMR
    re-ranking of the scorer's `pool` best (xnrs_mmr_rerank over the encoded news vectors); inv = their inverse row norms."""
    from . import ops
    got, inv = [], None
    for lo, sess, rows, scores in _pool_batches(model, None, parts, None, store, behaviors, l_hist, k if lam is None else pool, pool,
                                                sessions, batch, exclude_history, windows, vecs_out=got):
        if inv is None:
            inv = ops.row_inv_norms(got[0])
        if lam is not None:
            rows, scores, _ = ops.mmr_rerank(got[0], inv, rows, scores, k, lam, rel)
        yield lo, sess, rows, scores, got[0], inv


@torch.no_grad()
def recommend_diverse(model, store: NewsStore, behaviors: Behaviors, l_hist: int, k: int, lam: float, pool=None,
                      rel: str = "minmax", sessions=None, batch: int = 4096, exclude_history: bool = True, windows=None):
    """recommend() with variety: per session the scorer lists its `pool` best news of the whole table (topk / topk_deep, as
    recommend(pool): exclusions, the pad row and `windows` apply there) and greedy MMR picks k of them -> (rows:(n,k) int32,
    scores:(n,k) fp32) on the device in the order picked; the scores are the model's relevance scores of the picks, bit for
    bit the pool's.  Step by step the pick is the candidate with the largest lam * relevance - (1 - lam) * (largest cosine to
    a news picked so far), cosines between the ENCODED news vectors (not the scorer's prepared table), equal objectives to
    the better-ranked candidate (include/xnrs_hip.h: xnrs_mmr_rerank).  rel "minmax" rescales a session's pool scores to
    [0, 1] first, so one lam means the same for every session and scorer; "raw" takes the scores as they are.  lam = 1 returns
    recommend(k) in rows and score bits.  pool: k <= pool <= 1024, default min(1024, max(8 k, 128)).  With fewer than k
    eligible news the tail is row -1 / score -inf.

    The table is encoded once.  Refusals are those of recommend(), raised before anything is encoded.  There is no `generator`
    form: a model whose news vectors depend on the user (NPA) has no table vectors to compare."""
    if lam is None:
        raise ValueError("recommend_diverse(): lam in [0, 1] is required (recommend() lists by relevance alone)")
    k, lam, pool = _rerank_args("recommend_diverse()", k, lam, pool, rel, "variety")
    parts = _recommending_model_parts(model, behaviors, pool, windows is not None)
    windows = _session_windows(windows, behaviors, behaviors.hist_off.device, "recommend_diverse()")
    return _fill_lists(behaviors, sessions, k, batch, _ROWS_SCORES,
                       ((lo, r, s) for lo, _, r, s, _, _ in _diverse_batches(model, parts, store, behaviors, l_hist, k, lam, pool, rel,
                                                                            sessions, batch, exclude_history, windows)))


def _diversity_check(rows: torch.Tensor, who: str):
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.dtype != torch.int32:
        raise ValueError(f"{who}: lists are a (n, k) int32 tensor, got {tuple(getattr(rows, 'shape', ()))} "
                         f"{getattr(rows, 'dtype', type(rows))}")
    if not 1 <= rows.shape[1] <= DIVERSITY_MAX_K:
        raise ValueError(f"{who}: k = {rows.shape[1]} must lie in [1, {DIVERSITY_MAX_K}], the longest list of xnrs_list_diversity")


def _diversity_sums(vecs, inv, rows, pad_row: int, row_category, n_categories: int, counts: torch.Tensor) -> torch.Tensor:
    """fp64 sums over the lists rows:(b,k): [lists, lists with n >= 1, lists with n >= 2, ild, cat_ild, n_categories]; adds the
    lists' rows to the exposure counts:(n_rows,) int64.  A pad-row entry is no place."""
    from . import ops
    if pad_row >= 0:
        rows = torch.where(rows == pad_row, torch.full_like(rows, -1), rows)
    ild, n, n_cat, diff_cat = ops.list_diversity(vecs, inv, rows, row_category, n_categories)
    ok = (rows >= 0) & (rows < counts.numel())
    counts += torch.bincount(rows[ok].long(), minlength=counts.numel())
    n = n.double()
    two = n >= 2
    zero = torch.zeros((), dtype=torch.float64, device=rows.device)
    out = [zero + rows.shape[0], (n >= 1).double().sum(), two.double().sum(), torch.where(two, ild.double(), zero).sum()]
    if row_category is None:
        out += [zero, zero]
    else:
        pairs = (n * (n - 1) / 2).clamp(min=1)
        out += [torch.where(two, diff_cat.double() / pairs, zero).sum(), n_cat.double().sum()]
    return torch.stack(out)


def _diversity_dict(sums: torch.Tensor, counts: torch.Tensor, k: int, pad_row: int, with_categories: bool) -> Dict[str, float]:
    """The dict of diversity_metrics out of the added _diversity_sums and the exposure counts (fp64, one host read)."""
    c = counts.double()
    if 0 <= pad_row < c.numel():
        c = torch.cat((c[:pad_row], c[pad_row + 1:]))
    n = c.numel()
    total = c.sum()
    asc = torch.sort(c).values
    weighted = (torch.arange(1, n + 1, dtype=torch.float64, device=c.device) * asc).sum()
    gini = torch.where(total > 0, 2 * weighted / (max(n, 1) * total.clamp(min=1)) - (n + 1) / max(n, 1), torch.zeros_like(total))
    cover = (c > 0).double().sum() / max(n, 1)
    v = torch.cat((sums, torch.stack((gini, cover, total)))).tolist()
    out = {f"ild@{k}": v[3] / max(v[2], 1.0), f"catalog_coverage@{k}": v[7], f"gini@{k}": v[6], "n_lists": int(v[0]),
           "n_listed": int(v[8])}
    if with_categories:
        out.update({f"cat_ild@{k}": v[4] / max(v[2], 1.0), f"n_categories@{k}": v[5] / max(v[1], 1.0)})
    return out


@torch.no_grad()
def diversity_metrics(vecs: torch.Tensor, rows: torch.Tensor, n_rows: int, pad_row: int, row_category=None,
                      n_categories: int = 0) -> Dict[str, float]:
    """Beyond-accuracy measures of recommended lists from anywhere: rows:(n,k) int32 on the device (k <= 128; -1, an id outside
    [0, n_rows) or pad_row: no place) over the first n_rows encoded news vectors `vecs`.
      ild@k              the mean over the lists with two or more places of the intra-list distance, the mean of 1 - cos(news
                         vectors) over the list's pairs (include/xnrs_hip.h: xnrs_list_diversity)
      catalog_coverage@k the share of the non-pad rows that appear in any list
      gini@k             the Gini coefficient of the exposure counts c over the non-pad rows, 2 sum_i i c_(i) / (n sum c) -
                         (n + 1) / n over the ascending counts, i from 1: 0 for even exposure, (n - 1) / n when one news takes
                         it all; 0 when nothing was listed
      n_lists, n_listed  the lists given, the places they fill
    and with row_category:(n_rows,) int32 (values in [0, n_categories); another value is a news without a category, which
    counts in no pair and as no category):
      cat_ild@k          the mean over the same lists of the share of pairs whose categories differ
      n_categories@k     the mean over the lists with a place of the number of distinct categories.
    Means, coverage and Gini are taken in fp64 on the device (bincount, sort): index bookkeeping, as full_ranking_metrics."""
    _diversity_check(rows, "diversity_metrics()")
    from . import ops
    n_rows = int(n_rows)
    vecs = hip.dev_f32(vecs, "news vectors")
    if vecs.dim() != 2 or not 0 <= n_rows <= vecs.shape[0]:
        raise ValueError(f"diversity_metrics(): n_rows = {n_rows} rows of a (rows, E) table of news vectors, got {tuple(vecs.shape)}")
    vecs = vecs[:n_rows]
    if row_category is not None:
        row_category = row_category[:n_rows]
    counts = torch.zeros((n_rows,), dtype=torch.int64, device=vecs.device)
    sums = _diversity_sums(vecs, ops.row_inv_norms(vecs), rows.contiguous(), int(pad_row), row_category, n_categories, counts)
    return _diversity_dict(sums, counts, rows.shape[1], int(pad_row), row_category is not None)


@torch.no_grad()
def evaluate_diversity(model, store: NewsStore, behaviors: Behaviors, l_hist: int, k: int, lam=None, pool=None,
                       rel: str = "minmax", row_category=None, n_categories: int = 0, sessions=None, batch: int = 4096,
                       exclude_history: bool = True, windows=None) -> Dict[str, float]:
    """Diversity, exposure and accuracy of the model's lists in one place: the dict of diversity_metrics over the lists of
    recommend(k) (lam None) or recommend_diverse(k, lam, pool, rel), plus hit@k and ndcg@k of the clicked news WITHIN the
    returned list with the definitions of evaluate_full_ranking -- every (session, clicked news) is a query, hit = the list
    holds it, ndcg = 1 / log2(2 + position), averaged in fp64 over n_queries (a clicked pad row is no query) -- so a sweep
    over lam shows what variety costs.  (A clicked news of the session's history is never listed under exclude_history, while
    evaluate_full_ranking ranks it all the same: the two agree where no click lies in its history.)

    The sums are added batch by batch: beyond the exposure counts no more than one batch of lists is resident.  k <= 128 (the
    lists go through xnrs_list_diversity); a larger k raises ValueError.  Refusals as recommend(), before anything is encoded."""
    k, lam, pool = _rerank_args("evaluate_diversity()", k, lam, pool, rel, "variety")
    if k > DIVERSITY_MAX_K:
        raise ValueError(f"evaluate_diversity(): k = {k} is above the longest list of xnrs_list_diversity, {DIVERSITY_MAX_K}")
    parts = _recommending_model_parts(model, behaviors, k if lam is None else pool, windows is not None)
    dev = behaviors.hist_off.device
    windows = _session_windows(windows, behaviors, dev, "evaluate_diversity()")
    pad = int(store.pad_row)
    counts = torch.zeros((store.n_rows,), dtype=torch.int64, device=dev)
    sums = torch.zeros((6,), dtype=torch.float64, device=dev)
    acc = torch.zeros((3,), dtype=torch.float64, device=dev)  # queries, hits, dcg
    for _, sess, rows, _, vecs, inv in _diverse_batches(model, parts, store, behaviors, l_hist, k, lam, pool, rel, sessions, batch,
                                                         exclude_history, windows):
        sums += _diversity_sums(vecs, inv, rows, pad, row_category, n_categories, counts)
        acc += _list_accuracy_sums(behaviors, sess, rows, store.n_rows, pad)
    hip.check_status(dev)
    out = _diversity_dict(sums, counts, k, pad, row_category is not None)
    out.update(_list_accuracy_dict(acc, k))
    return out


def _list_accuracy_sums(behaviors: Behaviors, sess: torch.Tensor, rows: torch.Tensor, n_rows: int, pad: int) -> torch.Tensor:
    """fp64 [queries, hits, dcg] of the clicked news of the sessions `sess` WITHIN their lists rows:(b,k): every (session,
    clicked news) is a query (a clicked pad row or a row outside the table is none), hit = the list holds it, dcg = 1 / log2(2 +
    position)."""
    dev = rows.device
    off, clicked = _session_csr(behaviors.pos_off, behaviors.pos_val, sess, None)  # (gathered: offsets from 0)
    q = torch.repeat_interleave(torch.arange(sess.numel(), device=dev), off[1:] - off[:-1])
    asked = (clicked >= 0) & (clicked < n_rows) & (clicked != pad)
    at = rows[q] == clicked.to(torch.int32)[:, None]
    hit = at.any(dim=1) & asked
    place = at.to(torch.int8).argmax(dim=1).double()
    return torch.stack((asked.double().sum(), hit.double().sum(),
                        torch.where(hit, 1.0 / torch.log2(2.0 + place), torch.zeros_like(place)).sum()))


def _list_accuracy_dict(acc: torch.Tensor, k: int) -> Dict[str, float]:
    """hit@k, ndcg@k and n_queries out of the added _list_accuracy_sums (one host read)."""
    nq, hits, dcg = acc.tolist()
    return {f"hit@{k}": hits / max(nq, 1.0), f"ndcg@{k}": dcg / max(nq, 1.0), "n_queries": int(nq)}


LIST_RECALL_CHUNK = 1 << 24  # most elements of the (sessions, k, P) comparison that exist at once


def list_recall(found_rows: torch.Tensor, wanted_rows: torch.Tensor) -> torch.Tensor:
    """Per session the share of its wanted rows:(n, k) that its other list found_rows:(n, P) holds -> (n,) fp32 on the lists'
    device.  Only rows >= 0 count (-1 is the filler of both lists); a session that wants nothing gets 0.  What a two-stage
    list is judged by -- how much of the re-ranker's top k the candidate generator's pool of P contains (found = the
    generator's pool, wanted = the re-ranker's list) -- and what losses.distillation_loss is there to raise.  Device
    arithmetic, in chunks of sessions so that no comparison array beyond LIST_RECALL_CHUNK elements exists."""
    if found_rows.dim() != 2 or wanted_rows.dim() != 2 or found_rows.shape[0] != wanted_rows.shape[0]:
        raise ValueError(f"list_recall(): two lists per session, (n, P) and (n, k); got {tuple(found_rows.shape)} and "
                         f"{tuple(wanted_rows.shape)}")
    n, P = found_rows.shape
    k = wanted_rows.shape[1]
    out = torch.zeros((n,), dtype=torch.float32, device=wanted_rows.device)
    step = max(1, LIST_RECALL_CHUNK // max(1, k * P))
    for lo in range(0, n, step):
        want, found = wanted_rows[lo:lo + step], found_rows[lo:lo + step]
        asked = want >= 0
        hit = (want[:, :, None] == found[:, None, :]).any(dim=2) & asked
        out[lo:lo + step] = hit.sum(dim=1).float() / asked.sum(dim=1).clamp(min=1).float()
    return out


# -------------------------------------------------------------------------------------------- calibrated recommendations
CALIBRATION_MAX_CATEGORIES = hip._CONSTANTS["DIVERSITY_MAX_CATEGORIES"]  # include/xnrs_hip.h


def _calibrated_args(who: str, behaviors, k: int, lam, pool, rel: str, alpha, row_category, n_categories, target, two_stage: bool):
    """(k, lam, pool, alpha, n_categories) of a calibration call checked against include/xnrs_hip.h: xnrs_calibrated_rerank, or
    the ValueError; lam None (no re-ranking) passes, with pool None unless a generator lists the pool.  target: "history", a
    (n_categories,) tensor or -- behaviors given -- a (len(behaviors), n_categories) tensor."""
    k, lam, pool = _rerank_args(who, k, lam, pool, rel, "the category mix", two_stage)
    n_categories = int(n_categories)
    if not 1 <= n_categories <= CALIBRATION_MAX_CATEGORIES:
        raise ValueError(f"{who}: n_categories = {n_categories} must lie in [1, {CALIBRATION_MAX_CATEGORIES}]")
    if not isinstance(row_category, torch.Tensor) or row_category.dim() != 1 or row_category.dtype != torch.int32:
        raise ValueError(f"{who}: row_category is a (n_rows,) int32 tensor, one category per table row; got "
                         f"{tuple(getattr(row_category, 'shape', ()))} {getattr(row_category, 'dtype', type(row_category))}")
    alpha = float(alpha)
    if not 0.0 < alpha < 1.0:  # (NaN too)
        raise ValueError(f"{who}: alpha = {alpha} must lie in (0, 1): the share of the target mixed into the list's mix")
    if isinstance(target, str):
        if target != "history" or behaviors is None:
            forms = "a tensor of weights" if behaviors is None else "'history' or a tensor of weights"
            raise ValueError(f"{who}: target is {forms}, ({n_categories},) or one row per "
                             f"{'list' if behaviors is None else 'session'}; got {target!r}")
    else:
        per = (len(behaviors), n_categories) if behaviors is not None else None
        if not isinstance(target, torch.Tensor) or target.dim() not in (1, 2) or target.shape[-1] != n_categories \
                or (target.dim() == 2 and per is not None and tuple(target.shape) != per) or not target.is_floating_point():
            raise ValueError(f"{who}: target is a ({n_categories},) tensor of weights or one row per "
                             f"{'session, ' + str(per) if per else 'list'}; got {tuple(getattr(target, 'shape', ()))} "
                             f"{getattr(target, 'dtype', type(target))}")
    return k, lam, pool, alpha, n_categories


def _target_rows(target, n: int, index, dev) -> torch.Tensor:
    """(n, C) fp32 target mix on `dev` out of a (C,) tensor (one mix for everybody) or a (m, C) tensor gathered by `index`
    (None: as it lies)."""
    t = target.to(device=dev, dtype=torch.float32)
    if t.dim() == 1:
        return t.expand(n, t.numel()).contiguous()
    return (t if index is None else t[index]).contiguous()


def _calibrated_batches(model, generator, parts, uidx, store, behaviors, l_hist, k, lam, pool, rel, alpha, row_category,
                        n_categories, target, sessions, batch, exclude_history, windows):
    """Per batch of sessions (lo, sess, rows:(b,k), scores:(b,k), target:(b,C)): the lists of recommend(k) (lam None) or the
    calibrated re-ranking of the `pool` best -- the scorer's own (table form) or the generator's as `model` re-scored them
    (two stages, in the order of recommend(pool))."""
    from . import ops
    every = sessions is None
    if not isinstance(target, str):
        target = target.to(device=behaviors.hist_off.device, dtype=torch.float32)
    for lo, sess, rows, scores in _pool_batches(model, generator, parts, uidx, store, behaviors, l_hist, k if lam is None else pool,
                                                pool, sessions, batch, exclude_history, windows):
        if isinstance(target, str):  # the mix of the session's FULL history, the one exclude_history excludes
            off, val = _history_csr(behaviors, sess, lo if every else None)
            tgt = ops.csr_category_counts(off.contiguous(), val, row_category, n_categories, store.pad_row).float()
        else:
            tgt = _target_rows(target, sess.numel(), sess, rows.device)
        if lam is not None:
            rows, scores, _, _ = ops.calibrated_rerank(rows.contiguous(), scores.contiguous(), k, lam, row_category, n_categories,
                                                       tgt, alpha, rel)
        yield lo, sess, rows, scores, tgt


def _calibrated_parts(who, model, store, behaviors, k, lam, pool, rel, alpha, row_category, n_categories, target, windows, generator):
    """Every refusal of a calibration call, before anything is encoded -> (k, lam, pool, alpha, n_categories, parts, uidx,
    windows, row_category on the device)."""
    k, lam, pool, alpha, n_categories = _calibrated_args(who, behaviors, k, lam, pool, rel, alpha, row_category, n_categories,
                                                         target, generator is not None)
    if generator is None:
        parts, uidx = _recommending_model_parts(model, behaviors, k if lam is None else pool, windows is not None), None
    else:
        pool, parts, uidx = _two_stage_parts(model, generator, behaviors, k, pool, windows is not None)
    dev = behaviors.hist_off.device
    if row_category.numel() < store.n_rows:
        raise ValueError(f"{who}: row_category holds {row_category.numel()} categories for a store of {store.n_rows} rows")
    return k, lam, pool, alpha, n_categories, parts, uidx, _session_windows(windows, behaviors, dev, who), \
        row_category.to(dev).contiguous()


@torch.no_grad()
def recommend_calibrated(model, store: NewsStore, behaviors: Behaviors, l_hist: int, k: int, lam: float, row_category,
                         n_categories: int, target="history", alpha: float = 0.01, pool=None, rel: str = "minmax", sessions=None,
                         batch: int = 4096, exclude_history: bool = True, windows=None, generator=None):
    """recommend() steered towards a category mix (Steck, "Calibrated Recommendations", RecSys 2018): per session the scorer
    lists its `pool` best news of the whole table (as recommend(pool): exclusions, the pad row and `windows` apply there) and a
    greedy picks k of them -> (rows:(n,k) int32, scores:(n,k) fp32) on the device in the order picked; the scores are the
    model's relevance scores of the picks, bit for bit the pool's.  Step by step the pick is the candidate with the largest
    lam * relevance - (1 - lam) * KL(p || q~), p the session's target mix and q~ = (1 - alpha) * (category mix of the list with
    the candidate added) + alpha * p; equal objectives go to the better-ranked candidate (include/xnrs_hip.h:
    xnrs_calibrated_rerank).  row_category:(n_rows,) int32 with values in [0, n_categories) (another value: a news without a
    category, which never changes the mix) -- e.g. store.category_index, whose 0 is the padding, with n_categories =
    cfg.n_categories + 1.
      target "history"   the category counts of the session's FULL history (hist_off / hist_val, the one exclude_history
                         excludes; xnrs_csr_category_counts)
      target (C,)        one mix for everybody, e.g. the catalogue's or an editor's
      target (len(behaviors), C)  one row of weights per session, indexed by session id like `windows`
    Weights need not be normalised; a session whose weights are all <= 0 has no target and gets recommend(k)'s list.  rel and
    pool as recommend_diverse (default pool min(1024, max(8 k, 128))); lam = 1 returns recommend(k) in rows and score bits.

    `generator`: the two-stage form of recommend() (NPA) -- the generator lists the pool, `model` re-scores it, and the
    re-scored pool is calibrated; only categories are compared, so no table of news vectors is needed.  The table is encoded
    once; no more than one batch of pools is resident.  Refusals are those of recommend(), raised before anything is encoded."""
    if lam is None:
        raise ValueError("recommend_calibrated(): lam in [0, 1] is required (recommend() lists by relevance alone)")
    k, lam, pool, alpha, n_categories, parts, uidx, windows, row_category = _calibrated_parts(
        "recommend_calibrated()", model, store, behaviors, k, lam, pool, rel, alpha, row_category, n_categories, target, windows,
        generator)
    return _fill_lists(behaviors, sessions, k, batch, _ROWS_SCORES,
                       ((lo, r, s) for lo, _, r, s, _ in
                        _calibrated_batches(model, generator, parts, uidx, store, behaviors, l_hist, k, lam, pool, rel, alpha,
                                            row_category, n_categories, target, sessions, batch, exclude_history, windows)))


def _calibration_sums(rows, row_category, n_categories: int, target: torch.Tensor, pad_row: int, alpha: float) -> torch.Tensor:
    """fp64 [lists, lists with a target, sum of their KL] over the lists rows:(b,k) against target:(b,C).  A pad-row entry is no
    place."""
    from . import ops
    if pad_row >= 0:
        rows = torch.where(rows == pad_row, torch.full_like(rows, -1), rows)
    kl, _, _ = ops.list_calibration(rows.contiguous(), row_category, n_categories, target, alpha)
    has = ((target > 0) & torch.isfinite(target)).any(dim=1)
    zero = torch.zeros((), dtype=torch.float64, device=rows.device)
    return torch.stack((zero + rows.shape[0], has.double().sum(), torch.where(has, kl.double(), zero).sum()))


def _calibration_dict(sums: torch.Tensor, k: int) -> Dict[str, float]:
    n, n_cal, kl = sums.tolist()
    return {f"calibration_kl@{k}": kl / max(n_cal, 1.0), "n_lists": int(n), "n_calibrated": int(n_cal)}


@torch.no_grad()
def calibration_metrics(rows: torch.Tensor, row_category, n_categories: int, target, pad_row: int, alpha: float = 0.01) -> Dict[str, float]:
    """How far recommended lists from anywhere are from a target category mix: rows:(n,k) int32 on the device (k <= 1024; -1, an
    id outside the table or pad_row: no place), row_category:(n_rows,) int32, target a (n_categories,) tensor of weights or one
    row per list.
      calibration_kl@k   the fp64 mean over the lists that have a target (a positive weight) of KL(p || q~), p the target mix,
                         q~ = (1 - alpha) * (the mix of the list's places that have a category) + alpha * p
                         (include/xnrs_hip.h: xnrs_list_calibration); 0 is a list in exactly the target's proportion, -ln alpha
                         a list without one categorised place
      n_lists, n_calibrated  the lists given, and those with a target."""
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.dtype != torch.int32:
        raise ValueError(f"calibration_metrics(): lists are a (n, k) int32 tensor, got {tuple(getattr(rows, 'shape', ()))} "
                         f"{getattr(rows, 'dtype', type(rows))}")
    k, _, _, alpha, n_categories = _calibrated_args("calibration_metrics()", None, rows.shape[1], None, None, "minmax", alpha,
                                                    row_category, n_categories, target, False)
    if target.dim() == 2 and target.shape[0] != rows.shape[0]:
        raise ValueError(f"calibration_metrics(): target holds {target.shape[0]} rows of weights for {rows.shape[0]} lists")
    tgt = _target_rows(target, rows.shape[0], None, rows.device)
    return _calibration_dict(_calibration_sums(rows, row_category.to(rows.device).contiguous(), n_categories, tgt, int(pad_row), alpha), k)


@torch.no_grad()
def evaluate_calibration(model, store: NewsStore, behaviors: Behaviors, l_hist: int, k: int, lam=None, row_category=None,
                         n_categories: int = 0, target="history", alpha: float = 0.01, pool=None, rel: str = "minmax",
                         sessions=None, batch: int = 4096, exclude_history: bool = True, windows=None, generator=None) -> Dict[str, float]:
    """Calibration and accuracy of the model's lists in one place: the dict of calibration_metrics over the lists of
    recommend(k) (lam None) or recommend_calibrated(k, lam, ...) against the same target, plus hit@k, ndcg@k and n_queries of
    the clicked news WITHIN the returned list with the definitions of evaluate_diversity -- so a sweep over lam shows what
    calibration costs.  Keywords as recommend_calibrated; the sums are added batch by batch.  Refusals as recommend(), before
    anything is encoded."""
    k, lam, pool, alpha, n_categories, parts, uidx, windows, row_category = _calibrated_parts(
        "evaluate_calibration()", model, store, behaviors, k, lam, pool, rel, alpha, row_category, n_categories, target, windows,
        generator)
    dev = behaviors.hist_off.device
    pad = int(store.pad_row)
    sums = torch.zeros((3,), dtype=torch.float64, device=dev)
    acc = torch.zeros((3,), dtype=torch.float64, device=dev)  # queries, hits, dcg
    for _, sess, rows, _, tgt in _calibrated_batches(model, generator, parts, uidx, store, behaviors, l_hist, k, lam, pool, rel,
                                                     alpha, row_category, n_categories, target, sessions, batch, exclude_history,
                                                     windows):
        sums += _calibration_sums(rows, row_category, n_categories, tgt, pad, alpha)
        acc += _list_accuracy_sums(behaviors, sess, rows, store.n_rows, pad)
    hip.check_status(dev)
    out = _calibration_dict(sums, k)
    out.update(_list_accuracy_dict(acc, k))
    return out
