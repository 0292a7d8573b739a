"""fp64 CPU reference of the softmax ranking loss over per-user row lists (include/xnrs_hip.h: xnrs_list_loss_fwd / _bwd),
written from its definition: gather the listed rows, mask the empty slots, logsumexp, logaddexp, autograd for the gradients."""
import torch


def _cpu(t, dtype=None):
    return None if t is None else t.detach().to("cpu", dtype) if dtype else t.detach().cpu()


def filled_slots(neg_rows, n_rows, tgt_off, tgt_rows, pad_row=-1):
    """(B, L) bool: slot j of user b is a negative -- its row is inside the table, not pad_row and no target row of b."""
    neg_rows = _cpu(neg_rows).long()
    B = neg_rows.shape[0]
    off, rows = _cpu(tgt_off).tolist(), _cpu(tgt_rows).tolist()
    ok = (neg_rows >= 0) & (neg_rows < n_rows) & (neg_rows != pad_row)
    for b in range(B):
        for t in set(rows[off[b]:off[b + 1]]):
            ok[b] &= neg_rows[b] != t
    return ok


def list_loss_ref(table, up, tgt_off, tgt_rows, neg_rows, pad_row=-1, bias=None, g=None):
    """-> dict(loss (T,), scores (T,), lse (B,), neg_scores (B, L) with NaN in the empty slots, filled (B, L) bool, valid (T,)
    bool, d_up, d_table), all fp64 on the CPU; the gradients are those of sum(g * loss) (g = 1 when not given)."""
    table = _cpu(table, torch.float64).requires_grad_(True)
    up = _cpu(up, torch.float64).reshape(-1, table.shape[1]).requires_grad_(True)
    B, n_rows = up.shape[0], table.shape[0]
    nr = _cpu(neg_rows).long().reshape(B, -1)
    L = nr.shape[1]
    off, rows = _cpu(tgt_off).tolist(), _cpu(tgt_rows).long()
    T = rows.numel()
    shift = 0.0 if bias is None else _cpu(bias, torch.float64).reshape(-1)[0]
    filled = filled_slots(nr, n_rows, tgt_off, tgt_rows, pad_row)
    gathered = table[nr.clamp(0, max(n_rows - 1, 0))] if n_rows else torch.zeros((B, L, table.shape[1]), dtype=torch.float64)
    s = (gathered * up[:, None, :]).sum(-1) + shift  # (B, L): the same row twice is two slots
    has = filled.any(dim=1)
    lse = torch.full((B,), float("-inf"), dtype=torch.float64)
    if has.any():
        lse = lse.index_put((has.nonzero().reshape(-1),), torch.logsumexp(s[has].masked_fill(~filled[has], float("-inf")), dim=1))
    user = torch.zeros((T,), dtype=torch.int64)
    for b in range(B):
        user[off[b]:off[b + 1]] = b
    inside = torch.zeros((T,), dtype=torch.bool)
    inside[off[0]:off[B]] = True
    valid = inside & (rows >= 0) & (rows < n_rows) & (rows != pad_row)
    loss = torch.zeros((T,), dtype=torch.float64)
    scores = torch.full((T,), float("nan"), dtype=torch.float64)
    e = valid.nonzero().reshape(-1)
    if e.numel():
        st = (table[rows[e]] * up[user[e]]).sum(-1) + shift
        scores = scores.index_put((e,), st.detach())
        le = torch.where(has[user[e]], torch.logaddexp(st, lse[user[e]]) - st, torch.zeros_like(st))
        loss = loss.index_put((e,), le)
    g = torch.ones((T,), dtype=torch.float64) if g is None else _cpu(g, torch.float64).reshape(-1)
    d_up, d_table = torch.zeros_like(up), torch.zeros_like(table)
    if loss.requires_grad:
        d_up, d_table = torch.autograd.grad((g * loss).sum(), [up, table])
    neg_scores = s.detach().masked_fill(~filled, float("nan"))
    return dict(loss=loss.detach(), scores=scores, lse=lse.detach(), neg_scores=neg_scores, filled=filled, valid=valid, d_up=d_up,
                d_table=d_table)
