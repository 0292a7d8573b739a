"""fp64 CPU reference of the full-table softmax ranking loss (include/xnrs_hip.h: xnrs_table_loss_fwd / _bwd), written
from its definition: a dense (B, n_rows) eligibility mask, logsumexp, logaddexp, autograd for the gradients."""
import torch


def _cpu(t, dtype=None):
    return None if t is None else t.detach().to("cpu", dtype) if dtype else t.detach().cpu()


def negatives_mask(B, n_rows, tgt_off, tgt_rows, excl_off=None, excl_rows=None, pad_row=-1, win_lo=None, win_hi=None):
    """(B, n_rows) bool: row n is a negative of user b -- inside the table, not pad_row, not on b's exclusion list, inside
    b's window, and not a target of b."""
    neg = torch.ones((B, n_rows), dtype=torch.bool)
    if 0 <= pad_row < n_rows:
        neg[:, pad_row] = False
    tgt_off, tgt_rows = _cpu(tgt_off).tolist(), _cpu(tgt_rows).tolist()
    lists = [(tgt_off, tgt_rows)]
    if excl_off is not None:
        lists.append((_cpu(excl_off).tolist(), _cpu(excl_rows).tolist()))
    for off, rows in lists:
        for b in range(B):
            for r in rows[off[b]:off[b + 1]]:
                if 0 <= r < n_rows:
                    neg[b, r] = False
    if win_lo is not None:
        lo, hi = _cpu(win_lo).tolist(), _cpu(win_hi).tolist()
        n = torch.arange(n_rows)
        for b in range(B):
            neg[b] &= (n >= lo[b]) & (n < hi[b])
    return neg


def table_loss_ref(table, up, tgt_off, tgt_rows, excl_off=None, excl_rows=None, pad_row=-1, win_lo=None, win_hi=None, bias=None,
                   g=None):
    """-> dict(loss (T,), scores (T,), lse (B,), valid (T,) bool, d_up, d_table), all fp64 on the CPU; the gradients are those
    of sum(g * loss) (g = 1 when not given)."""
    table = _cpu(table, torch.float64).requires_grad_(True)
    up = _cpu(up, torch.float64).reshape(-1, table.shape[1]).requires_grad_(True)
    B, n_rows = up.shape[0], table.shape[0]
    off, rows = _cpu(tgt_off).tolist(), _cpu(tgt_rows)
    T = rows.numel()
    s = up @ table.T
    if bias is not None:
        s = s + _cpu(bias, torch.float64).reshape(-1)[0]
    neg = negatives_mask(B, n_rows, tgt_off, tgt_rows, excl_off, excl_rows, pad_row, win_lo, win_hi)
    has = neg.any(dim=1)
    lse = torch.full((B,), float("-inf"), dtype=torch.float64)
    if has.any():
        lse = lse.index_put((has.nonzero().reshape(-1),), torch.logsumexp(s[has].masked_fill(~neg[has], float("-inf")), dim=1))
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
        st = s[user[e], rows[e].long()]
        scores = scores.index_put((e,), st.detach())
        le = torch.where(has[user[e]], torch.logaddexp(st, lse[user[e]]) - st, torch.zeros_like(st))
        loss = loss.index_put((e,), le)
    g = torch.ones((T,), dtype=torch.float64) if g is None else _cpu(g, torch.float64).reshape(-1)
    d_up, d_table = torch.zeros_like(up), torch.zeros_like(table)
    if loss.requires_grad:
        d_up, d_table = torch.autograd.grad((g * loss).sum(), [up, table])
    return dict(loss=loss.detach(), scores=scores, lse=lse.detach(), valid=valid, d_up=d_up, d_table=d_table)
