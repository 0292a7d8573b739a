"""fp64 CPU reference of the soft-target loss over per-user row lists (include/xnrs_hip.h: xnrs_list_xent_fwd / _bwd),
written from its definition: gather the listed rows, mask the empty slots, logsumexp, sum w (lse - s), autograd."""
import torch


def _cpu(t, dtype=None):
    return None if t is None else t.detach().to("cpu", dtype) if dtype else t.detach().cpu()


def filled_slots(rows, n_rows, pad_row=-1):
    """(B, L) bool: the row of slot j of user b is inside the table and not pad_row."""
    rows = _cpu(rows).long()
    return (rows >= 0) & (rows < n_rows) & (rows != pad_row)


def list_xent_ref(table, up, rows, weights, pad_row=-1, bias=None, g=None):
    """-> dict(loss (B,), lse (B,), slot_scores (B, L) with NaN in the empty slots, filled (B, L) bool, d_up, d_table), all
    fp64 on the CPU; the gradients are those of sum(g * loss) (g = 1 when not given)."""
    table = _cpu(table, torch.float64).requires_grad_(True)
    up = _cpu(up, torch.float64).reshape(-1, table.shape[1]).requires_grad_(True)
    B, n_rows = up.shape[0], table.shape[0]
    nr = _cpu(rows).long().reshape(B, -1)
    L = nr.shape[1]
    shift = 0.0 if bias is None else _cpu(bias, torch.float64).reshape(-1)[0]
    filled = filled_slots(nr, n_rows, pad_row)
    w = torch.where(filled, _cpu(weights, torch.float64).reshape(B, L), torch.zeros((), dtype=torch.float64))  # (ignored when empty)
    gathered = table[nr.clamp(0, max(n_rows - 1, 0))] if n_rows else torch.zeros((B, L, table.shape[1]), dtype=torch.float64)
    s = (gathered * up[:, None, :]).sum(-1) + shift  # (B, L): the same row twice is two slots
    has = filled.any(dim=1)
    lse = torch.full((B,), float("-inf"), dtype=torch.float64)
    loss = torch.zeros((B,), dtype=torch.float64)
    if has.any():
        idx = has.nonzero().reshape(-1)
        l = torch.logsumexp(s[has].masked_fill(~filled[has], float("-inf")), dim=1)
        lse = lse.index_put((idx,), l)
        terms = w[has] * (l[:, None] - s[has]).masked_fill(~filled[has], 0.0)
        loss = loss.index_put((idx,), terms.sum(dim=1))
    g = torch.ones((B,), dtype=torch.float64) if g is None else _cpu(g, torch.float64).reshape(-1)
    d_up, d_table = torch.zeros_like(up), torch.zeros_like(table)
    if loss.requires_grad:
        d_up, d_table = torch.autograd.grad((g * loss).sum(), [up, table])
    return dict(loss=loss.detach(), lse=lse.detach(), slot_scores=s.detach().masked_fill(~filled, float("nan")), filled=filled,
                d_up=d_up, d_table=d_table)
