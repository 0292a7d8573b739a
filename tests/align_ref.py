"""Tensors at a chosen offset from a 16-byte boundary, inside guarded buffers (tests/test_hip_pointer_alignment.py).

include/xnrs_hip.h asks for contiguous device pointers and nothing more, so a pointer that is aligned for its element type but
not on a 16-byte boundary is a legal argument everywhere.  shifted() makes one: a contiguous view into a flat buffer with GUARD
elements of a sentinel in front and behind, at data_ptr() % 16 == nbytes.  guards_intact() compares the guards bit for bit."""
import torch

GUARD = 16
#: what the guards (and a not-yet-written output) hold: a finite value no kernel of the project produces
SENTINEL = -7.0625e33
_INT_VIEW = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _sentinel(dtype):
    return SENTINEL if dtype.is_floating_point else -7


def shifted_empty(shape, nbytes, dtype=torch.float32, device="cpu"):
    """A contiguous tensor of `shape` filled with the sentinel whose data_ptr() % 16 == nbytes: a view into a flat buffer of
    the sentinel with at least GUARD elements in front and behind (an output operand: the same buffer, pre-filled)."""
    esz = torch.empty((), dtype=dtype).element_size()
    if nbytes % esz or not 0 <= nbytes < 16:
        raise ValueError(f"a shift of {nbytes} bytes is no address of a {dtype} element below 16")
    n = 1
    for s in shape:
        n *= int(s)
    buf = torch.full((n + 2 * GUARD + 16 // esz,), _sentinel(dtype), dtype=dtype, device=device)
    first = buf.data_ptr() + GUARD * esz
    off = GUARD + ((nbytes - first) % 16) // esz
    v = buf[off:off + n].view(*shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == nbytes, (v.data_ptr(), nbytes)
    assert off >= GUARD and buf.numel() - (off + n) >= GUARD
    v._align_guard = (buf, off, n)  # (an attribute of THIS tensor object: views and clones of it do not carry it)
    return v


def shifted(t, nbytes, device=None):
    """The values of `t` as a contiguous tensor on `device` (default: t's) whose data_ptr() % 16 == nbytes."""
    v = shifted_empty(tuple(t.shape), nbytes, t.dtype, t.device if device is None else device)
    v.copy_(t)
    return v


def guards_intact(v):
    """Are the GUARD-and-more elements on both sides of a shifted() / shifted_empty() tensor what they were, bit for bit?"""
    buf, off, n = v._align_guard
    bits = buf.view(_INT_VIEW[buf.element_size()])
    want = torch.full((1,), _sentinel(buf.dtype), dtype=buf.dtype, device=buf.device).view(bits.dtype)
    return bool((bits[:off] == want).all().item()) and bool((bits[off + n:] == want).all().item())


def unwritten(v):
    """How many elements of an output made by shifted_empty() still hold the sentinel."""
    bits = v.contiguous().view(_INT_VIEW[v.element_size()])
    want = torch.full((1,), _sentinel(v.dtype), dtype=v.dtype, device=v.device).view(bits.dtype)
    return int((bits == want).sum().item())


def misalign_parameters(module, nbytes=4):
    """Rebind every parameter's .data to a view at `nbytes` off a 16-byte boundary inside ONE flat buffer -- what a
    flattened-parameter wrapper or a checkpoint loaded as one blob gives when a (1,) tensor (every reference encoder's
    dummy_param, fc2.bias) sits in front of a weight.  Between two parameters lie GUARD sentinel elements and the padding that
    puts the next one at the same offset.  -> the flat buffer (its guards: flat_guards_intact)."""
    params = [p for p in module.parameters()]
    if not params:
        return None
    dev, dtype = params[0].device, params[0].dtype
    assert all(p.dtype == dtype and p.device == dev for p in params)
    esz = params[0].element_size()
    assert nbytes % esz == 0 and 0 <= nbytes < 16
    per16 = 16 // esz
    total = sum((p.numel() + per16 - 1) // per16 * per16 + 2 * per16 + GUARD for p in params) + GUARD + 2 * per16
    flat = torch.full((total,), _sentinel(dtype), dtype=dtype, device=dev)
    pos, spans = GUARD, []
    for p in params:
        pos += ((nbytes - (flat.data_ptr() + pos * esz)) % 16) // esz
        v = flat[pos:pos + p.numel()].view(p.shape)
        v.copy_(p.data)
        p.data = v
        assert p.data_ptr() % 16 == nbytes and p.is_contiguous()
        spans.append((pos, p.numel()))
        pos += p.numel() + GUARD
    assert pos <= total
    flat._align_spans = spans
    return flat


def flat_guards_intact(flat):
    """Every element of misalign_parameters()'s buffer that belongs to no parameter still holds the sentinel."""
    own = torch.zeros(flat.numel(), dtype=torch.bool, device=flat.device)
    for pos, n in flat._align_spans:
        own[pos:pos + n] = True
    bits = flat.view(_INT_VIEW[flat.element_size()])
    want = torch.full((1,), _sentinel(flat.dtype), dtype=flat.dtype, device=flat.device).view(bits.dtype)
    return bool((bits[~own] == want).all().item())
