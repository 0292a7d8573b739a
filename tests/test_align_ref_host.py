"""CPU: the helper of tests/test_hip_pointer_alignment.py does what it says -- the address property, the guards, and the
parameters of a module rebound into one flat buffer."""
import pytest
import torch

from tests import align_ref as AR


@pytest.mark.parametrize("dtype,shifts", [(torch.float32, (0, 4, 8, 12)), (torch.bfloat16, (0, 2, 4, 8, 14)), (torch.int16, (2, 6)),
                                          (torch.int32, (4,))])
@pytest.mark.parametrize("shape", [(1,), (3, 5), (2, 4, 8), (130, 24)])
def test_shifted_has_the_address_the_values_and_the_guards(dtype, shifts, shape):
    g = torch.Generator().manual_seed(5)
    t = (torch.randn(shape, generator=g) * 100).to(dtype)
    for nbytes in shifts:
        v = AR.shifted(t, nbytes)
        assert v.data_ptr() % 16 == nbytes and v.is_contiguous() and v.shape == t.shape and v.dtype == dtype
        assert torch.equal(v, t)
        buf, off, n = v._align_guard
        assert off >= AR.GUARD and buf.numel() - off - n >= AR.GUARD and n == t.numel()
        assert AR.guards_intact(v)
        o = AR.shifted_empty(shape, nbytes, dtype)
        assert o.data_ptr() % 16 == nbytes and AR.unwritten(o) == o.numel() and AR.guards_intact(o)


def test_a_write_next_to_the_view_is_seen_on_either_side():
    for where in ("front", "behind"):
        v = AR.shifted(torch.ones(3, 4), 4)
        buf, off, n = v._align_guard
        v.fill_(2.0)  # writes inside the view leave the guards alone
        assert AR.guards_intact(v) and AR.unwritten(v) == 0
        buf[off - 1 if where == "front" else off + n] = 0.0
        assert not AR.guards_intact(v), where
    # bit for bit: the sentinel with its lowest mantissa bit flipped is not the sentinel
    v = AR.shifted(torch.ones(2), 8)
    buf, off, n = v._align_guard
    buf.view(torch.int32)[0] ^= 1
    assert not AR.guards_intact(v)


def test_a_shift_that_is_no_element_address_is_refused():
    with pytest.raises(ValueError):
        AR.shifted(torch.ones(4), 2)
    with pytest.raises(ValueError):
        AR.shifted(torch.ones(4), 16)
    with pytest.raises(ValueError):
        AR.shifted(torch.ones(4, dtype=torch.bfloat16), 3)


@pytest.mark.parametrize("nbytes", [4, 8, 12])
def test_misalign_parameters_rebinds_every_parameter_and_keeps_the_module(nbytes):
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(8, 6), torch.nn.Tanh(), torch.nn.Linear(6, 1))
    x = torch.randn(5, 8)
    want = net(x).detach().clone()
    values = [p.detach().clone() for p in net.parameters()]
    flat = AR.misalign_parameters(net, nbytes)
    for p, v in zip(net.parameters(), values):
        assert p.data_ptr() % 16 == nbytes and p.is_contiguous() and torch.equal(p.detach(), v)
        assert flat.data_ptr() <= p.data_ptr() < flat.data_ptr() + flat.numel() * 4
    assert torch.equal(net(x), want) and AR.flat_guards_intact(flat)
    net(x).sum().backward()  # still leaves of the graph, and an optimizer step writes through the views only
    assert all(p.grad is not None for p in net.parameters())
    torch.optim.SGD(net.parameters(), lr=0.1).step()
    assert AR.flat_guards_intact(flat) and not torch.equal(next(net.parameters()).detach(), values[0])
    flat[0] = 0.0
    assert not AR.flat_guards_intact(flat)
