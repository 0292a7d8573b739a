"""CPU: the restated draw of the input dropout (tests/input_dropout_ref.py) against the attention dropout's oracle, its keep
fraction on the seeds the GPU tests use, the header's declaration and the host-side contract of ops.input_dropout."""
import numpy as np
import pytest
import torch

from oracle import xnrs_oracle as O
from tests import input_dropout_ref as R
from xnrs_amd import hip, ops
from xnrs_amd.models.components import layers, news_encoding, user_encoding


@pytest.mark.parametrize("seed", [0, 20240607, 2 ** 63 + 12345, -5, -2 ** 63])
@pytest.mark.parametrize("n,S", [(1, 1), (5, 7), (3, 50)])
def test_restatement_equals_the_attention_oracle_where_they_overlap(seed, n, S):
    """One head, sequence = row, element index j = query * S + key: the same bits as attention_drop_uniform; negative int64
    seeds are taken mod 2^64."""
    u = R.input_drop_uniform(seed, n, S * S).reshape(n, 1, S, S)
    assert np.array_equal(u, O.attention_drop_uniform(seed, n, 1, S))
    assert np.array_equal(u, R.input_drop_uniform(seed % 2 ** 64, n, S * S).reshape(n, 1, S, S))


def gpu_test_seeds():
    return list(R.SEEDS) + [s for k in R.TORCH_SEEDS for s in R.draw_seeds(k, 2)]


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_fraction_of_every_seed_the_gpu_tests_use(p):
    """N = 512 x 400 = 204 800 draws per seed: |kept / N - (1 - p)| <= 4 sqrt(p (1 - p) / N) (a 4-sigma band of the binomial);
    no two adjacent rows and no two adjacent columns carry the same mask (independent draws would agree on all of 400 or
    512 positions with probability (p^2 + (1 - p)^2)^400 < 1e-34 per pair)."""
    n, rf = 512, 400
    N = n * rf
    for seed in gpu_test_seeds():
        keep = R.keep_mask(seed, n, rf, p)
        frac = keep.sum() / N
        assert abs(frac - (1 - p)) <= 4 * np.sqrt(p * (1 - p) / N), (seed, p, frac)
        assert not (keep[1:] == keep[:-1]).all(axis=1).any(), f"seed {seed}: two adjacent rows share a mask"
        assert not (keep[:, 1:] == keep[:, :-1]).all(axis=0).any(), f"seed {seed}: two adjacent columns share a mask"
        u = R.input_drop_uniform(seed, n, rf)
        assert u.min() >= 0 and u.max() < 1


def test_dropped_edge_values():
    x = np.arange(12, dtype=np.float32).reshape(3, 4) + 1
    assert np.array_equal(R.dropped(x, 0.0, 1), x)
    assert not R.dropped(x, 1.0, 1).any()
    d = R.dropped(x, 0.5, R.SEEDS[0])
    assert set(np.unique(d / x)) <= {0.0, 2.0}
    x[0, 0] = np.inf  # a dropped slot is the literal 0, never inf * 0
    assert np.isfinite(R.dropped(x, 0.5, R.SEEDS[0])[~R.keep_mask(R.SEEDS[0], 3, 4, 0.5)]).all()


def test_header_declares_dropout_rows_with_nine_arguments():
    _, _, protos = hip.parse_header(open(hip.HEADER_PATH).read())
    assert "xnrs_dropout_rows" in protos and "xnrs_dropout_rows" in hip.SYMBOLS
    restype, argtypes = protos["xnrs_dropout_rows"]
    import ctypes as C
    assert restype is C.c_int32
    assert argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float, C.c_uint64, C.c_void_p, C.c_void_p]
    assert hip.ABI_VERSION == 6


def test_input_dropout_host_contract():
    x = torch.randn(3, 4)
    with pytest.raises(hip.XnrsHipError):
        ops.input_dropout(x, 0.5, True)
    with pytest.raises(hip.XnrsHipError):
        ops.input_dropout(x, 0.5, True, seed=3)
    assert ops.input_dropout(x, 0.5, False) is x
    assert ops.input_dropout(x, 0.0, True) is x
    with pytest.raises(hip.XnrsHipError):
        ops.gather_dropout(torch.randn(4, 3), torch.zeros(2, dtype=torch.int32), 0.5, 1)


def test_no_draw_from_the_generator_without_active_dropout():
    """training=False / p == 0 leave torch's CPU generator alone (the draw order of a step does not depend on idle towers)."""
    torch.manual_seed(5)
    state = torch.get_rng_state()
    x = torch.randn(2, 2)
    torch.set_rng_state(state)
    ops.input_dropout(x, 0.5, False)
    ops.input_dropout(x, 0.0, True)
    assert torch.equal(torch.get_rng_state(), state)


def test_hip_dropout_defaults_to_off():
    assert news_encoding.TextEncoder.hip_dropout is False and user_encoding.UserEncoder.hip_dropout is False
    enc = news_encoding.TextEncoder(pooler=layers.AdditiveAttention(8, 4), p_dropout=0.2, out_features=4, in_features=8)
    assert enc.hip_dropout is False and isinstance(enc.dropout, torch.nn.Dropout)
