"""CPU: the oracle's restatement of the attention-dropout generator (oracle/xnrs_oracle.py: attention_drop_uniform,
attention_keep_mask -- bit for bit `drop_uniform` of xnrs_amd/csrc/kernels.h) and the `drop=` argument of the oracle's
attention.  The GPU side of the contract is tests/test_hip_attention_dropout.py: every dropout kernel variant against the
fp64 oracle under this mask."""
import math

import numpy as np
import pytest
import torch

from oracle import xnrs_oracle as O
from tests import helpers as H
from xnrs_amd import synth

SEEDS = [0, 1, 12345, 2 ** 63 - 1]
N_SEQ, HEADS, S = 64, 4, 50  # 640 000 draws per seed


def _u_scalar(seed, n_heads, S, seq, hd, query, key):
    """drop_uniform of kernels.h for ONE probability in Python integers (masks written out: nothing wraps by itself)."""
    M64, M32 = (1 << 64) - 1, (1 << 32) - 1
    z = (seed % (1 << 64) + 0x9E3779B97F4A7C15 * (seq * n_heads + hd + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    x = (z & M32) ^ (((query * S + key) * 0x9E3779B9) & M32)
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    x ^= z >> 32
    return np.float32(x >> 8) * np.float32(2.0 ** -24)


@pytest.mark.parametrize("seed", SEEDS + [-1, -(2 ** 63)])
def test_vectorised_draw_equals_the_scalar_integer_form(seed):
    """The numpy uint64 / uint32 array form against the generator written in unbounded Python integers with explicit
    masks, at a sample of (sequence, head, query, key) that includes the last of each."""
    n_seq, h, s = 5, 3, 37
    u = O.attention_drop_uniform(seed, n_seq, h, s)
    assert u.dtype == np.float32 and u.shape == (n_seq, h, s, s)
    assert (u >= 0).all() and (u < 1).all()
    rng = synth.rng_for(900)
    picks = [(0, 0, 0, 0), (n_seq - 1, h - 1, s - 1, s - 1), (1, 2, 0, s - 1), (1, 2, s - 1, 0)]
    picks += [tuple(int(rng.integers(0, k)) for k in (n_seq, h, s, s)) for _ in range(60)]
    for seq, hd, q, k in picks:
        assert u[seq, hd, q, k] == _u_scalar(seed, h, s, seq, hd, q, k), (seq, hd, q, k)


def test_negative_int64_seed_equals_its_value_mod_2_64():
    """The host draws an int64 (ops._att_dropout); the kernel argument is unsigned."""
    for seed in (-1, -12345, -(2 ** 63)):
        a = O.attention_drop_uniform(seed, 3, 2, 17)
        b = O.attention_drop_uniform(seed + 2 ** 64, 3, 2, 17)
        assert np.array_equal(a, b)
    assert not np.array_equal(O.attention_drop_uniform(-1, 3, 2, 17), O.attention_drop_uniform(1, 3, 2, 17))


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", SEEDS)
def test_keep_rate(seed, p):
    """Over 640 000 draws the keep rate lies within 5 sigma (binomial) of keep = 1 - p."""
    mask = O.attention_keep_mask(seed, N_SEQ, HEADS, S, p)
    assert mask.dtype == np.bool_
    n = mask.size
    assert n >= 5e5
    keep = 1.0 - p
    sigma = math.sqrt(keep * (1 - keep) / n)
    assert abs(mask.mean() - keep) <= 5 * sigma, (mask.mean(), keep, sigma)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_masks_of_different_streams_agree_at_the_independent_rate(p):
    """Two independent Bernoulli(keep) masks agree with probability keep^2 + (1 - keep)^2: neighbouring (sequence, head)
    pairs, pairs a whole sequence apart, and the same pairs under two seeds (neighbouring and far apart), 5 sigma each."""
    keep = 1.0 - p
    q = keep * keep + (1 - keep) * (1 - keep)
    for seed in SEEDS:
        m = O.attention_keep_mask(seed, N_SEQ, HEADS, S, p).reshape(N_SEQ * HEADS, S * S)
        for a, b in ((m[:-1], m[1:]), (m[:-HEADS], m[HEADS:])):
            sigma = math.sqrt(q * (1 - q) / a.size)
            assert a.size >= 5e5 and abs((a == b).mean() - q) <= 5 * sigma, (seed, (a == b).mean(), q, sigma)
    for s0, s1 in ((0, 1), (12345, 12346), (0, 2 ** 63 - 1), (1, 12345)):
        a = O.attention_keep_mask(s0, N_SEQ, HEADS, S, p)
        b = O.attention_keep_mask(s1, N_SEQ, HEADS, S, p)
        sigma = math.sqrt(q * (1 - q) / a.size)
        assert abs((a == b).mean() - q) <= 5 * sigma, (s0, s1, (a == b).mean(), q, sigma)


def test_no_two_sequences_of_a_chunked_call_share_a_stream():
    """The chunked inference forward (encoder_fwd.hip) hands every pass the seed advanced by c0 * n_heads counter steps, so
    a pass's local (sequence, head) pairs continue the counter where the pass before stopped: the per-pass masks, stacked,
    are the mask of the unchunked call, for every head count and chunk size -- no two (sequence, head) pairs of one call
    draw from the same stream."""
    G = 0x9E3779B97F4A7C15
    n, s = 11, 9
    for h in (1, 2, 3):
        whole = O.attention_drop_uniform(77, n, h, s)
        assert len({whole[i, j].tobytes() for i in range(n) for j in range(h)}) == n * h
        for chunk in (1, 4, 5):
            parts = [O.attention_drop_uniform(77 + c0 * h * G, min(chunk, n - c0), h, s) for c0 in range(0, n, chunk)]
            assert np.array_equal(np.concatenate(parts), whole), (h, chunk)


def _mha_case(dtype):
    S_, D, h, n = 13, 24, 3, 4
    sd = {k: v.to(dtype) for k, v in H.state_for(H.mha_shapes(D), 21).items()}
    rng = synth.rng_for(22)
    x = torch.from_numpy(rng.standard_normal((n, S_, D))).to(dtype)
    m = torch.ones(n, S_, 1, dtype=dtype)
    m[0, 5:] = 0
    m[1, 3] = 0
    m[2] = 0
    return sd, x, m, h


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_all_ones_keep_mask_reproduces_the_eval_mode_oracle(dtype):
    """drop=(all ones, 0) IS the eval-mode oracle, bit for bit (P / 1 selected everywhere) -- attention alone and through
    both encoders; drop=None is the code path the golden tests pin."""
    sd, x, m, h = _mha_case(dtype)
    n, S_, D = x.shape
    ones = np.ones((n, h, S_, S_), dtype=bool)
    assert torch.equal(O.multi_head_attention(x, m, sd, h, drop=(ones, 0.0)), O.multi_head_attention(x, m, sd, h))
    esd = {"att." + k: v for k, v in sd.items()}
    esd.update({k: v.to(dtype) for k, v in H.state_for(H.additive_shapes(D, 16, "pooler"), 23).items()})
    y0, hm0 = O.text_encoder(x.unsqueeze(0), m.unsqueeze(0), esd, h)
    y1, hm1 = O.text_encoder(x.unsqueeze(0), m.unsqueeze(0), esd, h, drop=(ones, 0.0))
    assert torch.equal(y0, y1) and torch.equal(hm0, hm1)
    assert torch.equal(O.user_encoder(x, m, esd, h), O.user_encoder(x, m, esd, h, drop=(ones, 0.0)))


def test_drop_argument_zeroes_and_rescales_the_probabilities():
    """With V = identity-like values the output rows ARE the probabilities: dropped entries are exactly 0, kept ones are
    P / fp32(1 - p), masked queries' uniform rows are dropped like the rest (layers.py:142-148)."""
    S_, h, p = 6, 1, 0.5
    D = S_
    z = torch.zeros(D, D, dtype=torch.float64)
    sd = {"q_linear.weight": z, "q_linear.bias": torch.zeros(D, dtype=torch.float64), "k_linear.weight": z,
          "k_linear.bias": torch.zeros(D, dtype=torch.float64), "v_linear.weight": torch.eye(D, dtype=torch.float64),
          "v_linear.bias": torch.zeros(D, dtype=torch.float64), "out.weight": torch.eye(D, dtype=torch.float64),
          "out.bias": torch.zeros(D, dtype=torch.float64)}
    x = torch.eye(S_, dtype=torch.float64).unsqueeze(0)  # V = I: out[q] = sum_k P[q, k] e_k = P[q]
    m = torch.ones(1, S_, 1, dtype=torch.float64)
    m[0, 2] = 0  # a masked query: uniform row, dropped like the others
    keep = O.attention_keep_mask(5, 1, h, S_, p)
    assert keep.any() and not keep.all()
    y = O.multi_head_attention(x, m, sd, h, drop=(keep, p))
    want = torch.where(torch.from_numpy(keep[0, 0]), torch.full((S_, S_), (1.0 / S_) / 0.5, dtype=torch.float64),
                       torch.zeros(S_, S_, dtype=torch.float64))
    assert torch.equal(y[0], want)
