"""Helper (not a test): the draw of xnrs_dropout_rows (include/xnrs_hip.h) restated in numpy integer arithmetic, in the style
of oracle.xnrs_oracle.attention_drop_uniform, and nn.Dropout under that exact mask in fp32.

The kernel calls drop_uniform (xnrs_amd/csrc/kernels.h) with one head, the row's position in the call as the sequence and
the element's index in the row where the attention kernels pass query * S + key; tests/test_input_dropout_host.py holds this
restatement to the oracle's bit for bit where the two overlap."""
import numpy as np
import torch

#: the fixed host seeds of the GPU tests (tests/test_hip_input_dropout.py); the last one is >= 2^63
SEEDS = (20240607, 77, 2 ** 63 + 12345)
#: torch.manual_seed values whose first CPU-generator draws the GPU tests recover as seeds (draw_seeds)
TORCH_SEEDS = (1234, 4321)


def draw_seeds(torch_seed, count=1):
    """The next `count` dropout seeds after torch.manual_seed(torch_seed), as xnrs_amd.ops draws them."""
    torch.manual_seed(torch_seed)
    return [int(torch.empty((), dtype=torch.int64).random_().item()) for _ in range(count)]


def input_drop_uniform(seed, n, row_floats):
    """float32 [n, row_floats]: the uniform of every element of one launch.  One splitmix64 of (seed, row + 1) per row; per
    element the murmur3 fmix32 finaliser of its low word xor j * 0x9E3779B9, xor its high word; u = (x >> 8) * 2^-24.
    `seed` is taken mod 2^64 (the host draws an int64, the kernel argument is unsigned)."""
    seed = int(seed) % (1 << 64)
    row = np.arange(n, dtype=np.uint64) + np.uint64(1)
    z = np.full_like(row, seed) + np.uint64(0x9E3779B97F4A7C15) * row
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    lo = (z & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (z >> np.uint64(32)).astype(np.uint32)
    idx = np.arange(row_floats, dtype=np.uint32) * np.uint32(0x9E3779B9)
    x = lo[:, None] ^ idx[None, :]
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    x ^= hi[:, None]
    return (x >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def keep_mask(seed, n, row_floats, p):
    """bool [n, row_floats]: u < 1.f - p in fp32, as the kernel compares it."""
    return input_drop_uniform(seed, n, row_floats) < (np.float32(1) - np.float32(p))


def dropped(x, p, seed):
    """nn.Dropout(p) on x (rows = its first dim) under the restated mask, fp32 numpy of x's shape: a kept element is ONE fp32
    multiply by 1.f / (1.f - p), a dropped one the literal 0; p <= 0 copies, p >= 1 gives zeros."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.ascontiguousarray(x, dtype=np.float32)
    if p <= 0:
        return x.copy()
    if p >= 1 or x.size == 0:
        return np.zeros_like(x)
    flat = x.reshape(x.shape[0], -1)
    scale = np.float32(1) / (np.float32(1) - np.float32(p))
    out = np.where(keep_mask(seed, flat.shape[0], flat.shape[1], p), flat * scale, np.float32(0))
    return out.astype(np.float32).reshape(x.shape)
