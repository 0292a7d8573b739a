"""Helper (not a test): the draw of xnrs_topk_sample* (include/xnrs_hip.h; csrc/kernels.h: drop_pair, drop_word, drop_gumbel)
restated in numpy integer arithmetic, the fp64 perturbed keys of a case, and the validator "top-k within tol".

The word x of a (user key, table row) pair is the 32-bit value of the dropout stream before its `>> 8`: one splitmix64 of
(seed, user key + 1), per row the murmur3 fmix32 finaliser of its low word xor row * 0x9E3779B9, xor its high word --
tests/input_dropout_ref.py holds the same stream for xnrs_dropout_rows, and tests/test_sample_host.py holds the two together.
The uniform is w = min((fp32(x) + 0.5) * 2^-32, 1 - 2^-24) in fp32, the Gumbel draw g = -log(-log1p(-w)); the reference takes
the EXACT fp32 w and both logarithms in fp64."""
import numpy as np

#: the range of the draw: g(x = 2^32 - 1) and an upper bound of g(x = 0) = 33 ln 2 = 22.87386 (kernels.h: DROP_GUMBEL_MAX)
GUMBEL_MIN, GUMBEL_MAX = -2.8116, 22.874
#: the shared score vector of the statistical cases (8 rows): a spread of 0.5, so that at temperature 0.5 the least likely
#: ordered pair is still expected some 30 times among 8192 users and a binomial standard deviation means something
PL_SCORES = np.array([0.0, 0.1, 0.2, -0.1, 0.3, -0.2, 0.15, 0.05])


def draw_words(seed, user_keys, n_rows, rows=None):
    """uint32 [len(user_keys), n_rows]: the word x of every (user key, row) pair; `rows` (default 0 .. n_rows-1) picks the rows.
    seed and the keys are taken mod 2^64 (the kernel argument is unsigned, the keys are int64 two's complement)."""
    seed = int(seed) % (1 << 64)
    keys = np.array([(int(k) + 1) % (1 << 64) for k in np.asarray(user_keys).reshape(-1)], dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.full_like(keys, seed) + np.uint64(0x9E3779B97F4A7C15) * keys
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        lo = (z & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        hi = (z >> np.uint64(32)).astype(np.uint32)
        j = np.arange(n_rows, dtype=np.uint32) if rows is None else np.asarray(rows, dtype=np.uint32)
        x = lo[:, None] ^ (j * np.uint32(0x9E3779B9))[None, :]
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x85EBCA6B)
        x ^= x >> np.uint32(13)
        x *= np.uint32(0xC2B2AE35)
        x ^= x >> np.uint32(16)
        x ^= hi[:, None]
    return x


def uniform32(x):
    """The fp32 uniform of a word, every step in fp32 as the kernel rounds it: uint32 -> fp32 (nearest even), + 0.5, * 2^-32
    (exact), min with 1 - 2^-24."""
    x = np.asarray(x, dtype=np.uint32)
    w = (x.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)
    return np.minimum(w, np.float32(1.0 - 2.0 ** -24)).astype(np.float32)


def gumbel64(x):
    """fp64 g = -log(-log1p(-w)) of the exact fp32 uniform w of the word x."""
    w = uniform32(x).astype(np.float64)
    return -np.log(-np.log1p(-w))


def gumbel_bound32(x):
    """The kernel's logarithm-free upper bound of the draw (kernels.h: drop_gumbel_bound), in fp32 as it rounds:
    e * fp32(log 2) + 1e-4 with e = 127 - the biased exponent of w, so w in [2^-e, 2^(1-e))."""
    e = 127 - ((uniform32(x).view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int32)
    return (e.astype(np.float64) * float(np.float32(0.69314718)) + float(np.float32(1e-4))).astype(np.float32)


def keys64(scores64, temperature, seed, user_keys):
    """fp64 perturbed keys s / temperature + g of a (B, N) fp64 score matrix; NaN and +-inf scores pass through as the
    arithmetic has them."""
    s = np.asarray(scores64, dtype=np.float64)
    return s / float(temperature) + gumbel64(draw_words(seed, user_keys, s.shape[1]))


def tolerance(key64, eligible):
    """tol = 32 * 2^-23 * max(1, max |key64|) over the finite eligible keys of the case: the two logarithms a few ulp each,
    product and sum one each, the fp32 score chain against fp64."""
    k = np.abs(key64[eligible & np.isfinite(key64)])
    return 32.0 * 2.0 ** -23 * max(1.0, float(k.max()) if k.size else 1.0)


def eligible_mask(B, N, excl=None, pad_row=-1, win=None):
    """bool (B, N): inside the table, not the pad row, not on the user's exclusion list, inside the user's window."""
    ok = np.ones((B, N), dtype=bool)
    if 0 <= pad_row < N:
        ok[:, pad_row] = False
    if excl is not None:
        for b, l in enumerate(excl):
            e = np.asarray(list(l), dtype=np.int64)
            ok[b, e[(e >= 0) & (e < N)]] = False
    if win is not None:
        r = np.arange(N)[None, :]
        lo, hi = np.asarray(win[0], dtype=np.int64)[:, None], np.asarray(win[1], dtype=np.int64)[:, None]
        ok &= (r >= lo) & (r < hi)
    return ok


def close_calls(key64, eligible, k, tol):
    """On the reference alone: the share of the users whose k-th and (k+1)-th eligible fp64 keys are closer than 2 tol (the
    users for whom the validator cannot tell the sets apart)."""
    key = np.where(eligible & ~np.isnan(key64), key64, -np.inf)
    order = -np.sort(-key, axis=1)
    if order.shape[1] <= k:
        return 0.0
    a, b = order[:, k - 1], order[:, k]
    with np.errstate(invalid="ignore"):
        close = np.isfinite(a) & np.isfinite(b) & (a - b < 2 * tol)
    return float(np.mean(close))


def check_sampled_topk(rows, keys, key64, eligible, k, tol):
    """The validator "top-k within tol" of every user -> the largest |device key - fp64 key| over the finite returned places.
    rows:(B,k) int32 and keys:(B,k) fp32 as the device returned them; key64:(B,N) fp64 reference keys (NaN: the row never
    wins); eligible:(B,N) bool.
      (a) the returned rows are distinct and eligible, min(k, eligible non-NaN rows) of them, fillers -1 / -inf behind;
      (b) the device keys are non-increasing, equal keys lower row first;
      (c) each device key is within tol of its fp64 key (an infinite key is returned as it is);
      (d) the lowest fp64 key returned >= the highest eligible fp64 key not returned - 2 tol."""
    rows, keys = np.asarray(rows), np.asarray(keys)
    B, N = key64.shape
    assert rows.shape == keys.shape == (B, k), (rows.shape, keys.shape, (B, k))
    worst = 0.0
    for b in range(B):
        ok = eligible[b] & ~np.isnan(key64[b])
        n_real = min(k, int(ok.sum()))
        r, s = rows[b, :n_real].astype(np.int64), keys[b, :n_real]
        assert (r >= 0).all() and (r < N).all() and len(set(r.tolist())) == n_real and ok[r].all(), (b, r)
        assert (rows[b, n_real:] == -1).all() and np.isneginf(keys[b, n_real:]).all(), b
        if n_real == 0:
            continue
        assert (s[:-1] >= s[1:]).all(), b
        eq = s[:-1] == s[1:]
        assert (r[:-1][eq] < r[1:][eq]).all(), b
        want = key64[b, r]
        fin = np.isfinite(want)
        assert (s[~fin] == want[~fin]).all(), b
        if fin.any():
            err = float(np.abs(s[fin].astype(np.float64) - want[fin]).max())
            worst = max(worst, err)
            assert err <= tol, (b, err, tol)
        left = ok.copy()
        left[r] = False
        if left.any():
            assert want.min() >= key64[b, left].max() - 2 * tol, (b, want.min(), key64[b, left].max(), tol)
    return worst


def plackett_luce_first_two(scores, temperature):
    """(p1:(n,), p2:(n,n)) of one score vector: P(row i first) and P(row i first, row j second) of the Plackett-Luce
    distribution exp(s / temperature); the diagonal of p2 is 0."""
    s = np.asarray(scores, dtype=np.float64) / float(temperature)
    e = np.exp(s - s.max())
    p1 = e / e.sum()
    p2 = p1[:, None] * (e[None, :] / (e.sum() - e[:, None]))
    np.fill_diagonal(p2, 0.0)
    return p1, p2


def worst_sigma(rows, scores, temperature):
    """The largest deviation, in binomial standard deviations, of the observed first-place frequencies and ordered first-two
    pairs of rows:(n_users, >=2) from Plackett-Luce over one shared score vector -> (first places, ordered pairs)."""
    rows = np.asarray(rows)
    n, m = rows.shape[0], len(scores)
    p1, p2 = plackett_luce_first_two(scores, temperature)
    c1 = np.bincount(rows[:, 0], minlength=m).astype(np.float64)
    c2 = np.bincount(rows[:, 0].astype(np.int64) * m + rows[:, 1], minlength=m * m).reshape(m, m).astype(np.float64)
    z1 = np.abs(c1 - n * p1) / np.sqrt(n * p1 * (1 - p1))
    off = ~np.eye(m, dtype=bool)
    z2 = np.abs(c2 - n * p2)[off] / np.sqrt(n * p2 * (1 - p2))[off]
    return float(z1.max()), float(z2.max())


def reference_lists(key64, eligible, k):
    """rows (B, k) int64 of the fp64 keys: the k greatest eligible non-NaN keys, equal keys lower row first, -1 fillers."""
    B, N = key64.shape
    out = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        idx = np.nonzero(eligible[b] & ~np.isnan(key64[b]))[0]
        order = idx[np.lexsort((idx, -key64[b, idx]))][:k]
        out[b, :len(order)] = order
    return out
