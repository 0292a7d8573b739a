"""GPU: per-user row windows for the top-k and the rank sweep (include/xnrs_hip.h: xnrs_topk_deep*_win / xnrs_rank*_win,
csrc/sweep.h, topk.hip, rank.hip) and evaluation.recommend / rank_clicked / evaluate_full_ranking on top of them.

The specification is one sentence: the windowed result equals the parent's result with every row outside the user's window
appended to the user's exclusion list.  So every exact case draws integer operands (entries in [-3, 3], |score| < 2^24: every
fp32 product and sum is exact in any order) and compares rows, ranks AND score bits with torch.equal against the NumPy
references of the order contract (tests/topk_ref.py, tests/rank_ref.py), called with that longer exclusion list.  The MLP form
and one real-valued dot case are compared with the parent entry point over the longer list on the GPU: the same score-tile
function, so again the same bits.  No tolerance anywhere in this file.

1. one chunk; 2. several slices and two user tiles; 3. several chunks per slice, sorted and shuffled; 4. deep lists, the floor
and the prefix property; 5. the MLP and a real-valued case against the parent; 6. NULL windows are the parent call; 7. rank;
8. batch invariance; 9. refusals; 10. hipGraph; 11. end to end.

Two arithmetic mutations of csrc/topk.hip and csrc/sweep.h were built and run against this file (neither is committed):
 (a) the upper window bound dropped from the candidate mask of topk_partial_kernel (rows at and behind win_hi, up to the
     table's end, pass): 38 of
     the 57 cases fail -- test_one_chunk for every window that ends inside the table (edges inside, lo == hi, lo < 0, the
     window holds pad_row, fewer than k rows; "hi > n_rows", "lo > hi" and the full window pass, as they must), both two-tile
     cases at k = 10 and 128, sorted and shuffled, both deep shapes, all five parent comparisons, rank-agrees-with-the-list,
     batch invariance and the three end-to-end cases.  The NULL, refusal, hipGraph and rank-only cases pass: that code was not
     touched.
 (b) the tile's chunk range one chunk short at its upper end, in tk_tile_range, which both sweeps share (the union's last
     chunk is not swept): 43 of the 57 cases fail -- test_one_chunk for every case with a row to list or count (the last chunk
     is the only one, or holds the window's end), the full window included; the two-tile cases, sorted and shuffled, both
     deep shapes, the parent comparisons, rank-agrees-with-the-list, batch invariance and the end-to-end cases.
"""
import functools

import numpy as np
import pytest
import torch

from tests.rank_ref import rank_reference
from tests.test_hip_topk import DEEP_SHAPES, dev, excl_csr, histories, int_case, real_case
from tests.topk_ref import topk_reference
from xnrs_amd import evaluation as EV
from xnrs_amd import hip, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------- the specification, restated
def outside(lo, hi, N):
    """Per user the rows outside [lo, hi) clamped to [0, N]: what the specification appends to the exclusion list."""
    out = []
    for l, h in zip(np.asarray(lo).tolist(), np.asarray(hi).tolist()):
        l, h = max(l, 0), min(h, N)
        out.append(list(range(N)) if l >= h else list(range(0, l)) + list(range(h, N)))
    return out


def longer_lists(excl, lo, hi, N):
    out = outside(lo, hi, N)
    return out if excl is None else [list(e) + o for e, o in zip(excl, out)]


def win_dev(lo, hi):
    return dev(np.asarray(lo, dtype=np.int32)), dev(np.asarray(hi, dtype=np.int32))


@functools.lru_cache(maxsize=None)
def int_scores(B, N, E, form):
    """-> (table, users, weight, bias as device tensors; the exact (B, N) score matrix as fp32): once per shape"""
    t, u, W, bias = int_case(B, N, E)
    ref = (u @ t.T) if form == "dot" else ((u @ W) @ t.T + bias)
    assert np.abs(ref).max() < 2 ** 24
    return (dev(t, torch.float32), dev(u, torch.float32), dev(W[None], torch.float32), dev(np.array([bias]), torch.float32),
            ref.astype(np.float32))


def win_topk(B, N, E, form, k, lo, hi, excl=None, pad_row=-1, users=None):
    """One windowed call over the users `users` (default: all) of the shape's case -> ((rows, scores), the score matrix)"""
    td, ud, Wd, bd, ref = int_scores(B, N, E, form)
    if users is not None:
        ud, ref = ud[dev(np.asarray(users, dtype=np.int64))].contiguous(), ref[np.asarray(users)]
    eo, er = (None, None) if excl is None else (dev(a) for a in excl_csr(excl))
    wl, wh = win_dev(lo, hi)
    if form == "dot":
        got = ops.topk_deep_dot(td, ud, k, eo, er, pad_row, win_lo=wl, win_hi=wh)
    else:
        got = ops.topk_deep_bilinear(td, ud, Wd, bd, k, eo, er, pad_row, win_lo=wl, win_hi=wh)
    return got, ref


def win_rank(B, N, E, form, targets, lo, hi, excl=None, pad_row=-1):
    td, ud, Wd, bd, ref = int_scores(B, N, E, form)
    eo, er = (None, None) if excl is None else (dev(a) for a in excl_csr(excl))
    to, tr = (dev(a) for a in excl_csr(targets))
    wl, wh = win_dev(lo, hi)
    if form == "dot":
        got = ops.rank_dot(td, ud, to, tr, eo, er, pad_row, win_lo=wl, win_hi=wh)
    else:
        got = ops.rank_bilinear(td, ud, Wd, bd, to, tr, eo, er, pad_row, win_lo=wl, win_hi=wh)
    return got, ref


def equal(got, want, what):
    a, b = got
    assert torch.equal(a.cpu(), torch.from_numpy(want[0])), f"{what}: rows / ranks"
    # (bit for bit: the scores of a rank query without an answer are NaN on both sides)
    assert torch.equal(b.cpu().view(torch.int32), torch.from_numpy(want[1]).view(torch.int32)), f"{what}: score bits"


def some_targets(rng, lo, hi, N, n=3):
    """Per user n targets: random rows, the first replaced by a row inside the window (when it has one), the second by the
    row just outside it (when there is one; every row is outside an empty window)"""
    out = []
    for l, h in zip(np.asarray(lo).tolist(), np.asarray(hi).tolist()):
        l, h = max(l, 0), min(h, N)
        t = rng.integers(0, N, size=n).tolist()
        if l < h:
            t[0] = int(rng.integers(l, h))
            if h < N:
                t[1] = h
            elif l > 0:
                t[1] = l - 1
        out.append(t)
    return out


def check_both(B, N, E, form, k, lo, hi, excl=None, pad_row=-1, what=""):
    """top-k and rank of one windowed case against the references over the longer exclusion lists"""
    lists = longer_lists(excl, lo, hi, N)
    got, ref = win_topk(B, N, E, form, k, lo, hi, excl, pad_row)
    want = topk_reference(ref, k, lists, pad_row)
    equal(got, want, f"topk {what}")
    targets = some_targets(synth.rng_for(77 + B + N), lo, hi, N)
    got_r, _ = win_rank(B, N, E, form, targets, lo, hi, excl, pad_row)
    equal(got_r, rank_reference(ref, targets, lists, pad_row), f"rank {what}")
    return got, want


# ------------------------------------------------------------------------------------------- 1. one chunk
ONE_CHUNK = {  # per case: (lo, hi) of the three users as a function of N, pad_row, with an exclusion list
    "edges inside the chunk": (lambda N: ([5, 40, 100], [20, 90, N - 1]), -1, False),
    "lo == hi": (lambda N: ([7, 0, N], [7, 50, N]), -1, False),
    "lo > hi": (lambda N: ([90, 60, N + 5], [30, 59, 2]), -1, False),
    "lo < 0": (lambda N: ([-1, -(2 ** 31), -500], [30, 60, N]), -1, False),
    "hi > n_rows": (lambda N: ([100, 0, 64], [N + 1, 2 ** 31 - 1, N + 4000]), -1, False),
    "the window holds pad_row": (lambda N: ([40, 50, 0], [60, 51, 51]), 50, False),
    "fewer than k eligible rows": (lambda N: ([10, 20, 30], [14, 29, 33]), 31, True),
    "the full window": (lambda N: ([0, 0, 0], [N, N, N]), -1, True),
}


@pytest.mark.parametrize("form", ["dot", "bilinear"])
@pytest.mark.parametrize("case", list(ONE_CHUNK))
@pytest.mark.parametrize("B,N,E", [(3, 127, 8), (3, 129, 70)])
def test_one_chunk(B, N, E, case, form):
    make, pad_row, with_excl = ONE_CHUNK[case]
    lo, hi = make(N)
    excl = [[11, 12, 300, -4], [], [31, 31, 25]] if with_excl else None
    got, want = check_both(B, N, E, form, 10, lo, hi, excl, pad_row, f"{case} {(B, N, E)}")
    if case in ("lo == hi", "lo > hi"):
        empty = [b for b in range(B) if max(lo[b], 0) >= min(hi[b], N)]
        assert empty and (want[0][empty] == -1).all() and np.isneginf(want[1][empty]).all()
    if case == "fewer than k eligible rows":
        assert (want[0][:, :2] >= 0).all() and (want[0][:, 9] == -1).all()  # fillers at the tail
    if case == "the window holds pad_row":
        assert pad_row not in want[0] and (want[0][1] == -1).all()  # (user 1 sees the pad row alone)


# ------------------------------------------------------------------------------------------- 2. slices and user tiles
def two_tile_windows(kind):
    """130 users = two user tiles (128 + 2), 1000 rows = 8 chunks, one chunk per slice"""
    lo, hi = np.zeros(130, dtype=np.int64), np.full(130, 1000, dtype=np.int64)
    if kind == "edges":
        edges = [(a, b) for a in (127, 128, 129) for b in (255, 256, 257)]
        for i, (a, b) in enumerate(edges):
            lo[i], hi[i] = a, b
        lo[9], hi[9] = 256, 384  # exactly one chunk
        lo[10], hi[10] = 128, 129  # one row, the first of a chunk
        lo[11], hi[11] = 255, 256  # one row, the last of a chunk
        for i in range(12, 128):
            lo[i] = (37 * i) % 900
            hi[i] = lo[i] + 1 + (53 * i) % 400
        lo[64], hi[64] = 0, 1000  # one user per tile with the full window
        lo[128], hi[128] = 300, 301
        lo[129], hi[129] = 0, 1000
    else:  # two groups with disjoint windows and unused chunks (384 .. 639) between them; the second tile empty
        for i in range(128):
            if i % 2:
                lo[i], hi[i] = (7 * i) % 100, 200 + (11 * i) % 184   # inside [0, 384)
            else:
                lo[i], hi[i] = 640 + (5 * i) % 120, 800 + (13 * i) % 200  # inside [640, 1000)
        lo[128], hi[128] = 500, 500
        lo[129], hi[129] = 700, 600
    return lo, hi


@pytest.mark.parametrize("k", [10, 128])
@pytest.mark.parametrize("kind", ["edges", "disjoint"])
def test_several_slices_and_two_user_tiles(kind, k):
    B, N, E = 130, 1000, 8
    assert hip.lib().xnrs_topk_slices(B, N) == 8
    lo, hi = two_tile_windows(kind)
    if kind == "disjoint":
        assert hi[1:128:2].max() <= 384 and lo[0:128:2].min() >= 640
    excl = [[int((b * 31 + j * 17) % 1000) for j in range(b % 5)] for b in range(B)]
    for form in ("dot", "bilinear"):
        got, want = check_both(B, N, E, form, k, lo, hi, excl, 3, f"{kind} k={k} {form}")
    if kind == "disjoint":
        assert (want[0][128:] == -1).all()


# ------------------------------------------------------------------------------------------- 3. several chunks per slice
@functools.lru_cache(maxsize=None)
def random_windows(B, N, seed):
    rng = synth.rng_for(seed)
    width = np.maximum(1, (rng.uniform(0.01, 1.0, size=B) * N).astype(np.int64))
    lo = (rng.uniform(0, 1, size=B) * (N - width + 1)).astype(np.int64)
    return lo, lo + width


def test_several_chunks_per_slice_sorted_and_shuffled():
    B, N, E, k = DEEP_SHAPES[0]
    assert (B, N, E, k) == (1100, 8000, 8, 10)
    lo, hi = random_windows(B, N, 5)
    assert (hi - lo).min() < 0.03 * N and (hi - lo).max() > 0.9 * N and hi.max() <= N
    ref = int_scores(B, N, E, "dot")[4]
    by_user = topk_reference(ref, k, outside(lo, hi, N))  # the reference, once: rows of the result follow their users
    targets = some_targets(synth.rng_for(78), lo, hi, N, n=2)
    by_user_rank = rank_reference(ref, targets, outside(lo, hi, N))
    for order in (np.argsort(lo, kind="stable"), synth.rng_for(6).permutation(B)):
        got, _ = win_topk(B, N, E, "dot", k, lo[order], hi[order], users=order)
        equal(got, (by_user[0][order], by_user[1][order]), "sorted / shuffled")
    got_r, _ = win_rank(B, N, E, "dot", targets, lo, hi)
    equal(got_r, by_user_rank, "rank, random windows")


# ------------------------------------------------------------------------------------------- 4. deep lists
@pytest.mark.parametrize("B,N,E,k", [(130, 1000, 8, 129), (66, 1025, 256, 1024)])
def test_deep_lists_the_floor_and_the_prefix(B, N, E, k):
    rng = synth.rng_for(9 + k)
    lo, hi = np.zeros(B, dtype=np.int64), np.full(B, N, dtype=np.int64)
    for b in range(B):
        if b % 3 == 0:    # narrower than k: slice lists stay empty or short, and no floor of k rows exists
            width = int(rng.integers(1, k))
            lo[b] = int(rng.integers(0, N - width + 1))
            hi[b] = lo[b] + width
        elif b % 3 == 1:  # wider than k where the table allows it, not the whole table
            width = min(N, k + int(rng.integers(1, 300)))
            lo[b] = int(rng.integers(0, N - width + 1))
            hi[b] = lo[b] + width
    lo[5], hi[5] = 400, 400  # an empty window among them
    assert ((hi - lo)[0::3] < k).all()
    ref = int_scores(B, N, E, "dot")[4]
    lists = outside(lo, hi, N)
    got, _ = win_topk(B, N, E, "dot", k, lo, hi)
    want = topk_reference(ref, k, lists)
    equal(got, want, f"deep {(B, N, E, k)}")
    assert (want[0][0::3, -1] == -1).all() and (want[0][5] == -1).all()
    for j in (1, 10, 128, k - 1):  # the prefix property, across the shallow and the deep kernels
        short, _ = win_topk(B, N, E, "dot", j, lo, hi)
        assert torch.equal(short[0], got[0][:, :j]) and torch.equal(short[1], got[1][:, :j]), j
    if k == 129:
        got_b, ref_b = win_topk(B, N, E, "bilinear", k, lo, hi)
        equal(got_b, topk_reference(ref_b, k, lists), "deep bilinear")


# ------------------------------------------------------------------------------------------- 5. the forms
def csr_dev(lists):
    return tuple(dev(a) for a in excl_csr(lists))


@pytest.mark.parametrize("kind,k", [("fc", 10), ("fc", 130), ("dot", 10), ("dot", 300), ("bilin_norm", 128)])
def test_mlp_and_real_valued_operands_equal_the_parent_over_the_longer_list(kind, k):
    B, N, E = 130, 1000, 70
    scorer, table, u, _, _ = real_case(kind, B, N, E)
    lo, hi = random_windows(B, N, 17)
    lo, hi = lo.copy(), hi.copy()
    lo[3], hi[3] = 250, 250
    lo[4], hi[4] = -7, 5000
    excl = [[int((b * 29 + j * 13) % N) for j in range(b % 4)] for b in range(B)]
    eo, er = csr_dev(excl)
    lo_d, hi_d = win_dev(lo, hi)
    le, lr = csr_dev(longer_lists(excl, lo, hi, N))
    rng = synth.rng_for(3)
    targets = [rng.integers(0, N, size=2).tolist() for _ in range(B)]
    to, tr = csr_dev(targets)
    with torch.no_grad():
        got = scorer.topk_deep(table, u, k, eo, er, 2, win_lo=lo_d, win_hi=hi_d)
        want = scorer.topk_deep(table, u, k, le, lr, 2)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), kind
        if k <= 128:  # topk() with a window goes through the deep entry: the same bits
            via = scorer.topk(table, u, k, eo, er, 2, win_lo=lo_d, win_hi=hi_d)
            assert torch.equal(via[0], got[0]) and torch.equal(via[1], got[1])
        got_r = scorer.rank(table, u, to, tr, eo, er, 2, win_lo=lo_d, win_hi=hi_d)
        want_r = scorer.rank(table, u, to, tr, le, lr, 2)
        assert torch.equal(got_r[0], want_r[0]) and torch.equal(got_r[1].view(torch.int32), want_r[1].view(torch.int32)), kind
    assert (got[0][3] == -1).all() and int((got[0] >= 0).sum()) > B * min(k, 5)


# ------------------------------------------------------------------------------------------- 6. NULL windows
@pytest.mark.parametrize("k", [10, 128, 300])
def test_null_windows_are_the_parent_call(k):
    """the _win entry point itself with both pointers NULL (the Python layer never calls it without windows)"""
    B, N, E = 130, 1000, 70
    l = hip.lib()
    scorer, table, u, _, _ = real_case("dot", B, N, E)
    eo, er = csr_dev([[int((b * 29 + j * 13) % N) for j in range(b % 4)] for b in range(B)])
    with torch.no_grad():
        parent = scorer.topk_deep(table, u, k, eo, er, 2)
    rows = torch.full((B, k), -7, dtype=torch.int32, device=DEV)
    scores = torch.full((B, k), 123.0, dtype=torch.float32, device=DEV)
    nbytes = l.xnrs_topk_deep_workspace_bytes(B, N, 0, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    rc = l.xnrs_topk_deep_win(hip.ptr(table), N, E, hip.ptr(u), B, hip.ptr(eo), hip.ptr(er), None, None, 2, k, hip.ptr(rows),
                              hip.ptr(scores), hip.ptr(ws), nbytes, hip.stream_ptr(DEV))
    assert rc == 0
    assert torch.equal(rows, parent[0]) and torch.equal(scores.view(torch.int32), parent[1].view(torch.int32))
    if k <= 128:
        with torch.no_grad():
            shallow = scorer.topk(table, u, k, eo, er, 2)
        assert torch.equal(rows, shallow[0]) and torch.equal(scores, shallow[1])


def test_null_windows_are_the_parent_call_rank():
    B, N, E = 130, 1000, 70
    l = hip.lib()
    scorer, table, u, _, _ = real_case("dot", B, N, E)
    rng = synth.rng_for(4)
    targets = [rng.integers(0, N, size=int(rng.integers(0, 7))).tolist() for _ in range(B)]
    to, tr = csr_dev(targets)
    eo, er = csr_dev([[int((b * 29 + j * 13) % N) for j in range(b % 4)] for b in range(B)])
    with torch.no_grad():
        parent = scorer.rank(table, u, to, tr, eo, er, 2)
    ranks = torch.full((tr.numel(),), -7, dtype=torch.int32, device=DEV)
    scores = torch.full((tr.numel(),), 123.0, dtype=torch.float32, device=DEV)
    rc = l.xnrs_rank_win(hip.ptr(table), N, E, hip.ptr(u), B, hip.ptr(to), hip.ptr(tr), hip.ptr(eo), hip.ptr(er), None, None, 2,
                         hip.ptr(ranks), hip.ptr(scores), None, 0, hip.stream_ptr(DEV))
    assert rc == 0
    assert torch.equal(ranks, parent[0]) and torch.equal(scores.view(torch.int32), parent[1].view(torch.int32))


# ------------------------------------------------------------------------------------------- 7. rank
@pytest.mark.parametrize("form", ["dot", "bilinear"])
def test_rank_agrees_with_the_windowed_list(form):
    """An eligible target has rank < k exactly when the windowed list holds it, at that position with the same score bits;
    a target outside its window is still ranked; duplicates; more targets than the LDS slots (4)."""
    B, N, E, k = 130, 1000, 8, 128
    lo, hi = two_tile_windows("edges")
    excl = [[int((b * 31 + j * 17) % 1000) for j in range(b % 5)] for b in range(B)]
    lists = longer_lists(excl, lo, hi, N)
    (rows, scores), ref = win_topk(B, N, E, form, k, lo, hi, excl, 3)
    rows_h, scores_h = rows.cpu().numpy(), scores.cpu().numpy()
    rng = synth.rng_for(12)
    targets = []
    for b in range(B):
        listed = [int(r) for r in rows_h[b] if r >= 0]
        t = (listed[:2] + listed[-1:] + rng.integers(0, N, size=3).tolist())[:3]  # three listed rows, where there are three
        t += rng.integers(0, N, size=4).tolist()  # seven targets: past the four LDS slots
        t += t[:1] + [int(max(lo[b], 0) - 1) % N, int(min(hi[b], N)) % N]  # a duplicate; two rows just outside the window
        targets.append(t)
    assert min(len(t) for t in targets) > 4
    (ranks, rscores), _ = win_rank(B, N, E, form, targets, lo, hi, excl, 3)
    want = rank_reference(ref, targets, lists, 3)
    equal((ranks, rscores), want, f"rank {form}")
    ranks_h, rscores_h = ranks.cpu().numpy(), rscores.cpu().numpy()
    e, n_out = 0, 0
    for b in range(B):
        inside = set(range(max(int(lo[b]), 0), min(int(hi[b]), N))) - set(excl[b]) - {3}
        for t in targets[b]:
            if t in inside:  # eligible: in the list exactly when rank < k, at that position, the same bits
                where = np.nonzero(rows_h[b] == t)[0]
                assert (ranks_h[e] < k) == (where.size == 1), (b, t)
                if where.size:
                    assert where[0] == ranks_h[e] and scores_h[b, where[0]].view(np.int32) == rscores_h[e].view(np.int32)
            elif t != 3:  # outside its window (or excluded): still scored and ranked among the eligible rows
                assert ranks_h[e] >= 0 and rscores_h[e] == ref[b, t]
                n_out += 1
            e += 1
    assert n_out > B
    # the first target of a user is listed and is its duplicate: two queries, one answer
    off = np.cumsum([0] + [len(t) for t in targets])
    assert all(ranks_h[off[b]] == ranks_h[off[b] + 7] for b in range(B) if targets[b])


def test_rank_of_a_scored_target_in_an_empty_window_is_zero():
    B, N, E = 3, 129, 70
    (ranks, scores), ref = win_rank(B, N, E, "dot", [[5, 128], [0], [64, 64, 7, 8, 9]], [9, 0, 200], [9, 0, 100])
    assert ranks.tolist() == [0] * 8 and scores.tolist() == [ref[0, 5], ref[0, 128], ref[1, 0]] + [ref[2, t] for t in (64, 64, 7, 8, 9)]


# ------------------------------------------------------------------------------------------- 8. batch invariance
def test_a_users_windowed_result_does_not_depend_on_the_batch():
    B, N, E, k = 130, 1000, 8, 128
    lo, hi = two_tile_windows("edges")
    full, _ = win_topk(B, N, E, "dot", k, lo, hi)
    again, _ = win_topk(B, N, E, "dot", k, lo, hi)
    assert torch.equal(full[0], again[0]) and torch.equal(full[1], again[1])  # run to run
    targets = [[int(lo[b]) % N, 500] for b in range(B)]
    full_r, _ = win_rank(B, N, E, "dot", targets, lo, hi)
    for b in (0, 9, 64, 127, 129):  # alone: its tile's range is its own window
        one, _ = win_topk(B, N, E, "dot", k, lo[b:b + 1], hi[b:b + 1], users=[b])
        assert torch.equal(one[0][0], full[0][b]) and torch.equal(one[1][0], full[1][b]), b
    # at another position, among other users with other windows
    order = synth.rng_for(8).permutation(B)
    moved, _ = win_topk(B, N, E, "dot", k, lo[order], hi[order], users=order)
    assert torch.equal(moved[0].cpu(), full[0].cpu()[order]) and torch.equal(moved[1].cpu(), full[1].cpu()[order])
    td, ud = int_scores(B, N, E, "dot")[:2]
    for b in (0, 9, 129):
        to, tr = csr_dev([targets[b]])
        wl, wh = win_dev(lo[b:b + 1], hi[b:b + 1])
        one = ops.rank_dot(td, ud[b:b + 1].contiguous(), to, tr, win_lo=wl, win_hi=wh)
        assert torch.equal(one[0], full_r[0][2 * b:2 * b + 2]) and torch.equal(one[1], full_r[1][2 * b:2 * b + 2]), b


# ------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_come_before_the_launch_and_write_nothing():
    B, N, E, k = 3, 200, 8, 10
    td, ud = int_scores(B, N, E, "dot")[:2]
    ok = torch.zeros(B, dtype=torch.int32, device=DEV)
    to, tr = csr_dev([[1], [2], [3]])
    for lo, hi, err in ((ok, None, ValueError), (None, ok, ValueError), (ok.long(), ok.long(), ValueError),
                        (ok[:2], ok[:2], ValueError), (ok.float(), ok, ValueError), (ok.cpu(), ok.cpu(), hip.XnrsHipError),
                        (torch.zeros(2 * B, dtype=torch.int32, device=DEV)[::2], ok, hip.XnrsHipError)):
        with pytest.raises(err, match="windows"):
            ops.topk_deep_dot(td, ud, k, win_lo=lo, win_hi=hi)
        with pytest.raises(err, match="windows"):
            ops.rank_dot(td, ud, to, tr, win_lo=lo, win_hi=hi)
    # the C entry points with exactly one pointer: XNRS_EINVAL, outputs and workspace untouched
    l = hip.lib()
    rows = torch.full((B, k), -7, dtype=torch.int32, device=DEV)
    scores = torch.full((B, k), 123.0, dtype=torch.float32, device=DEV)
    nbytes = l.xnrs_topk_deep_workspace_bytes(B, N, 0, k)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    st = hip.stream_ptr(DEV)
    for lo, hi in ((ok, None), (None, ok)):
        assert l.xnrs_topk_deep_win(hip.ptr(td), N, E, hip.ptr(ud), B, None, None, hip.ptr(lo), hip.ptr(hi), -1, k, hip.ptr(rows),
                                    hip.ptr(scores), hip.ptr(ws), nbytes, st) == -1
        assert l.xnrs_rank_win(hip.ptr(td), N, E, hip.ptr(ud), B, hip.ptr(to), hip.ptr(tr), None, None, hip.ptr(lo), hip.ptr(hi), -1,
                               hip.ptr(rows), hip.ptr(scores), None, 0, st) == -1
    torch.cuda.synchronize()
    assert (rows == -7).all() and (scores == 123.0).all() and not ws.any()


# ------------------------------------------------------------------------------------------- 10. hipGraph
def test_one_windowed_call_captured_in_a_hip_graph():
    B, N, E, k = 130, 1000, 70, 10
    scorer, table, u, _, _ = real_case("bilin", B, N, E)
    lo, hi = random_windows(B, N, 17)
    lo_s, hi_s = win_dev(lo, hi)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad():
        with torch.cuda.stream(side):
            first = scorer.topk_deep(table, u, k, win_lo=lo_s, win_hi=hi_s)  # warm-up on the capture stream (workspace growth)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rows_g, scores_g = scorer.topk_deep(table, u, k, win_lo=lo_s, win_hi=hi_s)
        flip_lo, flip_hi = win_dev(lo[::-1].copy(), hi[::-1].copy())
        lo_s.copy_(flip_lo)  # other windows in the same buffers: the replay reads them on the device
        hi_s.copy_(flip_hi)
        graph.replay()
        torch.cuda.synchronize()
        eager = scorer.topk_deep(table, u, k, win_lo=flip_lo, win_hi=flip_hi)
    assert torch.equal(rows_g, eager[0]) and torch.equal(scores_g, eager[1]) and not torch.equal(rows_g, first[0])


# ------------------------------------------------------------------------------------------- 11. end to end
def world_with_times(n_news, n_sess, horizon_seed=0):
    store, beh = synth.click_world(n_news=n_news, n_sess=n_sess)
    rng = synth.rng_for(40 + horizon_seed)
    row_time = torch.from_numpy(np.arange(store.n_rows) // 3)  # non-decreasing, with ties; the pad row is the oldest
    time = rng.integers(0, store.n_rows // 3 + 2, size=n_sess).astype(np.int64)
    # every other session happens shortly after its clicked news was published, so that the click lies inside its window
    clicked = beh.pos_val[beh.pos_off[:-1]].numpy()
    time[0::2] = row_time.numpy()[clicked[0::2]] + np.arange(n_sess)[0::2] % 4
    beh.time = torch.from_numpy(time)
    return store.to(DEV), beh.to(DEV), row_time.to(DEV)


def session_lists(beh, lo, hi, N):
    return longer_lists(histories(beh), lo.cpu().numpy(), hi.cpu().numpy(), N)


def recommend_over_lists(monkeypatch, model, store, beh, l_hist, k, lists):
    """recommend() with each session's exclusion list replaced by `lists`: the call a user had to make before the windows"""
    off, val = excl_csr(lists)
    other = beh.to(DEV)
    other.hist_off, other.hist_val = dev(off), dev(val)

    class Batcher(EV.DeviceBatcher):  # (the user tower still reads the real histories: the lists only exclude)
        def __init__(self, behaviors, l, pad_row):
            super().__init__(beh, l, pad_row)
    with monkeypatch.context() as m:
        m.setattr(EV, "DeviceBatcher", Batcher)
        return EV.recommend(model, store, other, l_hist=l_hist, k=k, batch=16)


@pytest.mark.parametrize("kind", ["dot", "fc"])
def test_recommend_and_rank_clicked_with_windows_end_to_end(kind, monkeypatch):
    from tests.test_hip_scorers import _eval_model
    store, beh, row_time = world_with_times(300, 40)
    model = _eval_model(kind)
    k, l_hist, n, N = 10, 8, len(beh), store.n_rows
    windows = EV.row_windows(row_time, beh.time, horizon=30)
    lo, hi = windows
    assert lo.dtype == torch.int32 and lo.is_cuda and int((hi - lo).min()) < 60 < int((hi - lo).max())
    rows, scores = EV.recommend(model, store, beh, l_hist=l_hist, k=k, batch=16, windows=windows)
    r, lo_h, hi_h = rows.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()
    listed = r >= 0
    assert listed.any() and ((r >= lo_h[:, None]) & (r < hi_h[:, None]))[listed].all()  # no row outside a session's window
    assert store.pad_row not in r
    # ... and it is recommend() over per-session exclusion lists, bit for bit
    want = recommend_over_lists(monkeypatch, model, store, beh, l_hist, k, session_lists(beh, lo, hi, N))
    assert torch.equal(rows, want[0]) and torch.equal(scores.view(torch.int32), want[1].view(torch.int32))
    assert not torch.equal(rows, EV.recommend(model, store, beh, l_hist=l_hist, k=k, batch=16)[0])
    # a subset of the sessions takes its own windows along
    pick = [5, 30, 3, 38, 0, 12]
    sub = EV.recommend(model, store, beh, l_hist=l_hist, k=k, sessions=pick, batch=2, windows=windows)
    assert torch.equal(sub[0], rows[pick]) and torch.equal(sub[1], scores[pick])
    # rank_clicked: a clicked news inside its window is listed exactly when rank < k, at that position with those bits
    for sessions in (None, pick):
        q_sess, q_row, rank, score = EV.rank_clicked(model, store, beh, l_hist=l_hist, sessions=sessions, batch=16, windows=windows)
        hists = histories(beh)
        n_in = 0
        for s, t, rk, sc in zip(q_sess.tolist(), q_row.tolist(), rank.tolist(), score.tolist()):
            if lo_h[s] <= t < hi_h[s] and t not in hists[s] and t != store.pad_row:
                where = np.nonzero(r[s] == t)[0]
                assert (rk < k) == (where.size == 1), (s, t, rk)
                if where.size:
                    assert where[0] == rk and float(scores[s, rk]) == sc
                n_in += 1
            else:
                assert rk >= 0 or t == store.pad_row
        assert n_in > 0
    ranks_all = EV.rank_clicked(model, store, beh, l_hist=l_hist, batch=16, windows=windows)[2]
    ks = (1, 5, 10)
    got = EV.evaluate_full_ranking(model, store, beh, l_hist=l_hist, ks=ks, batch=16, windows=windows)
    assert got == EV.full_ranking_metrics(EV.full_ranking_sums(ranks_all, ks), ks) and got["n_queries"] == n
    plain = EV.evaluate_full_ranking(model, store, beh, l_hist=l_hist, ks=ks, batch=16)
    assert got["mean_rank"] < plain["mean_rank"]  # fewer competitors


def test_two_stage_recommend_lists_only_rows_inside_the_window():
    from tests.test_hip_topk_deep import _npa_and_nrms
    store, beh, row_time = world_with_times(40, 10, 1)
    npa, nrms = _npa_and_nrms()
    beh.user_index = torch.arange(len(beh), device=DEV) % 7
    windows = EV.row_windows(row_time, beh.time, horizon=6)
    lo, hi = (w.cpu().numpy() for w in windows)
    rows, scores = EV.recommend(npa, store, beh, l_hist=5, k=5, generator=nrms, pool=16, batch=4, windows=windows)
    r = rows.cpu().numpy()
    listed = r >= 0
    assert listed.any() and ((r >= lo[:, None]) & (r < hi[:, None]))[listed].all() and store.pad_row not in r
    # the generator's own windowed list is where the rows come from
    gen = EV.recommend(nrms, store, beh, l_hist=5, k=16, windows=windows)[0].cpu().numpy()
    assert all(set(r[i][r[i] >= 0].tolist()) <= set(gen[i].tolist()) for i in range(len(beh)))
    assert (listed.sum(1) == np.minimum(5, (gen >= 0).sum(1))).all()
