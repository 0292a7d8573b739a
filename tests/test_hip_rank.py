"""GPU: where given rows rank within a whole news table per user (include/xnrs_hip.h: xnrs_rank / _bilinear / _mlp,
csrc/rank.hip) and evaluation.rank_clicked / evaluate_full_ranking on top of it.

1. exact-integer operands: every fp32 product and sum is exact in any order, so ranks AND scores must equal the NumPy reference
   of the contract (tests/rank_ref.py) bit for bit -- integer scores tie massively, which pins the tie rule;
2. exclusions, 3. agreement with top-k (GPU against GPU, exact), 4. real-valued operands against the scorer's own CSR path
   over all pairs, 5. NaN and -inf, 6. batch invariance, 7. hipGraph, 8. the evaluation end to end, 9. two ranks on one GPU.
Every real-valued case prints MARGIN = observed error / bar."""
import os
import socket
import tempfile

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.rank_ref import eligible, rank_reference
from tests.test_hip_topk import SWITCH_TOL, all_pairs, dev, excl_csr, int_case, make_scorer, real_case  # noqa: F401
from xnrs_amd import evaluation as EV
from xnrs_amd import hip, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the smallest shapes at which each loop takes a second trip: rows past one chunk, features past one LDS stage, users past
# one wave's half and past one tile, several slices
INT_SHAPES = [(1, 1, 8), (3, 127, 8), (3, 129, 70), (66, 129, 256), (130, 1000, 8), (3, 2100, 300)]
DEEP_SHAPES = [(1100, 8000, 8), (1100, 15900, 8)]  # several chunks per slice, a ragged last slice
SCORERS = ["dot", "dot_norm", "bilin", "bilin_norm", "fc"]


def pad_of(N):
    return N // 2 if N > 1 else -1


def target_lists(B, N, seed):
    """Per user one of: no target, one, 9, 40, EVERY row of the table (300 drawn rows of a table past 2100 rows), a duplicate,
    ids outside the table, the pad row.  A batch of fewer than 8 users folds the kinds onto its users."""
    rng = synth.rng_for(seed)
    draw = lambda n: rng.integers(0, N, size=n).tolist()  # noqa: E731
    kinds = [
        lambda: [],
        lambda: draw(1),
        lambda: draw(9),
        lambda: draw(40),
        lambda: list(range(N)) if N <= 2100 else draw(300),
        lambda: (lambda r: [r[0], r[0], r[1], r[0]])(draw(2)),
        lambda: [N, -1, N + 5, 2 ** 31 - 1, -2 ** 31] + draw(1),
        lambda: [pad_of(N)] + draw(1),
    ]
    fold = min(B, len(kinds))
    return [[t for p, kind in enumerate(kinds) if p % fold == b % fold for t in kind()] for b in range(B)]


def int_scores(form, t, u, W, bias):
    ref = (u @ t.T) if form == "dot" else ((u @ W) @ t.T + bias)
    assert np.abs(ref).max() < 2 ** 24
    return ref.astype(np.float32)


def int_rank(form, t, u, W, bias, targets, excl=None, pad_row=-1, tgt_dev=None, excl_dev=None, out=None):
    """The device result of one exact-integer call; tgt_dev / excl_dev: the CSRs as handed to the device, when they are not
    simply those of `targets` / `excl`."""
    if tgt_dev is None:
        tgt_dev = tuple(dev(a) for a in excl_csr(targets))
    if excl_dev is None and excl is not None:
        excl_dev = tuple(dev(a) for a in excl_csr(excl))
    eo, er = excl_dev if excl_dev is not None else (None, None)
    td, ud = dev(t, torch.float32), dev(u, torch.float32)
    if form == "dot":
        return ops.rank_dot(td, ud, tgt_dev[0], tgt_dev[1], eo, er, pad_row, out=out)
    return ops.rank_bilinear(td, ud, dev(W[None], torch.float32), dev(np.array([bias]), torch.float32), tgt_dev[0], tgt_dev[1],
                             eo, er, pad_row, out=out)


def assert_exact(got, ref, what):
    """ranks equal, scores bit-equal (NaN where the reference has NaN)"""
    ranks, scores = got
    assert ranks.dtype == torch.int32 and scores.dtype == torch.float32 and ref[1].dtype == np.float32
    assert torch.equal(ranks.cpu(), torch.from_numpy(ref[0])), f"{what}: ranks"
    s, nan = scores.cpu().numpy(), np.isnan(ref[1])
    assert np.array_equal(np.isnan(s), nan) and np.array_equal(s[~nan].view(np.uint32), ref[1][~nan].view(np.uint32)), f"{what}: scores"
    assert np.array_equal(nan, ref[0] == -1)


# ------------------------------------------------------------------------------------------- 1. exact integers
@pytest.mark.parametrize("form", ["dot", "bilinear"])
@pytest.mark.parametrize("B,N,E", INT_SHAPES)
def test_exact_integer_operands(B, N, E, form):
    t, u, W, bias = int_case(B, N, E)
    targets = target_lists(B, N, 100 + B + N)
    if N == 129:
        assert max(len(l) for l in targets) > 128  # more targets than a 128-row tile
    got = int_rank(form, t, u, W, bias, targets, pad_row=pad_of(N))
    ref = rank_reference(int_scores(form, t, u, W, bias), targets, pad_row=pad_of(N))
    assert_exact(got, ref, f"{form} {(B, N, E)}")
    assert (ref[0] >= 0).any() and ((ref[0] == -1).any() or B * N == 1)


@pytest.mark.parametrize("B,N,E,form", [s + ("dot",) for s in DEEP_SHAPES] + [DEEP_SHAPES[0] + ("bilinear",)])
def test_exact_integer_operands_over_several_chunks_per_slice(B, N, E, form):
    l = hip.lib()
    slices, chunks = l.xnrs_topk_slices(B, N), -(-N // 128)
    per = -(-chunks // slices)
    assert 1 < slices < chunks and per > 1 and 0 < chunks - (slices - 1) * per < per and N % 128 != 0
    t, u, W, bias = int_case(B, N, E)
    targets = target_lists(B, N, 100 + B + N)
    got = int_rank(form, t, u, W, bias, targets, pad_row=pad_of(N))
    ref = rank_reference(int_scores(form, t, u, W, bias), targets, pad_row=pad_of(N))
    assert_exact(got, ref, f"{form} {(B, N, E)}")
    assert ref[0].max() > 128 * per  # ranks that add up over several chunks and slices


# ------------------------------------------------------------------------------------------- 2. exclusions
@pytest.mark.parametrize("form", ["dot", "bilinear"])
def test_exclusions(form):
    B, N, E = 6, 300, 8
    t, u, W, bias = int_case(B, N, E)
    full = int_scores(form, t, u, W, bias)
    best = np.lexsort((np.arange(N)[None, :].repeat(B, 0), -full), axis=1)  # every user's rows, best first
    fixed = (0, 7, 107, 150, 207, 299)  # rows the lists below name
    pad_row = next(int(r) for r in best[4] if r not in fixed)  # the pad row is the fifth user's best row (but for those)
    b4 = [int(r) for r in best[4] if r != pad_row]
    rng = synth.rng_for(31)
    excl = [
        [int(best[0, 3]), N + 7, int(best[0, 0]), -3, int(best[0, 3]), int(best[0, 1]), int(best[0, 0])],  # unsorted, duplicates,
        [r for r in range(N - 1, -1, -1) if r % 100 != 7],                                                 # foreign ids; > 128
        list(range(N)),                                                                                    # everything
        [],
        [b4[1]],
        rng.integers(-5, N + 5, size=70).tolist(),                                                         # longer than 64
    ]
    assert len(excl[1]) > 128 and len(set(excl[5])) < 70 <= len(excl[5])
    targets = [
        [int(best[0, 0]), int(best[0, 2]), int(best[0, 5]), int(best[0, N - 1])],  # the first: on its own list
        [7, 107, 207, 150, 299],                                                    # three kept rows, two on the list
        [0, 299],
        list(range(0, N, 7)),
        [b4[0], b4[2], pad_row, b4[1]],
        excl[5][:3] + [int(best[5, 0])],
    ]
    ref = rank_reference(full, targets, excl, pad_row)
    got = int_rank(form, t, u, W, bias, targets, excl, pad_row)
    assert_exact(got, ref, f"{form} exclusions")
    r, at = ref[0], np.cumsum([0] + [len(l) for l in targets])
    assert r[0] == 0 and r[1] == 0  # best[0, 0] and best[0, 1] are excluded: the third best row has nothing before it
    assert sorted(r[at[1]:at[1] + 3].tolist()) == [0, 1, 2]  # the three rows the list keeps, among themselves
    assert (r[at[2]:at[3]] == 0).all()  # a list of everything leaves rank 0
    # the pad row is not counted, and not answered; a target on its own list (b4[1]) is ranked behind b4[0] alone
    assert r[at[4]:at[5]].tolist() == [0, 1, -1, 1]
    # both CSRs as slices of longer arrays with non-zero first offsets; nothing outside the span is written
    e_off, e_val = excl_csr([[1, 2, 3, 4, 5, 6, 7]] + excl + [[9, 9]])
    t_off, t_val = excl_csr([[5, 6, 7]] + targets + [[1], [2, 3]])
    ranks = torch.full((t_val.size,), -7, dtype=torch.int32, device=DEV)
    scores = torch.full((t_val.size,), 123.0, dtype=torch.float32, device=DEV)
    got2 = int_rank(form, t, u, W, bias, targets, tgt_dev=(dev(t_off)[1:B + 2], dev(t_val)), excl_dev=(dev(e_off)[1:B + 2], dev(e_val)),
                    pad_row=pad_row, out=(ranks, scores))
    assert got2[0] is ranks and got2[1] is scores
    assert_exact((ranks[3:-3], scores[3:-3]), ref, f"{form} exclusions through slices of longer offset arrays")
    assert (ranks[:3] == -7).all() and (ranks[-3:] == -7).all() and (scores[:3] == 123.0).all() and (scores[-3:] == 123.0).all()


# ------------------------------------------------------------------------------------------- 3. agreement with top-k
def random_exclusions(B, N, seed):
    rng = synth.rng_for(seed)
    return [rng.integers(-3, N + 3, size=int(rng.integers(0, 200))).tolist() for _ in range(B)]


@pytest.mark.parametrize("kind", SCORERS)
@pytest.mark.parametrize("B,N,E", [(130, 1000, 70), (3, 2100, 300)])
def test_agreement_with_topk(B, N, E, kind):
    """rank < k exactly when top-k returns the row, at position rank, with the same score bits: GPU against GPU, exact."""
    scorer, table, u, _, _ = real_case(kind, B, N, E)
    k, pad_row = 128, 17
    excl = random_exclusions(B, N, 5 * B + N)
    eo, er = (dev(a) for a in excl_csr(excl))
    with torch.no_grad():
        rows, scores = scorer.topk(table, u, k, eo, er, pad_row)
        assert (rows >= 0).all()
        t_off = torch.arange(B + 1, device=DEV, dtype=torch.int64) * k
        ranks, rscores = scorer.rank(table, u, t_off, rows.reshape(-1).contiguous(), eo, er, pad_row)
        assert torch.equal(ranks.reshape(B, k), torch.arange(k, device=DEV, dtype=torch.int32).expand(B, k))
        assert torch.equal(rscores.view(torch.int32), scores.reshape(-1).view(torch.int32))
        # rows the top-k did not return
        got = rows.cpu().numpy()
        rng = synth.rng_for(77 + B)
        others = []
        for b in range(B):
            ok = np.ones(N, dtype=bool)
            ok[got[b]] = False
            ok[pad_row] = False
            e = np.asarray(excl[b], dtype=np.int64)
            ok[e[(e >= 0) & (e < N)]] = False
            others.append(rng.choice(np.nonzero(ok)[0], size=16, replace=False).tolist())
        o_off, o_val = (dev(a) for a in excl_csr(others))
        ranks, _ = scorer.rank(table, u, o_off, o_val, eo, er, pad_row)
        assert (ranks >= k).all() and (ranks < N).all()


# ------------------------------------------------------------------------------------------- 4. real-valued operands
def rank_bounds(ref_b, t, tol, ok=None):
    """(lower, upper) bounds of the rank of row t given one user's reference scores: #{ref > s_t + 2 tol} and
    #{ref >= s_t - 2 tol} over the eligible rows other than t."""
    r = ref_b.astype(np.float64)
    ok = np.ones(r.shape, dtype=bool) if ok is None else ok.copy()
    t = np.asarray(t, dtype=np.int64)
    srt = np.sort(r[ok])
    lower = srt.size - np.searchsorted(srt, r[t] + 2 * tol, side="right")
    upper = srt.size - np.searchsorted(srt, r[t] - 2 * tol, side="left") - ok[t]  # (an eligible t counts itself in `>=`)
    return lower, upper


# (the four kinds whose scores spread widely enough for the condition below -- at least 95 % of the queries decided on the
# reference alone -- at both shapes; the scores of bilin_norm lie closer together than 2 tol too often at (3, 2100, 300).  All
# five kinds are held to exact agreement with top-k above)
@pytest.mark.parametrize("kind", ["dot", "dot_norm", "bilin", "fc"])
@pytest.mark.parametrize("B,N,E", [(130, 1000, 70), (3, 2100, 300)])
def test_real_valued_operands(B, N, E, kind):
    scorer, table, u, ref, ref64 = real_case(kind, B, N, E)
    tol = SWITCH_TOL * float(np.abs(ref).max())
    if N == 1000:
        targets = [list(range(N))] * B  # every row is a target of every user
    else:
        rng = synth.rng_for(9000 + SCORERS.index(kind) + 7 * B + 3 * N + 11 * E)  # (the seed of real_case)
        targets = [rng.choice(N, size=64, replace=False).tolist() for _ in range(B)]
    bounds = [rank_bounds(ref[b], targets[b], tol) for b in range(B)]
    lower, upper = (np.concatenate([bd[i] for bd in bounds]) for i in (0, 1))
    decided = float(np.mean(lower == upper))
    assert decided >= 0.95  # on the reference alone
    t_off, t_val = (dev(a) for a in excl_csr(targets))
    with torch.no_grad():
        ranks, scores = scorer.rank(table, u, t_off, t_val)
    ranks, s = ranks.cpu().numpy(), scores.cpu().numpy()
    users = np.repeat(np.arange(B), [len(l) for l in targets])
    flat = np.concatenate([np.asarray(l, dtype=np.int64) for l in targets])
    err = float(np.abs(s.astype(np.float64) - ref[users, flat]).max())
    e64 = H.assert_close(scores, ref64[users, flat], H.RTOL, f"{kind} {(B, N, E)} scores vs fp64")
    exact = float(np.mean(ranks[lower == upper] == lower[lower == upper]))
    print(f"MARGIN rank {kind} {(B, N, E)}: vs CSR scorer {err / tol:.3f}  vs fp64 {e64 / H.RTOL:.3f}  (error / bar); "
          f"{100 * decided:.1f} % of the queries decided, {100 * exact:.2f} % of those exact")
    assert err <= tol
    assert (lower <= ranks).all() and (ranks <= upper).all()


# ------------------------------------------------------------------------------------------- 5. NaN, -inf
def test_a_nan_row_is_never_counted_and_a_nan_target_has_no_answer():
    B, N, E = 3, 130, 12
    t, u, _, _ = int_case(B, N, E)
    t = t.astype(np.float32)
    t[5] = np.nan
    t[77, 3] = np.nan
    ref = u.astype(np.float32) @ np.where(np.isnan(t), 0, t).T
    ref[:, [5, 77]] = np.nan
    targets = [list(range(N)), [5, 77, 0, 129], [4, 6, 76, 78]]
    got = ops.rank_dot(dev(t), dev(u, torch.float32), *(dev(a) for a in excl_csr(targets)))
    want = rank_reference(ref, targets)
    assert_exact(got, want, "NaN rows")
    r = got[0].cpu().numpy()
    assert r[5] == -1 and r[77] == -1 and r[N] == -1 and r[N + 1] == -1 and (np.delete(r[:N], [5, 77]) >= 0).all()
    assert sorted(np.delete(r[:N], [5, 77]).tolist()) == list(range(N - 2))  # 128 finite rows: a permutation of 0 .. 127
    # a normalising scorer: a zero vector has no direction (0 / 0), as a table row and as a user
    from xnrs_amd.models.blocks import DotScoring
    t[5] = 0
    t[77] = 1
    uu = u.astype(np.float32)
    uu[1] = 0
    scorer = DotScoring(normalize=True)
    with torch.no_grad():
        ranks, scores = scorer.rank(scorer.prepare_csr(dev(t)), dev(uu), *(dev(a) for a in excl_csr([list(range(N))] * B)))
    ranks, scores = ranks.reshape(B, N).cpu().numpy(), scores.reshape(B, N).cpu().numpy()
    assert (ranks[1] == -1).all() and np.isnan(scores[1]).all()
    assert (ranks[[0, 2], 5] == -1).all() and sorted(np.delete(ranks[0], 5).tolist()) == list(range(N - 1))


def test_infinite_scores_are_legal():
    """-inf is a score like any other: its rows rank behind every finite score, in row order; +inf ranks first."""
    B, N, E = 3, 40, 12
    t, u, _, _ = int_case(B, N, E)
    t, u = t.astype(np.float32), u.astype(np.float32)
    u[:, 0] = 2
    t[[3, 17, 30], 0] = -np.inf
    t[22, 0] = np.inf
    with np.errstate(invalid="ignore"):
        ref = u @ t.T
    assert np.isneginf(ref[:, [3, 17, 30]]).all() and np.isposinf(ref[:, 22]).all() and not np.isnan(ref).any()
    targets = [list(range(N))] * B
    got = ops.rank_dot(dev(t), dev(u), *(dev(a) for a in excl_csr(targets)))
    assert_exact(got, rank_reference(ref, targets), "infinite scores")
    r = got[0].reshape(B, N).cpu().numpy()
    assert (r[:, 22] == 0).all() and (r[:, [3, 17, 30]] == [N - 3, N - 2, N - 1]).all()
    s = got[1].reshape(B, N).cpu().numpy()
    assert np.isneginf(s[:, [3, 17, 30]]).all() and np.isposinf(s[:, 22]).all()


# ------------------------------------------------------------------------------------------- 6. batch invariance
@pytest.mark.parametrize("kind", ["dot", "fc"])
def test_a_querys_result_does_not_depend_on_the_batch(kind):
    B, N, E = 130, 1000, 70
    scorer, table, u, _, _ = real_case(kind, B, N, E)
    rng = synth.rng_for(606)
    targets = [rng.integers(0, N, size=5).tolist() for _ in range(B)]
    t_off, t_val = (dev(a) for a in excl_csr(targets))
    excl = random_exclusions(B, N, 607)
    e_off, e_val = (dev(a) for a in excl_csr(excl))
    with torch.no_grad():
        ranks, scores = scorer.rank(table, u, t_off, t_val, e_off, e_val, 3)
        again = scorer.rank(table, u, t_off, t_val, e_off, e_val, 3)
        assert torch.equal(ranks, again[0]) and torch.equal(scores.view(torch.int32), again[1].view(torch.int32))  # run to run
        assert (ranks >= 0).sum() >= 5 * B - 10
        scores = scores.view(torch.int32)  # (bits: a NaN equals itself)
        for b in (0, 63, 64, 127, 129):  # a user alone: slices of the CSRs, their offsets absolute
            r1, s1 = scorer.rank(table, u[b:b + 1], t_off[b:b + 2], t_val, e_off[b:b + 2], e_val, 3)
            assert torch.equal(r1[5 * b:5 * b + 5], ranks[5 * b:5 * b + 5]), (kind, b)
            assert torch.equal(s1.view(torch.int32)[5 * b:5 * b + 5], scores[5 * b:5 * b + 5]), (kind, b)
        # the batch in reversed order
        r_off, r_val = (dev(a) for a in excl_csr(targets[::-1]))
        re_off, re_val = (dev(a) for a in excl_csr(excl[::-1]))
        rr, rs = scorer.rank(table, torch.flip(u, dims=[0]).contiguous(), r_off, r_val, re_off, re_val, 3)
        assert torch.equal(torch.flip(rr.reshape(B, 5), dims=[0]), ranks.reshape(B, 5))
        assert torch.equal(torch.flip(rs.view(torch.int32).reshape(B, 5), dims=[0]), scores.reshape(B, 5))


# ------------------------------------------------------------------------------------------- 7. hipGraph
def test_one_call_captured_in_a_hip_graph():
    B, N, E = 130, 1000, 70
    scorer, table, u, _, _ = real_case("bilin", B, N, E)
    rng = synth.rng_for(707)
    t_off, t_val = (dev(a) for a in excl_csr([rng.integers(0, N, size=int(rng.integers(0, 4))).tolist() for _ in range(B)]))
    u_static = u.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad():
        with torch.cuda.stream(side):
            first = scorer.rank(table, u_static, t_off, t_val)  # warm-up on the capture stream (workspace growth)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            ranks_g, scores_g = scorer.rank(table, u_static, t_off, t_val)
        u_static.copy_(torch.flip(u, dims=[0]))
        for _ in range(2):  # replayed twice: the counts start from 0 again
            graph.replay()
            torch.cuda.synchronize()
            eager = scorer.rank(table, torch.flip(u, dims=[0]).contiguous(), t_off, t_val)
            assert torch.equal(ranks_g, eager[0]) and torch.equal(scores_g, eager[1])
    assert not torch.equal(ranks_g, first[0])


# ------------------------------------------------------------------------------------------- 8. the evaluation end to end
def histories(beh):
    off, val = beh.hist_off.cpu().numpy(), beh.hist_val.cpu().numpy()
    return [val[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


def clicks(beh):
    off, val = beh.pos_off.cpu().numpy(), beh.pos_val.cpu().numpy()
    return [val[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


def check_rank_clicked(out, ref, beh, tol, excl, pad_row, sessions=None):
    """rank_clicked's four tensors against the all-pairs scores `ref`:(sessions, N) -> (the share of decided queries, the worst
    score error)."""
    q_sess, q_row, ranks, scores = (a.cpu().numpy() for a in out)
    sessions = list(range(len(beh))) if sessions is None else list(sessions)
    cl = clicks(beh)
    assert q_sess.tolist() == [s for s in sessions for _ in cl[s]] and q_row.tolist() == [t for s in sessions for t in cl[s]]
    decided, worst = 0, 0.0
    for i, (s, t) in enumerate(zip(q_sess, q_row)):
        if t == pad_row:
            assert ranks[i] == -1 and np.isnan(scores[i])
            decided += 1
            continue
        ok = eligible(ref[s], None if excl is None else excl[s], pad_row)
        ok[t] = False
        lower, upper = rank_bounds(ref[s], [t], tol, ok)
        assert lower[0] <= ranks[i] <= upper[0], (s, t, ranks[i], lower, upper)
        worst = max(worst, abs(float(scores[i]) - float(ref[s, t])))
        decided += int(lower[0] == upper[0])
    assert worst <= tol
    return decided / max(len(q_sess), 1), worst


@pytest.mark.parametrize("kind", ["dot", "bilin", "fc"])
def test_rank_clicked_and_evaluate_full_ranking_end_to_end(kind):
    from tests.test_hip_scorers import _eval_model
    from tests.test_hip_topk import recommend_reference
    store, beh = synth.click_world(n_news=150, n_sess=120)
    # session 3 without a click, session 4 with two
    beh.pos_off[4] = beh.pos_off[3]
    store, beh = store.to(DEV), beh.to(DEV)
    model = _eval_model(kind)
    ref = recommend_reference(model, store, beh, 8)
    tol = SWITCH_TOL * float(np.abs(ref).max())
    hists = histories(beh)
    out = EV.rank_clicked(model, store, beh, l_hist=8, batch=32)
    assert all(a.is_cuda for a in out) and [a.dtype for a in out] == [torch.int64, torch.int32, torch.int32, torch.float32]
    assert out[0].numel() == 120 and 3 not in out[0].tolist() and out[0].tolist().count(4) == 2
    share, worst = check_rank_clicked(out, ref, beh, tol, hists, store.pad_row)
    out_h = EV.rank_clicked(model, store, beh, l_hist=8, batch=32, exclude_history=False)
    share_h, worst_h = check_rank_clicked(out_h, ref, beh, tol, None, store.pad_row)
    assert (out_h[2] >= out[2]).all() and (out_h[2] > out[2]).any() and torch.equal(out_h[3], out[3])
    assert share >= 0.95 and share_h >= 0.95
    # a selection of the sessions, gathered: those queries of the full call, bit for bit
    pick = [5, 77, 3, 119, 4, 31, 32, 0]
    out_s = EV.rank_clicked(model, store, beh, l_hist=8, sessions=pick, batch=3)
    idx = [i for s in pick for i in torch.nonzero(out[0] == s).flatten().tolist()]
    assert out_s[0].tolist() == [s for s in pick for _ in range(out[0].tolist().count(s))]
    assert all(torch.equal(a, b[idx]) for a, b in zip(out_s[1:], out[1:]))
    # the metrics are those of the rank vector
    ks = (5, 10, 100)
    res = EV.evaluate_full_ranking(model, store, beh, l_hist=8, ks=ks, batch=32)
    assert res == EV.full_ranking_metrics(EV.full_ranking_sums(out[2], ks), ks) and res["n_queries"] == 120
    r = out[2].cpu().numpy().astype(np.float64)
    assert res["hit@10"] == pytest.approx(float(np.mean(r < 10)), rel=1e-12) and res["mean_rank"] == pytest.approx(float(r.mean()), rel=1e-12)
    assert res["mrr"] == pytest.approx(float(np.mean(1 / (1 + r))), rel=1e-12)
    # against recommend(k = 10), GPU against GPU: hit@10 is the share of the queries whose news is on the recommended list.
    # With the history excluded a clicked news of the history is ranked but never recommended: there the statement holds for
    # the eligible queries, one by one, and the news sits at position rank
    for eh, o in ((False, out_h), (True, out)):
        rows, rscores = EV.recommend(model, store, beh, l_hist=8, k=10, batch=32, exclude_history=eh)
        rows, rscores = rows.cpu().numpy(), rscores.cpu().numpy()
        q_sess, q_row, ranks, scores = (a.cpu().numpy() for a in o)
        listed = np.array([t in rows[s] for s, t in zip(q_sess, q_row)])
        own = np.array([eh and t in hists[s] for s, t in zip(q_sess, q_row)])
        assert ((ranks < 10) == listed)[~own].all() and not listed[own].any()
        for i in np.nonzero(listed)[0]:
            assert rows[q_sess[i], ranks[i]] == q_row[i] and rscores[q_sess[i], ranks[i]] == scores[i]
        if not eh:
            got = EV.evaluate_full_ranking(model, store, beh, l_hist=8, ks=(10,), batch=32, exclude_history=False)
            assert got["hit@10"] == float(np.mean(listed))
    print(f"MARGIN rank_clicked {kind}: vs CSR scorer {max(worst, worst_h) / tol:.3f}  (error / bar); decided "
          f"{100 * share:.1f} % / {100 * share_h:.1f} % of the queries")


def test_rank_clicked_lstur():
    from tests.golden import lstur_cases as LC
    from tests.test_hip_lstur import Cfg
    from tests.test_hip_topk import recommend_reference
    from xnrs_amd.models.lstur import make_lstur
    store, beh = synth.click_world(n_news=60, n_sess=40)
    store, beh = store.to(DEV), beh.to(DEV)
    store.columns["category_index"] = (torch.arange(store.n_rows, device=DEV, dtype=torch.int32) % 19 + 1) * (
        torch.arange(store.n_rows, device=DEV) > 0).to(torch.int32)
    c = dict(LC.SHAPES["tiny"], D=32, n_users=50, H=5, st=3, ltm="embedding", lstm="con", scoring="dot", hole=False)
    torch.manual_seed(4)
    model = make_lstur(Cfg(LC.model_cfg(c))).to(DEV).eval()
    with pytest.raises(ValueError, match="user index"):
        EV.rank_clicked(model, store, beh, l_hist=5)
    beh.user_index = torch.arange(len(beh), device=DEV) % 7
    ref = recommend_reference(model, store, beh, 5)
    tol = SWITCH_TOL * float(np.abs(ref).max())
    out = EV.rank_clicked(model, store, beh, l_hist=5, batch=16)
    share, worst = check_rank_clicked(out, ref, beh, tol, histories(beh), store.pad_row)
    assert share >= 0.95
    res = EV.evaluate_full_ranking(model, store, beh, l_hist=5, batch=16)
    assert res["n_queries"] == 40 and 0 < res["mrr"] <= 1
    print(f"MARGIN rank_clicked LSTUR: vs CSR scorer {worst / tol:.3f}  (error / bar); decided {100 * share:.1f} % of the queries")


def test_rank_clicked_refuses_npa():
    from tests.golden import npa_cases as NC
    from tests.test_hip_npa import Cfg
    from xnrs_amd.models.npa import make_npa
    store, beh = synth.click_world(n_news=40, n_sess=10)
    model = make_npa(Cfg(NC.model_cfg(dict(NC.CASES["tiny"], D=32, n_users=50), "dot"))).to(DEV).eval()
    with pytest.raises(NotImplementedError, match="depend on the user"):
        EV.evaluate_full_ranking(model, store.to(DEV), beh.to(DEV), l_hist=5)


# ------------------------------------------------------------------------------------------- 9. two ranks on one GPU
def _full_ranking_rank(rank, world, port, path):
    import torch.distributed as dist

    from tests.test_hip_two_ranks import _model, _world
    from xnrs_amd import distributed as D
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev_ = torch.device("cuda", 0)
    store, beh = _world()
    store, beh = store.to(dev_), beh.to(dev_)
    model = _model(dev_)
    D.broadcast_parameters(model)
    res = EV.evaluate_full_ranking(model, store, beh, l_hist=8, batch=10, distributed=True)  # several batches per rank
    torch.save(res, f"{path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_on_one_gpu_equal_the_single_process_metrics():
    """evaluate_full_ranking(distributed=True): the sessions split by shard_range, one fp64 all-reduce of the sums (RCCL
    refuses two ranks on one device: the collective rides on gloo, as in tests/test_hip_two_ranks.py)."""
    import torch.multiprocessing as mp

    from tests.test_hip_two_ranks import _model, _world
    store, beh = _world()
    store, beh = store.to(DEV), beh.to(DEV)
    ref = EV.evaluate_full_ranking(_model(torch.device(DEV)), store, beh, l_hist=8, batch=10)
    assert ref["n_queries"] == 64 and 0 < ref["mrr"] < 1
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "res")
        mp.spawn(_full_ranking_rank, args=(2, port, path), nprocs=2, join=True)  # 2 GPU processes + this one
        got = [torch.load(f"{path}.{r}", weights_only=True) for r in range(2)]
    for res in got:
        assert res.keys() == ref.keys() and res["n_queries"] == ref["n_queries"]
        for k in ref:
            assert abs(res[k] - ref[k]) <= 1e-12 * max(1.0, abs(ref[k])), (k, res[k], ref[k])
    assert got[0] == got[1]  # every rank holds the same dict
