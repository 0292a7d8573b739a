#!/usr/bin/env python
"""Fingerprint of the list paths behind recommend(): for seeded cases the SHA-256 of every output tensor of the two greedy
re-rankers (ops.mmr_rerank, ops.calibrated_rerank: pools of every size, both table routes, every rel and lam, invalid places,
targets that do not count), of the other kernels of their units, and of every public list function of xnrs_amd/evaluation.py
over a small click world -- and the repr of every metrics dict.  None of these paths has float atomics: two trees that
differ only in structure give equal files.

    python tools/hash_rerank_paths.py OUT.json
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xnrs_amd import evaluation as EV, hip, ops, synth  # noqa: E402
from xnrs_amd.models import make_model  # noqa: E402

DEV = "cuda:0"
N_ROWS = 600
POOLS = (1, 37, 129, 257, 1024)
B = 5
REL_LAM = [(rel, lam) for rel in ("raw", "minmax") for lam in (0.0, 0.3, 0.7, 1.0)]


class Cfg(dict):
    __getattr__ = dict.__getitem__


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def sha_all(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pool(P, seed):
    """(rows:(B,P) int32, scores:(B,P) fp32) with -1 fillers, rows beyond the table, NaN and +-inf scores, ties, a session
    without a valid place and one of a single score."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, N_ROWS, size=(B, P)).astype(np.int32)
    scores = (rng.standard_normal((B, P)) * 3).astype(np.float32)
    scores[0] = np.round(scores[0] * 2) / 2  # ties
    for b in range(B):
        junk = rng.choice(P, size=P // 4, replace=False)
        kinds = np.arange(junk.size) % 5
        rows[b, junk[kinds == 0]] = -1
        rows[b, junk[kinds == 1]] = N_ROWS
        scores[b, junk[kinds == 2]] = np.nan
        scores[b, junk[kinds == 3]] = np.inf
        scores[b, junk[kinds == 4]] = -np.inf
    rows[3] = -1
    scores[4] = 1.25
    return dev(rows), dev(scores)


def ks_of(P):
    return sorted({1, min(P, 10), P})


def table(E, shift=False):
    """(600, E) fp32 on the device; shift: a view that starts 4 bytes behind a 16-byte boundary."""
    x = dev(np.random.default_rng(E).standard_normal((N_ROWS, E)).astype(np.float32))
    x[7] = 0  # a zero row
    if not shift:
        return x
    buf = torch.empty(x.numel() + 8, device=DEV)
    off = ((4 - buf.data_ptr()) % 16) // 4
    v = buf[off:off + x.numel()].view_as(x).copy_(x)
    assert v.data_ptr() % 16 == 4
    return v


def mmr_cases(out):
    for E, shift in ((8, False), (20, False), (21, False), (256, False), (20, True)):
        vecs = table(E, shift)
        inv = ops.row_inv_norms(vecs)
        out[f"inv/E{E}/shift{int(shift)}"] = sha(inv)
        for P in POOLS:
            rows, scores = pool(P, 100 + P)
            for k in ks_of(P):  # (one digest over rel x lam, in this order)
                out[f"mmr/E{E}/shift{int(shift)}/P{P}/k{k}"] = sha_all(t for rel, lam in REL_LAM
                                                                       for t in ops.mmr_rerank(vecs, inv, rows, scores, k, lam, rel))


def targets(C, seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 5, size=(B, C)).astype(np.float32)
    t[:, 0] += 1
    t[0, C // 2] = 0            # a zero entry
    t[1] = 0                    # an all-zero row: no target
    t[2, C - 1] = np.inf        # weights that do not count
    t[2, 0] = np.nan if C > 1 else t[2, 0]
    return dev(t)


def cal_cases(out):
    for C in (1, 4, 33, 4096):
        cat = dev(np.random.default_rng(C).integers(-1, C + 1, size=N_ROWS).astype(np.int32))
        tgt = targets(C, 7 + C)
        for P in POOLS:
            rows, scores = pool(P, 100 + P)
            for k in ks_of(P):
                out[f"cal/C{C}/P{P}/k{k}"] = sha_all(t for rel, lam in REL_LAM
                                                     for t in ops.calibrated_rerank(rows, scores, k, lam, cat, C, tgt, 0.01, rel))


def list_cases(out):
    vecs = table(20)
    inv = ops.row_inv_norms(vecs)
    cat = dev(np.random.default_rng(3).integers(-1, 34, size=N_ROWS).astype(np.int32))
    rows, _ = pool(37, 5)
    out["list_diversity"] = [sha(t) for t in ops.list_diversity(vecs, inv, rows, cat, 33)]
    out["list_calibration"] = [sha(t) for t in ops.list_calibration(rows, cat, 33, targets(33, 9), 0.01, want_counts=True)]
    off = dev(np.array([0, 5, 5, 30, 37 * B], dtype=np.int64))
    out["csr_category_counts"] = sha(ops.csr_category_counts(off, rows.reshape(-1), cat, 33, pad_row=0))


def api_cases(out):
    n_cat = 5
    store, beh = synth.click_world(n_news=60, n_sess=40, seed=2)
    store, beh = store.to(DEV), beh.to(DEV)
    torch.manual_seed(11)
    model = make_model(Cfg(synth.model_cfg(dict(model="NRMS", E=32, bias=True, h=4, D=32, H=8, S=6)))).to(DEV).eval()
    cat = dev(np.random.default_rng(6).integers(0, n_cat + 1, size=store.n_rows).astype(np.int32))
    n = len(beh)
    win = (torch.full((n,), 5, dtype=torch.int32), torch.full((n,), 45, dtype=torch.int32))
    per = torch.from_numpy(np.random.default_rng(1).integers(0, 4, size=(n, n_cat)).astype(np.float32))
    catalogue = torch.bincount(cat[cat < n_cat].long(), minlength=n_cat).float()
    kw = dict(l_hist=8, batch=16)
    ckw = dict(row_category=cat, n_categories=n_cat, pool=30, **kw)

    def put(name, got):
        out["api/" + name] = repr(got) if isinstance(got, dict) else [sha(t) for t in got]

    put("recommend", EV.recommend(model, store, beh, k=10, **kw))
    put("recommend/deep", EV.recommend(model, store, beh, k=30, sessions=[7, 3, 30], **kw))
    put("recommend/windows", EV.recommend(model, store, beh, k=10, windows=win, **kw))
    put("recommend_sampled", EV.recommend_sampled(model, store, beh, 8, 10, 0.7, 5, batch=16, return_keys=True))
    put("recommend_sampled/windows", EV.recommend_sampled(model, store, beh, 8, 10, 2.0, 5, batch=16, windows=win))
    for rel in ("raw", "minmax"):
        put(f"recommend_diverse/{rel}", EV.recommend_diverse(model, store, beh, k=8, lam=0.3, pool=30, rel=rel, **kw))
    put("recommend_diverse/windows", EV.recommend_diverse(model, store, beh, k=8, lam=0.7, windows=win, **kw))
    for name, target in (("history", "history"), ("catalogue", catalogue), ("per_session", per)):
        put(f"recommend_calibrated/{name}", EV.recommend_calibrated(model, store, beh, k=8, lam=0.3, target=target, **ckw))
    put("recommend_calibrated/windows", EV.recommend_calibrated(model, store, beh, k=8, lam=0.3, windows=win, **ckw))
    for lam in (None, 0.3):
        pl = None if lam is None else 30
        put(f"evaluate_diversity/lam{lam}", EV.evaluate_diversity(model, store, beh, k=8, lam=lam, pool=pl, row_category=cat,
                                                                  n_categories=n_cat, **kw))
        put(f"evaluate_calibration/lam{lam}", EV.evaluate_calibration(model, store, beh, k=8, lam=lam, row_category=cat,
                                                                      n_categories=n_cat, pool=pl, **kw))
    # two stages: NPA behind an NRMS generator (the world of tests/test_hip_calibration.py's generator test)
    from tests.helpers import npa_and_nrms
    store, beh = synth.click_world(n_news=40, n_sess=10)
    store, beh = store.to(DEV), beh.to(DEV)
    beh.user_index = torch.arange(len(beh), device=DEV) % 7
    npa, nrms = npa_and_nrms(DEV)
    cat = dev(np.random.default_rng(3).integers(0, n_cat, size=store.n_rows).astype(np.int32))
    gkw = dict(l_hist=5, generator=nrms, pool=16)
    put("generator/recommend", EV.recommend(npa, store, beh, k=5, **gkw))
    put("generator/recommend_calibrated", EV.recommend_calibrated(npa, store, beh, k=5, lam=0.3, row_category=cat,
                                                                  n_categories=n_cat, **gkw))
    for lam in (None, 0.3):
        put(f"generator/evaluate_calibration/lam{lam}", EV.evaluate_calibration(npa, store, beh, k=5, lam=lam, row_category=cat,
                                                                                n_categories=n_cat, **gkw))


def main(path):
    result = {}
    for fn in (mmr_cases, cal_cases, list_cases, api_cases):
        with torch.no_grad():
            fn(result)
        torch.cuda.synchronize()
        hip.check_status()
        print(fn.__name__, len(result), flush=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
