#!/usr/bin/env python
"""Fingerprint of everything that reads a row list built on the device (csrc/row_lists.hip): for a list of seeded cases --
xnrs_build_row_lists called directly, the device-compacted encoder at S = 20 (compact_rows64_kernel) and S = 70
(compact_rows_kernel), the dense passes on their list route (dense_row_lists_kernel; at S = 70 live_tiles_kernel alone) and a
training forward with device lists -- the SHA-256 of every output tensor, the library's launch counters and, where the
launch timer gives them, the launches and executed FLOPs per stage (it reads the device counts).  Two builds whose list
kernels differ only in structure give byte-identical files (no list kernel has an atomic that decides a place).
All shapes: D = 64, 4 heads, A = 32.

    python tools/hash_row_list_paths.py OUT.json
"""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_hip_dense_lists_split as DL  # noqa: E402
from tests import test_hip_mha_live_o as L  # noqa: E402
from xnrs_amd import autograd as AG, hip, ops, synth  # noqa: E402
from xnrs_amd.models.components import layers, news_encoding  # noqa: E402

DEV = L.DEV
D, A = L.D, L.A
COUNTERS = ("xnrs_qkv_launch_count", "xnrs_fc1_in_tail_count", "xnrs_mha_live_o_count")


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


# ---- xnrs_build_row_lists, called directly
def build_row_lists(n, Lt, with_ids, dead=()):
    """The four index buffers (whole capacity: what lies past the counts must stay as filled) and the counts."""
    rng = synth.rng_for(9000 + 7 * n + Lt)
    n_tab = n + 17 if with_ids else n
    m = torch.from_numpy((rng.random((n_tab, Lt)) < 0.5).astype("float32"))
    m[torch.from_numpy(rng.random(n_tab) < 0.3)] = 0
    ids = torch.from_numpy(rng.integers(0, n_tab, size=(n,)).astype("int32")) if with_ids else None
    for a, b in dead:  # runs of empty SEQUENCES (through the ids, when there are any)
        m[(ids[a:b].long() if with_ids else slice(a, b))] = 0
    md, idd = m.to(DEV), (ids.to(DEV) if with_ids else None)
    buf = torch.full((4, n * Lt), -7, dtype=torch.int32, device=DEV)
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    l = hip.lib()
    nws = l.xnrs_row_lists_workspace_bytes(n)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    hip.check(l.xnrs_build_row_lists(hip.ptr(md), hip.ptr(idd), n, Lt, hip.ptr(buf[0]), hip.ptr(buf[2]) if with_ids else None,
                                     hip.ptr(buf[1]), hip.ptr(buf[3]) if with_ids else None, hip.ptr(counts), hip.ptr(ws), nws,
                                     hip.stream_ptr(torch.device(DEV))), "xnrs_build_row_lists")
    return dict(live=buf[0], kv=buf[1], live_src=buf[2], kv_src=buf[3], counts=counts)


# ---- the device-compacted encoder
def compact_encoder(S):
    """Self-attention + additive pooler + head at S <= 64; the additive tower alone beyond (the compacted attention ends there)."""
    enc = L.encoder()
    return (enc.att if S <= 64 else None), enc.pooler, enc.head


def compact(S, n, chunk, dead, with_ids=False, nonbinary=False):
    x, m = DL.news(n, S, 700 + S + n, dead, nonbinary=False)  # prefix masks, holes in every third news, 0 / 1
    if nonbinary:
        m[n // 2, S - 1] = 0.5
    if with_ids:
        xd, md, ids = L.table_of(x, m)
    else:
        xd, md, ids = x.to(DEV), m.to(DEV), None
    att, pooler, head = compact_encoder(S)
    hip.clear_status()
    with torch.no_grad():
        for _ in range(2):  # (the first call sizes the workspace; the second runs in it, filled with NaN bytes)
            hip.workspace(DEV, 1).fill_(0xFF)
            y, hm = ops.text_encoder_forward_compact(xd, md, att, pooler, head, ids=ids, chunk=chunk)
    torch.cuda.synchronize()
    try:
        hip.check_status()
        status = "clean"
    except hip.XnrsHipError as e:
        status = str(e)
    if nonbinary:  # the outputs are NaN: their pattern, and what the status word said
        return dict(y_nan=torch.isnan(y), hm_nan=torch.isnan(hm)), status
    return dict(y=y, hm=hm), status


# ---- the dense passes on their list route
def dense(S, n, chunk, dead, route):
    enc = L.encoder()
    x, m = DL.news(n, S, 500 + n + chunk, dead)  # (the inputs of tests/test_hip_dense_lists_split.py: non-binary values too)
    if route == "ids":
        xd, md, ids = L.table_of(x, m)
    else:
        xd, md, ids = x.to(DEV), m.to(DEV), None
    y, hm, live_o, _ = L.encode(xd, md, enc, chunk, L.ON, ids)
    with torch.no_grad(), hip.knobs(**L.ON):
        hip.profile_enable(0b1001)
        try:
            ops.text_encoder(xd, md, enc, ids=ids, chunk=chunk)
            torch.cuda.synchronize()
            prof = hip.profile_read()
        finally:
            hip.profile_enable(0)
    return dict(y=y, hm=hm), dict(live_o_launches=live_o, profile={k: [v[1], v[2]] for k, v in sorted(prof.items()) if v[1]})


# ---- a training forward (and its backward) with the lists built on the device
def train_forward():
    S, E, n_tab, n = 24, 32, 260, 300
    enc = news_encoding.TextEncoder(pooler=layers.AdditiveAttention(D, A), p_dropout=0.0, out_features=E, in_features=D,
                                    att=layers.MultiHeadAttention(4, D))
    shapes = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    enc.load_state_dict(synth.fill_state_dict(shapes, 271))
    enc.train().to(DEV)
    enc.att.dropout.p = 0.1
    rng = synth.rng_for(272)
    x = torch.from_numpy(rng.standard_normal((n_tab, S, D)).astype("float32")).to(DEV)
    m = torch.from_numpy((rng.random((n_tab, S)) < 0.55).astype("float32"))
    m[torch.from_numpy(rng.random(n_tab) < 0.3)] = 0
    m = m.to(DEV)
    w = torch.from_numpy(rng.standard_normal((n, E)).astype("float32")).to(DEV)
    ids = torch.from_numpy(rng.integers(0, n_tab, size=(1, n)).astype("int32")).to(DEV)
    saved = AG.DEVICE_LISTS, AG.LIVE_ROWS_MIN
    AG.DEVICE_LISTS, AG.LIVE_ROWS_MIN = True, 1
    before = AG.STATS["device_list_forwards"]
    try:
        torch.manual_seed(31)
        y, hm = enc.forward_ids(x, m, ids)
        loss = (y[0] * w).sum()
        loss.backward()
    finally:
        AG.DEVICE_LISTS, AG.LIVE_ROWS_MIN = saved
    out = dict(loss=loss, y=y, hm=hm)
    out.update({"grad/" + k: p.grad for k, p in enc.named_parameters() if p.grad is not None})
    return out, dict(device_list_forwards=AG.STATS["device_list_forwards"] - before)


CASES = []
for n_ in (1, 63, 64, 65, 200):
    for L_ in (20, 70):
        for ids_ in (False, True):
            CASES.append((f"build n={n_} L={L_} ids={int(ids_)}", lambda n_=n_, L_=L_, ids_=ids_: (build_row_lists(n_, L_, ids_), None)))
for L_ in (20, 70):
    for ids_ in (False, True):
        CASES.append((f"build n=200 L={L_} ids={int(ids_)} empty run over 60..70",
                      lambda L_=L_, ids_=ids_: (build_row_lists(200, L_, ids_, dead=[(60, 70)]), None)))
        CASES.append((f"build n=130 L={L_} ids={int(ids_)} last sequence empty",
                      lambda L_=L_, ids_=ids_: (build_row_lists(130, L_, ids_, dead=[(129, 130)]), None)))
for S_ in (20, 70):
    CASES += [(f"compact S={S_} 41 news in passes of 12, one pass empty", lambda S_=S_: compact(S_, 41, 12, [(12, 24), (30, 33)])),
              (f"compact S={S_} 1100 news in one pass", lambda S_=S_: compact(S_, 1100, 1100, [(100, 180), (1000, 1030)])),
              (f"compact S={S_} 1100 news in one pass, ids", lambda S_=S_: compact(S_, 1100, 1100, [(100, 180), (1020, 1030)], with_ids=True)),
              (f"compact S={S_} 41 news in passes of 12, ids", lambda S_=S_: compact(S_, 41, 12, [(12, 24)], with_ids=True)),
              (f"compact S={S_} non-binary mask", lambda S_=S_: compact(S_, 41, 12, [(12, 24)], nonbinary=True))]
for S_, n_, chunk_, dead_ in DL.CASES:
    for route_ in ("rows", "ids"):
        CASES.append((f"dense S={S_} n={n_} chunk={chunk_} {route_}",
                      lambda S_=S_, n_=n_, chunk_=chunk_, dead_=dead_, route_=route_: dense(S_, n_, chunk_, dead_, route_)))
for route_ in ("rows", "ids"):
    CASES.append((f"dense S=70 n=250 chunk=100 {route_} (tile list alone)",
                  lambda route_=route_: dense(70, 250, 100, [(64, 100), (130, 140)], route_)))
CASES.append(("training forward and backward, device lists", train_forward))


def main(path):
    l = hip.lib()
    result = {}
    for name, fn in CASES:
        for c in COUNTERS:
            getattr(l, c)(1)
        out, extra = fn()
        torch.cuda.synchronize()
        result[name] = dict(sha256={k: sha(v) for k, v in sorted(out.items())}, extra=extra,
                            counters={c: getattr(l, c)(1) for c in COUNTERS})
        print(name, result[name]["extra"], result[name]["counters"], flush=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
