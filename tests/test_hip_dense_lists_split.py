"""The list launch of a dense encoder call, one pass spread over several workgroups (row_lists.hip dense_row_lists_kernel).

A pass is cut into slices of 64 news, a workgroup each; a slice finds its place in the pass's live-row list by counting the
live tokens of the news before it, and the workgroup of the pass's last slice writes the counts and the tile list.  The
lists decide which rows and tiles every later launch of the call computes, so they are checked through the call: the
encoder outputs must be ``torch.equal`` to the dense launches (no list), in a workspace filled with NaN bytes, and the
launch timer's executed FLOPs -- it reads the device counts -- must be those of the live tiles and live rows counted on the
host from the same mask (the formula of test_hip_live_rows.py).  Small shapes: D = 64, 4 heads, A = 32."""
import pytest
import torch

from tests import test_hip_mha_live_o as L
from xnrs_amd import hip, ops

pytestmark = pytest.mark.gpu
DEV = L.DEV
D, A = L.D, L.A
BM = 128      # tile height of the tile list (kernels.h LIVE_TILE_BM)
SLICE = 64    # news per workgroup of the list launch (row_lists.hip DL_SLICE)
ON = L.ON
DENSE = L.DENSE

# S, n news, news per pass, [first, last + 1) runs of all-masked news
CASES = [
    (34, 1100, 1100, [(100, 180), (1000, 1030)]),   # one pass of more than 1 024 news: 18 slices, the last one short
    (50, 41, 12, [(12, 24), (30, 33)]),             # one slice per pass; the second pass all empty; a short last pass
    (50, 250, 100, [(64, 100), (130, 140)]),        # pass = 64 + 36 news (no multiple of the slice); slice 1 of pass 0 empty
    (34, 330, 128, [(128, 256), (300, 330)]),       # pass = 2 full slices; an all-empty pass; the short last pass ends empty
    (50, 130, 65, [(0, 64)]),                       # pass = 64 + 1 news: a whole first slice empty, the last slice one news
    (34, 70, 70, [(0, 70)]),                        # every news empty: every count 0
]


def news(n, S, seed, dead, nonbinary=True):
    """n news with prefix masks of random lengths, holes in every third news, values 0.5 / 2.0 on some live tokens."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, S, D, generator=g)
    length = torch.randint(1, S + 1, (n,), generator=g)
    m = (torch.arange(S)[None, :] < length[:, None]).float()
    holes = torch.rand(n, S, generator=g) < 0.3
    holes[torch.arange(n) % 3 != 0] = False
    m[holes] = 0
    if nonbinary:
        u = torch.rand(n, S, generator=g)
        m[(u < 0.1) & (m != 0)] = 0.5
        m[(u > 0.9) & (m != 0)] = 2.0
    for a, b in dead:
        m[a:b] = 0
    return x, m.reshape(n, S, 1)


def lists_host(m, S, chunk):
    """[(live tiles, rows, live rows)] per pass, counted on the host from the same mask (mask != 0)."""
    on = m.reshape(-1, S).ne(0).numpy()
    alive = on.any(axis=1)
    n = alive.shape[0]
    out = []
    for c0 in range(0, n, chunk):
        nc = min(chunk, n - c0)
        rows = nc * S
        live = 0
        for t in range((rows + BM - 1) // BM):
            r0, r1 = t * BM, min((t + 1) * BM, rows) - 1
            live += bool(alive[c0 + r0 // S: c0 + r1 // S + 1].any())
        out.append((live, rows, int(on[c0:c0 + nc].sum())))
    return out


def flops(x, m, enc, chunk, ids=None):
    """(qkv_gemm, fc1_tanh_gemm) executed FLOPs of one call on the list route."""
    with torch.no_grad(), hip.knobs(**ON):
        hip.profile_enable(0b1001)
        try:
            ops.text_encoder(x, m, enc, ids=ids, chunk=chunk)
            torch.cuda.synchronize()
            prof = hip.profile_read()
        finally:
            hip.profile_enable(0)
    return prof["qkv_gemm"][2], prof["fc1_tanh_gemm"][2]


@pytest.mark.parametrize("route", ["rows", "ids"])
@pytest.mark.parametrize("S,n,chunk,dead", CASES)
def test_lists_through_the_encoder(S, n, chunk, dead, route):
    enc = L.encoder()
    x, m = news(n, S, 500 + n + chunk, dead)
    passes = lists_host(m, S, chunk)
    if (S, n) == (34, 1100):
        assert n > 1024 and len(passes) == 1
    if (n, chunk) == (250, 100):
        assert chunk % SLICE and passes[-1][1] < passes[0][1]
    if (n, chunk) in ((41, 12), (330, 128)):
        assert any(p[2] == 0 for p in passes) and any(p[2] > 0 for p in passes)   # an all-empty pass among live ones
    if route == "ids":
        xd, md, ids = L.table_of(x, m)
    else:
        xd, md, ids = x.to(DEV), m.to(DEV), None
    yd, hmd, _, _ = L.encode(xd, md, enc, chunk, DENSE, ids)
    y1, hm1, c1, _ = L.encode(xd, md, enc, chunk, ON, ids)
    assert torch.isfinite(y1).all()
    assert c1 == len(passes)                       # the list route ran (one attention launch per pass took the lists' flag)
    assert torch.equal(y1, yd) and torch.equal(hm1, hmd)
    qkv, fc1 = flops(xd, md, enc, chunk, ids)
    tile_rows = sum(p[0] for p in passes) * BM
    live = sum(p[2] for p in passes)
    print(f"S={S} n={n} chunk={chunk} {route}: live rows {live} of {sum(p[1] for p in passes)}, live tiles {tile_rows // BM}; "
          f"qkv flops {qkv:.6g}, fc1 flops {fc1:.6g}")
    assert qkv == 2.0 * tile_rows * 2 * D * D + 2.0 * live * D * D   # K|V over the live tiles, Q over the live rows
    assert fc1 == 2.0 * live * A * D
