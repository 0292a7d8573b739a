"""Host-side tests of the bf16 news table (xnrs_amd/data.py: NewsStore.astype / save / load; include/xnrs_hip.h: the
*_bf16 entry points).  No GPU: conversion, the on-disk format and the C declarations."""
import json
import os

import pytest
import torch

from xnrs_amd import hip
from xnrs_amd.data import NewsStore


def _store(n=5, S=3, D=8, seed=0):
    """n rows x S x D with one extra text feature and one column; row 0 is the empty slot."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, S, D, generator=g) * 3.0
    a = torch.randn(n, S + 1, D // 2, generator=g)
    m = (torch.rand(n, S, generator=g) > 0.3).float()
    am = (torch.rand(n, S + 1, generator=g) > 0.3).float()
    x[0], m[0], a[0], am[0] = 0, 0, 0, 0
    cols = {"category_index": torch.arange(n, dtype=torch.int32)}
    return NewsStore(x, m, [f"N{i}" for i in range(1, n)], cols, {"abstract_emb": (a, am)}, "title_emb")


def test_astype_rounds_like_torch_and_keeps_the_rest():
    s = _store()
    b = s.astype(torch.bfloat16, rows_per_chunk=2)  # three chunks
    assert b.x.dtype == torch.bfloat16 and b.dtype == torch.bfloat16
    assert torch.equal(b.x, s.x.to(torch.bfloat16))
    ax, am = b.text("abstract_emb")
    assert ax.dtype == torch.bfloat16 and torch.equal(ax, s.texts["abstract_emb"][0].to(torch.bfloat16))  # texts follow
    assert torch.equal(b.m, s.m) and torch.equal(am, s.texts["abstract_emb"][1])
    assert b.ids == s.ids and b.feature == s.feature and b.index == s.index
    assert torch.equal(b.columns["category_index"], s.columns["category_index"])
    assert not b.x[0].any() and not ax[0].any()  # row 0 stays the empty slot
    assert s.x.dtype == torch.float32  # the source store is untouched
    f = b.astype(torch.float32)
    assert f.x.dtype == torch.float32 and torch.equal(f.x, s.x.to(torch.bfloat16).float())
    assert torch.equal(f.text("abstract_emb")[0], s.texts["abstract_emb"][0].to(torch.bfloat16).float())
    assert s.astype(torch.float32) is s
    with pytest.raises(ValueError):
        s.astype(torch.float16)


def test_one_dtype_per_store():
    s = _store()
    with pytest.raises(AssertionError):
        NewsStore(s.x.to(torch.bfloat16), s.m, s.ids, s.columns, s.texts, s.feature)


@pytest.mark.parametrize("mmap", [True, False])
def test_bf16_save_load_roundtrip(tmp_path, mmap):
    s = _store().astype(torch.bfloat16)
    path = str(tmp_path / "store")
    s.save(path, rows_per_chunk=2)
    with open(path + ".json") as f:
        h = json.load(f)
    assert h["dtype"] == "bf16"
    n = s.n_rows
    assert os.path.getsize(path + ".x.bf16") == n * 3 * 8 * 2
    assert os.path.getsize(path + ".abstract_emb.x.bf16") == n * 4 * 4 * 2
    assert not os.path.exists(path + ".x.f32") and not os.path.exists(path + ".abstract_emb.x.f32")
    l = NewsStore.load(path, mmap=mmap)
    assert l.x.dtype == torch.bfloat16 and l.text("abstract_emb")[0].dtype == torch.bfloat16
    assert torch.equal(l.x, s.x) and torch.equal(l.text("abstract_emb")[0], s.text("abstract_emb")[0])
    assert torch.equal(l.m, s.m) and torch.equal(l.text("abstract_emb")[1], s.text("abstract_emb")[1])
    assert l.ids == s.ids and l.feature == s.feature
    assert torch.equal(l.columns["category_index"], s.columns["category_index"])


def test_bf16_payload_one_byte_short_is_refused(tmp_path):
    s = _store().astype(torch.bfloat16)
    path = str(tmp_path / "store")
    s.save(path)
    with open(path + ".x.bf16", "r+b") as f:
        f.truncate(s.n_rows * 3 * 8 * 2 - 1)
    with pytest.raises(ValueError):
        NewsStore.load(path)


def test_fp32_store_is_written_as_before(tmp_path):
    """An fp32 store's files and header do not change: the copy saved after an astype round trip of ANOTHER object is byte
    for byte the copy saved before, the header has no dtype key, and a header without the key loads as fp32."""
    s = _store()
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    s.save(a)
    s.astype(torch.bfloat16)  # (must not touch s)
    s.save(b)
    for ext in (".json", ".x.f32", ".m.u8", ".abstract_emb.x.f32", ".abstract_emb.m.u8", ".category_index.i32"):
        with open(a + ext, "rb") as fa, open(b + ext, "rb") as fb:
            assert fa.read() == fb.read(), ext
    with open(a + ".json") as f:
        h = json.load(f)
    assert "dtype" not in h
    assert os.path.getsize(a + ".x.f32") == s.n_rows * 3 * 8 * 4
    l = NewsStore.load(a, mmap=False)
    assert l.x.dtype == torch.float32 and torch.equal(l.x, s.x)


def test_header_declares_the_bf16_entry_points():
    with open(hip.HEADER_PATH) as f:
        consts, _, protos = hip.parse_header(f.read())
    want = {"xnrs_gather_rows_bf16": 6, "xnrs_dropout_rows_bf16": 9, "xnrs_linear_fwd_bf16": 13,
            "xnrs_linear_bf16_workspace_bytes": 2, "xnrs_text_encoder_fwd_bf16": 16,
            "xnrs_text_encoder_bf16_workspace_bytes": 9}
    for name, n_args in want.items():
        assert name in protos, name
        assert len(protos[name][1]) == n_args, (name, len(protos[name][1]))
    # same arguments as the fp32 twins (plus the workspace pair of the linear primitive)
    assert len(protos["xnrs_text_encoder_fwd"][1]) == 16 and len(protos["xnrs_text_encoder_workspace_bytes"][1]) == 9
    assert len(protos["xnrs_gather_rows"][1]) == 6 and len(protos["xnrs_dropout_rows"][1]) == 9
    assert len(protos["xnrs_linear_fwd"][1]) == 11
    assert consts["ABI_VERSION"] == 6  # new entry points only: the ABI version stays
