"""CPU: CAUM's host side -- xnrs_amd.models.CAUM builds the reference's state_dict (keys, shapes, order, parameter count and
initial values of mind_small_LSTUR.yml's flat keys + model CAUM / scoring CAUMScoring / n_heads 16: tests/golden/caum.json /
.npz), make_caum builds the scorer first and refuses other models, CPU inputs raise, and the header declares the new entry
points with the argument types hip.py binds."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.golden import caum_cases as CC

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = H.golden("caum")
META = json.load(open(os.path.join(HERE, "golden", "caum.json")))


class Cfg(dict):
    __getattr__ = dict.__getitem__


def test_caum_is_exported_from_the_models_package():
    import xnrs_amd.models as M
    from xnrs_amd.models import caum
    for name in ("CAUM", "CAUMNewsEncoder", "CAUMUserEncoder", "CAUMScoring", "CategoryEncoder", "DenseAttention"):
        assert getattr(M, name) is getattr(caum, name), name
    assert callable(caum.make_caum)


def test_caum_builds_the_reference_state_dict_bitwise():
    from xnrs_amd.models import CAUM, CAUMScoring
    from xnrs_amd.models.caum import make_caum
    con = META["contract"]
    torch.manual_seed(CC.INIT["seed"])
    model = make_caum(Cfg(con["cfg"]))
    assert type(model) is CAUM and type(model.rec_model) is CAUMScoring and con["scorer"] == "CAUMScoring"
    sd = model.state_dict()
    assert list(sd) == con["keys"]
    assert [list(v.shape) for v in sd.values()] == con["shapes"]
    assert sum(p.numel() for p in model.parameters()) == con["n_params"]
    assert len(list(model.parameters())) == con["n_param_tensors"]
    for k, v in sd.items():
        assert np.array_equal(CC.sample(v), GOLD[f"init/{k}"]), k
        assert v.double().sum().item() == float(GOLD[f"init_sum/{k}"]), k


@pytest.mark.parametrize("name", ["tiny", "subcat", "odd_dk"])
def test_cases_construct_with_the_reference_layout(name):
    from xnrs_amd.models.caum import make_caum
    c = CC.CASES[name]
    model = make_caum(Cfg(CC.model_cfg(c)))
    e = CC.emb_dim(c)
    ue = model.user_encoder
    assert tuple(ue.linear1.weight.shape) == (e, 4 * e) and tuple(ue.linear2.weight.shape) == (e, 2 * e)
    assert tuple(ue.linear3.weight.shape) == (e, 2 * e) and tuple(ue.dense_att.linear.weight.shape) == (e, 2 * e)
    assert tuple(ue.dense_att.linear2.weight.shape) == (e // 2, e) and tuple(ue.dense_att.linear3.weight.shape) == (1, e // 2)
    assert tuple(ue.multihead_attention.in_proj_weight.shape) == (3 * e, e) and not ue.multihead_attention.batch_first
    assert hasattr(model.news_encoder, "subcat_embedder") == c["subcat"]
    assert (model.news_encoder.title_encoder.head[0].bias is not None) == c["bias"]


def test_make_caum_builds_the_scorer_first_and_rejects_other_models():
    from xnrs_amd.models.caum import make_caum
    c = CC.CASES["tiny"]
    # with a scorer that owns parameters, building it first moves every later draw: the model's first weight differs from
    # the one a CAUMScoring build (no parameters) draws under the same seed
    torch.manual_seed(3)
    a = make_caum(Cfg(CC.model_cfg(c)))
    torch.manual_seed(3)
    b = make_caum(Cfg(dict(CC.model_cfg(c), scoring="bilin")))
    assert type(b.rec_model).__name__ == "BilinScoring"
    ka = "news_encoder.title_encoder.att.q_linear.weight"
    assert not torch.equal(a.state_dict()[ka], b.state_dict()[ka])
    torch.manual_seed(3)
    torch.nn.Bilinear(CC.emb_dim(c), CC.emb_dim(c), 1, bias=True)
    from xnrs_amd.models import CAUM, CAUMScoring
    ref = CAUM(Cfg(CC.model_cfg(c)), CAUMScoring())
    assert torch.equal(ref.state_dict()[ka], b.state_dict()[ka])
    with pytest.raises(ValueError, match="cfg.model"):
        make_caum(Cfg(dict(CC.model_cfg(c), model="NRMS")))
    with pytest.raises(ValueError):
        make_caum(Cfg(dict(CC.model_cfg(c), scoring="nonlin")))


def test_a_cpu_call_raises_with_no_fallback():
    from xnrs_amd import hip, ops
    from xnrs_amd.models.caum import make_caum
    c = CC.CASES["tiny"]
    model = make_caum(Cfg(CC.model_cfg(c))).eval()
    e = CC.emb_dim(c)
    with pytest.raises(hip.XnrsHipError):
        model(CC.batch(c))
    with pytest.raises(hip.XnrsHipError):
        model.user_encoder((torch.randn(2, 3, e), None), (torch.randn(2, 4, e), None))
    with pytest.raises(hip.XnrsHipError):
        model.rec_model(torch.randn(2, 4, e), torch.randn(2, 4, e))
    with pytest.raises(hip.XnrsHipError):
        ops.attn_long(torch.randn(5, 2, 3 * 8), 2)
    with pytest.raises(hip.XnrsHipError):
        ops.caum_pair(torch.randn(6, 16), torch.randn(4, 8), 2, 2, 3)
    with pytest.raises(hip.XnrsHipError):
        ops.caum_pool(torch.randn(6, 2), torch.randn(1, 2), None, torch.randn(6, 4), 3)
    with pytest.raises(hip.XnrsHipError):
        ops.caum_bias_tanh(torch.randn(6, 4), torch.randn(2, 4), 3)
    with pytest.raises(hip.XnrsHipError):
        model.news_encoder.cat_embedder(torch.zeros(2, 3, dtype=torch.int32))


def test_evaluate_refuses_caum():
    from xnrs_amd import evaluation as EV
    from xnrs_amd.models.caum import make_caum
    model = make_caum(Cfg(CC.model_cfg(CC.CASES["tiny"])))
    with pytest.raises(NotImplementedError, match="CAUMScoring"):
        EV.evaluate(model, None, None, l_hist=5)
    with pytest.raises(NotImplementedError, match="candidate"):
        model.encode_user(None, None)


_F, _I64, _I32, _SZ, _P = C.c_void_p, C.c_int64, C.c_int32, C.c_size_t, C.c_void_p
_ATTN = [_F, _I64, _I64, _F, _I64, _I64, _I64, _I64, _I32, _I32]
EXPECTED = {
    "xnrs_attn_long_saved_bytes": (_SZ, [_I64, _I64, _I32, _I32]),
    "xnrs_attn_long_workspace_bytes": (_SZ, [_I64, _I64, _I32, _I32]),
    "xnrs_attn_long_fwd": (_I32, _ATTN + [_P]),
    "xnrs_attn_long_fwd_train": (_I32, _ATTN + [_P, _SZ, _P]),
    "xnrs_attn_long_bwd": (_I32, [_F, _I64, _I64, _F, _F, _I64, _I64, _P, _SZ, _F, _I64, _I64, _I32, _I32, _P, _SZ, _P]),
    "xnrs_caum_pair_fwd": (_I32, [_F, _F, _I64, _F, _F, _I64, _I32, _I32, _I32, _P]),
    "xnrs_caum_pair_bwd": (_I32, [_F, _F, _F, _F, _I64, _I64, _I32, _I32, _I32, _P]),
    "xnrs_caum_bias_tanh_fwd": (_I32, [_F, _F, _I64, _F, _I64, _I32, _I32, _P]),
    "xnrs_caum_bias_tanh_bwd": (_I32, [_F, _F, _F, _F, _I64, _I32, _I32, _P]),
    "xnrs_act_bwd": (_I32, [_F, _F, _F, _I64, _I32, _P]),
    "xnrs_caum_pool_fwd": (_I32, [_F, _F, _F, _F, _F, _F, _I64, _I32, _I32, _I32, _P]),
    "xnrs_caum_pool_bwd_workspace_bytes": (_SZ, [_I64, _I32, _I32]),
    "xnrs_caum_pool_bwd": (_I32, [_F] * 9 + [_I64, _I32, _I32, _I32, _P, _SZ, _P]),
}


def test_the_header_declares_the_new_entry_points_and_hip_binds_them():
    from xnrs_amd import hip
    text = open(hip.HEADER_PATH).read()
    l = hip.lib()
    for name, (restype, argtypes) in EXPECTED.items():
        assert f"{name}(" in text, name
        assert hip.PROTOTYPES[name] == (restype, argtypes), name
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert hip.ABI_VERSION == 6


def test_size_queries_are_pure_host_calls():
    from xnrs_amd import hip
    l = hip.lib()
    L, Nb, E, heads = 320, 25, 272, 16
    assert l.xnrs_attn_long_saved_bytes(L, Nb, E, heads) >= L * Nb * heads * 4
    assert l.xnrs_attn_long_saved_bytes(L, Nb, E, heads) < 2 * L * Nb * heads * 4   # the log-sum-exp rows, never L x L
    assert l.xnrs_attn_long_workspace_bytes(L, Nb, E, heads) >= L * Nb * heads * 4
    assert l.xnrs_attn_long_saved_bytes(L, Nb, E, 5) == 0            # E % n_heads != 0
    assert l.xnrs_attn_long_saved_bytes(L, Nb, 258, 2) == 0          # d_k = 129
    assert l.xnrs_caum_pool_bwd_workspace_bytes(320, 25, 136) >= 320 * 25 * 4
