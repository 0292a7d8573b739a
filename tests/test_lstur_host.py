"""CPU: LSTUR's host side -- xnrs_amd.models.LSTUR builds the reference's state_dict (keys, shapes and initial values of
config/mind_small_LSTUR.yml at a small n_users, tests/golden/lstur_model.json / .npz; shapes and parameter count of the
shipped n_users, shipped_configs.json), the GRU prototypes parse, the default install() routing of LSTUR is unchanged and
install(hip_models=("LSTUR",)) routes it to ours (over a stub package, as tests/test_install.py sets one up)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.golden import lstur_cases as LC
from tests.test_install import make_stub, run

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = H.golden("lstur_model")
META = json.load(open(os.path.join(HERE, "golden", "lstur_model.json")))
SHIPPED = json.load(open(os.path.join(HERE, "golden", "shipped_configs.json")))["mind_small_LSTUR"]


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _stub(tmp_path):
    """tests/test_install.py's stub package plus a full_models/lstur.py of its own."""
    stub = make_stub(tmp_path)
    (tmp_path / "xnrs" / "models" / "full_models" / "lstur.py").write_text("class LSTUR:\n    marker = 'stub-lstur'\n")
    return stub


def test_lstur_builds_the_reference_state_dict_bitwise():
    from xnrs_amd.models import LSTUR
    from xnrs_amd.models.lstur import make_lstur
    con = META["contract"]
    cfg = Cfg(dict(con["cfg"], n_users=LC.INIT["n_users"]))
    torch.manual_seed(LC.INIT["seed"])
    model = make_lstur(cfg)
    assert type(model) is LSTUR
    sd = model.state_dict()
    assert list(sd) == con["keys"]
    assert [list(v.shape) for v in sd.values()] == con["shapes"]
    assert sum(p.numel() for p in model.parameters()) == con["n_params"]
    for k, v in sd.items():
        assert np.array_equal(LC.sample(v), GOLD[f"init/{k}"]), k
        assert v.double().sum().item() == float(GOLD[f"init_sum/{k}"]), k


def test_shipped_config_builds_the_recorded_state_dict():
    """shipped_configs.json["mind_small_LSTUR"] plus the three keys the YAML adds ('mean', 'con', p_user_dropout 0.07)."""
    from xnrs_amd.models.lstur import make_lstur
    cfg = Cfg(dict(SHIPPED["cfg"], long_term_method="mean", long_short_term_method="con", p_user_dropout=0.07))
    model = make_lstur(cfg)
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert got == SHIPPED["state_dict"]
    assert sum(p.numel() for p in model.parameters()) == SHIPPED["n_params"] == 774835


@pytest.mark.parametrize("ltm,lstm", LC.COMBOS)
def test_every_combination_constructs_with_the_reference_layout(ltm, lstm):
    from xnrs_amd.models.lstur import make_lstur
    c = dict(LC.SHAPES["tiny"], ltm=ltm, lstm=lstm, scoring="dot", hole=False)
    model = make_lstur(Cfg(LC.model_cfg(c)))
    e = c["Et"] + c["Ec"]
    hd = e // 2 if lstm == "con" else e
    assert tuple(model.user_encoder.gru.weight_hh_l0.shape) == (3 * hd, hd)
    assert tuple(model.user_encoder.gru.weight_ih_l0.shape) == (3 * hd, e)
    if ltm == "embedding":
        table = model.user_encoder.long_term_encoder
        assert tuple(table.weight.shape) == (c["n_users"] + 1, hd) and table.padding_idx == 0
        assert float(table.weight.detach()[0].abs().max()) == 0.0
    else:
        assert tuple(model.user_encoder.long_term_encoder.head[0].weight.shape) == (e, e)


def test_lstur_is_not_exported_from_the_mirrored_components():
    from xnrs_amd.models.components import layers, news_encoding, parent, scoring, user_encoding
    for mod in (layers, news_encoding, user_encoding, scoring, parent):
        assert not hasattr(mod, "LSTUR") and not hasattr(mod, "LSTURUserEncoder"), mod.__name__


def test_gru_prototypes_parse():
    from xnrs_amd import hip
    for name in ("xnrs_gru_workspace_bytes", "xnrs_gru_saved_bytes", "xnrs_gru_fwd", "xnrs_gru_fwd_train",
                 "xnrs_gru_bwd_workspace_bytes", "xnrs_gru_bwd"):
        assert name in hip.PROTOTYPES, name
    assert [f for f, _ in hip.STRUCTS["xnrs_gru_params"]._fields_] == ["w_ih", "w_hh", "b_ih", "b_hh", "hidden"]
    assert [f for f, _ in hip.STRUCTS["xnrs_gru_grads"]._fields_] == ["w_ih", "w_hh", "b_ih", "b_hh"]
    assert hip.ABI_VERSION == 6 and hip.STATUS_QUERY_RANGE == 4


def test_gru_size_queries_are_pure_host_calls():
    from xnrs_amd import hip
    l = hip.lib()
    B, T, E, Hd = 64, 25, 272, 136
    saved = l.xnrs_gru_saved_bytes(B, T, E, Hd)
    assert saved >= B * T * 5 * Hd * 4 and saved < 2 * B * T * 5 * Hd * 4       # r | z | n, W_hn h + b_hn, the states
    assert l.xnrs_gru_workspace_bytes(B, T, E, Hd) >= B * T * 3 * Hd * 4
    assert l.xnrs_gru_bwd_workspace_bytes(B, T, E, Hd) >= 2 * B * T * 3 * Hd * 4   # dGi and dGh over the stacked rows
    assert l.xnrs_gru_saved_bytes(B, 0, E, Hd) == 0


def test_a_cpu_call_raises_with_no_fallback():
    from xnrs_amd import hip, ops
    from xnrs_amd.models.lstur import make_lstur
    c = LC.CASES["tiny/embedding_ini"]
    model = make_lstur(Cfg(LC.model_cfg(c))).eval()
    with pytest.raises(hip.XnrsHipError):
        model(LC.batch(c))
    with pytest.raises(hip.XnrsHipError):
        model.user_encoder((torch.randn(4, 6, 12), torch.ones(4, 6, 1)), torch.zeros(4, 1, dtype=torch.int32))
    with pytest.raises(hip.XnrsHipError):
        ops.gru(torch.randn(2, 3, 12), None, None, torch.nn.GRU(12, 12, batch_first=True))
    with pytest.raises(hip.XnrsHipError):
        ops.embedding_rows(torch.zeros(2, dtype=torch.int32), torch.randn(5, 3))


def test_default_install_keeps_lstur_on_the_reference(tmp_path):
    stub = _stub(tmp_path)
    r = run("""
        import xnrs_amd
        assert xnrs_amd.install() is True
        from xnrs.models import make_model
        from xnrs.models.full_models import LSTUR
        assert LSTUR.__module__ == 'xnrs.models.full_models.lstur'      # the package's own file
        class Cfg(dict):
            __getattr__ = dict.__getitem__
        from tests.golden import lstur_cases as LC
        cfg = Cfg(LC.model_cfg(LC.CASES['tiny/embedding_ini']))
        assert make_model(cfg) == ('stub-model', 'LSTUR')
        try:
            from xnrs_amd.models import make_model as ours
            ours(cfg)
            raise SystemExit('make_model(LSTUR) must still raise')
        except NotImplementedError:
            pass
        print('ok')
        """, stub)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr + r.stdout


def test_install_with_hip_models_routes_lstur_to_ours(tmp_path):
    stub = _stub(tmp_path)
    r = run("""
        import xnrs_amd
        assert xnrs_amd.install(hip_models=("LSTUR",)) is True
        from xnrs.models import make_model
        from xnrs.models.full_models import LSTUR, NPA, NRMS
        from xnrs_amd.models import lstur, assemblies
        assert LSTUR is lstur.LSTUR and NRMS is assemblies.NRMS
        assert NPA.__module__ == 'xnrs.models.full_models.npa'         # the other opt-in stays where it was
        class Cfg(dict):
            __getattr__ = dict.__getitem__
        from tests.golden import lstur_cases as LC
        m = make_model(Cfg(LC.model_cfg(LC.CASES['tiny/bilin'])))
        assert type(m) is lstur.LSTUR and type(m.rec_model).__name__ == 'BilinScoring'
        try:
            xnrs_amd.install(force=True, hip_models=("CAUM",))
            raise SystemExit('an unknown opt-in must raise')
        except ValueError:
            pass
        print('ok')
        """, stub)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr + r.stdout
