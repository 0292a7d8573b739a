"""CPU: the bilinear and MLP scorers (cfg.scoring 'bilin' / 'fc', xnrs/models/components/scoring.py:41-102) as make_model
builds them -- state_dict contract of the shipped configs and initial values against tests/golden/scorers.json (made by the
real reference, make_golden_scorers.py), the refusals that stay, and the import-path mirrors after install()."""
import json
import os

import pytest
import torch
import torch.nn as nn

from tests.golden import scorer_cases as SC
from tests.test_install import make_stub, run
from xnrs_amd import synth
from xnrs_amd.models import make_model
from xnrs_amd.models.blocks import BilinScoring, FCScoring

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
META = json.load(open(os.path.join(GOLDEN, "scorers.json")))
SHIPPED = json.load(open(os.path.join(GOLDEN, "shipped_configs.json")))


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _shipped_cfg(name, scoring):
    cfg = dict(SHIPPED[name]["cfg"], scoring=scoring)
    return Cfg(cfg)


@pytest.mark.parametrize("name", ["mind_small_NRMS", "mind_small_CL", "mind_small_NAML"])
@pytest.mark.parametrize("scoring", ["bilin", "fc"])
def test_state_dict_contract_of_the_shipped_configs(name, scoring):
    ref = META["contract"][f"{name}/{scoring}"]
    model = make_model(_shipped_cfg(name, scoring))
    sd = model.state_dict()
    assert list(sd) == ref["keys"]
    assert [list(v.shape) for v in sd.values()] == ref["shapes"]
    assert sum(p.numel() for p in model.parameters()) == ref["n_params"]
    # the reference's checkpoint loads strictly (values: the contract's shapes, synthetic numbers)
    ref_sd = synth.fill_state_dict({k: tuple(s) for k, s in zip(ref["keys"], ref["shapes"])}, 5)
    model.load_state_dict(ref_sd, strict=True)
    assert type(model.rec_model) is (BilinScoring if scoring == "bilin" else FCScoring)


@pytest.mark.parametrize("label", ["bilin_bias", "bilin_nobias", "fc_bias", "fc_nobias"])
def test_initial_parameters_equal_the_reference_under_the_same_seed(label):
    E = SC.INIT["E"]
    torch.manual_seed(SC.INIT["seed"])
    bias = label.endswith("_bias")
    mod = BilinScoring(E, bias=bias) if label.startswith("bilin") else FCScoring(E, hidden_dim=E // 2, bias=bias)
    ref = META["init"][label]
    sd = mod.state_dict()
    assert sorted(sd) == sorted(ref)  # (key order: test_state_dict_contract_of_the_shipped_configs)
    for k, v in sd.items():
        assert v.reshape(-1).tolist() == ref[k], k  # bit for bit


def test_make_model_scorer_arguments():
    """emb_dim = cfg.total_emb_dim, bias = cfg.bias, hidden = emb_dim // 2 (make_model.py:17-28), for every model."""
    for model in ("standard", "base", "mean", "NRMS", "NAML"):
        c = dict(model=model, E=16, bias=False, h=4, D=32, H=3, S=8)
        m = make_model(Cfg(dict(synth.model_cfg(c), scoring="fc")))
        assert (m.rec_model.fc1.in_features, m.rec_model.fc1.out_features, m.rec_model.fc1.bias) == (32, 8, None)
        m = make_model(Cfg(dict(synth.model_cfg(dict(c, bias=True)), scoring="bilin")))
        assert tuple(m.rec_model.bilin.weight.shape) == (1, 16, 16) and m.rec_model.bilin.bias is not None
        assert m.rec_model.normalize is False


def test_refusals_that_stay():
    with pytest.raises(NotImplementedError):
        FCScoring(8, 4, activation=torch.relu)
    with pytest.raises(NotImplementedError):
        FCScoring(8, 4, activation=nn.ReLU())
    for act in (torch.tanh, torch.nn.functional.tanh, nn.Tanh()):
        assert FCScoring(8, 4, activation=act).activation is act
    c = synth.model_cfg(dict(model="NRMS", E=16, bias=False, h=4, D=32, H=3, S=8))
    with pytest.raises(ValueError):
        make_model(Cfg(dict(c, scoring="nonlin")))
    with pytest.raises(ValueError):
        make_model(Cfg(dict(c, scoring="cosine")))
    with pytest.raises(NotImplementedError):
        make_model(Cfg(dict(c, scoring="CAUMScoring")))
    with pytest.raises(NotImplementedError):
        make_model(Cfg(dict(c, model="CAUM")))
    for model in ("NPA", "LSTUR", "smallNAML"):
        with pytest.raises(NotImplementedError):
            make_model(Cfg(dict(c, model=model, scoring="fc")))


def test_cpu_inputs_raise_the_library_error():
    """No CPU fallback (test_abi.py::test_no_silent_cpu_fallback): a CPU call raises before anything runs."""
    from xnrs_amd.hip import XnrsHipError
    u, c = torch.randn(2, 1, 8), torch.randn(2, 3, 8)
    for mod in (BilinScoring(8), BilinScoring(8, normalize=True), FCScoring(8, 4)):
        with pytest.raises(XnrsHipError):
            mod(u, c)


def test_install_mirrors_the_scorers(tmp_path):
    stub = make_stub(tmp_path)
    (tmp_path / "xnrs" / "models" / "components" / "scoring.py").write_text(
        "class CAUMScoring:\n    marker = 'stub-scoring'\n\nclass BilinScoring:\n    marker = 'stub-must-lose'\n")
    r = run("""
        import xnrs_amd
        assert xnrs_amd.install() is True
        from xnrs.models.components.scoring import BilinScoring, FCScoring, CAUMScoring, DotScoring
        from xnrs_amd.models import blocks
        assert BilinScoring is blocks.BilinScoring and FCScoring is blocks.FCScoring and DotScoring is blocks.DotScoring
        assert CAUMScoring.marker == 'stub-scoring'      # not on the path: the package's own class
        from xnrs.models import make_model
        from xnrs_amd import synth

        class Cfg(dict):
            __getattr__ = dict.__getitem__
        c = synth.model_cfg(dict(model='standard', E=16, bias=True, h=4, D=32, H=3, S=8))
        assert type(make_model(Cfg(dict(c, scoring='bilin'))).rec_model) is blocks.BilinScoring
        assert type(make_model(Cfg(dict(c, scoring='fc'))).rec_model) is blocks.FCScoring
        assert make_model(Cfg(dict(c, model='NPA'))) == ('stub-model', 'NPA')   # outside the path: the package's factory
        print('ok')
    """, stub)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().endswith("ok")
