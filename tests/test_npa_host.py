"""CPU: NPA's host side -- xnrs_amd.models.NPA builds the reference's state_dict (keys, shapes and initial values of
config/mind_small_NPA.yml at a small n_users, tests/golden/npa.json / npa.npz), the new C prototypes parse, the default
install() routing of NPA is unchanged and install(hip_models=("NPA",)) routes it to ours (over a stub package, as
tests/test_install.py sets one up)."""
import json
import os

import numpy as np
import torch

from tests import helpers as H
from tests.golden import npa_cases as NC
from tests.test_install import make_stub, run

GOLD = H.golden("npa")
META = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "npa.json")))


class Cfg(dict):
    __getattr__ = dict.__getitem__


def test_npa_builds_the_reference_state_dict_bitwise():
    from xnrs_amd.models import NPA
    from xnrs_amd.models.npa import make_npa
    con = META["contract"]
    cfg = Cfg(dict(con["cfg"], n_users=NC.INIT["n_users"]))
    torch.manual_seed(NC.INIT["seed"])
    model = make_npa(cfg)
    assert type(model) is NPA
    sd = model.state_dict()
    assert list(sd) == con["keys"]
    assert [list(v.shape) for v in sd.values()] == con["shapes"]
    for k, v in sd.items():
        assert np.array_equal(NC.sample(v), GOLD[f"init/{k}"]), k
        assert v.double().sum().item() == float(GOLD[f"init_sum/{k}"]), k


def test_npa_is_not_exported_from_the_mirrored_components():
    from xnrs_amd.models.components import layers, news_encoding, parent, scoring, user_encoding
    for mod in (layers, news_encoding, user_encoding, scoring, parent):
        assert not hasattr(mod, "PersonalizedAttention") and not hasattr(mod, "NPA"), mod.__name__


def test_personalized_prototypes_parse():
    from xnrs_amd import hip
    for name in ("xnrs_personalized_saved_bytes", "xnrs_personalized_fwd", "xnrs_personalized_fwd_train",
                 "xnrs_personalized_bwd_workspace_bytes", "xnrs_personalized_bwd", "xnrs_embedding_grad_sparse",
                 "xnrs_embedding_linear_bwd_sparse_workspace_bytes", "xnrs_embedding_linear_bwd_sparse"):
        assert name in hip.PROTOTYPES, name
    fields = [f for f, _ in hip.STRUCTS["xnrs_personalized_params"]._fields_]
    assert fields == ["wx", "bx", "q", "q_idx", "hidden", "q_ld", "n_q"]
    assert hip.STATUS_QUERY_RANGE == 4
    assert hip.ABI_VERSION == 6


def test_default_install_keeps_npa_on_the_reference(tmp_path):
    stub = make_stub(tmp_path)
    r = run("""
        import xnrs_amd
        assert xnrs_amd.install() is True
        from xnrs.models import make_model
        from xnrs.models.full_models import NPA
        assert NPA.__module__ == 'xnrs.models.full_models.npa'      # the package's own file
        class Cfg(dict):
            __getattr__ = dict.__getitem__
        from tests.golden import npa_cases as NC
        assert make_model(Cfg(NC.model_cfg(NC.CASES['tiny']))) == ('stub-model', 'NPA')
        try:
            from xnrs_amd.models import make_model as ours
            ours(Cfg(NC.model_cfg(NC.CASES['tiny'])))
            raise SystemExit('make_model(NPA) must still raise')
        except NotImplementedError:
            pass
        print('ok')
        """, stub)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr + r.stdout


def test_install_with_hip_models_routes_npa_to_ours(tmp_path):
    stub = make_stub(tmp_path)
    r = run("""
        import xnrs_amd
        assert xnrs_amd.install(hip_models=("NPA",)) is True
        from xnrs.models import make_model
        from xnrs.models.full_models import NPA, NRMS
        from xnrs_amd.models import npa, assemblies
        assert NPA is npa.NPA and NRMS is assemblies.NRMS
        class Cfg(dict):
            __getattr__ = dict.__getitem__
        from tests.golden import npa_cases as NC
        m = make_model(Cfg(NC.model_cfg(NC.CASES['tiny'], 'bilin')))
        assert type(m) is npa.NPA and type(m.rec_model).__name__ == 'BilinScoring'
        try:
            xnrs_amd.install(force=True, hip_models=("CAUM",))
            raise SystemExit('an unknown opt-in must raise')
        except ValueError:
            pass
        print('ok')
        """, stub)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr + r.stdout


def test_install_opt_in_after_a_plain_install_is_applied(tmp_path):
    stub = make_stub(tmp_path)
    r = run("""
        import xnrs_amd
        assert xnrs_amd.install() is True
        from xnrs.models.full_models import NPA
        assert NPA.__module__ == 'xnrs.models.full_models.npa'      # plain install: the package's own file
        assert xnrs_amd.install(hip_models=("NPA",)) is True       # the opt-in is applied, not ignored
        from xnrs.models.full_models import NPA
        from xnrs.models import make_model
        from xnrs_amd.models import npa
        assert NPA is npa.NPA
        class Cfg(dict):
            __getattr__ = dict.__getitem__
        from tests.golden import npa_cases as NC
        assert type(make_model(Cfg(NC.model_cfg(NC.CASES['tiny'])))) is npa.NPA
        assert xnrs_amd.install() is True                           # a later plain call keeps the opt-in
        from xnrs.models.full_models import NPA
        assert NPA is npa.NPA
        print('ok')
        """, stub)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr + r.stdout
