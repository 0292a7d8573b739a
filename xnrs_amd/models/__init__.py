"""Drop-in for `xnrs.models`: same factory, same class names, HIP kernels underneath."""
from .assemblies import (NAML, NRMS, NRMS_LF, BaseRec, LSTURNewsEncoder, MeanRec, ParamFreeRec, StandardRec,  # noqa: F401
                         make_model)
from .blocks import ParentRec, TextEncoder, UserEncoder  # noqa: F401
from .components import layers, scoring  # noqa: F401
from .npa import NPA, PersonalizedAttention  # noqa: F401  (not in components.*: install() mirrors those)
from .lstur import LSTUR, LSTURUserEncoder  # noqa: F401  (opt-in like NPA: install(hip_models=("LSTUR",)))
from .caum import (CAUM, CAUMNewsEncoder, CAUMScoring, CAUMUserEncoder, CategoryEncoder,  # noqa: F401  (not routed by
                   DenseAttention)                                                         # install(): INTEGRATION.md)
