"""Import-path mirror of xnrs.models.components.scoring (implementation: xnrs_amd/models/blocks.py)."""
from ..blocks import BilinScoring, DotScoring, FCScoring  # noqa: F401
