"""`from src.training.ranger import Ranger` (src/training/coach.py:23) lands on the fused, capturable optimiser: same constructor,
param_groups and state keys as the reference's class (e4s_amd/optim.py:Ranger)."""
from e4s_amd.optim import Ranger

__all__ = ["Ranger"]
