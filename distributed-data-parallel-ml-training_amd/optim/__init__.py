"""Optimizers and flat parameter/gradient arenas."""
from .arena import ParamArena, arena_for  # noqa: F401
from .sgd import FusedSGD  # noqa: F401
from .lars import LARS  # noqa: F401
from .adamw import AdamW  # noqa: F401
from .lamb import LAMB  # noqa: F401
from .schedule import LRSchedule  # noqa: F401
