"""Alias of :mod:`dmd_era5_amd.forecast` (full-field reconstruction, DMD forecast and their score)."""
from dmd_era5_amd.forecast import *  # noqa: F401,F403
from dmd_era5_amd.forecast import __all__  # noqa: F401
