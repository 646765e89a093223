"""Alias of :mod:`dmd_era5_amd.spells` (spell and exceedance-count indices per grid point)."""
from dmd_era5_amd.spells import *  # noqa: F401,F403
from dmd_era5_amd.spells import __all__  # noqa: F401
