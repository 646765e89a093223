"""Alias of :mod:`dmd_era5_amd.gapfill` (DINEOF gap filling of missing values from the rank-k factors, on the device)."""
from dmd_era5_amd.gapfill import *  # noqa: F401,F403
from dmd_era5_amd.gapfill import __all__  # noqa: F401
