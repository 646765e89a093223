"""Alias of :mod:`dmd_era5_amd.extremes` (per-period extremes and totals of a daily statistic per grid point)."""
from dmd_era5_amd.extremes import *  # noqa: F401,F403
from dmd_era5_amd.extremes import __all__  # noqa: F401
