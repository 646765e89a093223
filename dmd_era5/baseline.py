"""Alias of :mod:`dmd_era5_amd.baseline` (lagged moments per grid point: autocorrelation, persistence baselines, skill)."""
from dmd_era5_amd.baseline import *  # noqa: F401,F403
from dmd_era5_amd.baseline import __all__  # noqa: F401
