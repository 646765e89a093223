"""Alias of :mod:`dmd_era5_amd.trend` (per-grid-point trend and harmonic regression, fitted and removed on device)."""
from dmd_era5_amd.trend import *  # noqa: F401,F403
from dmd_era5_amd.trend import __all__  # noqa: F401
