"""Alias of :mod:`dmd_era5_amd.mktrend` (the Mann-Kendall test and the Theil-Sen slope per grid point, on the device)."""
from dmd_era5_amd.mktrend import *  # noqa: F401,F403
from dmd_era5_amd.mktrend import __all__  # noqa: F401
