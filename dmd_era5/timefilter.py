"""Alias of :mod:`dmd_era5_amd.timefilter` (temporal FIR filtering and decimation of the snapshots on the device)."""
from dmd_era5_amd.timefilter import *  # noqa: F401,F403
from dmd_era5_amd.timefilter import __all__  # noqa: F401
