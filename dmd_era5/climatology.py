"""Alias of :mod:`dmd_era5_amd.climatology` (slot climatology of the snapshots and anomalies against it)."""
from dmd_era5_amd.climatology import *  # noqa: F401,F403
from dmd_era5_amd.climatology import __all__  # noqa: F401
