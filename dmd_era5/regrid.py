"""Alias of :mod:`dmd_era5_amd.regrid` (area-weighted coarsening and conservative remapping of the snapshots on the device)."""
from dmd_era5_amd.regrid import *  # noqa: F401,F403
from dmd_era5_amd.regrid import __all__  # noqa: F401
