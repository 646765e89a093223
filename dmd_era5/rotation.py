"""Alias of :mod:`dmd_era5_amd.rotation` (varimax / orthomax rotation of the leading modes, iterated on the device)."""
from dmd_era5_amd.rotation import *  # noqa: F401,F403
from dmd_era5_amd.rotation import __all__  # noqa: F401
