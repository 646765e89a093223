from dmd_era5_amd.era5_svd import (  # noqa: F401
    add_config_attributes,
    combine_svd_results,
    main,
    project_onto_svd_results,
    reconstruct_from_svd_results,
    retrieve_era5_slice,
    retrieve_svd_results,
    svd_on_era5,
    write_forecast_slice,
)

__all__ = ["svd_on_era5", "combine_svd_results", "retrieve_era5_slice", "retrieve_svd_results",
           "add_config_attributes", "main", "reconstruct_from_svd_results",
           "project_onto_svd_results", "write_forecast_slice"]
