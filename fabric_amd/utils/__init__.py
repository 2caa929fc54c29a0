from .objects import check_cc_args, component_table, label_components, object_scores, remove_small_objects  # noqa: F401
from .distance import boundary_scores, check_edt_args, distance_transform_sq, signed_distance  # noqa: F401
from .morphology import (binary_closing, binary_dilation, binary_erosion, binary_opening, clear_border, fill_holes, hysteresis_mask,  # noqa: F401
                         reconstruct)
from .registration import apply_shift, check_apply_args, check_estimate_args, coregister, coregister_cities, estimate_shift  # noqa: F401
from .radiometry import (apply_transfer, band_quantiles, check_fit_args, check_quantile_args, check_transfer_args, fit_transfer,  # noqa: F401
                         match_histograms, match_range, normalize_cities)
from .mad import MadResult, auto_change_mask, change_mask, check_mad_args, irmad  # noqa: F401
from .thresholds import RasterHistogram, ThresholdTable, auto_threshold, bin_edges  # noqa: F401
