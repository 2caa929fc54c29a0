from .objects import check_cc_args, component_table, label_components, object_scores, remove_small_objects  # noqa: F401
from .distance import boundary_scores, check_edt_args, distance_transform_sq, signed_distance  # noqa: F401
from .registration import apply_shift, check_apply_args, check_estimate_args, coregister, coregister_cities, estimate_shift  # noqa: F401
