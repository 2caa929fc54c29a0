from .objects import check_cc_args, component_table, label_components, object_scores, remove_small_objects  # noqa: F401
