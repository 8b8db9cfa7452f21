"""mcptam_amd: the HIP path of the multi-camera tracker and map maker.  The modules load the native library when first used, not on import."""


def __getattr__(name):
    # MapGraph and the selection's restatements, without importing numpy-heavy modules for callers that only want a submodule
    if name in ("MapGraph", "bundle_select_ref", "bundle_select_host", "kf_lists_ref", "kf_lists_host", "MeasParcel", "parcel_commit_ref", "parcel_commit_host",
                "cull_outliers_ref", "cull_outliers_host", "cull_sweep_ref", "cull_sweep_host", "neighbours_ref", "neighbours_host", "cull_mkf_ref", "cull_mkf_host",
                "collect_nearest_ref", "collect_nearest_host",
                "init_depth_ref", "init_depth_host", "mark_optimized_ref", "mark_optimized_host", "map_transform_ref", "map_transform_host"):
        from . import map_graph
        return getattr(map_graph, name)
    raise AttributeError("module 'mcptam_amd' has no attribute %r" % name)
