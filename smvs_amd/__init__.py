"""smvs_amd -- MI355X-native depth-optimisation hot path of smvs.

The product is csrc/libsmvs_hip.so behind the C ABI of include/smvs_hip.h;
this package is the thin host-side handle used by tests and bench.py.
"""
from . import _capi  # noqa: F401
from .device import (ViewContext, device_count, sgm_run, bilateral_upsample,  # noqa: F401
                     sgm_depth_for_view, sgm_check_merge, sgm_sweep_for_view,
                     sgm_fold_costs, sgm_filter_speckles, sgm_photo_check, sgm_plane_refine, cut_depth_maps, generate_points,
                     generate_mesh,
                     generate_simplified, simplify_triangulate, fuse_tsdf, tsdf_bounds,
                     tsdf_brick_cull, tsdf_depth_pyramid, clean_mesh, TsdfVolume,
                     SparseTsdfVolume)

__all__ = ["ViewContext", "device_count", "sgm_run", "bilateral_upsample",
           "sgm_depth_for_view", "sgm_check_merge", "sgm_sweep_for_view", "sgm_fold_costs", "sgm_filter_speckles", "sgm_photo_check", "sgm_plane_refine",
           "cut_depth_maps", "generate_points", "generate_mesh",
           "generate_simplified", "simplify_triangulate", "fuse_tsdf", "tsdf_bounds",
           "tsdf_brick_cull", "tsdf_depth_pyramid", "clean_mesh", "TsdfVolume",
           "SparseTsdfVolume"]
