"""ctypes loader for the C ABI (include/smvs_hip.h -> csrc/libsmvs_hip.so).

There is no CPU fallback: if the HIP library is missing or no GPU is visible
the product path raises.  (The CPU oracle lives under oracle/ and is test
infrastructure; this package never imports it.)
"""
import ctypes as C
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libsmvs_hip.so")
HEADER = os.path.join(HERE, "..", "include", "smvs_hip.h")

_lib = None


class SmvsError(RuntimeError):
    def __init__(self, status, text):
        super().__init__("smvs_hip status %d: %s" % (status, text))
        self.status = status


class LoopParams(C.Structure):
    _fields_ = [("regularization", C.c_double),
                ("light_surf_regularization", C.c_double),
                ("full_optimization", C.c_int),
                ("max_newton_steps", C.c_int),
                ("cg_max_iterations", C.c_int),
                ("cg_q_tolerance", C.c_double),
                ("active_threshold", C.c_double),
                ("full_opt_threshold", C.c_double),
                ("use_lighting", C.c_int),
                ("lighting", C.c_double * 16),
                ("reset_active", C.c_int)]


class LoopStats(C.Structure):
    _fields_ = [("newton_steps", C.c_int),
                ("linear_iterations", C.c_int),
                ("active_patch_steps", C.c_longlong),
                ("final_active_nodes", C.c_int),
                ("nan_break", C.c_int)]


class TsdfOptions(C.Structure):
    """smvs_tsdf_options of include/smvs_hip.h."""
    _fields_ = [("cut_surfaces", C.c_int), ("origin", C.c_float * 3),
                ("voxel_size", C.c_float), ("dims", C.c_int * 3),
                ("trunc", C.c_float), ("min_weight", C.c_int)]


class TsdfSparseOptions(C.Structure):
    """smvs_tsdf_sparse_options of include/smvs_hip.h."""
    _fields_ = [("max_bricks", C.c_int64)]


class TsdfSparseStats(C.Structure):
    """smvs_tsdf_sparse_stats of include/smvs_hip.h."""
    _fields_ = [("bricks", C.c_int64), ("seed_bricks", C.c_int64),
                ("allocated_bricks", C.c_int64), ("state_bytes", C.c_int64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class TsdfSparseOpts(C.Structure):
    """smvs_tsdf_sparse_opts of include/smvs_hip.h."""
    _fields_ = [("max_bricks", C.c_int64), ("cull", C.c_int)]


class TsdfSparseOptsStats(C.Structure):
    """smvs_tsdf_sparse_opts_stats of include/smvs_hip.h."""
    _fields_ = TsdfSparseStats._fields_ + [("tested_bricks", C.c_int64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class TsdfVolumeOptions(C.Structure):
    """smvs_tsdf_volume_options of include/smvs_hip.h."""
    _fields_ = [("origin", C.c_float * 3), ("voxel_size", C.c_float), ("dims", C.c_int * 3),
                ("trunc", C.c_float)]


class TsdfSparseVolumeOptions(C.Structure):
    """smvs_tsdf_sparse_volume_options of include/smvs_hip.h."""
    _fields_ = TsdfVolumeOptions._fields_ + [("max_bricks", C.c_int64)]


class TsdfSparseVolumeStats(C.Structure):
    """smvs_tsdf_sparse_volume_stats of include/smvs_hip.h."""
    _fields_ = [("bricks", C.c_int64), ("seed_bricks", C.c_int64),
                ("allocated_bricks", C.c_int64), ("pending_bricks", C.c_int64),
                ("late_bricks", C.c_int64), ("state_bytes", C.c_int64), ("n_views", C.c_int64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class MeshCleanOptions(C.Structure):
    """smvs_mesh_clean_options of include/smvs_hip.h."""
    _fields_ = [("threshold", C.c_float), ("percentile", C.c_float),
                ("component_size", C.c_int), ("keep_unreferenced", C.c_int)]


class MeshCleanStats(C.Structure):
    """smvs_mesh_clean_stats of include/smvs_hip.h."""
    _fields_ = [("cut_value", C.c_float), ("n_cut", C.c_int64), ("n_components", C.c_int64),
                ("n_small_components", C.c_int64), ("n_small_vertices", C.c_int64),
                ("n_unreferenced", C.c_int64), ("largest_component", C.c_int64)]

    def as_dict(self):
        out = {name: int(getattr(self, name)) for name, _ in self._fields_[1:]}
        out["cut_value"] = float(self.cut_value)
        return out


K_NAMES = ["patch", "assemble", "cg_spmv", "cg_update", "cg_init",
           "reactivate", "misc", "cg_resident"]


def declared_symbols():
    """Entry points declared in include/smvs_hip.h."""
    with open(HEADER) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(smvs_[a-z_0-9]+)\s*\(", text)))


def load():
    """Load libsmvs_hip.so (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SmvsError(-2, "HIP extension %s is missing: run "
                        "`python -c 'import __graft_entry__ as g; g.build()'`"
                        % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    lib.smvs_last_error.restype = C.c_char_p
    _lib = lib
    return lib


def check(status):
    if status != 0:
        raise SmvsError(status, load().smvs_last_error().decode())
