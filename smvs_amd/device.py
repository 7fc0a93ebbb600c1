"""Thin Python handle on one smvs_ctx (one reference view on one GPU).

All arithmetic happens in libsmvs_hip.so; this module only marshals numpy
buffers across the C ABI of include/smvs_hip.h.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import LoopParams, LoopStats, check

_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_u8p = C.POINTER(C.c_uint8)
_u16p = C.POINTER(C.c_uint16)
_u32p = C.POINTER(C.c_uint32)
_i32p = C.POINTER(C.c_int32)


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None else None


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def device_count():
    return _capi.load().smvs_device_count()


class ViewContext:
    """One reference view + its neighbours on one GPU."""

    def __init__(self, width, height, n_subs, device=0):
        self.lib = _capi.load()
        self.width, self.height, self.n_subs = width, height, n_subs
        self.handle = C.c_void_p()
        check(self.lib.smvs_ctx_create(device, width, height, n_subs,
                                       C.byref(self.handle)))
        self.num_nodes = 0
        self.num_patches = 0

    def close(self):
        if self.handle:
            self.lib.smvs_ctx_destroy(self.handle)
            self.handle = C.c_void_p()
            for ptr in getattr(self, "_pinned", []):
                self.lib.smvs_pinned_free(ptr)
            self._pinned = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    SOLVERS = dict(auto=0, streaming=1, resident_ref=2)

    def set_solver(self, mode):
        """smvs_ctx_set_solver: 'auto' | 'streaming' | 'resident_ref'."""
        check(self.lib.smvs_ctx_set_solver(self.handle, self.SOLVERS[mode]))

    # ------------------------------------------------------------ uploads
    def set_views(self, views):
        """views: dict as produced by smvs_amd.synth.make_problem."""
        M = _f64(views["M"]).reshape(-1, 9); t = _f64(views["t"]).reshape(-1, 3)
        assert M.shape[0] == self.n_subs
        check(self.lib.smvs_ctx_set_cameras(self.handle, _p(M, _dp), _p(t, _dp),
              C.c_float(views["flen"]), C.c_float(views["inv_flen"])))
        grad = _f32(views["grad"])
        assert grad.shape == (self.height, self.width, 2)
        sh = _f32(views["shading"]) if views.get("shading") is not None else None
        shg = _f32(views["shading_grad"]) if views.get("shading_grad") is not None else None
        check(self.lib.smvs_ctx_upload_main(self.handle, _p(grad, _fp),
                                            _p(sh, _fp), _p(shg, _fp)))
        for j, (g, h) in enumerate(views["subs"]):
            g = _f32(g); h = _f32(h)
            check(self.lib.smvs_ctx_upload_sub(self.handle, j, g.shape[1],
                  g.shape[0], _p(g, _fp), _p(h, _fp)))

    def upload_image(self, view, img_u8):
        """view = -1: main view, otherwise neighbour index."""
        img = np.ascontiguousarray(img_u8, dtype=np.uint8)
        if img.ndim == 2:
            img = img[:, :, None]
        h, w, c = img.shape
        check(self.lib.smvs_ctx_upload_image(self.handle, view, w, h, c,
                                             _p(img, _u8p)))
        if not hasattr(self, "_image_shapes"):
            self._image_shapes = {}
        self._image_shapes[view] = (h, w)

    def upload_image_async(self, view, img_u8):
        """smvs_ctx_upload_image_async from page-locked memory: the image is
        copied into a smvs_pinned_alloc buffer that this object keeps until
        close(); the transfer and the conversion are only enqueued."""
        img = np.ascontiguousarray(img_u8, dtype=np.uint8)
        if img.ndim == 2:
            img = img[:, :, None]
        h, w, c = img.shape
        ptr = C.c_void_p()
        check(self.lib.smvs_pinned_alloc(C.c_size_t(img.size), C.byref(ptr)))
        if not hasattr(self, "_pinned"):
            self._pinned = []
        self._pinned.append(ptr)
        C.memmove(ptr, img.ctypes.data, img.size)
        check(self.lib.smvs_ctx_upload_image_async(self.handle, view, w, h, c,
                                                   C.cast(ptr, _u8p)))
        if not hasattr(self, "_image_shapes"):
            self._image_shapes = {}
        self._image_shapes[view] = (h, w)

    def sgm_init_depth(self, dm, sigma=5.0, kernel_size=5):
        """depthmap_bilateral_filter(dm, main image) guided by the uploaded main
        image; the result also stays in the context for topology_subviews()."""
        if dm is None:
            check(self.lib.smvs_ctx_sgm_init_depth(self.handle, None, 0, 0,
                  C.c_float(sigma), kernel_size, None))
            return None
        d = _f32(dm)
        out = np.zeros((self.height, self.width), dtype=np.float32)
        check(self.lib.smvs_ctx_sgm_init_depth(self.handle, _p(d, _fp), d.shape[1],
              d.shape[0], C.c_float(sigma), kernel_size, _p(out, _fp)))
        return out

    def sgm_init_depth_mve(self, dm_mve, inv_calibration9, sigma=5.0, kernel_size=5,
                           dm_is_z_depth=False):
        """sgm_init_depth() from the map as the view stores it (MVE's ray-length
        convention): converted to z-depth on the device (smvs_ctx_sgm_init_depth_mve)."""
        d = _f32(dm_mve)
        inv = _f32(np.asarray(inv_calibration9).reshape(9))
        out = np.zeros((self.height, self.width), dtype=np.float32)
        check(self.lib.smvs_ctx_sgm_init_depth_mve(self.handle, _p(d, _fp), d.shape[1],
              d.shape[0], _p(inv, _fp), 1 if dm_is_z_depth else 0, C.c_float(sigma),
              kernel_size, _p(out, _fp)))
        return out

    def sgm_init_slants(self, slant, want_plane=True):
        """smvs_ctx_sgm_init_slants: the slant plane of the context from the
        SGM-scale slants (dm_h, dm_w, 2), after sgm_init_depth[_mve]; returns the
        (H, W, 2) plane (None with want_plane=False).  slant None forgets it."""
        if slant is None:
            check(self.lib.smvs_ctx_sgm_init_slants(self.handle, None, 0, 0, None))
            return None
        s = _f32(slant)
        if s.ndim != 3 or s.shape[2] != 2:
            raise ValueError("slant must be (dm_h, dm_w, 2)")
        out = np.zeros((self.height, self.width, 2), np.float32) if want_plane else None
        check(self.lib.smvs_ctx_sgm_init_slants(self.handle, _p(s, _fp), s.shape[1],
              s.shape[0], _p(out, _fp)))
        return out

    def create_surface(self, scale, depth=None, slant=None, planes=None):
        """smvs_surface_create from depth (H, W), or from the resident filtered
        SGM map with depth None; slant (H, W, 2) -- or planes=True with both
        None: the resident ones -- makes it smvs_surface_create_planes.  Returns
        the surface as surface_download() does, plus valid_patches."""
        use_planes = slant is not None if planes is None else bool(planes)
        d = None if depth is None else _f32(depth)
        valid = C.c_int(0)
        if use_planes:
            s = None if slant is None else _f32(slant)
            check(self.lib.smvs_surface_create_planes(self.handle, scale, _p(d, _fp),
                  _p(s, _fp), C.byref(valid)))
        else:
            check(self.lib.smvs_surface_create(self.handle, scale, _p(d, _fp), None, None, 0,
                  C.byref(valid)))
        out = self.surface_download()
        out["valid_patches"] = valid.value
        return out

    def surface_download(self):
        """smvs_surface_info + smvs_surface_download: geometry and arrays."""
        g = (C.c_int * 6)()
        check(self.lib.smvs_surface_info(self.handle, C.cast(g, C.c_void_p), None))
        scale, _, npx, npy, sx, sy = (int(x) for x in g)
        self.num_nodes, self.num_patches = (npx + 1) * (npy + 1), npx * npy
        nodes = np.zeros((self.num_nodes, 4))
        nv = np.zeros(self.num_nodes, np.uint8)
        pv = np.zeros(self.num_patches, np.uint8)
        check(self.lib.smvs_surface_download(self.handle, _p(nodes, _dp), _p(nv, _u8p),
              _p(pv, _u8p), None))
        return dict(scale=scale, npx=npx, npy=npy, start_x=sx, start_y=sy, nodes=nodes,
                    node_valid=nv, patch_valid=pv)

    def surface_slants(self):
        """smvs_surface_slants: the slant plane the surface keeps, (H, W, 2)."""
        out = np.zeros((self.height, self.width, 2), np.float32)
        check(self.lib.smvs_surface_slants(self.handle, _p(out, _fp)))
        return out

    def set_scale(self, scale):
        check(self.lib.smvs_ctx_set_scale(self.handle, scale))

    def download_planes(self, view):
        h, w = self._image_shapes[view]
        grad = np.zeros((h, w, 2), np.float32)
        hess = np.zeros((h, w, 3), np.float32) if view >= 0 else None
        check(self.lib.smvs_ctx_download_planes(self.handle, view, _p(grad, _fp),
                                                _p(hess, _fp)))
        return grad, hess

    def prepare_shading(self, gamma_lut=None):
        """smvs_ctx_prepare_shading: the main view's shading planes from its
        uploaded image; gamma_lut = host.gamma_inv_srgb_lut() for --gamma-srgb.
        Only enqueues."""
        lut = None
        if gamma_lut is not None:
            lut = _f32(gamma_lut).reshape(-1)
            if lut.size != 256:
                raise ValueError("prepare_shading: the table has 256 entries")
        check(self.lib.smvs_ctx_prepare_shading(self.handle, _p(lut, _fp)))

    def download_shading(self):
        """(shading (h, w), shading gradients (h, w, 2)) of the context."""
        shading = np.zeros((self.height, self.width), np.float32)
        grad = np.zeros((self.height, self.width, 2), np.float32)
        check(self.lib.smvs_ctx_download_shading(self.handle, _p(shading, _fp),
                                                 _p(grad, _fp)))
        return shading, grad

    def upload_shading(self, shading, shading_grad):
        """smvs_ctx_upload_shading: planes computed elsewhere."""
        sh = _f32(shading); shg = _f32(shading_grad)
        assert sh.shape == (self.height, self.width)
        assert shg.shape == (self.height, self.width, 2)
        check(self.lib.smvs_ctx_upload_shading(self.handle, _p(sh, _fp), _p(shg, _fp)))

    def set_surface(self, surf):
        nodes = _f64(surf["nodes"]).reshape(-1, 4)
        nv = np.ascontiguousarray(surf["node_valid"], dtype=np.uint8)
        pv = np.ascontiguousarray(surf["patch_valid"], dtype=np.uint8)
        vis = np.ascontiguousarray(surf["patch_vis"], dtype=np.uint32)
        self.num_nodes = (surf["npx"] + 1) * (surf["npy"] + 1)
        self.num_patches = surf["npx"] * surf["npy"]
        assert nodes.shape[0] == self.num_nodes and pv.size == self.num_patches
        check(self.lib.smvs_ctx_set_surface(self.handle, surf["scale"],
              surf["npx"], surf["npy"], surf["start_x"], surf["start_y"],
              _p(nodes, _dp), _p(nv, _u8p), _p(pv, _u8p), _p(vis, _u32p)))

    def set_active(self, active=None):
        a = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
        check(self.lib.smvs_ctx_set_active(self.handle, _p(a, _u8p)))

    def get_active(self):
        a = np.zeros(self.num_nodes, dtype=np.uint8); n = C.c_int(0)
        check(self.lib.smvs_get_active(self.handle, _p(a, _u8p), C.byref(n)))
        return a, n.value

    def get_nodes(self):
        nodes = np.zeros((self.num_nodes, 4))
        check(self.lib.smvs_get_nodes(self.handle, _p(nodes, _dp)))
        return nodes

    def set_nodes(self, nodes):
        nodes = _f64(nodes).reshape(-1, 4)
        assert nodes.shape[0] == self.num_nodes
        check(self.lib.smvs_set_nodes(self.handle, _p(nodes, _dp)))

    def save_nodes(self):
        """Keep a device-resident copy of the nodes (restore_nodes brings it
        back without a transfer)."""
        check(self.lib.smvs_ctx_save_nodes(self.handle))

    def restore_nodes(self):
        check(self.lib.smvs_ctx_restore_nodes(self.handle))

    def clone_loop_state(self):
        """smvs_ctx_clone_loop_state: a second context holding what this one's
        Newton loop reads now (planes, cameras, surface, masks), nodes saved."""
        other = ViewContext.__new__(ViewContext)
        other.lib = self.lib
        other.width, other.height, other.n_subs = self.width, self.height, self.n_subs
        other.handle = C.c_void_p()
        check(self.lib.smvs_ctx_clone_loop_state(self.handle, C.byref(other.handle)))
        other.num_nodes, other.num_patches = self.num_nodes, self.num_patches
        return other

    # ------------------------------------------------------------ GN step
    def gn_construct(self, regularization, light_reg=0.0, lighting=None):
        lt = _f64(lighting) if lighting is not None else None
        n = C.c_int(0)
        check(self.lib.smvs_gn_construct(self.handle, C.c_double(regularization),
              C.c_double(light_reg), _p(lt, _dp), C.byref(n)))
        return n.value

    def gn_download(self):
        N = self.num_nodes
        H9 = np.zeros((N, 9, 16)); g = np.zeros(4 * N); P = np.zeros((N, 16))
        check(self.lib.smvs_gn_download(self.handle, _p(H9, _dp), _p(g, _dp),
                                        _p(P, _dp)))
        return H9, g, P

    def gn_upload(self, H9, g, P):
        H9 = _f64(H9); g = _f64(g); P = _f64(P)
        check(self.lib.smvs_gn_upload(self.handle, _p(H9, _dp), _p(g, _dp),
                                      _p(P, _dp)))

    def gn_patch_systems(self):
        Hp = np.zeros((self.num_patches, 16, 16)); gp = np.zeros((self.num_patches, 16))
        check(self.lib.smvs_gn_download_patch_systems(self.handle, _p(Hp, _dp),
                                                      _p(gp, _dp)))
        return Hp, gp

    def cg_solve(self, max_iterations=200, error_tolerance=-1.0, q_tolerance=1e-3):
        it = C.c_int(0); info = C.c_int(0)
        check(self.lib.smvs_cg_solve(self.handle, max_iterations,
              C.c_double(error_tolerance), C.c_double(q_tolerance),
              C.byref(it), C.byref(info)))
        return it.value, info.value

    def cg_x(self):
        x = np.zeros(4 * self.num_nodes)
        check(self.lib.smvs_cg_download_x(self.handle, _p(x, _dp)))
        return x

    def cg_set_x(self, x):
        x = _f64(x)
        check(self.lib.smvs_cg_upload_x(self.handle, _p(x, _dp)))

    def update_and_reactivate(self, threshold=0.15, full_optimization=False):
        n = C.c_int(0); mean = C.c_double(0.0); nan = C.c_int(0)
        check(self.lib.smvs_update_and_reactivate(self.handle, C.c_double(threshold),
              1 if full_optimization else 0, C.byref(n), C.byref(mean), C.byref(nan)))
        return n.value, mean.value, nan.value

    def run_loop(self, regularization, light_reg=0.0, lighting=None,
                 full_optimization=False, max_newton_steps=200,
                 cg_max_iterations=200, reset_active=True,
                 active_threshold=0.15, full_opt_threshold=0.01):
        # (the struct of the previous call is reused when nothing changed: a
        # Newton batch is short enough for the marshalling to show)
        key = (regularization, light_reg, full_optimization, max_newton_steps,
               cg_max_iterations, reset_active, active_threshold, full_opt_threshold)
        cached = getattr(self, "_loop_params", None)
        if lighting is None and cached is not None and cached[0] == key:
            p = cached[1]
            s = LoopStats()
            check(self.lib.smvs_gn_run_loop(self.handle, C.byref(p), C.byref(s)))
            return dict(newton_steps=s.newton_steps,
                        linear_iterations=s.linear_iterations,
                        active_patch_steps=s.active_patch_steps,
                        final_active_nodes=s.final_active_nodes,
                        nan_break=s.nan_break)
        p = LoopParams()
        p.regularization = regularization
        p.light_surf_regularization = light_reg
        p.full_optimization = 1 if full_optimization else 0
        p.max_newton_steps = max_newton_steps
        p.cg_max_iterations = cg_max_iterations
        p.cg_q_tolerance = 1e-3
        p.active_threshold = active_threshold
        p.full_opt_threshold = full_opt_threshold
        p.use_lighting = 1 if lighting is not None else 0
        if lighting is not None:
            for i in range(16):
                p.lighting[i] = float(lighting[i])
        p.reset_active = 1 if reset_active else 0
        self._loop_params = (key, p) if lighting is None else None
        s = LoopStats()
        check(self.lib.smvs_gn_run_loop(self.handle, C.byref(p), C.byref(s)))
        return dict(newton_steps=s.newton_steps,
                    linear_iterations=s.linear_iterations,
                    active_patch_steps=s.active_patch_steps,
                    final_active_nodes=s.final_active_nodes,
                    nan_break=s.nan_break)

    # ------------------------------------------------------------ outputs
    def depth_map(self):
        out = np.zeros((self.height, self.width), dtype=np.float32)
        check(self.lib.smvs_get_depth_map(self.handle, _p(out, _fp)))
        return out

    def normal_map(self):
        out = np.zeros((self.height, self.width, 3), dtype=np.float32)
        check(self.lib.smvs_get_normal_map(self.handle, _p(out, _fp)))
        return out

    def maps(self, inv_calibration=None, pinned=False):
        """smvs_get_maps: depth and normal map in one pass; inv_calibration
        (9 floats) -> the depth in MVE's ray-length convention; pinned: the
        outputs live in page-locked memory from smvs_pinned_alloc (direct DMA)."""
        import ctypes as C
        inv = None if inv_calibration is None \
            else np.ascontiguousarray(inv_calibration, dtype=np.float32).reshape(9)
        n = self.height * self.width
        if not pinned:
            depth = np.zeros((self.height, self.width), dtype=np.float32)
            normals = np.zeros((self.height, self.width, 3), dtype=np.float32)
            check(self.lib.smvs_get_maps(self.handle, _p(inv, _fp) if inv is not None else None,
                                         _p(depth, _fp), _p(normals, _fp)))
            return depth, normals
        pd, pn = C.c_void_p(), C.c_void_p()
        check(self.lib.smvs_pinned_alloc(C.c_size_t(4 * n), C.byref(pd)))
        check(self.lib.smvs_pinned_alloc(C.c_size_t(12 * n), C.byref(pn)))
        try:
            check(self.lib.smvs_get_maps(self.handle, _p(inv, _fp) if inv is not None else None,
                                         C.cast(pd, _fp), C.cast(pn, _fp)))
            depth = np.ctypeslib.as_array(C.cast(pd, _fp), (self.height, self.width)).copy()
            normals = np.ctypeslib.as_array(C.cast(pn, _fp),
                                            (self.height, self.width, 3)).copy()
        finally:
            check(self.lib.smvs_pinned_free(pd))
            check(self.lib.smvs_pinned_free(pn))
        return depth, normals

    def light_accumulate(self):
        A = np.zeros((16, 16)); b = np.zeros(16)
        check(self.lib.smvs_light_accumulate(self.handle, _p(A, _dp), _p(b, _dp)))
        return A, b

    def light_accumulate_dev(self):
        """Leaves A (256) + b (16) doubles in the context's device buffer and
        returns its device address (for an in-place RCCL all-reduce)."""
        ptr = C.c_void_p()
        check(self.lib.smvs_light_accumulate_dev(self.handle, C.byref(ptr)))
        return ptr.value

    def light_upload(self, A, b):
        A = _f64(A).reshape(16, 16); b = _f64(b).reshape(16)
        check(self.lib.smvs_light_upload(self.handle, _p(A, _dp), _p(b, _dp)))

    def light_download(self):
        A = np.zeros((16, 16)); b = np.zeros(16)
        check(self.lib.smvs_light_download(self.handle, _p(A, _dp), _p(b, _dp)))
        return A, b

    # ------------------------------------------------------------ topology
    def topology_subviews(self, sgm_depth=None, use_ncc=True):
        """create_subview_surfaces' per-(patch, neighbour) tests -> bit masks.
        sgm_depth None: the map sgm_init_depth() left in the context, if any."""
        sd = _f32(sgm_depth) if sgm_depth is not None else None
        if sd is not None:
            assert sd.shape == (self.height, self.width)
        vis = np.zeros(self.num_patches, dtype=np.uint32)
        check(self.lib.smvs_topology_subviews(self.handle, _p(sd, _fp),
              1 if use_ncc else 0, _p(vis, _u32p)))
        return vis

    def topology_patch_mse(self):
        mse = np.zeros(self.num_patches)
        check(self.lib.smvs_topology_patch_mse(self.handle, _p(mse, _dp)))
        return mse

    def topology_cut_boundaries(self, inv_calibration):
        """`while (deleted > 10) cut_boundaries()` -> (patch_valid, node_valid, deleted)."""
        k = _f32(inv_calibration).reshape(9)
        pv = np.zeros(self.num_patches, dtype=np.uint8)
        nv = np.zeros(self.num_nodes, dtype=np.uint8)
        n = C.c_int(0)
        check(self.lib.smvs_topology_cut_boundaries(self.handle, _p(k, _fp),
              _p(pv, _u8p), _p(nv, _u8p), C.byref(n)))
        return pv, nv, n.value

    def synchronize(self):
        check(self.lib.smvs_ctx_synchronize(self.handle))

    # ---------------------------------------------------------- profiling
    def profile(self, on=True):
        check(self.lib.smvs_profile_enable(self.handle, 1 if on else 0))

    def profile_reset(self):
        check(self.lib.smvs_profile_reset(self.handle))

    def profile_get(self):
        ms = (C.c_double * 8)(); cnt = (C.c_longlong * 8)()
        check(self.lib.smvs_profile_get(self.handle, ms, cnt))
        return {k: (ms[i], cnt[i]) for i, k in enumerate(_capi.K_NAMES)}


P2_CONSTANT, P2_ADAPTIVE = 0, 1   # smvs_sgm_p2_mode of include/smvs_hip.h
WINNER_PLANE, WINNER_SUBPLANE = 0, 1   # smvs_sgm_winner


class SgmOptions(C.Structure):
    """smvs_sgm_options of include/smvs_hip.h."""
    _fields_ = [("p2_mode", C.c_int), ("winner", C.c_int)]


def _sgm_options(adaptive_p2, subplane):
    return SgmOptions(P2_ADAPTIVE if adaptive_p2 else P2_CONSTANT,
                      WINNER_SUBPLANE if subplane else WINNER_PLANE)


MERGE_REFERENCE, MERGE_CONSENSUS = 0, 1   # smvs_sgm_merge
MAX_SUBS = 16                             # SMVS_MAX_SUBS


class SgmViewOptions(C.Structure):
    """smvs_sgm_view_options of include/smvs_hip.h."""
    _fields_ = [("p2_mode", C.c_int), ("winner", C.c_int), ("merge", C.c_int),
                ("min_agree", C.c_int), ("agree_ratio", C.c_float)]


class SgmCheckNeighbor(C.Structure):
    """smvs_sgm_check_neighbor of include/smvs_hip.h."""
    _fields_ = [("bwd", _fp), ("width", C.c_int), ("height", C.c_int),
                ("M_fwd", C.c_float * 9), ("t_fwd", C.c_float * 3)]


def _sgm_view_options(adaptive_p2, subplane, consensus, agree_ratio, min_agree):
    return SgmViewOptions(P2_ADAPTIVE if adaptive_p2 else P2_CONSTANT,
                          WINNER_SUBPLANE if subplane else WINNER_PLANE,
                          MERGE_CONSENSUS if consensus else MERGE_REFERENCE,
                          int(min_agree), float(agree_ratio))


class SgmFilterOptions(C.Structure):
    """smvs_sgm_filter_options of include/smvs_hip.h."""
    _fields_ = [("uniqueness", C.c_int), ("uniqueness_window", C.c_int),
                ("speckle_size", C.c_int), ("speckle_ratio", C.c_float)]


# (uniqueness, uniqueness_window, speckle_size, speckle_ratio) of the Python
# fronts: both filters off.  Defaults of a user option, untuned; nobody has
# measured them on real scenes.
SGM_FILTER_DEFAULTS = (0, 1, 0, 0.95)


def _sgm_filter(uniqueness, uniqueness_window, speckle_size, speckle_ratio):
    """The filter options, or None where they are the defaults (the entries
    without the filters are called then)."""
    if (uniqueness, uniqueness_window, speckle_size, speckle_ratio) == SGM_FILTER_DEFAULTS:
        return None
    return SgmFilterOptions(int(uniqueness), int(uniqueness_window), int(speckle_size),
                            float(speckle_ratio))


class SgmPhotoOptions(C.Structure):
    """smvs_sgm_photo_options of include/smvs_hip.h."""
    _fields_ = [("radius", C.c_int), ("best_k", C.c_int), ("min_views", C.c_int),
                ("min_score", C.c_float)]


# (photo_radius, photo_best_k, photo_min_views, photo_min_score) of the Python
# fronts: the photo-consistency test off.  Defaults of a user option, untuned;
# nobody has measured them on real scenes.
SGM_PHOTO_DEFAULTS = (0, 2, 2, 0.49)


def _sgm_photo(radius, best_k, min_views, min_score, witnesses):
    """The photo options, or None where they are the defaults and there is no
    witness (the entries without the test are called then)."""
    if (radius, best_k, min_views, min_score) == SGM_PHOTO_DEFAULTS and not witnesses:
        return None
    return SgmPhotoOptions(int(radius), int(best_k), int(min_views), float(min_score))


def _sgm_witnesses(neighbors, witnesses):
    """The front's neighbours followed by the further witnesses of the photo test
    as full neighbour dicts (of a witness only image, M_fwd and t_fwd are read)."""
    return list(neighbors) + [
        dict(M_bwd=np.zeros(9), t_bwd=np.zeros(3), range_main=(0, 0), range_neighbor=(0, 0),
             **{k: nb[k] for k in ("image", "M_fwd", "t_fwd")}) for nb in witnesses or ()]


def sgm_photo_check(main_img, depth, witnesses, radius=2, best_k=2, min_views=2, min_score=0.49,
                    device=0):
    """smvs_sgm_photo_check: the multi-view photo-consistency test of
    include/smvs_hip.h alone (not in the reference), on a map of the caller.
    main_img (h, w) u8 at SGM scale; depth (h, w) float in the depth convention of
    the SGM planes; witnesses: 1 .. 16 dicts {image (nh, nw) u8, M_fwd, t_fwd} (the
    float reprojection main -> witness).  Per valid pixel (depth > 0) and witness
    the (2 radius + 1)^2 window of the main image against its warp into the
    witness at the pixel's own depth: the signed squared correlation, where every
    sample lies inside the witness.  confidence = the mean of the best_k largest
    scores (0: of all), -1 with fewer than max(min_views, 1) of them; no depth
    where confidence < min_score (-1 drops nothing).  Returns (out (h, w) f32,
    confidence (h, w) f32, views (h, w) u8: the witnesses with a score).  The
    defaults are defaults of a user option, untuned."""
    lib = _capi.load()
    main_img = np.ascontiguousarray(main_img, dtype=np.uint8)
    depth = _f32(depth)
    if main_img.ndim != 2 or depth.shape != main_img.shape:
        raise ValueError("main_img and depth: (h, w)")
    h, w = depth.shape
    keep = []
    arr = _sgm_neighbors(_sgm_witnesses([], witnesses), keep) if len(witnesses) else None
    if any(k.ndim != 2 for k in keep):
        raise ValueError("witness images: (nh, nw), one channel at SGM scale")
    opts = SgmPhotoOptions(int(radius), int(best_k), int(min_views), float(min_score))
    out = np.zeros((h, w), dtype=np.float32)
    conf = np.zeros((h, w), dtype=np.float32)
    views = np.zeros((h, w), dtype=np.uint8)
    check(lib.smvs_sgm_photo_check(device, _p(main_img, _u8p), w, h, _p(depth, _fp), arr,
          len(witnesses), C.byref(opts), _p(out, _fp), _p(conf, _fp), _p(views, _u8p)))
    return out, conf, views


class SgmRefineOptions(C.Structure):
    """smvs_sgm_refine_options of include/smvs_hip.h."""
    _fields_ = [("sweeps", C.c_int), ("samples", C.c_int), ("depth_step", C.c_float),
                ("slant_step", C.c_float), ("seed", C.c_uint32), ("fill", C.c_int)]


# (refine_sweeps, refine_samples, refine_depth_step, refine_slant_step,
# refine_seed, refine_fill) of the Python fronts: the plane refinement sweeps off.
# Defaults of a user option, untuned; nobody has measured them on real scenes.
SGM_REFINE_DEFAULTS = (0, 2, 0.02, 0.01, 1, 1)


def _sgm_refine(sweeps, samples, depth_step, slant_step, seed, fill):
    """The refine options, or None where they are the defaults (the entries
    without the sweeps are called then)."""
    if (sweeps, samples, depth_step, slant_step, seed, fill) == SGM_REFINE_DEFAULTS:
        return None
    return SgmRefineOptions(int(sweeps), int(samples), float(depth_step), float(slant_step),
                            int(seed) & 0xFFFFFFFF, int(fill))


def sgm_plane_refine(main_img, depth, witnesses, radius=2, best_k=2, min_views=2, min_score=0.49,
                     sweeps=0, samples=2, depth_step=0.02, slant_step=0.01, seed=1, fill=1,
                     device=0):
    """smvs_sgm_plane_refine: the multi-view plane refinement sweeps of
    include/smvs_hip.h alone (not in the reference), on a map of the caller.
    main_img, depth, witnesses, radius, best_k, min_views, min_score: as for
    sgm_photo_check, whose confidence is the objective.  Every pixel holds a plane
    (depth, two slants); in each of `sweeps` red-black sweeps (0 .. 8) a pixel
    adopts a 4-neighbour's extrapolated plane, or one of `samples` (0 .. 8) hashed
    perturbations of its own (relative steps depth_step and slant_step, halved per
    sweep; seed), whenever that raises its confidence; fill = 1 lets pixels
    without a depth adopt a neighbour's plane.  sweeps = 0 gives sgm_photo_check's
    outputs and zero slants.  Returns (out (h, w) f32, slant (h, w, 2) f32,
    confidence (h, w) f32, views (h, w) u8).  The defaults are defaults of a user
    option, untuned."""
    lib = _capi.load()
    main_img = np.ascontiguousarray(main_img, dtype=np.uint8)
    depth = _f32(depth)
    if main_img.ndim != 2 or depth.shape != main_img.shape:
        raise ValueError("main_img and depth: (h, w)")
    h, w = depth.shape
    keep = []
    arr = _sgm_neighbors(_sgm_witnesses([], witnesses), keep) if len(witnesses) else None
    if any(k.ndim != 2 for k in keep):
        raise ValueError("witness images: (nh, nw), one channel at SGM scale")
    photo = SgmPhotoOptions(int(radius), int(best_k), int(min_views), float(min_score))
    refine = SgmRefineOptions(int(sweeps), int(samples), float(depth_step), float(slant_step),
                              int(seed) & 0xFFFFFFFF, int(fill))
    out = np.zeros((h, w), dtype=np.float32)
    slant = np.zeros((h, w, 2), dtype=np.float32)
    conf = np.zeros((h, w), dtype=np.float32)
    views = np.zeros((h, w), dtype=np.uint8)
    check(lib.smvs_sgm_plane_refine(device, _p(main_img, _u8p), w, h, _p(depth, _fp), arr,
          len(witnesses), C.byref(photo), C.byref(refine), _p(out, _fp), _p(slant, _fp),
          _p(conf, _fp), _p(views, _u8p)))
    return out, slant, conf, views


def sgm_filter_speckles(depth, speckle_size, speckle_ratio=0.95, device=0):
    """smvs_sgm_filter_speckles: the speckle kernels of include/smvs_hip.h alone
    (not in the reference).  depth (h, w) float; pixels > 0 are valid, two valid
    4-neighbours are linked where min / max >= speckle_ratio, and every
    component with fewer than speckle_size pixels is set to 0.  Returns
    (out (h, w) f32, size (h, w) u32: the pixel count of each pixel's component,
    0 for a pixel that is not valid)."""
    lib = _capi.load()
    depth = _f32(depth)
    if depth.ndim != 2:
        raise ValueError("depth: (h, w)")
    h, w = depth.shape
    out = np.zeros((h, w), dtype=np.float32)
    size = np.zeros((h, w), dtype=np.uint32)
    check(lib.smvs_sgm_filter_speckles(device, _p(depth, _fp), w, h, int(speckle_size),
          C.c_float(speckle_ratio), _p(out, _fp), _p(size, C.POINTER(C.c_uint32))))
    return out, size


def sgm_run(main_img, neighbor_img, M, t, min_depth, max_depth, num_steps=128,
            p1=6, p2=96, device=0, want_volumes=False, adaptive_p2=False, subplane=False,
            uniqueness=0, uniqueness_window=1):
    """SGMStereo::run_sgm on the device.  adaptive_p2: the path aggregation of
    the reference's build without SSE (lib/sgm_stereo.cc:310-346, penalty2
    adapted to the intensity step); off by default.
    subplane: the depth of the winning plane refined by the parabola through
    its aggregated cost and its two neighbours' (SMVS_SGM_WINNER_SUBPLANE of
    include/smvs_hip.h, not in the reference); argmin and the volumes are the
    same; off by default.
    uniqueness (0 .. 99, a percentage; 0 is off), uniqueness_window (1 .. 256
    planes): the uniqueness test of include/smvs_hip.h (not in the reference): no
    depth where a plane more than the window away from the winner has a sum r
    with r * (100 - uniqueness) < S[winner] * 100.  With uniqueness > 0 and
    want_volumes the dict also holds runner_up (h, w) u16.  (0, 1) are defaults
    of a user option, untuned."""
    lib = _capi.load()
    main_img = np.ascontiguousarray(main_img, dtype=np.uint8)
    neighbor_img = np.ascontiguousarray(neighbor_img, dtype=np.uint8)
    M = _f32(M).reshape(9); t = _f32(t).reshape(3)
    h, w = main_img.shape; nh, nw = neighbor_img.shape
    depth = np.zeros((h, w), dtype=np.float32)
    argmin = np.zeros((h, w), dtype=np.int32)
    cost = np.zeros((h, w, num_steps), dtype=np.uint16) if want_volumes else None
    sgm = np.zeros((h, w, num_steps), dtype=np.uint16) if want_volumes else None
    opts = _sgm_options(adaptive_p2, subplane)
    filt = _sgm_filter(uniqueness, uniqueness_window, *SGM_FILTER_DEFAULTS[2:])
    if filt is not None:
        runner = np.zeros((h, w), dtype=np.uint16) \
            if want_volumes and filt.uniqueness != 0 else None
        check(lib.smvs_sgm_run_filtered(device, _p(main_img, _u8p), w, h,
              _p(neighbor_img, _u8p), nw, nh, _p(M, _fp), _p(t, _fp),
              C.c_float(min_depth), C.c_float(max_depth), num_steps,
              C.c_uint16(p1), C.c_uint16(p2), C.byref(opts), C.byref(filt),
              _p(depth, _fp), _p(argmin, _i32p), _p(cost, _u16p), _p(sgm, _u16p),
              _p(runner, _u16p)))
        out = dict(depth=depth, argmin=argmin, cost=cost, sgm=sgm)
        if runner is not None:
            out["runner_up"] = runner
        return out
    check(lib.smvs_sgm_run_opts(device, _p(main_img, _u8p), w, h,
          _p(neighbor_img, _u8p), nw, nh, _p(M, _fp), _p(t, _fp),
          C.c_float(min_depth), C.c_float(max_depth), num_steps,
          C.c_uint16(p1), C.c_uint16(p2), C.byref(opts),
          _p(depth, _fp), _p(argmin, _i32p), _p(cost, _u16p), _p(sgm, _u16p)))
    return dict(depth=depth, argmin=argmin, cost=cost, sgm=sgm)


def bilateral_upsample(dm, ci, sigma=5.0, kernel_size=5, device=0):
    lib = _capi.load()
    dm = _f32(dm); ci = _f32(ci)
    if ci.ndim == 2:
        ci = ci[:, :, None]
    h, w, c = ci.shape; dh, dw = dm.shape
    out = np.zeros((h, w), dtype=np.float32)
    check(lib.smvs_bilateral_upsample(device, _p(dm, _fp), dw, dh, _p(ci, _fp),
          w, h, c, C.c_float(sigma), kernel_size, _p(out, _fp)))
    return out


def _halved(w, h, halvings):
    """(w, h) after `halvings` half-size steps, (s + 1) // 2 each: the size of
    the device's output for a raw image."""
    for _ in range(max(int(halvings or 0), 0)):
        w, h = (w + 1) // 2, (h + 1) // 2
    return w, h


def rescale_half_gaussian(image, halvings=1, device=0):
    """smvs_rescale_half_gaussian: `halvings` chained rescale_half_size_gaussian
    of a u8 image (h, w) or (h, w, c), c = 1..4, on the device
    (app/smvsrecon.cc:634-647); bit-identical with the host mirror's function."""
    lib = _capi.load()
    a = np.ascontiguousarray(image, dtype=np.uint8)
    squeeze = a.ndim == 2
    if squeeze:
        a = a[:, :, None]
    h, w, c = a.shape
    ow, oh = _halved(w, h, halvings)
    out = np.zeros((oh, ow, c), np.uint8)
    gw, gh = C.c_int(0), C.c_int(0)
    check(lib.smvs_rescale_half_gaussian(C.c_int(device), _p(a, _u8p), C.c_int(w),
          C.c_int(h), C.c_int(c), C.c_int(halvings), _p(out, _u8p),
          C.c_size_t(out.size), C.byref(gw), C.byref(gh)))
    assert (gw.value, gh.value) == (ow, oh)
    return out[:, :, 0] if squeeze else out


class Lens(C.Structure):
    """smvs_lens of include/smvs_hip.h: the source camera in pixels, COLMAP's
    convention (the centre of pixel (0, 0) is (0.5, 0.5))."""
    _fields_ = [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")]


def make_lens(lens):
    """A Lens from a Lens, a dict with fx, fy, cx, cy and optionally k1, k2, p1,
    p2 (or f for fx = fy), or a sequence in the struct's order."""
    if isinstance(lens, Lens):
        return lens
    if isinstance(lens, dict):
        d = dict(lens)
        if "f" in d:
            d.setdefault("fx", d["f"]); d.setdefault("fy", d["f"])
        return Lens(*[float(d.get(k, 0.0)) for k, _ in Lens._fields_])
    v = [float(x) for x in lens]
    return Lens(*(v + [0.0] * (8 - len(v))))


def undistort(image, lens, out_focal, out_size=None, device=0, return_blank=False):
    """smvs_undistort_u8: a u8 image (h, w) or (h, w, c), c = 1..4, of the camera
    `lens` resampled on the device into the pinhole camera of focal length
    out_focal pixels with a centred principal point; out_size = (width, height),
    the input's by default.  return_blank: (image, number of blank pixels)."""
    lib = _capi.load()
    a = np.ascontiguousarray(image, dtype=np.uint8)
    squeeze = a.ndim == 2
    if squeeze:
        a = a[:, :, None]
    h, w, c = a.shape
    ow, oh = (w, h) if out_size is None else (int(out_size[0]), int(out_size[1]))
    out = np.zeros((max(oh, 0), max(ow, 0), c), np.uint8)
    blank = C.c_int64(0)
    L = make_lens(lens)
    check(lib.smvs_undistort_u8(C.c_int(device), _p(a, _u8p), C.c_int(w), C.c_int(h),
          C.c_int(c), C.byref(L), C.c_float(out_focal), C.c_int(ow), C.c_int(oh),
          _p(out, _u8p), C.byref(blank)))
    out = out[:, :, 0] if squeeze else out
    return (out, blank.value) if return_blank else out


class SgmNeighbor(C.Structure):
    """smvs_sgm_neighbor of include/smvs_hip.h."""
    _fields_ = [("image", _u8p), ("width", C.c_int), ("height", C.c_int),
                ("M_fwd", C.c_float * 9), ("t_fwd", C.c_float * 3),
                ("M_bwd", C.c_float * 9), ("t_bwd", C.c_float * 3),
                ("range_main", C.c_float * 2), ("range_neighbor", C.c_float * 2)]


def sgm_depth_for_view(main_img, neighbors, num_steps=128, p1=6, p2=96, device=0,
                       adaptive_p2=False, halvings=None, subplane=False,
                       consensus=False, agree_ratio=0.95, min_agree=2, want_checked=False,
                       uniqueness=0, uniqueness_window=1, speckle_size=0, speckle_ratio=0.95,
                       photo_radius=0, photo_best_k=2, photo_min_views=2, photo_min_score=0.49,
                       witnesses=None,
                       refine_sweeps=0, refine_samples=2, refine_depth_step=0.02,
                       refine_slant_step=0.01, refine_seed=1, refine_fill=1):
    """reconstruct_sgm_depth_for_view on the device.  neighbors: list of dicts
    {image, M_fwd, t_fwd, M_bwd, t_bwd, range_main, range_neighbor} (SGM-scale
    u8 images, float reprojections).  adaptive_p2, subplane: as for sgm_run
    (all four runs of the view).
    halvings (an int): the images are full-resolution u8 embeddings of one or
    three channels, desaturated and halved that often on the device
    (smvs_sgm_depth_for_view_raw_opts); the map has the SGM-scale size.
    consensus: SMVS_SGM_MERGE_CONSENSUS of include/smvs_hip.h (not in the
    reference, which merges the first two neighbours): 1 .. 16 neighbours, per
    pixel the mean of the largest group of checked depths whose ratio to one of
    them is at least agree_ratio, or 0 with fewer than min_agree of them; off by
    default.  0.95 and 2 are defaults of a user option, not tuned values (0.95
    admits about two of 128 planes at the far end of a 3 .. 12 range; the
    left/right check uses 0.8); nobody has measured their effect on real scenes.
    want_checked (with consensus): returns a dict {depth, checked (n, h, w),
    support (h, w) u8} instead of the depth map.
    uniqueness, uniqueness_window: the uniqueness test of sgm_run in every run of
    the view.  speckle_size, speckle_ratio: the speckle removal of
    sgm_filter_speckles on the merged map (sizes 0 and 1 are off).  Both are
    filters of include/smvs_hip.h, not in the reference and off by default;
    (0, 1, 0, 0.95) are defaults of a user option, untuned, and nobody has
    measured them on real scenes.
    photo_radius (1 .. 3; 0 is off), photo_best_k, photo_min_views,
    photo_min_score, witnesses: the photo-consistency test of sgm_photo_check on
    the view's final map, before the speckle removal.  Its witnesses are the
    neighbours followed by `witnesses` (dicts {image, M_fwd, t_fwd}, images as the
    neighbours'; at most 16 in all).  Returns a dict {depth, confidence, views}
    (and checked, support with want_checked).  Off by default; witnesses or a
    changed option with photo_radius = 0 is an error.  (0, 2, 2, 0.49) are
    defaults of a user option, untuned.
    refine_sweeps (1 .. 8; 0 is off), refine_samples, refine_depth_step,
    refine_slant_step, refine_seed, refine_fill: the plane refinement sweeps of
    sgm_plane_refine in the photo test's place (they need photo_radius > 0); the
    dict then also holds slant (h, w, 2).  Off by default; a changed option with
    refine_sweeps = 0 goes to the entry with the sweeps, which gives the photo
    test's bytes.  (0, 2, 0.02, 0.01, 1, 1) are defaults of a user option,
    untuned."""
    lib = _capi.load()
    main_img = np.ascontiguousarray(main_img, dtype=np.uint8)
    filt = _sgm_filter(uniqueness, uniqueness_window, speckle_size, speckle_ratio)
    photo = _sgm_photo(photo_radius, photo_best_k, photo_min_views, photo_min_score, witnesses)
    refine = _sgm_refine(refine_sweeps, refine_samples, refine_depth_step, refine_slant_step,
                         refine_seed, refine_fill)
    if refine is not None and photo is None:
        photo = SgmPhotoOptions(*SGM_PHOTO_DEFAULTS)
    if photo is not None:
        if want_checked and not consensus:
            raise ValueError("want_checked: the checked maps and the support are "
                             "outputs of the consensus merge")
        return _sgm_depth_for_view_photo(
            lib, main_img, neighbors, witnesses, num_steps, p1, p2, device,
            _sgm_view_options(adaptive_p2, subplane, consensus, agree_ratio, min_agree),
            halvings, want_checked,
            filt if filt is not None else SgmFilterOptions(*SGM_FILTER_DEFAULTS), photo,
            refine)
    if consensus or want_checked or filt is not None:
        if want_checked and not consensus:
            raise ValueError("want_checked: the checked maps and the support are "
                             "outputs of the consensus merge")
        return _sgm_depth_for_view_merge(
            lib, main_img, neighbors, num_steps, p1, p2, device,
            _sgm_view_options(adaptive_p2, subplane, consensus, agree_ratio, min_agree),
            None if halvings is None else int(halvings), want_checked, filt)
    return _sgm_depth_for_view_raw(lib, main_img, neighbors, num_steps, p1, p2, device,
                                   _sgm_options(adaptive_p2, subplane),
                                   None if halvings is None else int(halvings))


def _sgm_neighbors(neighbors, keep):
    arr = (SgmNeighbor * len(neighbors))()
    for k, nb in enumerate(neighbors):
        img = np.ascontiguousarray(nb["image"], dtype=np.uint8)
        keep.append(img)
        arr[k].image = _p(img, _u8p)
        arr[k].height, arr[k].width = img.shape[:2]
        for name, n in (("M_fwd", 9), ("t_fwd", 3), ("M_bwd", 9), ("t_bwd", 3),
                        ("range_main", 2), ("range_neighbor", 2)):
            v = _f32(nb[name]).reshape(n)
            for i in range(n):
                getattr(arr[k], name)[i] = float(v[i])
    return arr


def _sgm_depth_for_view_raw(lib, main_img, neighbors, num_steps, p1, p2, device, opts,
                            halvings):
    """smvs_sgm_depth_for_view_opts (halvings None) / _raw_opts."""
    keep = []
    arr = _sgm_neighbors(neighbors, keep)
    h, w = main_img.shape[:2]
    ow, oh = _halved(w, h, halvings)
    depth = np.zeros((oh, ow), dtype=np.float32)
    if halvings is None:
        if main_img.ndim != 2 or any(k.ndim != 2 for k in keep):
            raise ValueError("one-channel images at SGM scale (or pass halvings)")
        check(lib.smvs_sgm_depth_for_view_opts(device, _p(main_img, _u8p), w, h, arr,
              len(neighbors), num_steps, C.c_uint16(p1), C.c_uint16(p2), C.byref(opts),
              _p(depth, _fp)))
        return depth
    channels = 1 if main_img.ndim == 2 else main_img.shape[2]
    nch = (C.c_int * len(neighbors))(*[1 if k.ndim == 2 else k.shape[2] for k in keep])
    check(lib.smvs_sgm_depth_for_view_raw_opts(device, _p(main_img, _u8p), w, h, channels,
          arr, nch, len(neighbors), halvings, num_steps, C.c_uint16(p1), C.c_uint16(p2),
          C.byref(opts), _p(depth, _fp)))
    return depth


def _sgm_depth_for_view_merge(lib, main_img, neighbors, num_steps, p1, p2, device, vopts,
                              halvings, want_checked, filt=None):
    """smvs_sgm_depth_for_view_merge (halvings None) / _raw_merge; with filt
    (SgmFilterOptions) smvs_sgm_depth_for_view_filtered / _raw_filtered."""
    keep = []
    arr = _sgm_neighbors(neighbors, keep)
    n = len(neighbors)
    h, w = main_img.shape[:2]
    ow, oh = _halved(w, h, halvings)
    depth = np.zeros((oh, ow), dtype=np.float32)
    checked = np.zeros((n, oh, ow), dtype=np.float32) if want_checked else None
    support = np.zeros((oh, ow), dtype=np.uint8) if want_checked else None
    if halvings is None:
        if main_img.ndim != 2 or any(k.ndim != 2 for k in keep):
            raise ValueError("one-channel images at SGM scale (or pass halvings)")
        if filt is not None:
            check(lib.smvs_sgm_depth_for_view_filtered(device, _p(main_img, _u8p), w, h, arr,
                  n, num_steps, C.c_uint16(p1), C.c_uint16(p2), C.byref(vopts),
                  C.byref(filt), _p(depth, _fp), _p(checked, _fp), _p(support, _u8p)))
        else:
            check(lib.smvs_sgm_depth_for_view_merge(device, _p(main_img, _u8p), w, h, arr, n,
                  num_steps, C.c_uint16(p1), C.c_uint16(p2), C.byref(vopts), _p(depth, _fp),
                  _p(checked, _fp), _p(support, _u8p)))
    else:
        channels = 1 if main_img.ndim == 2 else main_img.shape[2]
        nch = (C.c_int * n)(*[1 if k.ndim == 2 else k.shape[2] for k in keep])
        if filt is not None:
            check(lib.smvs_sgm_depth_for_view_raw_filtered(device, _p(main_img, _u8p), w, h,
                  channels, arr, nch, n, halvings, num_steps, C.c_uint16(p1),
                  C.c_uint16(p2), C.byref(vopts), C.byref(filt), _p(depth, _fp),
                  _p(checked, _fp), _p(support, _u8p)))
        else:
            check(lib.smvs_sgm_depth_for_view_raw_merge(device, _p(main_img, _u8p), w, h,
                  channels, arr, nch, n, halvings, num_steps, C.c_uint16(p1), C.c_uint16(p2),
                  C.byref(vopts), _p(depth, _fp), _p(checked, _fp), _p(support, _u8p)))
    if want_checked:
        return dict(depth=depth, checked=checked, support=support)
    return depth


def _raw_images(main_img, keep, halvings):
    """(channels, neighbour channel array, halvings) for a raw entry; halvings
    None: one-channel images at SGM scale, as (1, ones, 0)."""
    if halvings is None and (main_img.ndim != 2 or any(k.ndim != 2 for k in keep)):
        raise ValueError("one-channel images at SGM scale (or pass halvings)")
    channels = 1 if main_img.ndim == 2 else main_img.shape[2]
    nch = (C.c_int * max(len(keep), 1))(*[1 if k.ndim == 2 else k.shape[2] for k in keep])
    return channels, nch, 0 if halvings is None else int(halvings)


def _sgm_depth_for_view_photo(lib, main_img, neighbors, witnesses, num_steps, p1, p2, device,
                              vopts, halvings, want_checked, filt, photo, refine=None):
    """smvs_sgm_depth_for_view_raw_photo; with refine (SgmRefineOptions)
    smvs_sgm_depth_for_view_raw_refine."""
    keep = []
    every = _sgm_witnesses(neighbors, witnesses)
    arr = _sgm_neighbors(every, keep) if every else None
    n = len(neighbors)
    channels, nch, halvings = _raw_images(main_img, keep, halvings)
    h, w = main_img.shape[:2]
    ow, oh = _halved(w, h, halvings)
    depth = np.zeros((oh, ow), dtype=np.float32)
    checked = np.zeros((n, oh, ow), dtype=np.float32) if want_checked else None
    support = np.zeros((oh, ow), dtype=np.uint8) if want_checked else None
    on = photo.radius != 0
    conf = np.zeros((oh, ow), dtype=np.float32) if on else None
    views = np.zeros((oh, ow), dtype=np.uint8) if on else None
    args = (device, _p(main_img, _u8p), w, h, channels, arr, nch, n, halvings, num_steps,
            C.c_uint16(p1), C.c_uint16(p2), C.byref(vopts), C.byref(filt), _p(depth, _fp),
            _p(checked, _fp), _p(support, _u8p), len(every) - n, C.byref(photo), _p(conf, _fp),
            _p(views, _u8p))
    out = dict(depth=depth, confidence=conf, views=views)
    if refine is not None:
        slant = np.zeros((oh, ow, 2), dtype=np.float32) if refine.sweeps != 0 else None
        check(lib.smvs_sgm_depth_for_view_raw_refine(*args, C.byref(refine), _p(slant, _fp)))
        out["slant"] = slant
    else:
        check(lib.smvs_sgm_depth_for_view_raw_photo(*args))
    if want_checked:
        out.update(checked=checked, support=support)
    return out


def sgm_check_merge(fwd, neighbors, agree_ratio=0.95, min_agree=2, device=0):
    """smvs_sgm_check_merge: the kernel of the consensus front end alone, on
    maps of the caller.  fwd (n, h, w): the unchecked forward maps of the main
    view; neighbors: n dicts {bwd (nh, nw), M_fwd, t_fwd} (the neighbour's own
    backward map, the float reprojection main -> neighbour of the check).
    Returns dict(merged (h, w), checked (n, h, w), support (h, w) u8)."""
    lib = _capi.load()
    fwd = _f32(fwd)
    if fwd.ndim != 3 or fwd.shape[0] != len(neighbors):
        raise ValueError("fwd: (n, h, w) with one map per neighbour")
    n, h, w = fwd.shape
    keep = []
    arr = (SgmCheckNeighbor * max(n, 1))()
    for k, nb in enumerate(neighbors):
        b = _f32(nb["bwd"])
        keep.append(b)
        arr[k].bwd = _p(b, _fp)
        arr[k].height, arr[k].width = b.shape
        for name, cnt in (("M_fwd", 9), ("t_fwd", 3)):
            v = _f32(nb[name]).reshape(cnt)
            for i in range(cnt):
                getattr(arr[k], name)[i] = float(v[i])
    vopts = _sgm_view_options(False, False, True, agree_ratio, min_agree)
    merged = np.zeros((h, w), dtype=np.float32)
    checked = np.zeros((n, h, w), dtype=np.float32)
    support = np.zeros((h, w), dtype=np.uint8)
    check(lib.smvs_sgm_check_merge(device, _p(fwd, _fp), w, h, arr, n, C.byref(vopts),
          _p(merged, _fp), _p(checked, _fp), _p(support, _u8p)))
    return dict(merged=merged, checked=checked, support=support)


class SgmSweepOptions(C.Structure):
    """smvs_sgm_sweep_options of include/smvs_hip.h."""
    _fields_ = [("p2_mode", C.c_int), ("winner", C.c_int), ("min_views", C.c_int),
                ("best_k", C.c_int), ("support_cost", C.c_int), ("min_support", C.c_int)]


def sgm_sweep_defaults(n):
    """(min_views, best_k, support_cost, min_support) for n neighbours: defaults
    of a user option, untuned; nobody has measured them on real scenes."""
    return min(2, n), (n + 1) // 2, 20, min(2, n)


def sgm_sweep_for_view(main_img, neighbors, depth_range, num_steps=128, p1=6, p2=96, device=0,
                       adaptive_p2=False, subplane=False, halvings=None, min_views=None,
                       best_k=None, support_cost=20, min_support=None, want_volumes=False,
                       uniqueness=0, uniqueness_window=1, speckle_size=0, speckle_ratio=0.95,
                       photo_radius=0, photo_best_k=2, photo_min_views=2, photo_min_score=0.49,
                       witnesses=None,
                       refine_sweeps=0, refine_samples=2, refine_depth_step=0.02,
                       refine_slant_step=0.01, refine_seed=1, refine_fill=1):
    """The multi-neighbour plane sweep of include/smvs_hip.h (not in the
    reference; opt-in): one cost volume of the main view from all n = 1 .. 16
    neighbours -- per cell the rounded mean of the best_k smallest of the
    neighbours' cost bytes (0: of all), no cost with fewer than min_views of them
    -- aggregated once, one winner; support = the neighbours whose own cost at
    the winner plane is at most support_cost, and no depth below min_support of
    them.  No neighbour-side runs and no left/right check.
    neighbors: dicts of which image, M_fwd and t_fwd are read; depth_range:
    (min, max) of the main view.  halvings (an int): full-resolution embeddings
    of one or three channels, as for sgm_depth_for_view.  adaptive_p2, subplane:
    as for sgm_run.  min_views, best_k, min_support: None is min(2, n),
    (n + 1) // 2 and min(2, n); with support_cost = 20 these are defaults of a
    user option, untuned, and nobody has measured them on real scenes.
    uniqueness, uniqueness_window, speckle_size, speckle_ratio: the two filters of
    sgm_depth_for_view -- the uniqueness test in the sweep's one WTA step, the
    speckle removal behind the support test; off by default, defaults untuned.
    photo_radius, photo_best_k, photo_min_views, photo_min_score, witnesses: the
    photo-consistency test of sgm_depth_for_view behind the support test (the
    sweep's neighbours followed by `witnesses`); the dict then also holds
    confidence and views.  Off by default, defaults untuned.
    refine_sweeps, refine_samples, refine_depth_step, refine_slant_step,
    refine_seed, refine_fill: the plane refinement sweeps of sgm_depth_for_view in
    the photo test's place; the dict then also holds slant.  Off by default,
    defaults untuned.
    Returns dict(depth, argmin, support[, cost, sgm][, runner_up: with
    want_volumes and uniqueness > 0]); with halvings dict(depth, support)."""
    lib = _capi.load()
    n = len(neighbors)
    filt = _sgm_filter(uniqueness, uniqueness_window, speckle_size, speckle_ratio)
    photo = _sgm_photo(photo_radius, photo_best_k, photo_min_views, photo_min_score, witnesses)
    refine = _sgm_refine(refine_sweeps, refine_samples, refine_depth_step, refine_slant_step,
                         refine_seed, refine_fill)
    if refine is not None and photo is None:
        photo = SgmPhotoOptions(*SGM_PHOTO_DEFAULTS)
    d_views, d_k, _, d_support = sgm_sweep_defaults(n)
    opts = SgmSweepOptions(P2_ADAPTIVE if adaptive_p2 else P2_CONSTANT,
                           WINNER_SUBPLANE if subplane else WINNER_PLANE,
                           d_views if min_views is None else int(min_views),
                           d_k if best_k is None else int(best_k), int(support_cost),
                           d_support if min_support is None else int(min_support))
    main_img = np.ascontiguousarray(main_img, dtype=np.uint8)
    keep = []
    full = [dict(M_bwd=np.zeros(9), t_bwd=np.zeros(3), range_main=depth_range,
                 range_neighbor=depth_range, **{k: nb[k] for k in ("image", "M_fwd", "t_fwd")})
            for nb in neighbors]
    if photo is not None:
        full = _sgm_witnesses(full, witnesses)
    arr = _sgm_neighbors(full, keep) if full else None
    rng = (C.c_float * 2)(float(depth_range[0]), float(depth_range[1]))
    h, w = main_img.shape[:2]
    if photo is not None:
        # smvs_sgm_sweep_for_view_raw_photo: every output at either scale
        if halvings is not None and want_volumes:
            raise ValueError("want_volumes: the volumes are outputs of the SGM-scale entry")
        channels, nch, hv = _raw_images(main_img, keep, halvings)
        ow, oh = _halved(w, h, hv)
        filt = filt if filt is not None else SgmFilterOptions(*SGM_FILTER_DEFAULTS)
        depth = np.zeros((oh, ow), dtype=np.float32)
        support = np.zeros((oh, ow), dtype=np.uint8)
        argmin = np.zeros((oh, ow), dtype=np.int32) if halvings is None else None
        cost = np.zeros((oh, ow, num_steps), dtype=np.uint16) if want_volumes else None
        sgm = np.zeros((oh, ow, num_steps), dtype=np.uint16) if want_volumes else None
        runner = np.zeros((oh, ow), dtype=np.uint16) \
            if want_volumes and filt.uniqueness != 0 else None
        on = photo.radius != 0
        conf = np.zeros((oh, ow), dtype=np.float32) if on else None
        views = np.zeros((oh, ow), dtype=np.uint8) if on else None
        args = (device, _p(main_img, _u8p), w, h, channels, arr, nch, n, hv, rng, num_steps,
                C.c_uint16(p1), C.c_uint16(p2), C.byref(opts), C.byref(filt), _p(depth, _fp),
                _p(argmin, _i32p), _p(support, _u8p), _p(cost, _u16p), _p(sgm, _u16p),
                _p(runner, _u16p), len(full) - n, C.byref(photo), _p(conf, _fp),
                _p(views, _u8p))
        out = dict(depth=depth, support=support, confidence=conf, views=views)
        if refine is not None:
            slant = np.zeros((oh, ow, 2), dtype=np.float32) if refine.sweeps != 0 else None
            check(lib.smvs_sgm_sweep_for_view_raw_refine(*args, C.byref(refine),
                                                         _p(slant, _fp)))
            out["slant"] = slant
        else:
            check(lib.smvs_sgm_sweep_for_view_raw_photo(*args))
        if halvings is None:
            out["argmin"] = argmin
        if runner is not None:
            out["runner_up"] = runner
        if want_volumes:
            out.update(cost=cost, sgm=sgm)
        return out
    if halvings is not None:
        if want_volumes:
            raise ValueError("want_volumes: the volumes are outputs of the SGM-scale entry")
        channels = 1 if main_img.ndim == 2 else main_img.shape[2]
        nch = (C.c_int * max(n, 1))(*[1 if k.ndim == 2 else k.shape[2] for k in keep])
        ow, oh = _halved(w, h, halvings)
        depth = np.zeros((oh, ow), dtype=np.float32)
        support = np.zeros((oh, ow), dtype=np.uint8)
        if filt is not None:
            check(lib.smvs_sgm_sweep_for_view_raw_filtered(device, _p(main_img, _u8p), w, h,
                  channels, arr, nch, n, int(halvings), rng, num_steps, C.c_uint16(p1),
                  C.c_uint16(p2), C.byref(opts), C.byref(filt), _p(depth, _fp),
                  _p(support, _u8p)))
        else:
            check(lib.smvs_sgm_sweep_for_view_raw(device, _p(main_img, _u8p), w, h, channels,
                  arr, nch, n, int(halvings), rng, num_steps, C.c_uint16(p1), C.c_uint16(p2),
                  C.byref(opts), _p(depth, _fp), _p(support, _u8p)))
        return dict(depth=depth, support=support)
    if main_img.ndim != 2 or any(k.ndim != 2 for k in keep):
        raise ValueError("one-channel images at SGM scale (or pass halvings)")
    depth = np.zeros((h, w), dtype=np.float32)
    argmin = np.zeros((h, w), dtype=np.int32)
    support = np.zeros((h, w), dtype=np.uint8)
    cost = np.zeros((h, w, num_steps), dtype=np.uint16) if want_volumes else None
    sgm = np.zeros((h, w, num_steps), dtype=np.uint16) if want_volumes else None
    runner = None
    if filt is not None:
        if want_volumes and filt.uniqueness != 0:
            runner = np.zeros((h, w), dtype=np.uint16)
        check(lib.smvs_sgm_sweep_for_view_filtered(device, _p(main_img, _u8p), w, h, arr, n,
              rng, num_steps, C.c_uint16(p1), C.c_uint16(p2), C.byref(opts), C.byref(filt),
              _p(depth, _fp), _p(argmin, _i32p), _p(support, _u8p), _p(cost, _u16p),
              _p(sgm, _u16p), _p(runner, _u16p)))
    else:
        check(lib.smvs_sgm_sweep_for_view(device, _p(main_img, _u8p), w, h, arr, n, rng,
              num_steps, C.c_uint16(p1), C.c_uint16(p2), C.byref(opts), _p(depth, _fp),
              _p(argmin, _i32p), _p(support, _u8p), _p(cost, _u16p), _p(sgm, _u16p)))
    out = dict(depth=depth, argmin=argmin, support=support)
    if runner is not None:
        out["runner_up"] = runner
    if want_volumes:
        out.update(cost=cost, sgm=sgm)
    return out


def sgm_fold_costs(costs, min_views=1, best_k=0, device=0):
    """smvs_sgm_fold_costs: the fold kernel of the plane sweep alone.  costs
    (n, ...) u8, one array of cost bytes per neighbour (255: no cost); returns the
    folded bytes in the shape of one of them."""
    lib = _capi.load()
    costs = np.ascontiguousarray(costs, dtype=np.uint8)
    if costs.ndim < 2:
        raise ValueError("costs: (n, ...) with one array per neighbour")
    n = costs.shape[0]
    out = np.zeros(costs.shape[1:], dtype=np.uint8)
    check(lib.smvs_sgm_fold_costs(device, _p(costs, _u8p), n, C.c_size_t(out.size),
          int(min_views), int(best_k), _p(out, _u8p)))
    return out


class MeshView(C.Structure):
    """smvs_mesh_view of include/smvs_hip.h."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("flen", C.c_float),
                ("rot", C.c_float * 9), ("trans", C.c_float * 3),
                ("depth", _fp), ("normals", _fp)]


def cut_depth_maps(cams, depths, normals, device=0):
    """MeshGenerator::cut_depth_maps over all views on the device.  cams:
    objects with .flen, .R, .t; depths[i] (h, w) ray-length depth; normals[i]
    (h, w, 3) camera space.  Returns (cut depth maps, world-space normals)."""
    lib = _capi.load()
    n = len(cams)
    d = [_f32(x).copy() for x in depths]
    nm = [_f32(x).copy() for x in normals]
    arr = (MeshView * n)()
    for i in range(n):
        arr[i].height, arr[i].width = d[i].shape
        arr[i].flen = float(cams[i].flen)
        for k, x in enumerate(np.asarray(cams[i].R, dtype=np.float32).reshape(9)):
            arr[i].rot[k] = float(x)
        for k, x in enumerate(np.asarray(cams[i].t, dtype=np.float32).reshape(3)):
            arr[i].trans[k] = float(x)
        arr[i].depth = _p(d[i], _fp)
        arr[i].normals = _p(nm[i], _fp)
    check(lib.smvs_cut_depth_maps(device, arr, n))
    return d, nm


class PointView(C.Structure):
    """smvs_point_view of include/smvs_hip.h."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("flen", C.c_float),
                ("rot", C.c_float * 9), ("trans", C.c_float * 3),
                ("depth", _fp), ("normals", _fp), ("image", _u8p),
                ("channels", C.c_int), ("cut_depth", _fp)]


class PointsOptions(C.Structure):
    """smvs_points_options of include/smvs_hip.h."""
    _fields_ = [("cut_surfaces", C.c_int), ("use_aabb", C.c_int),
                ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3),
                ("dd_factor", C.c_float), ("want_faces", C.c_int)]


def _point_views(cams, depths, normals, images, cut_maps):
    """smvs_point_view records of the views (and the arrays they point to,
    which have to outlive the call)."""
    n = len(cams)
    if not (len(depths) == len(normals) == len(images) == n):
        raise ValueError("cams, depths, normals and images differ in length")
    d = [_f32(x) for x in depths]
    nm = [_f32(x) for x in normals]
    im = [np.ascontiguousarray(x, dtype=np.uint8) for x in images]
    cuts = [np.zeros_like(x) for x in d] if cut_maps else None
    arr = (PointView * max(n, 1))()
    for i in range(n):
        h, w = d[i].shape
        if nm[i].shape != (h, w, 3) or im[i].shape[:2] != (h, w):
            raise ValueError("view %d: normals / image do not match the depth map" % i)
        arr[i].height, arr[i].width = h, w
        arr[i].flen = float(cams[i].flen)
        for k, x in enumerate(np.asarray(cams[i].R, dtype=np.float32).reshape(9)):
            arr[i].rot[k] = float(x)
        for k, x in enumerate(np.asarray(cams[i].t, dtype=np.float32).reshape(3)):
            arr[i].trans[k] = float(x)
        arr[i].depth = _p(d[i], _fp)
        arr[i].normals = _p(nm[i], _fp)
        arr[i].image = _p(im[i], _u8p)
        arr[i].channels = 1 if im[i].ndim == 2 else im[i].shape[2]
        arr[i].cut_depth = _p(cuts[i], _fp) if cut_maps else None
    return arr, cuts, (d, nm, im)


def generate_points(cams, depths, normals, images, cut=True, aabb=None, faces=False,
                    dd_factor=5.0, cut_maps=False, device=0):
    """MeshGenerator::generate_mesh's point cloud over all views on the device
    (smvs_points_generate).  cams: objects with .flen, .R, .t; depths[i] (h, w)
    ray-length depth; normals[i] (h, w, 3) camera space; images[i] (h, w) or
    (h, w, c) uint8 at the depth map's size.  aabb: None or (min3, max3).
    Returns a dict of numpy arrays: xyz, normals (n, 3) float32, rgb (n, 3)
    uint8, confidence, value (n,) float32, faces (m, 3) uint32 when asked
    for, cut_depth (the triangulated maps) when cut_maps."""
    lib = _capi.load()
    n = len(cams)
    arr, cuts, _keep = _point_views(cams, depths, normals, images, cut_maps)
    opt = PointsOptions()
    opt.cut_surfaces = int(bool(cut))
    opt.use_aabb = int(aabb is not None)
    if aabb is not None:
        for k in range(3):
            opt.aabb_min[k] = float(aabb[0][k])
            opt.aabb_max[k] = float(aabb[1][k])
    opt.dd_factor = float(dd_factor)
    opt.want_faces = int(bool(faces))
    handle = C.c_void_p()
    n_points = C.c_int64()
    check(lib.smvs_points_generate(device, arr if n else None, n, C.byref(opt),
                                   C.byref(handle), C.byref(n_points)))
    try:
        n_faces = C.c_int64()
        check(lib.smvs_points_info(handle, None, C.byref(n_faces)))
        k = n_points.value
        out = {"xyz": np.zeros((k, 3), np.float32), "normals": np.zeros((k, 3), np.float32),
               "rgb": np.zeros((k, 3), np.uint8), "confidence": np.zeros(k, np.float32),
               "value": np.zeros(k, np.float32)}
        fc = np.zeros((n_faces.value, 3), np.uint32) if faces else None
        check(lib.smvs_points_download(handle, _p(out["xyz"], _fp), _p(out["normals"], _fp),
                                       _p(out["rgb"], _u8p), _p(out["confidence"], _fp),
                                       _p(out["value"], _fp), _p(fc, _u32p)))
    finally:
        lib.smvs_points_release(handle)
    if faces:
        out["faces"] = fc
    if cut_maps:
        out["cut_depth"] = cuts
    return out


def _download_mesh(lib, handle, n_vertices, n_faces, cells=False):
    """The mesh behind `handle` as the dict generate_mesh returns (cells: with
    smvs_tsdf_vertex_cells' per-vertex cells); the handle is released."""
    try:
        k = n_vertices
        out = {"xyz": np.zeros((k, 3), np.float32), "normals": np.zeros((k, 3), np.float32),
               "rgb": np.zeros((k, 3), np.uint8), "confidence": np.zeros(k, np.float32),
               "faces": np.zeros((n_faces, 3), np.uint32)}
        check(lib.smvs_points_download(handle, _p(out["xyz"], _fp), _p(out["normals"], _fp),
                                       _p(out["rgb"], _u8p), _p(out["confidence"], _fp),
                                       None, _p(out["faces"], _u32p)))
        if cells:
            out["cells"] = np.zeros(k, np.int64)
            check(lib.smvs_tsdf_vertex_cells(handle, _p(out["cells"], C.POINTER(C.c_int64))))
    finally:
        lib.smvs_points_release(handle)
    return out


class MeshOptions(C.Structure):
    """smvs_mesh_options of include/smvs_hip.h."""
    _fields_ = [("cut_surfaces", C.c_int), ("use_aabb", C.c_int),
                ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3),
                ("dd_factor", C.c_float)]


def generate_mesh(cams, depths, normals, images, cut=True, aabb=None, dd_factor=5.0,
                  cut_maps=False, device=0):
    """smvsrecon --mesh's triangle mesh over all views on the device
    (smvs_mesh_generate): merged in view-list order, clipped to aabb (None or
    (min3, max3)) with delete_vertices_fix_faces, vertex normals of
    recalc_normals.  Inputs as generate_points.
    Returns a dict of numpy arrays: xyz, normals (n, 3) float32, rgb (n, 3)
    uint8, confidence (n,) float32, faces (m, 3) uint32, and cut_depth (the
    triangulated maps) when cut_maps."""
    lib = _capi.load()
    n = len(cams)
    arr, cuts, _keep = _point_views(cams, depths, normals, images, cut_maps)
    opt = MeshOptions()
    opt.cut_surfaces = int(bool(cut))
    opt.use_aabb = int(aabb is not None)
    if aabb is not None:
        for k in range(3):
            opt.aabb_min[k] = float(aabb[0][k])
            opt.aabb_max[k] = float(aabb[1][k])
    opt.dd_factor = float(dd_factor)
    handle = C.c_void_p()
    n_vertices, n_faces = C.c_int64(), C.c_int64()
    check(lib.smvs_mesh_generate(device, arr if n else None, n, C.byref(opt),
                                 C.byref(handle), C.byref(n_vertices), C.byref(n_faces)))
    out = _download_mesh(lib, handle, n_vertices.value, n_faces.value)
    if cut_maps:
        out["cut_depth"] = cuts
    return out


def _tsdf_views(cams, depths, normals, images):
    """smvs_point_view records for the fusion: normals may be None (no cut),
    images may be None (the bounds)"""
    n = len(cams)
    if normals is None:
        normals = [np.zeros(np.shape(d) + (3,), np.float32) for d in depths]
        no_normals = True
    else:
        no_normals = False
    if images is None:
        images = [np.zeros(np.shape(d), np.uint8) for d in depths]
    arr, _, keep = _point_views(cams, depths, normals, images, False)
    if no_normals:
        for i in range(n):
            arr[i].normals = None
    return arr, keep


def _fill_grid(opt, origin, voxel_size, dims, trunc):
    """the grid members every options record of the fusion has"""
    for k in range(3):
        opt.origin[k] = float(origin[k])
        opt.dims[k] = int(dims[k])
    opt.voxel_size = float(voxel_size)
    opt.trunc = float(trunc)
    return opt


def _tsdf_options(origin, voxel_size, dims, trunc, cut, min_weight=0):
    opt = _fill_grid(_capi.TsdfOptions(), origin, voxel_size, dims, trunc)
    opt.cut_surfaces = int(bool(cut))
    opt.min_weight = int(min_weight)
    return opt


def _brick_shape(dims):
    """(bz, by, bx): the 8 x 8 x 4 bricks of a grid of dims = (nx, ny, nz)"""
    nx, ny, nz = (max(int(d), 0) for d in dims[:3])
    return (-(-nz // 4), -(-ny // 8), -(-nx // 8))


def tsdf_bounds(cams, depths, normals, cut=True, device=0):
    """smvs_tsdf_bounds: the box of the world points of the valid pixels of the
    (cut) depth maps.  Inputs as generate_mesh; normals may be None when cut is
    off.  Returns (lo, hi), float32 (3,) each; lo > hi when no pixel is valid."""
    lib = _capi.load()
    n = len(cams)
    arr, _keep = _tsdf_views(cams, depths, normals, None)
    lo, hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
    check(lib.smvs_tsdf_bounds(device, arr if n else None, n, int(bool(cut)), _p(lo, _fp),
                               _p(hi, _fp)))
    return lo, hi


def fuse_tsdf(cams, depths, normals, images, origin, voxel_size, dims, trunc=0, min_weight=0,
              cut=True, volume=False, device=0, sparse=False, max_bricks=0, brick_state=False,
              cull=None, brick_candidate=False):
    """smvs_tsdf_fuse: the depth maps fused into one surface mesh through a
    truncated signed distance field on the voxel grid (origin, voxel_size,
    dims = (nx, ny, nz)); the definition is in include/smvs_hip.h.  Inputs as
    generate_mesh; normals may be None when cut is off.  trunc <= 0: 3 voxels;
    min_weight <= 0: 1.  Returns the dict generate_mesh returns (xyz, normals,
    rgb, confidence, faces) and, with volume, tsdf (nz, ny, nx) float32 with NaN
    for unknown and weight (nz, ny, nx) uint32.

    sparse: smvs_tsdf_fuse_sparse, the same mesh in the brick order from a
    volume allocated in 8 x 8 x 4 bricks near the surface (dims up to 4096;
    max_bricks <= 0: 1 << 20).  The dict gains cells (int64, per vertex the
    cell's linear index in the grid), stats (bricks, seed_bricks,
    allocated_bricks, state_bytes) and, with brick_state, brick_state
    (bz, by, bx) uint8: 0 none, 1 allocated, 2 seed.  An SmvsError of status -4
    (more than max_bricks needed) carries the stats as its `stats`.

    cull (with sparse; None: the entry above, the dict as above):
    smvs_tsdf_fuse_sparse_opts.  True puts the brick cull against the views'
    depth min/max pyramids in front of the seed pass:
    every array is the same to the bit, only stats' tested_bricks, the bricks
    the exact seed test ran on, falls below bricks.  With brick_candidate the
    dict gains brick_candidate (bz, by, bx) uint8, 1 where it ran.  An SmvsError
    of status -4 then carries `brick_candidate` as well."""
    if sparse:
        if brick_candidate and cull is None:
            raise ValueError("brick_candidate belongs to cull=True or cull=False")
        return _fuse_tsdf_sparse(cams, depths, normals, images, origin, voxel_size, dims, trunc,
                                 min_weight, cut, volume, device, max_bricks, brick_state, cull,
                                 brick_candidate)
    if max_bricks or brick_state or cull or brick_candidate:
        raise ValueError("max_bricks, brick_state, cull and brick_candidate belong to "
                         "sparse=True")
    lib = _capi.load()
    n = len(cams)
    arr, _keep = _tsdf_views(cams, depths, normals, images)
    opt = _tsdf_options(origin, voxel_size, dims, trunc, cut, min_weight)
    tsdf = weight = None
    if volume:
        shape = tuple(max(int(d), 0) for d in dims)[::-1]
        tsdf = np.zeros(shape, np.float32)
        weight = np.zeros(shape, np.uint32)
    handle = C.c_void_p()
    n_vertices, n_faces = C.c_int64(), C.c_int64()
    check(lib.smvs_tsdf_fuse(device, arr if n else None, n, C.byref(opt), _p(tsdf, _fp),
                             _p(weight, _u32p), C.byref(handle), C.byref(n_vertices),
                             C.byref(n_faces)))
    out = _download_mesh(lib, handle, n_vertices.value, n_faces.value)
    if volume:
        out["tsdf"] = tsdf
        out["weight"] = weight
    return out


def _fuse_tsdf_sparse(cams, depths, normals, images, origin, voxel_size, dims, trunc, min_weight,
                      cut, volume, device, max_bricks, brick_state, cull=None,
                      brick_candidate=False):
    """fuse_tsdf(sparse=True)"""
    lib = _capi.load()
    n = len(cams)
    arr, _keep = _tsdf_views(cams, depths, normals, images)
    opt = _tsdf_options(origin, voxel_size, dims, trunc, cut, min_weight)
    shape = tuple(max(int(d), 0) for d in dims)[::-1]
    bricks = _brick_shape(dims)
    tsdf = weight = state = candidate = None
    if volume:
        tsdf = np.zeros(shape, np.float32)
        weight = np.zeros(shape, np.uint32)
    if brick_state:
        state = np.zeros(bricks, np.uint8)
    if brick_candidate:
        candidate = np.zeros(bricks, np.uint8)
    handle = C.c_void_p()
    n_vertices, n_faces = C.c_int64(), C.c_int64()
    if cull is None:
        sopt = _capi.TsdfSparseOptions()
        sopt.max_bricks = int(max_bricks)
        stats = _capi.TsdfSparseStats()
        rc = lib.smvs_tsdf_fuse_sparse(device, arr if n else None, n, C.byref(opt),
                                       C.byref(sopt), _p(state, _u8p), _p(tsdf, _fp),
                                       _p(weight, _u32p), C.byref(stats), C.byref(handle),
                                       C.byref(n_vertices), C.byref(n_faces))
    else:
        sopt = _capi.TsdfSparseOpts()
        sopt.max_bricks = int(max_bricks)
        sopt.cull = int(bool(cull))
        stats = _capi.TsdfSparseOptsStats()
        rc = lib.smvs_tsdf_fuse_sparse_opts(device, arr if n else None, n, C.byref(opt),
                                            C.byref(sopt), _p(state, _u8p),
                                            _p(candidate, _u8p), _p(tsdf, _fp),
                                            _p(weight, _u32p), C.byref(stats), C.byref(handle),
                                            C.byref(n_vertices), C.byref(n_faces))
    if rc != 0:
        err = _capi.SmvsError(rc, lib.smvs_last_error().decode())
        if rc == -4:
            err.stats = stats.as_dict()
            if brick_candidate:
                err.brick_candidate = candidate
        raise err
    out = _download_mesh(lib, handle, n_vertices.value, n_faces.value, cells=True)
    out["stats"] = stats.as_dict()
    if volume:
        out["tsdf"] = tsdf
        out["weight"] = weight
    if brick_state:
        out["brick_state"] = state
    if brick_candidate:
        out["brick_candidate"] = candidate
    return out


class _VolumeHandle:
    """What TsdfVolume and SparseTsdfVolume share: the handle of a persistent
    volume (set by the class's __init__, released through the entry `_release`
    names) as a context manager."""
    _release = None
    _handle = None

    def _open(self):
        if self._handle is None:
            raise ValueError("%s: the volume is closed" % type(self).__name__)
        return self._handle

    def close(self):
        if self._handle is not None:
            getattr(self._lib, self._release)(self._handle)
            self._handle = None

    def __enter__(self):
        self._open()
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        self.close()


class TsdfVolume(_VolumeHandle):
    """smvs_tsdf_volume: the sums of fuse_tsdf's field kept on the device, so
    that the views are fused batch by batch (the
    definition is in include/smvs_hip.h).  The grid is fuse_tsdf's (origin,
    voxel_size, dims = (nx, ny, nz), trunc <= 0: 3 voxels).  With the cut off,
    every split of a view list into consecutive integrate() calls gives
    fuse_tsdf's arrays to the bit; the cut, when on, acts within a batch.  A
    context manager; after close() every method raises ValueError."""

    _release = "smvs_tsdf_volume_release"

    def __init__(self, origin, voxel_size, dims, trunc=0, device=0):
        self._handle = None
        self._lib = _capi.load()
        opt = _fill_grid(_capi.TsdfVolumeOptions(), origin, voxel_size, dims, trunc)
        handle = C.c_void_p()
        check(self._lib.smvs_tsdf_volume_create(int(device), C.byref(opt), C.byref(handle)))
        self._handle = handle
        self._shape = tuple(int(d) for d in dims)[::-1]

    def integrate(self, cams, depths, normals, images, cut=True):
        """smvs_tsdf_volume_integrate: one batch, inputs as fuse_tsdf's (normals
        may be None when cut is off)."""
        handle = self._open()
        n = len(cams)
        arr, _keep = _tsdf_views(cams, depths, normals, images)
        check(self._lib.smvs_tsdf_volume_integrate(handle, arr if n else None, n,
                                                   int(bool(cut))))

    def extract(self, min_weight=0, volume=False):
        """smvs_tsdf_volume_extract: the dict fuse_tsdf returns; changes no
        state."""
        handle = self._open()
        lib = self._lib
        tsdf = weight = None
        if volume:
            tsdf = np.zeros(self._shape, np.float32)
            weight = np.zeros(self._shape, np.uint32)
        mesh = C.c_void_p()
        n_vertices, n_faces = C.c_int64(), C.c_int64()
        check(lib.smvs_tsdf_volume_extract(handle, int(min_weight), _p(tsdf, _fp),
                                           _p(weight, _u32p), C.byref(mesh),
                                           C.byref(n_vertices), C.byref(n_faces)))
        out = _download_mesh(lib, mesh, n_vertices.value, n_faces.value)
        if volume:
            out["tsdf"] = tsdf
            out["weight"] = weight
        return out

    @property
    def n_views(self):
        handle = self._open()
        n = C.c_int64()
        check(self._lib.smvs_tsdf_volume_info(handle, None, C.byref(n), None))
        return n.value

    def state(self):
        """smvs_tsdf_volume_download: (S (nz, ny, nx) float32, W uint32, rgbc
        (nz, ny, nx, 4) uint32: the sums R, G, B, C)."""
        handle = self._open()
        S = np.zeros(self._shape, np.float32)
        W = np.zeros(self._shape, np.uint32)
        rgbc = np.zeros(self._shape + (4,), np.uint32)
        check(self._lib.smvs_tsdf_volume_download(handle, _p(S, _fp), _p(W, _u32p),
                                                  _p(rgbc, _u32p)))
        return S, W, rgbc

    def load_state(self, S, W, rgbc, n_views):
        """smvs_tsdf_volume_upload: what state() and n_views gave."""
        handle = self._open()
        S = np.ascontiguousarray(S, np.float32)
        W = np.ascontiguousarray(W, np.uint32)
        rgbc = np.ascontiguousarray(rgbc, np.uint32)
        if S.shape != self._shape or W.shape != self._shape or rgbc.shape != self._shape + (4,):
            raise ValueError("TsdfVolume.load_state: the arrays do not have the volume's shape")
        check(self._lib.smvs_tsdf_volume_upload(handle, _p(S, _fp), _p(W, _u32p),
                                                _p(rgbc, _u32p), C.c_int64(int(n_views))))

    def reset(self):
        handle = self._open()
        check(self._lib.smvs_tsdf_volume_reset(handle))


class SparseTsdfVolume(_VolumeHandle):
    """smvs_tsdf_sparse_volume: the sums of fuse_tsdf(sparse=True) kept on the
    device in 8 x 8 x 4 bricks, so that a grid of up to 4096 voxels per side is
    fused batch by batch (the definition is in
    include/smvs_hip.h).  mark() every batch first, then integrate() every batch
    with grow=False: with the cut off that is fuse_tsdf(sparse=True) over all
    views, to the bit.  integrate(grow=True) marks its own batch first; bricks
    that get their storage after the first integrate have missed the earlier
    views and are counted in stats()["late_bricks"].  max_bricks <= 0: 1 << 20;
    an SmvsError of status -4 names the bricks needed and changes nothing.  A
    context manager; after close() every method raises ValueError."""

    _release = "smvs_tsdf_sparse_volume_release"

    def __init__(self, origin, voxel_size, dims, trunc=0, max_bricks=0, device=0):
        self._handle = None
        self._lib = _capi.load()
        opt = _fill_grid(_capi.TsdfSparseVolumeOptions(), origin, voxel_size, dims, trunc)
        opt.max_bricks = int(max_bricks)
        handle = C.c_void_p()
        check(self._lib.smvs_tsdf_sparse_volume_create(int(device), C.byref(opt),
                                                       C.byref(handle)))
        self._handle = handle
        self._shape = tuple(int(d) for d in dims)[::-1]
        self._bricks = _brick_shape(dims)

    def mark(self, cams, depths, normals, cut=True, cull=False):
        """smvs_tsdf_sparse_volume_mark: the batch's seed bricks join the
        stored ones; no image is needed (normals may be None when cut is off)."""
        handle = self._open()
        n = len(cams)
        arr, _keep = _tsdf_views(cams, depths, normals, None)
        check(self._lib.smvs_tsdf_sparse_volume_mark(handle, arr if n else None, n,
                                                     int(bool(cut)), int(bool(cull))))

    def integrate(self, cams, depths, normals, images, cut=True, grow=True, cull=False):
        """smvs_tsdf_sparse_volume_integrate: one batch, inputs as fuse_tsdf's;
        grow marks the batch first (cull: with the brick cull in front)."""
        handle = self._open()
        n = len(cams)
        arr, _keep = _tsdf_views(cams, depths, normals, images)
        check(self._lib.smvs_tsdf_sparse_volume_integrate(handle, arr if n else None, n,
                                                          int(bool(cut)), int(bool(grow)),
                                                          int(bool(cull))))

    def extract(self, min_weight=0, volume=False, brick_state=False):
        """smvs_tsdf_sparse_volume_extract: the dict fuse_tsdf(sparse=True)
        returns (stats: this volume's, see stats()); changes no state."""
        handle = self._open()
        lib = self._lib
        tsdf = weight = state = None
        if volume:
            tsdf = np.zeros(self._shape, np.float32)
            weight = np.zeros(self._shape, np.uint32)
        if brick_state:
            state = np.zeros(self._bricks, np.uint8)
        mesh = C.c_void_p()
        n_vertices, n_faces = C.c_int64(), C.c_int64()
        check(lib.smvs_tsdf_sparse_volume_extract(handle, int(min_weight), _p(state, _u8p),
                                                  _p(tsdf, _fp), _p(weight, _u32p),
                                                  C.byref(mesh), C.byref(n_vertices),
                                                  C.byref(n_faces)))
        out = _download_mesh(lib, mesh, n_vertices.value, n_faces.value, cells=True)
        out["stats"] = self.stats()
        if volume:
            out["tsdf"] = tsdf
            out["weight"] = weight
        if brick_state:
            out["brick_state"] = state
        return out

    def stats(self):
        """smvs_tsdf_sparse_volume_info: bricks, seed_bricks, allocated_bricks
        (with storage), pending_bricks (marked, storage at the next integrate),
        late_bricks, state_bytes, n_views."""
        handle = self._open()
        st = _capi.TsdfSparseVolumeStats()
        check(self._lib.smvs_tsdf_sparse_volume_info(handle, None, C.byref(st), None))
        return st.as_dict()

    @property
    def n_views(self):
        return self.stats()["n_views"]

    def state(self):
        """smvs_tsdf_sparse_volume_download, the checkpoint as a dict:
        brick_state (bz, by, bx) uint8, list and birth (n,) uint32, S (n, 256)
        float32, W (n, 256) uint32, rgbc (n, 256, 4) uint32 (the sums R, G, B,
        C) and n_views; n the bricks with storage, in linear brick order."""
        handle = self._open()
        st = self.stats()
        n = st["allocated_bricks"]
        out = {"brick_state": np.zeros(self._bricks, np.uint8),
               "list": np.zeros(n, np.uint32), "birth": np.zeros(n, np.uint32),
               "S": np.zeros((n, 256), np.float32), "W": np.zeros((n, 256), np.uint32),
               "rgbc": np.zeros((n, 256, 4), np.uint32)}
        check(self._lib.smvs_tsdf_sparse_volume_download(
            handle, _p(out["brick_state"], _u8p), _p(out["list"], _u32p),
            _p(out["birth"], _u32p), _p(out["S"], _fp), _p(out["W"], _u32p),
            _p(out["rgbc"], _u32p)))
        out["n_views"] = st["n_views"]
        return out

    def load_state(self, brick_state, list, birth, S, W, rgbc, n_views):
        """smvs_tsdf_sparse_volume_upload: load_state(**state())."""
        handle = self._open()
        brick_state = np.ascontiguousarray(brick_state, np.uint8)
        slots = np.ascontiguousarray(list, np.uint32)
        birth = np.ascontiguousarray(birth, np.uint32)
        S = np.ascontiguousarray(S, np.float32)
        W = np.ascontiguousarray(W, np.uint32)
        rgbc = np.ascontiguousarray(rgbc, np.uint32)
        n = len(slots)
        if brick_state.shape != self._bricks or slots.shape != (n,) or birth.shape != (n,) \
                or S.shape != (n, 256) or W.shape != (n, 256) or rgbc.shape != (n, 256, 4):
            raise ValueError("SparseTsdfVolume.load_state: the arrays do not have the volume's "
                             "shape")
        check(self._lib.smvs_tsdf_sparse_volume_upload(
            handle, _p(brick_state, _u8p), _p(slots, _u32p), _p(birth, _u32p), C.c_int64(n),
            _p(S, _fp), _p(W, _u32p), _p(rgbc, _u32p), C.c_int64(int(n_views))))

    def reset(self):
        handle = self._open()
        check(self._lib.smvs_tsdf_sparse_volume_reset(handle))


def tsdf_brick_cull(cams, depths, normals, origin, voxel_size, dims, trunc=0, cut=True,
                    device=0):
    """smvs_tsdf_brick_cull: the preparation, the depth min/max pyramids and the
    brick cull of fuse_tsdf(sparse=True, cull=True) alone.  Inputs as
    tsdf_bounds, the grid as fuse_tsdf.  Returns brick_candidate (bz, by, bx)
    uint8: 1 where a view may put a voxel of the brick within its truncation
    band (every seed brick is one), 0 where provably none does."""
    lib = _capi.load()
    n = len(cams)
    arr, _keep = _tsdf_views(cams, depths, normals, None)
    opt = _tsdf_options(origin, voxel_size, dims, trunc, cut)
    out = np.zeros(_brick_shape(dims), np.uint8)
    check(lib.smvs_tsdf_brick_cull(device, arr if n else None, n, C.byref(opt), _p(out, _u8p),
                                   None))
    return out


def pyramid_bytes(w, h):
    """the device bytes of one w x h view's pyramid: 8 per texel of the levels >= 1"""
    texels = 0
    while w > 1 or h > 1:
        w, h = (w + 1) // 2, (h + 1) // 2
        texels += w * h
    return 8 * texels


def tsdf_depth_pyramid(cams, depths, normals, view, cut=True, device=0):
    """smvs_tsdf_depth_pyramid: the min/max pyramid of view `view`'s prepared
    (and cut) z-depth as the brick cull reads it.  Inputs as tsdf_bounds.
    Returns a list over the levels 1 .. (1 x 1) of (lo, hi), float32
    (h_l, w_l) each with (+inf, -inf) where no pixel is valid; level 0 is the
    map itself, and a 1 x 1 view gives an empty list."""
    n = len(cams)
    if not 0 <= int(view) < n:
        raise ValueError("tsdf_depth_pyramid: no view %r" % (view,))
    lib = _capi.load()
    arr, _keep = _tsdf_views(cams, depths, normals, None)
    count, n_levels = C.c_int64(), C.c_int()
    check(lib.smvs_tsdf_depth_pyramid(device, arr, n, int(bool(cut)), int(view), None, None,
                                      C.byref(count), C.byref(n_levels)))
    lo = np.zeros(count.value, np.float32)
    hi = np.zeros(count.value, np.float32)
    check(lib.smvs_tsdf_depth_pyramid(device, arr, n, int(bool(cut)), int(view), _p(lo, _fp),
                                      _p(hi, _fp), None, None))
    h, w = np.shape(depths[view])[:2]
    levels, at = [], 0
    while w > 1 or h > 1:
        w, h = (w + 1) // 2, (h + 1) // 2
        levels.append((lo[at:at + w * h].reshape(h, w), hi[at:at + w * h].reshape(h, w)))
        at += w * h
    assert at == count.value and len(levels) == n_levels.value
    return levels


def clean_mesh(mesh, threshold=0.0, percentile=0.0, component_size=1000, keep_unreferenced=False,
               labels=False, device=0):
    """smvs_mesh_clean (what MVE's meshclean does to a fused surface; the
    definition is in include/smvs_hip.h): the vertices
    whose confidence is below the cut value are removed -- threshold, or the
    percentile-th percentile of the confidences (the reference README's
    `meshclean -p10` is percentile=10) -- then the connected components of
    fewer than component_size vertices and, unless keep_unreferenced, the
    vertices no face uses.  The defaults (no cut, components below 1000) are
    defaults of a user option, untuned.

    mesh: the dict fuse_tsdf / generate_mesh return (xyz, normals, rgb,
    confidence, faces; cells is carried when present).  Returns the same kind of
    dict, order kept and attributes bit for bit, plus stats (cut_value, n_cut,
    n_components, n_small_components, n_small_vertices, n_unreferenced,
    largest_component) and, with labels, per input vertex component (uint32,
    the smallest vertex id of its component, 0xFFFFFFFF when cut),
    component_size (uint32) and new_id (int64, -1 when removed)."""
    lib = _capi.load()
    xyz, nrm = _f32(mesh["xyz"]), _f32(mesh["normals"])
    rgb = np.ascontiguousarray(mesh["rgb"], np.uint8)
    conf = _f32(mesh["confidence"])
    faces = np.ascontiguousarray(mesh["faces"], np.uint32)
    n, m = conf.size, faces.size // 3
    if xyz.size != 3 * n or nrm.size != 3 * n or rgb.size != 3 * n or faces.size != 3 * m:
        raise ValueError("clean_mesh: attribute shapes differ")
    cells = None
    if mesh.get("cells") is not None:
        cells = np.ascontiguousarray(mesh["cells"], np.int64)
        if cells.size != n:
            raise ValueError("clean_mesh: attribute shapes differ")
    opt = _capi.MeshCleanOptions(float(threshold), float(percentile), int(component_size),
                                 int(bool(keep_unreferenced)))
    stats = _capi.MeshCleanStats()
    comp = size = new_id = None
    if labels:
        comp, size = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        new_id = np.zeros(n, np.int64)
    i64p = C.POINTER(C.c_int64)
    handle = C.c_void_p()
    n_vertices, n_faces = C.c_int64(), C.c_int64()
    check(lib.smvs_mesh_clean(device, C.c_int64(n), C.c_int64(m), _p(xyz, _fp), _p(nrm, _fp),
                              _p(rgb, _u8p), _p(conf, _fp), _p(cells, i64p), _p(faces, _u32p),
                              C.byref(opt), _p(comp, _u32p), _p(size, _u32p), _p(new_id, i64p),
                              C.byref(stats), C.byref(handle), C.byref(n_vertices),
                              C.byref(n_faces)))
    out = _download_mesh(lib, handle, n_vertices.value, n_faces.value, cells=cells is not None)
    out["stats"] = stats.as_dict()
    if labels:
        out["component"], out["component_size"], out["new_id"] = comp, size, new_id
    return out


class SimplifyOptions(C.Structure):
    """smvs_simplify_options of include/smvs_hip.h."""
    _fields_ = [("cut_surfaces", C.c_int), ("use_aabb", C.c_int),
                ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3),
                ("create_triangle_mesh", C.c_int), ("max_vertices", C.c_int),
                ("max_error", C.c_double)]


def generate_simplified(cams, depths, normals, images, mesh=False, cut=True, aabb=None,
                        max_vertices=-1, max_error=-1.0, cut_maps=False, device=0):
    """smvsrecon --simplify over all views on the device
    (smvs_simplified_generate): every view's greedy
    Delaunay triangulation, merged in view-list order.  mesh=False: the point
    cloud (xyz, normals, rgb, confidence, value, and faces unless aabb);
    mesh=True: the mesh of --mesh --simplify (recalc_normals' normals, faces,
    no value).  max_vertices / max_error: -1 = the reference's defaults.
    Inputs as generate_points; cut_depth (the triangulated maps) when cut_maps."""
    lib = _capi.load()
    n = len(cams)
    arr, cuts, _keep = _point_views(cams, depths, normals, images, cut_maps)
    opt = SimplifyOptions()
    opt.cut_surfaces = int(bool(cut))
    opt.use_aabb = int(aabb is not None)
    if aabb is not None:
        for k in range(3):
            opt.aabb_min[k] = float(aabb[0][k])
            opt.aabb_max[k] = float(aabb[1][k])
    opt.create_triangle_mesh = int(bool(mesh))
    opt.max_vertices = int(max_vertices)
    opt.max_error = float(max_error)
    handle = C.c_void_p()
    n_vertices, n_faces = C.c_int64(), C.c_int64()
    check(lib.smvs_simplified_generate(device, arr if n else None, n, C.byref(opt),
                                       C.byref(handle), C.byref(n_vertices),
                                       C.byref(n_faces)))
    try:
        k = n_vertices.value
        out = {"xyz": np.zeros((k, 3), np.float32), "normals": np.zeros((k, 3), np.float32),
               "rgb": np.zeros((k, 3), np.uint8), "confidence": np.zeros(k, np.float32)}
        if not mesh:
            out["value"] = np.zeros(k, np.float32)
        with_faces = mesh or aabb is None
        fc = np.zeros((n_faces.value, 3), np.uint32) if with_faces else None
        check(lib.smvs_points_download(handle, _p(out["xyz"], _fp), _p(out["normals"], _fp),
                                       _p(out["rgb"], _u8p), _p(out["confidence"], _fp),
                                       _p(out.get("value"), _fp), _p(fc, _u32p)))
    finally:
        lib.smvs_points_release(handle)
    if with_faces:
        out["faces"] = fc
    if cut_maps:
        out["cut_depth"] = cuts
    return out


def simplify_triangulate(depth, max_vertices=-1, max_error=-1.0, device=0, clocks=False):
    """The greedy triangulation of one depth map in pixel space, before any
    clean-up (smvs_simplify_triangulate, rows S1-S8).  Returns a dict:
    iterations, vertices (n, 3) float64 (the four corners first), triangles
    (t, 3) uint32 per triangle id, num_zero_depths (t,) int32, and with clocks=True (the stamped
    diagnostic build of the kernel) clocks (4,) uint64: 100 MHz ticks in
    selection, Delaunay lane, rescans, total."""
    lib = _capi.load()
    d = _f32(depth)
    if d.ndim != 2:
        raise ValueError("depth must be (h, w)")
    h, w = d.shape
    budget = (w * h) // 40 if max_vertices < 0 else int(max_vertices)
    cap = min(max(budget, 0), w * h) + 5
    verts = np.zeros((cap, 3), np.float64)
    tris = np.zeros((2 * cap, 3), np.uint32)
    nzero = np.zeros(2 * cap, np.int32)
    ticks = np.zeros(4, np.uint64)
    it, nv, nt = C.c_int64(), C.c_int64(), C.c_int64()
    check(lib.smvs_simplify_triangulate(device, _p(d, _fp), w, h, int(max_vertices),
                                        C.c_double(max_error), C.byref(it), C.byref(nv),
                                        _p(verts, _dp), C.byref(nt), _p(tris, _u32p),
                                        _p(nzero, _i32p),
                                        _p(ticks if clocks else None,
                                           C.POINTER(C.c_uint64))))
    return {"iterations": it.value, "vertices": verts[:nv.value],
            "triangles": tris[:nt.value], "num_zero_depths": nzero[:nt.value],
            "clocks": ticks if clocks else None}
