"""numpy restatement of smvs_mesh_clean's definition (include/smvs_hip.h,
"Cleaning a triangle mesh"), step by step.  Test infrastructure: the product
never imports it.  Components come from min-label hooking plus pointer jumping
to a fixpoint; no scipy."""
import numpy as np

NO_COMPONENT = np.uint32(0xFFFFFFFF)
STATS = ("cut_value", "n_cut", "n_components", "n_small_components", "n_small_vertices",
         "n_unreferenced", "largest_component")


def float_key(conf):
    """the order-preserving key of step 1 on the floats' bits"""
    u = np.ascontiguousarray(conf, np.float32).view(np.uint32)
    return u ^ np.where(u >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def cut_value(conf, threshold, percentile):
    """step 1: t (float32); -inf is "no cut" """
    conf = np.ascontiguousarray(conf, np.float32)
    threshold, percentile = np.float32(threshold), np.float32(percentile)
    if threshold != 0 and percentile != 0:
        raise ValueError("threshold and percentile exclude each other")
    if percentile == 0:
        return threshold if threshold > 0 else np.float32(-np.inf)
    n = conf.size
    if n == 0:
        return np.float32(-np.inf)
    k = int(float(percentile) * float(n - 1) / 100.0)
    order = np.argsort(float_key(conf), kind="stable")
    return conf[order[k]]


def components(n, faces):
    """label[v] = the smallest vertex id of v's component under the links of
    `faces` (m, 3): hooking to the minimum and pointer jumping to a fixpoint"""
    label = np.arange(n, dtype=np.int64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if faces.shape[0] == 0:
        return label
    a = np.concatenate([faces[:, 0], faces[:, 1]])
    b = np.concatenate([faces[:, 1], faces[:, 2]])
    while True:
        la, lb = label[a], label[b]
        low = np.minimum(la, lb)
        new = label.copy()
        # the larger of the two labels' owners hooks to the smaller label
        np.minimum.at(new, la, low)
        np.minimum.at(new, lb, low)
        np.minimum.at(new, a, low)
        np.minimum.at(new, b, low)
        while True:   # pointer jumping
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, label):
            return label
        label = new


def clean(mesh, threshold=0.0, percentile=0.0, component_size=1000, keep_unreferenced=False):
    """The definition on a mesh dict (xyz, normals, rgb, confidence, faces,
    optionally cells) -> the result dict clean_mesh(..., labels=True) returns."""
    conf = np.ascontiguousarray(mesh["confidence"], np.float32)
    faces = np.ascontiguousarray(mesh["faces"], np.uint32).reshape(-1, 3)
    n = conf.size
    if faces.size and int(faces.max()) >= n:
        raise ValueError("a face holds a vertex id >= n")
    t = cut_value(conf, threshold, percentile)
    with np.errstate(invalid="ignore"):
        cut = conf < t                                   # 1 (a NaN compares false)
    fa, fb, fc = (faces[:, r].astype(np.int64) for r in range(3))
    survive = ~(cut[fa] | cut[fb] | cut[fc]) & (fa != fb) & (fb != fc) & (fa != fc)   # 2
    label = components(n, faces[survive])                # 3 (cut vertices stay alone)
    uncut = ~cut
    sizes = np.bincount(label[uncut], minlength=n) if n else np.zeros(0, np.int64)
    size = np.where(uncut, sizes[label] if n else 0, 0)
    small = uncut & (size < component_size) if component_size > 1 else np.zeros(n, bool)
    referenced = np.zeros(n, bool)
    referenced[faces[survive].astype(np.int64).ravel()] = True
    unref = uncut & ~referenced                          # 4
    keep = uncut & ~small
    if not keep_unreferenced:
        keep &= ~unref
    new_id = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)   # 5
    fkeep = survive & keep[fa] & keep[fb] & keep[fc]
    out = {"xyz": np.ascontiguousarray(mesh["xyz"], np.float32).reshape(-1, 3)[keep],
           "normals": np.ascontiguousarray(mesh["normals"], np.float32).reshape(-1, 3)[keep],
           "rgb": np.ascontiguousarray(mesh["rgb"], np.uint8).reshape(-1, 3)[keep],
           "confidence": conf[keep],
           "faces": new_id[faces[fkeep].astype(np.int64)].astype(np.uint32).reshape(-1, 3)}
    if mesh.get("cells") is not None:
        out["cells"] = np.ascontiguousarray(mesh["cells"], np.int64)[keep]
    roots = uncut & (label == np.arange(n))
    out["component"] = np.where(uncut, label, int(NO_COMPONENT)).astype(np.uint32)
    out["component_size"] = size.astype(np.uint32)
    out["new_id"] = new_id
    out["stats"] = {"cut_value": float(t), "n_cut": int(cut.sum()),
                    "n_components": int(roots.sum()),
                    "n_small_components": int((roots & small).sum()),
                    "n_small_vertices": int(small.sum()),
                    "n_unreferenced": int(unref.sum()),
                    "largest_component": int(size.max()) if n else 0}
    return out


ARRAYS = ("xyz", "normals", "rgb", "confidence", "faces", "component", "component_size",
          "new_id")


def assert_same(got, want, cells=False):
    """every array bit for bit, every stats field equal (cut_value by its bits)"""
    for name in ARRAYS + (("cells",) if cells else ()):
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), name
    for name in STATS[1:]:
        assert got["stats"][name] == want["stats"][name], (name, got["stats"], want["stats"])
    g, w = (np.float32(s["stats"]["cut_value"]).view(np.uint32) for s in (got, want))
    assert g == w, ("cut_value", got["stats"], want["stats"])
