"""Symmetric positive definite block systems for the PCG solvers, on any node
grid, in the layout smvs_gn_upload takes -- and a float64 CSR reference.

Layout (what orc_gn_construct writes and smvs_gn_upload reads):
  H9[n][s][16]  the 4 x 4 block of row node n and column node n + offset(s),
                s = (dy + 1) * 3 + (dx + 1), row-major in the block; slot 4 is
                the diagonal, slots 0..3 mirror the upper slots 5..8 of the
                neighbours (H9[c][8 - s] = H9[n][s]^T)
  present[n][s] which blocks exist (the oracle's block-sparse pattern)
  g[4 n + i]    the gradient; the solvers solve H x = -g
  P[n][16]      the inverted diagonal blocks (zero where a node has none)

The matrix is a sum of 8 x 8 element matrices M M^T, one per pair of
neighbouring nodes (the 9-point stencil), plus `shift` times the identity on
every node that has a block: SPD by construction, its condition set by
`shift`.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

# the four "forward" neighbour offsets (dx, dy): every pair once
_EDGES = [(1, 0), (-1, 1), (0, 1), (1, 1)]


def slot(dx, dy):
    return (dy + 1) * 3 + (dx + 1)


class System:
    def __init__(self, stride, rows, H9, present, g, P, nodes_with_block):
        self.stride, self.rows = stride, rows
        self.num_nodes = stride * rows
        self.H9, self.present, self.g, self.P = H9, present, g, P
        self.has_block = nodes_with_block
        self._csr = None

    @property
    def b(self):
        return -self.g

    def csr(self):
        if self._csr is None:
            self._csr = h9_to_csr(self.H9, self.present, self.stride)
        return self._csr

    def residual(self, x):
        """||H x + g|| in float64 (the system is H x = -g)."""
        return float(np.linalg.norm(self.csr() @ x + self.g))

    def spsolve(self):
        """x of H x = -g on the nodes that have a block (zero elsewhere)."""
        keep = np.repeat(self.has_block, 4)
        A = self.csr()[keep][:, keep].tocsc()
        x = np.zeros(4 * self.num_nodes)
        if keep.any():
            x[keep] = spla.spsolve(A, -self.g[keep])
        return x


def h9_to_csr(H9, present, stride):
    """The block stencil as a scipy CSR matrix (every present block, the lower
    slots included, exactly as orc_block_spmv multiplies)."""
    N = H9.shape[0]
    n_idx, s_idx = np.nonzero(present)
    dx = s_idx % 3 - 1
    dy = s_idx // 3 - 1
    col_node = n_idx + dy * stride + dx
    br, bc = np.divmod(np.arange(16), 4)
    rows = (4 * n_idx[:, None] + br[None, :]).ravel()
    cols = (4 * col_node[:, None] + bc[None, :]).ravel()
    vals = H9[n_idx, s_idx].ravel()
    return sp.csr_matrix((vals, (rows, cols)), shape=(4 * N, 4 * N))


def block_product(H9, present, stride, x):
    """y = H x block by block, in plain loops over the stencil (the
    definition the CSR form is checked against)."""
    N = H9.shape[0]
    rows = N // stride
    X = x.reshape(N, 4)
    y = np.zeros((N, 4))
    for s in range(9):
        dx, dy = s % 3 - 1, s // 3 - 1
        for n in range(N):
            if not present[n, s]:
                continue
            ix, iy = n % stride, n // stride
            cx, cy = ix + dx, iy + dy
            assert 0 <= cx < stride and 0 <= cy < rows
            y[n] += H9[n, s].reshape(4, 4) @ X[cy * stride + cx]
    return y.ravel()


def make_system(stride, rows, seed=0, shift=1.0, holes=(), isolated=(),
                g_mode="random", g_node=None, rank=8):
    """An SPD block system on a `stride` x `rows` node grid.

    shift     added to every diagonal block (smaller: worse conditioned)
    holes     node ids without any block (no row, no column, g = 0, P = 0)
    isolated  node ids that keep only their diagonal block
    g_mode    'random' | 'zero' | 'one' (g nonzero at node `g_node` only)
    """
    rng = np.random.default_rng(seed)
    N = stride * rows
    H9 = np.zeros((N, 9, 4, 4))
    present = np.zeros((N, 9), np.uint8)
    has_block = np.ones(N, bool)
    has_block[list(holes)] = False
    lonely = np.zeros(N, bool)
    lonely[list(isolated)] = True
    iy, ix = np.divmod(np.arange(N), stride)
    # diagonal: the shift plus a small random SPD part of its own
    Dd = rng.standard_normal((N, 4, 4)) * 0.3
    H9[:, 4] = Dd @ Dd.transpose(0, 2, 1) + shift * np.eye(4)
    for dx, dy in _EDGES:
        ok = (ix + dx >= 0) & (ix + dx < stride) & (iy + dy < rows)
        a = np.flatnonzero(ok)
        c = a + dy * stride + dx
        keep = has_block[a] & has_block[c] & ~lonely[a] & ~lonely[c]
        a, c = a[keep], c[keep]
        M = rng.standard_normal((a.size, 8, rank)) / np.sqrt(rank)
        K = M @ M.transpose(0, 2, 1)
        s = slot(dx, dy)
        np.add.at(H9, (a, 4), K[:, :4, :4])
        np.add.at(H9, (c, 4), K[:, 4:, 4:])
        H9[a, s] = K[:, :4, 4:]
        H9[c, 8 - s] = K[:, 4:, :4]
        present[a, s] = 1
        present[c, 8 - s] = 1
    present[has_block, 4] = 1
    H9[~has_block, 4] = 0.0
    H9 = H9.reshape(N, 9, 16)
    P = np.zeros((N, 16))
    P[has_block] = np.linalg.inv(H9[has_block, 4].reshape(-1, 4, 4)).reshape(-1, 16)
    if g_mode == "zero":
        g = np.zeros(4 * N)
    elif g_mode == "one":
        g = np.zeros(4 * N)
        g[4 * g_node:4 * g_node + 4] = rng.standard_normal(4)
    else:
        g = rng.standard_normal(4 * N)
    g[np.repeat(~has_block, 4)] = 0.0
    return System(stride, rows, H9, present, g, P, has_block)


def system_from_oracle(ref, stride):
    """The System of an orc_gn_construct result (its own H9, present, g, P)."""
    N = ref["H9"].shape[0]
    return System(stride, N // stride, ref["H9"], ref["present"], ref["g"], ref["P"],
                  ref["present"][:, 4] != 0)


def flat_surface(stride, rows):
    """A surface dict for ViewContext.set_surface on a stride x rows node grid
    (scale 0: one pixel per patch, image of max(stride - 1, 5) x max(rows - 1, 5)
    pixels).  Only the grid matters to a solve of an uploaded system."""
    npx, npy = stride - 1, rows - 1
    return dict(scale=0, npx=npx, npy=npy, start_x=0, start_y=0,
                width=max(npx, 5), height=max(npy, 5),
                nodes=np.zeros((stride * rows, 4)),
                node_valid=np.ones(stride * rows, np.uint8),
                patch_valid=np.ones(npx * npy, np.uint8),
                patch_vis=np.ones(npx * npy, np.uint32))


def oracle_cg(oracle, system, max_iterations, error_tolerance, q_tolerance, g=None):
    """orc_cg_solve on `system` (b = -g): (x, iterations, info)."""
    import ctypes as C
    dp = C.POINTER(C.c_double)
    g = system.g if g is None else g
    b = np.ascontiguousarray(-g, dtype=np.float64)
    x = np.zeros_like(b)
    H9 = np.ascontiguousarray(system.H9, dtype=np.float64)
    P = np.ascontiguousarray(system.P, dtype=np.float64)
    present = np.ascontiguousarray(system.present, dtype=np.uint8)
    it = C.c_int(0)
    info = oracle.lib().orc_cg_solve(system.num_nodes, system.stride,
        H9.ctypes.data_as(dp), present.ctypes.data_as(C.POINTER(C.c_uint8)),
        P.ctypes.data_as(dp), b.ctypes.data_as(dp), x.ctypes.data_as(dp),
        C.c_int(max_iterations), C.c_double(error_tolerance),
        C.c_double(q_tolerance), C.byref(it))
    return x, it.value, info
