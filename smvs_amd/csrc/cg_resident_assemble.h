// The resident PCG's fused assembly: one node's system gathered from the packed
// per-patch records.  A fragment of cg_resident.hip's translation unit, included
// there behind ResArgs and double4_r.
#pragma once

namespace smvs_hip {

// GaussNewtonStep::construct's scatter (gauss_newton_step.cc:88-142) in gather
// form for ONE node, as gn_assemble_kernel does it with four lanes: the <= 4
// incident patches in ascending patch id, local node order 0 (ix, iy),
// 1 (ix+1, iy), 2 (ix, iy+1), 3 (ix+1, iy+1); only stored slots (other node
// >= this node), blocks towards inactive nodes omitted (Q6).
struct NodeSystem {
    double hd[10];      // diagonal block, upper triangle (Q4)
    double hu[4][16];   // slots 5..8
    double g[4];
};

// `count` consecutive quads of patch p's record from element `e0` (a multiple
// of 4) on, or -- unconditionally, so that the loads of a thread stay
// independent of its flags -- the same number of loads from the block of zeros.
struct QuadSource {
    const double4_r *base;
    unsigned step;
    __device__ __forceinline__ double4_r operator[](int i) const { return base[(size_t)i * step]; }
};
__device__ __forceinline__ QuadSource
patch_quads(ResArgs const &A, int p, int e0, bool use)
{
    const double4_r *Hq = reinterpret_cast<const double4_r *>(A.Hp);
    QuadSource q;
    q.base = use ? Hq + ((size_t)(e0 >> 2) * A.layout.hq + (size_t)p * A.layout.hp)
        : reinterpret_cast<const double4_r *>(A.zeros);
    q.step = use ? A.layout.hq : 0u;
    return q;
}
__device__ __forceinline__ double4_r
patch_gradient(ResArgs const &A, int p, int ln, bool use)
{
    const double4_r *gq = reinterpret_cast<const double4_r *>(A.gp);
    return *(use ? gq + ((size_t)ln * A.layout.gq + (size_t)p * A.layout.gp)
        : reinterpret_cast<const double4_r *>(A.zeros));
}

// The loads below are unconditional: a block that does not contribute (patch
// outside the grid / invalid, other node inactive) is read from a block of
// zeros instead, so that all flag loads, then all block loads, are
// independent and in flight together -- with a branch per block every one of
// them cost a full memory latency, ~25 in a row at 2 waves per SIMD.  Adding
// +0.0 in place of an omitted term leaves every sum bit-identical (the sums
// start at +0.0 and can never be -0.0).
__device__ __forceinline__ void
assemble_node(ResArgs const &A, int ix, int iy, bool on, NodeSystem &S)
{
#pragma unroll
    for (int i = 0; i < 10; ++i)
        S.hd[i] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int i = 0; i < 16; ++i)
            S.hu[k][i] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        S.g[i] = 0.0;
    if (!on)
        return;
    int const n = iy * A.stride + ix;
    int const rows = A.npy + 1;
    // flags of the 3 x 3 nodes around (ix, iy) and of the four incident patches
    bool act[3][3], pv[4];
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            int const jx = ix + dx, jy = iy + dy;
            bool const inside = jx >= 0 && jx < A.stride && jy >= 0 && jy < rows;
            uint8_t const f = A.active[inside ? jy * A.stride + jx : n];
            act[dy + 1][dx + 1] = inside && f != 0;
        }
    int pidx[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int const pxq = ix - (1 - (q & 1));
        int const pyq = iy - (1 - (q >> 1));
        bool const inside = pxq >= 0 && pxq < A.npx && pyq >= 0 && pyq < A.npy;
        pidx[q] = inside ? pyq * A.npx + pxq : 0;
        uint8_t const f = A.patch_valid[pidx[q]];
        pv[q] = inside && f != 0;
    }
    if (!act[1][1])
        return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int const ln = 3 - q;   // local index of the node in that patch
#pragma unroll
        for (int lm = 0; lm < 4; ++lm) {
            if (lm < ln)
                continue;
            // the other node, relative to this one
            int const dx = (lm & 1) - (ln & 1), dy = (lm >> 1) - (ln >> 1);
            bool const use = pv[q] && act[dy + 1][dx + 1];
            if (lm == ln) {
                QuadSource const tri = patch_quads(A, pidx[q], patch_diag_offset(ln), use);
                double4_r const b0 = tri[0], b1 = tri[1], b2 = tri[2];
                S.hd[0] += b0.x; S.hd[1] += b0.y; S.hd[2] += b0.z; S.hd[3] += b0.w;
                S.hd[4] += b1.x; S.hd[5] += b1.y; S.hd[6] += b1.z;
                S.hd[7] += b1.w; S.hd[8] += b2.x;
                S.hd[9] += b2.y;
            } else {
                QuadSource const blk = patch_quads(A, pidx[q], patch_upper_offset(ln, lm), use);
                double4_r const b0 = blk[0], b1 = blk[1], b2 = blk[2], b3 = blk[3];
                int const k = (dy + 1) * 3 + dx + 1 - 5;
                S.hu[k][0] += b0.x; S.hu[k][1] += b0.y; S.hu[k][2] += b0.z; S.hu[k][3] += b0.w;
                S.hu[k][4] += b1.x; S.hu[k][5] += b1.y; S.hu[k][6] += b1.z; S.hu[k][7] += b1.w;
                S.hu[k][8] += b2.x; S.hu[k][9] += b2.y; S.hu[k][10] += b2.z; S.hu[k][11] += b2.w;
                S.hu[k][12] += b3.x; S.hu[k][13] += b3.y; S.hu[k][14] += b3.z; S.hu[k][15] += b3.w;
            }
        }
        double4_r const gv = patch_gradient(A, pidx[q], ln, pv[q]);
        S.g[0] += gv.x; S.g[1] += gv.y; S.g[2] += gv.z; S.g[3] += gv.w;
    }
}

// The diagonal block (upper triangle) and the gradient of node (ix, iy) alone,
// with assemble_node's sums in assemble_node's order: what the one-exchange
// solver needs of a HALO node to form that node's z = P r itself.
__device__ __forceinline__ void
assemble_diagonal(ResArgs const &A, int ix, int iy, double (&hd)[10], double (&g)[4])
{
#pragma unroll
    for (int i = 0; i < 10; ++i)
        hd[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        g[i] = 0.0;
    int const n = iy * A.stride + ix;
    uint8_t const fself = A.active[n];
    int pidx[4];
    bool pv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int const pxq = ix - (1 - (q & 1));
        int const pyq = iy - (1 - (q >> 1));
        bool const inside = pxq >= 0 && pxq < A.npx && pyq >= 0 && pyq < A.npy;
        pidx[q] = inside ? pyq * A.npx + pxq : 0;
        uint8_t const f = A.patch_valid[pidx[q]];
        pv[q] = inside && f != 0;
    }
    if (fself == 0)
        return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int const ln = 3 - q;   // local index of the node in that patch
        QuadSource const tri = patch_quads(A, pidx[q], patch_diag_offset(ln), pv[q]);
        double4_r const b0 = tri[0], b1 = tri[1], b2 = tri[2];
        hd[0] += b0.x; hd[1] += b0.y; hd[2] += b0.z; hd[3] += b0.w;
        hd[4] += b1.x; hd[5] += b1.y; hd[6] += b1.z;
        hd[7] += b1.w; hd[8] += b2.x;
        hd[9] += b2.y;
        double4_r const gv = patch_gradient(A, pidx[q], ln, pv[q]);
        g[0] += gv.x; g[1] += gv.y; g[2] += gv.z; g[3] += gv.w;
    }
}

// The four upper blocks (slots 5..8) of node (ix, iy) alone, with
// assemble_node's sums in assemble_node's order.
__device__ __forceinline__ void
assemble_upper(ResArgs const &A, int ix, int iy, bool on, double (&hu)[4][16])
{
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int i = 0; i < 16; ++i)
            hu[k][i] = 0.0;
    if (!on)
        return;
    int const n = iy * A.stride + ix;
    int const rows = A.npy + 1;
    bool act[2][3], pv[4];   // nodes (dx, dy) with dy in {0, 1}: the upper slots' ends
#pragma unroll
    for (int dy = 0; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            int const jx = ix + dx, jy = iy + dy;
            bool const inside = jx >= 0 && jx < A.stride && jy >= 0 && jy < rows;
            uint8_t const f = A.active[inside ? jy * A.stride + jx : n];
            act[dy][dx + 1] = inside && f != 0;
        }
    int pidx[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int const pxq = ix - (1 - (q & 1));
        int const pyq = iy - (1 - (q >> 1));
        bool const inside = pxq >= 0 && pxq < A.npx && pyq >= 0 && pyq < A.npy;
        pidx[q] = inside ? pyq * A.npx + pxq : 0;
        uint8_t const f = A.patch_valid[pidx[q]];
        pv[q] = inside && f != 0;
    }
    if (!act[0][1])
        return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int const ln = 3 - q;   // local index of the node in that patch
#pragma unroll
        for (int lm = 0; lm < 4; ++lm) {
            if (lm <= ln)
                continue;
            int const dx = (lm & 1) - (ln & 1), dy = (lm >> 1) - (ln >> 1);
            bool const use = pv[q] && act[dy][dx + 1];
            QuadSource const blk = patch_quads(A, pidx[q], patch_upper_offset(ln, lm), use);
            double4_r const b0 = blk[0], b1 = blk[1], b2 = blk[2], b3 = blk[3];
            int const k = (dy + 1) * 3 + dx + 1 - 5;
            hu[k][0] += b0.x; hu[k][1] += b0.y; hu[k][2] += b0.z; hu[k][3] += b0.w;
            hu[k][4] += b1.x; hu[k][5] += b1.y; hu[k][6] += b1.z; hu[k][7] += b1.w;
            hu[k][8] += b2.x; hu[k][9] += b2.y; hu[k][10] += b2.z; hu[k][11] += b2.w;
            hu[k][12] += b3.x; hu[k][13] += b3.y; hu[k][14] += b3.z; hu[k][15] += b3.w;
        }
    }
}

// One stored block of another node: row node (mx, my), its upper slot 5..8
// (a compile-time constant at every call: the loops fold to the <= 2 patches
// that hold both nodes).
__device__ __forceinline__ void
assemble_block(ResArgs const &A, int mx, int my, int slot, double *out16)
{
#pragma unroll
    for (int i = 0; i < 16; ++i)
        out16[i] = 0.0;
    int const mrow = my * A.stride + mx;
    bool const act_row = A.active[mrow] != 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int const ln = 3 - q;
#pragma unroll
        for (int lm = 0; lm < 4; ++lm) {
            if (lm <= ln)
                continue;
            int const dx = (lm & 1) - (ln & 1), dy = (lm >> 1) - (ln >> 1);
            if ((dy + 1) * 3 + dx + 1 != slot)
                continue;
            int const pxq = mx - (1 - (q & 1));
            int const pyq = my - (1 - (q >> 1));
            bool const inside = pxq >= 0 && pxq < A.npx && pyq >= 0 && pyq < A.npy;
            int const p = inside ? pyq * A.npx + pxq : 0;
            int const m = inside
                ? pyq * A.stride + pxq + (lm & 1) + (lm >> 1) * A.stride : mrow;
            uint8_t const fp = A.patch_valid[p];
            uint8_t const fm = A.active[m];
            bool const use = act_row && inside && fp != 0 && fm != 0;
            QuadSource const blk = patch_quads(A, p, patch_upper_offset(ln, lm), use);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                double4_r const v = blk[i];
                out16[4 * i + 0] += v.x; out16[4 * i + 1] += v.y;
                out16[4 * i + 2] += v.z; out16[4 * i + 3] += v.w;
            }
        }
    }
}

// A rim block for the tile's LDS: the stored block of row node (mx, my)
// towards its neighbour of LOWER slot s seen from the tile node (i.e. the row
// node's upper slot 8 - s), s chosen at run time so that one thread per rim
// block can do the work.  The <= 2 patches holding both nodes, in ascending
// patch id as in assemble_block:
//   s = 0 (slot 8): q 3 (ln 0, lm 3)
//   s = 1 (slot 7): q 2 (ln 1, lm 3), q 3 (ln 0, lm 2)
//   s = 2 (slot 6): q 2 (ln 1, lm 2)
//   s = 3 (slot 5): q 1 (ln 2, lm 3), q 3 (ln 0, lm 1)
// Flags in one batch, the two blocks in one batch (a missing contribution is
// read from the block of zeros).
__device__ __forceinline__ void
assemble_rim_block(ResArgs const &A, int mx, int my, int s, double *dst16)
{
    int const q[2] = { s == 0 ? 3 : (s == 3 ? 1 : 2), 3 };
    int const ln[2] = { s == 0 ? 0 : (s == 3 ? 2 : 1), 0 };
    int const lm[2] = { s == 2 ? 2 : 3, s == 1 ? 2 : 1 };
    bool const two = s == 1 || s == 3;
    int const mrow = my * A.stride + mx;
    uint8_t const frow = A.active[mrow];
    QuadSource src[2];
    uint8_t fp[2], fm[2];
    bool inside[2];
    int p[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        int const pxq = mx - (1 - (q[e] & 1));
        int const pyq = my - (1 - (q[e] >> 1));
        inside[e] = (e == 0 || two) && pxq >= 0 && pxq < A.npx && pyq >= 0
            && pyq < A.npy;
        p[e] = inside[e] ? pyq * A.npx + pxq : 0;
        int const m = inside[e]
            ? pyq * A.stride + pxq + (lm[e] & 1) + (lm[e] >> 1) * A.stride : mrow;
        fp[e] = A.patch_valid[p[e]];
        fm[e] = A.active[m];
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        bool const use = frow != 0 && inside[e] && fp[e] != 0 && fm[e] != 0;
        // (ln, lm depend on s at run time here: the offset is computed, not folded)
        src[e] = patch_quads(A, p[e], patch_upper_offset(ln[e], lm[e]), use);
    }
    double4_r v0[4], v1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v0[i] = src[0][i];
        v1[i] = src[1][i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        // (0 + first) + second, as assemble_block
        double4_r r;
        r.x = (0.0 + v0[i].x) + v1[i].x;
        r.y = (0.0 + v0[i].y) + v1[i].y;
        r.z = (0.0 + v0[i].z) + v1[i].z;
        r.w = (0.0 + v0[i].w) + v1[i].w;
        reinterpret_cast<double4_r *>(dst16)[i] = r;
    }
}

} // namespace smvs_hip
