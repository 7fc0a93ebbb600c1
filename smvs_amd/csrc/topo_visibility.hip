// The visibility mask of every patch: per (patch, neighbour) the image-border /
// occlusion test, the warp anisotropy test and ncc_for_patch
// (lib/depth_optimizer.cc:472-590, 792-912; topology.hip has the overview).
#include "topo_internal.h"
#include "topo_divide.h"
#include "topo_vis_plan.h"
#include "dpp.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace smvs_hip {

// ---- lane-group reductions of the visibility kernel on the VALU (round 6) ----
// __shfl_xor of a double is two ds_bpermute_b32 through the CU's one LDS pipe
// and a round trip per step; the kernel's eleven reductions of up to six steps
// each were ~5 us of every wave's life at patch size 8, more than its samples
// (wave life = 5.0 us + 1.9 us per pixel / sample slot, from the per-call times
// of a --no-sgm view).  DPP moves inside a row of 16 lanes and gfx950's
// v_permlane16_swap / v_permlane32_swap across the rows do the same butterflies
// without LDS.  Every lane of the group gets the result, bit-identical in all
// of them (each step adds / compares the same two numbers in both lanes of a
// pair).
// (the moves themselves: dpp.h)
template <int CTRL>
__device__ __forceinline__ double
vis_dpp(double v)
{
    return dpp_f64<CTRL>(v);
}

// the partner's value across rows (HALF = 16: rows 2k <-> 2k + 1) or halves of
// the wave (HALF = 32): both values of the pair, lower lane's first
template <int HALF>
__device__ __forceinline__ void
vis_swap(double v, double &lower, double &upper)
{
    permlane_swap_f64<HALF>(v, v, lower, upper);
}

// op over the min(G, 64) lanes of a group inside the wave (G a power of two)
template <typename Op>
__device__ __forceinline__ double
vis_lanes_reduce(double v, int G, Op const &op)
{
    if (G >= 2)
        v = op(v, vis_dpp<DPP_QUAD_SWAP1>(v));
    if (G >= 4)
        v = op(v, vis_dpp<DPP_QUAD_SWAP2>(v));
    if (G >= 8)
        v = op(v, vis_dpp<DPP_ROW_HALF_MIRROR>(v));
    if (G >= 16)
        v = op(v, vis_dpp<DPP_ROW_MIRROR>(v));
    if (G >= 32) {
        double a, b;
        vis_swap<16>(v, a, b);
        v = op(a, b);
    }
    if (G >= 64) {
        double a, b;
        vis_swap<32>(v, a, b);
        v = op(a, b);
    }
    return v;
}

// K sums over the group at once; G == 256: the per-wave sums of all K meet in
// LDS behind ONE pair of barriers (`red` holds K x 4 doubles; every thread of
// the workgroup must call)
template <int K>
__device__ __forceinline__ void
vis_group_sums(double (&v)[K], int G, double *red)
{
    auto const add = [](double a, double b) { return a + b; };
#pragma unroll
    for (int k = 0; k < K; ++k)
        v[k] = vis_lanes_reduce(v[k], G, add);
    if (G > 64) {
        __syncthreads();   // (the previous reduction's readers are done)
        if ((threadIdx.x & 63) == 0)
#pragma unroll
            for (int k = 0; k < K; ++k)
                red[k * 4 + (threadIdx.x >> 6)] = v[k];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; ++k)
            v[k] = ((red[k * 4] + red[k * 4 + 1]) + red[k * 4 + 2]) + red[k * 4 + 3];
    }
}

__device__ __forceinline__ double
vis_group_max(double v, int G, double *red)
{
    auto const larger = [](double a, double b) { return a < b ? b : a; };
    v = vis_lanes_reduce(v, G, larger);
    if (G > 64) {
        __syncthreads();
        if ((threadIdx.x & 63) == 0)
            red[threadIdx.x >> 6] = v;
        __syncthreads();
        for (int w = 0; w < 4; ++w)
            v = v < red[w] ? red[w] : v;
    }
    return v;
}

// ---- the surface at every pixel of every valid patch: depth w and its pixel
// derivatives wx, wy.  The visibility kernel needs them per (pixel, neighbour)
// and, for the NCC samples, per (sample, neighbour): evaluated here ONCE per
// pixel with the expressions that kernel used per neighbour (patch_eval of
// topo_math.h: the same bits), 8 x less bicubic arithmetic for 8 neighbours.
__global__ void __launch_bounds__(256)
topo_pixel_surface_kernel(TopoArgs A)
{
#pragma clang fp contract(off)
    int const pp = A.ps * A.ps;
    long long const gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int const p = (int)(gid >> (2 * A.ps_log2));
    int const k = (int)(gid & (pp - 1));
    if (p >= A.num_patches || !A.patch_valid[p])
        return;
    double n16[16];
    load_patch_nodes(A, p, n16);
    int const i = k & (A.ps - 1), j = k >> A.ps_log2;
    // (x / ps == x * (1 / ps) exactly: ps is a power of two)
    double const u = (i + 0.5) * A.inv_ps, v = (j + 0.5) * A.inv_ps;
    int const x = A.start_x + (p % A.npx) * A.ps + i;
    int const y = A.start_y + (p / A.npx) * A.ps + j;
    double *out = A.pix + ((size_t)y * A.W + x) * 3;
    out[0] = smvs_topo::patch_eval(n16, u, v, 0, 0);
    out[1] = smvs_topo::patch_eval(n16, u, v, 1, 0) * A.inv_ps;
    out[2] = smvs_topo::patch_eval(n16, u, v, 0, 1) * A.inv_ps;
}

// ---- visibility of every patch in every neighbour (:472-590), incl.
// ncc_for_patch (:792-912) ----
// (153 VGPRs: three waves per SIMD -- round 5: 159, round 4: 192 and two waves.
// Launch bounds that force 128 VGPRs and four waves put 116-128 bytes per lane
// into scratch: 610 -> 762 us when it was measured in round 5.)
// Round 6 (profiles/r6_visibility_groups.txt): the group's reductions on the
// VALU (vis_lanes_reduce), the lanes per (patch, neighbour) chosen by patch size
// on the host (A.vis_group), the NCC's warped colours beyond the kept ones in an
// LDS stash, a sample's depth and template entry from LDS, the neighbour
// wave-uniform (blockIdx.y): 9.1 -> 5.8 ms per --no-sgm view, masks unchanged.
__global__ void __launch_bounds__(256, 2)
topo_visibility_kernel(TopoArgs A)
{
#pragma clang fp contract(off)
    __shared__ double red[6 * 4];
    // Dynamic LDS, sized by the host (vis_launch_shape, topo_vis_plan.h):
    //  * the depths ncc_for_patch's samples take -- the surface at the patch's
    //    pixels and its four corner nodes, [group of the workgroup][ps^2 + 4]
    //    doubles, left there by the pass over the pixels;
    //  * the sample template of an interior patch (all five border predicates),
    //    two ints per entry;
    //  * the warped colours of the samples a lane does not keep in registers,
    //    [slot][channel][thread] floats.
    // A sample was three dependent round trips to memory (template entry ->
    // depth -> taps) in a kernel whose waves wait for memory half of their life;
    // with the first two in LDS it is one.
    extern __shared__ double vis_lds[];
    double *const lds_depth = vis_lds;
    int *const lds_tpl = reinterpret_cast<int *>(vis_lds + A.lds_depth_doubles);
    float *const ncc_stash = reinterpret_cast<float *>(lds_tpl + 2 * A.lds_tpl_n);
    int const ps = A.ps;
    int const G = A.vis_group;
    int const lane = threadIdx.x & 63;
    int const g_log2 = 31 - __clz(G);           // G = 1 << g_log2
    int const gl = threadIdx.x & (G - 1);     // lane inside the group
    int const dstride = ps * ps + 4;
    bool const depth_in_lds = A.lds_depth_doubles > 0;
    double *const my_depths = lds_depth + (threadIdx.x >> g_log2) * dstride;
    if (A.lds_tpl_n > 0) {
        const NccSample *src = A.ncc + A.ncc_off[31];
        for (int i = threadIdx.x; i < A.lds_tpl_n; i += 256) {
            NccSample const e = src[i];
            lds_tpl[2 * i] = (int)((unsigned)(unsigned short)e.dx | ((unsigned)(unsigned short)e.dy << 16));
            lds_tpl[2 * i + 1] = e.src;
        }
        __syncthreads();
    }
    // (group index < num_patches * n_subs: 32 bits)
    // (Round 6 measured two other orders of the groups, because the kernel
    // fetches 1,007 MB per call at 1920 x 1080 for ~340 MB of planes
    // (profiles/r6_hbm_traffic.txt): neighbour-major -- the groups in flight read
    // ONE neighbour's image -- and the workgroups dealt to the XCDs in contiguous
    // bands of the patch grid, as the patch kernel's are.  Neither changed the
    // traffic (1,007 MB) or the time (610 / 623 against 605-611 us): the fetches are
    // 12-byte taps and 4-byte z-buffer cells out of 128-byte lines, not lines
    // fetched by several XCDs.  Plain order.)
    // The neighbour is the workgroup's (blockIdx.y): its camera, image size and
    // pointers are wave-uniform -- scalar registers and scalar loads, operands
    // of the vector arithmetic instead of 30 vector registers of every lane.
    int const s = (int)blockIdx.y;
    int const p = (int)(((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) >> g_log2);
    bool alive = p < A.num_patches && A.patch_valid[p];
    int const pc = alive ? p : 0;
    int const px = A.start_x + (pc % A.npx) * ps;
    int const py = A.start_y + (pc / A.npx) * ps;
    const double *M = A.cams->M[s];
    const double *t = A.cams->t[s];
    TopoView const mv = A.views[0], sv = A.views[1 + s];
    double const sw = sv.w, sh = sv.h;
    int const zw = sv.w + 1;
    double const cutoffset = 0.03 * (sw < sh ? sh : sw);
    const float *zbuf = A.zbuf[s];

    // border / occlusion test and the warp anisotropy, one pass over the
    // patch's pixels
    bool visible = true;
    double worst = 0.0;
    // (one pixel with either kind of quotients; false: outside the neighbour's
    // image, the reference stops looking at the patch)
    auto const pixel = [&](auto const &wq, Warp const &wp, const double *sp, double w) -> bool {
        double const qx = wq.x(wp) - 0.5, qy = wq.y(wp) - 0.5;
        if (qx < cutoffset || qx >= sw - cutoffset || qy < cutoffset
            || qy >= sh - cutoffset) {
            visible = false;
            return false;
        }
        int const cx = (int)qx, cy = (int)qy;
        if (A.zbuf5) {
            // the minimum of the nine cells, formed once per cell (topo_dilate5_kernel)
            if (wp.d * 0.95 > zbuf[(unsigned)cy * (unsigned)zw + (unsigned)cx])
                visible = false;
        } else {
            for (int dx = -1; dx < 2; ++dx)
                for (int dy = -1; dy < 2; ++dy)
                    if (wp.d * 0.95 > zbuf[(unsigned)(cy + dy) * (unsigned)zw + (unsigned)(cx + dx)])
                        visible = false;
        }
        // ratio of the squared singular values of the warp Jacobian
        double const wx = sp[1], wy = sp[2];
        double jac[4];
        wq.jacobian(wp, M, w, wx, wy, jac);
        double const e = sqrt((jac[0] - jac[3]) * (jac[0] - jac[3])
            + (jac[1] + jac[2]) * (jac[1] + jac[2]));
        double const g = sqrt((jac[0] + jac[3]) * (jac[0] + jac[3])
            + (jac[1] - jac[2]) * (jac[1] - jac[2]));
        double const s0 = (e + g) / 2.0;
        double const s1 = fabs(s0 - e);
        double const hi = s0 < s1 ? s1 : s0, lo = s1 < s0 ? s1 : s0;
        double const ratio = (hi * hi) / (lo * lo);
        // std::max(worst, ratio): a NaN ratio leaves worst unchanged
        worst = worst < ratio ? ratio : worst;
        return true;
    };
    if (alive) {
        if (depth_in_lds) {
            int const n00 = (pc / A.npx) * A.stride + pc % A.npx;
            for (int c = gl; c < 4; c += G)
                my_depths[ps * ps + c] = A.nodes[4 * (size_t)(n00 + (c & 1) + (c >> 1) * A.stride)];
        }
        for (int k = gl; k < ps * ps; k += G) {
            int const i = k & (ps - 1), j = k >> A.ps_log2;
            // depth and pixel derivatives of the surface (topo_pixel_surface_kernel)
            const double *sp = A.pix + ((unsigned)(py + j) * (unsigned)A.W + (unsigned)(px + i)) * 3u;
            double const w = sp[0];
            if (depth_in_lds)
                my_depths[k] = w;
            Warp wp(M, t, px + i + 0.5, py + j + 0.5, w);
            WarpQuotients<true> const wq(wp, A.exact_divisions == 0);
            bool const go_on = wq.plain() ? pixel(wq, wp, sp, w)
                : pixel(WarpQuotients<false>(wp), wp, sp, w);
            if (!go_on)
                break;
        }
    }
    // (the depths are read by the other lanes of the group: LDS operations of a
    // wave complete in order, the fences keep the compiler from moving them; a
    // group of 256 meets in group_all's barrier below)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    visible = group_all(visible, G, lane, red);
    worst = vis_group_max(worst, G, red);
    alive = alive && visible && !(worst > 8.0);

    // ncc_for_patch
    double ncc = 1.0;
    if (A.use_ncc) {
        int const flags = smvs_topo::ncc_flags(px, py, ps, mv.w, mv.h);
        const NccSample *tpl = A.ncc + A.ncc_off[flags];
        int const n = A.ncc_off[flags + 1] - A.ncc_off[flags];
        bool const tpl_in_lds = A.lds_tpl_n > 0 && flags == 31;
        auto const sample_at = [&](int i) -> NccSample {
            if (tpl_in_lds) {
                int const a = lds_tpl[2 * i], b = lds_tpl[2 * i + 1];
                return NccSample{ (short)(a & 0xffff), (short)(a >> 16), (short)b };
            }
            return tpl[i];
        };
        bool inside = true;
        double sum0[3] = { 0, 0, 0 }, sum1[3] = { 0, 0, 0 };
        double mean0[3], mean1[3];
        double n0 = 0.0, n1 = 0.0, dot = 0.0;
        // The colours of a sample, main view and warped neighbour.  The second
        // pass (centred products) needs the same values as the first (sums):
        // a lane keeps its first NCC_KEEP samples in registers -- all of them
        // at the fine scales, where the border samples make the templates
        // 2 - 3 x the patch -- and recomputes the rest.
        // (float: the kept values ARE floats -- an image value, linear_at's
        // float result -- widened when they are used)
        float keep_m[NCC_KEEP][3], keep_s[NCC_KEEP][3];
        // Round 6: what does not fit the registers goes to LDS instead of being
        // recomputed in the second pass -- at patch sizes 32 and 64 a lane has
        // ~18 samples, so the second pass warped and interpolated 14 of them
        // again (only the thread itself reads its slots: no barrier)
        auto const stash_put = [&](int slot, float const (&cs)[3]) {
            if (slot - NCC_KEEP < A.ncc_stash_slots)
                for (int c = 0; c < 3; ++c)
                    ncc_stash[((slot - NCC_KEEP) * 3 + c) * 256 + threadIdx.x] = cs[c];
        };
        auto colours = [&](int i, double (&cm)[3], double (&cs)[3], bool check) -> bool {
            NccSample const smp = sample_at(i);
            // the depth of grid sample src is the surface at that pixel; the
            // corner samples take the corner node's depth (:803-857)
            double depth;
            if (depth_in_lds) {
                depth = my_depths[smp.src >= 0 ? smp.src : ps * ps - 1 - smp.src];
            } else if (smp.src >= 0) {
                // (32-bit offsets: the host checks that the planes have fewer than
                // 2^31 elements; 64-bit multiply-adds run at a quarter of the rate)
                depth = A.pix[((unsigned)(py + (smp.src >> A.ps_log2)) * (unsigned)A.W
                    + (unsigned)(px + (smp.src & (ps - 1)))) * 3u];
            } else {
                int const corner = -1 - smp.src;
                int const n00 = (pc / A.npx) * A.stride + pc % A.npx;
                depth = A.nodes[4 * (size_t)(n00 + (corner & 1) + (corner >> 1) * A.stride)];
            }
            double const sx = (double)(px + smp.dx);
            double const sy = (double)(py + smp.dy);
            Warp wp(M, t, sx + 0.5, sy + 0.5, depth);
            SharedDivisor const by_d(wp.d, A.exact_divisions == 0);
            double const qx = by_d.quotient(wp.a) - 0.5, qy = by_d.quotient(wp.b) - 0.5;
            if (check && (qx < 1 || qx > sv.w - 2 || qy < 1 || qy > sv.h - 2))
                return false;
            if (mv.c == 3 && sv.c == 3) {
                // RGB views: the three channels of a tap lie side by side, so a
                // sample is 1 + 4 twelve-byte loads instead of 3 + 12 four-byte
                // ones; per channel the arithmetic is linear_at's
                // (topo_math.h), term for term
                float3_r const m3 = *reinterpret_cast<const float3_r *>(mv.image
                    + ((unsigned)(py + smp.dy) * (unsigned)mv.w + (unsigned)(px + smp.dx)) * 3u);
                cm[0] = m3.x; cm[1] = m3.y; cm[2] = m3.z;
                float x = (float)qx, y = (float)qy;
                x = x < 0.0f ? 0.0f : (x > (float)(sv.w - 1) ? (float)(sv.w - 1) : x);
                y = y < 0.0f ? 0.0f : (y > (float)(sv.h - 1) ? (float)(sv.h - 1) : y);
                int const fx = (int)x, fy = (int)y;
                int const fx1 = fx + 1 < sv.w - 1 ? fx + 1 : sv.w - 1;
                int const fy1 = fy + 1 < sv.h - 1 ? fy + 1 : sv.h - 1;
                float const w1 = x - (float)fx, w0 = 1.0f - w1;
                float const w3 = y - (float)fy, w2 = 1.0f - w3;
                float const k00 = w0 * w2, k10 = w1 * w2, k01 = w0 * w3, k11 = w1 * w3;
                const float *img = sv.image;
                unsigned const row0 = (unsigned)fy * (unsigned)sv.w, row1 = (unsigned)fy1 * (unsigned)sv.w;
                float3_r const v00 = *reinterpret_cast<const float3_r *>(img + (row0 + (unsigned)fx) * 3u);
                float3_r const v10 = *reinterpret_cast<const float3_r *>(img + (row0 + (unsigned)fx1) * 3u);
                float3_r const v01 = *reinterpret_cast<const float3_r *>(img + (row1 + (unsigned)fx) * 3u);
                float3_r const v11 = *reinterpret_cast<const float3_r *>(img + (row1 + (unsigned)fx1) * 3u);
                cs[0] = v00.x * k00 + v10.x * k10 + v01.x * k01 + v11.x * k11;
                cs[1] = v00.y * k00 + v10.y * k10 + v01.y * k01 + v11.y * k11;
                cs[2] = v00.z * k00 + v10.z * k10 + v01.z * k01 + v11.z * k11;
                return true;
            }
            for (int c = 0; c < 3; ++c) {
                int const cmi = c < mv.c - 1 ? c : mv.c - 1;
                int const csi = c < sv.c - 1 ? c : sv.c - 1;
                cm[c] = mv.image[((size_t)(py + smp.dy) * mv.w + (px + smp.dx)) * mv.c + cmi];
                cs[c] = smvs_topo::linear_at(sv.image, sv.w, sv.h, sv.c, (float)qx,
                    (float)qy, csi);
            }
            return true;
        };
        // Two samples of an RGB pair of views side by side: both template
        // entries, then both depths, both warps, the nine taps of both, the
        // arithmetic.  A lane's samples were three chains of three dependent
        // round trips each (template entry -> depth -> taps), one after the
        // other: the waves of this kernel wait for memory more than half of
        // their life (profiles/r5_visibility_counters.txt).  Values and the
        // order they are summed in are those of `colours`; a sample outside the
        // neighbour's image reads clamped taps (the sums of such a patch are
        // never used: ncc = -1).
        bool const rgb = mv.c == 3 && sv.c == 3;
        struct NccTaps { unsigned o00, o10, o01, o11; float k00, k10, k01, k11; };
        auto const taps_at = [&](double qx, double qy) -> NccTaps {
            float x = (float)qx, y = (float)qy;
            x = x == x ? x : 0.0f;   // (outside anyway; keeps the conversion defined)
            y = y == y ? y : 0.0f;
            x = x < 0.0f ? 0.0f : (x > (float)(sv.w - 1) ? (float)(sv.w - 1) : x);
            y = y < 0.0f ? 0.0f : (y > (float)(sv.h - 1) ? (float)(sv.h - 1) : y);
            int const fx = (int)x, fy = (int)y;
            int const fx1 = fx + 1 < sv.w - 1 ? fx + 1 : sv.w - 1;
            int const fy1 = fy + 1 < sv.h - 1 ? fy + 1 : sv.h - 1;
            float const w1 = x - (float)fx, w0 = 1.0f - w1;
            float const w3 = y - (float)fy, w2 = 1.0f - w3;
            unsigned const row0 = (unsigned)fy * (unsigned)sv.w, row1 = (unsigned)fy1 * (unsigned)sv.w;
            NccTaps tp;
            tp.o00 = (row0 + (unsigned)fx) * 3u;  tp.o10 = (row0 + (unsigned)fx1) * 3u;
            tp.o01 = (row1 + (unsigned)fx) * 3u;  tp.o11 = (row1 + (unsigned)fx1) * 3u;
            tp.k00 = w0 * w2; tp.k10 = w1 * w2; tp.k01 = w0 * w3; tp.k11 = w1 * w3;
            return tp;
        };
        auto const depth_of = [&](NccSample const &smp) -> const double * {
            int const corner = -1 - smp.src;
            int const n00 = (pc / A.npx) * A.stride + pc % A.npx;
            const double *at_pixel = A.pix + ((unsigned)(py + (smp.src >> A.ps_log2)) * (unsigned)A.W
                + (unsigned)(px + (smp.src & (ps - 1)))) * 3u;
            const double *at_node = A.nodes + 4 * (size_t)(n00 + (corner & 1)
                + (corner >> 1) * A.stride);
            return smp.src >= 0 ? at_pixel : at_node;
        };
        auto const pair = [&](int ia, int ib, float (&ma)[3], float (&sa)[3], bool &oka,
                float (&mb)[3], float (&sb)[3], bool &okb) {
            NccSample const a = sample_at(ia), b = sample_at(ib);
            double da, db;
            if (depth_in_lds) {
                da = my_depths[a.src >= 0 ? a.src : ps * ps - 1 - a.src];
                db = my_depths[b.src >= 0 ? b.src : ps * ps - 1 - b.src];
            } else {
                const double *pa = depth_of(a), *pb = depth_of(b);
                da = *pa;
                db = *pb;
            }
            // (the scheduler would sink the second sample's loads below the first
            // one's arithmetic to save registers: both are asked for first)
            __builtin_amdgcn_sched_barrier(0);
            Warp const wa(M, t, (double)(px + a.dx) + 0.5, (double)(py + a.dy) + 0.5, da);
            Warp const wb(M, t, (double)(px + b.dx) + 0.5, (double)(py + b.dy) + 0.5, db);
            SharedDivisor const qa(wa.d, A.exact_divisions == 0), qb(wb.d, A.exact_divisions == 0);
            double ax, ay, bx, by;
            if (qa.plain && qb.plain) {
                ax = qa.under(wa.a) - 0.5;  ay = qa.under(wa.b) - 0.5;
                bx = qb.under(wb.a) - 0.5;  by = qb.under(wb.b) - 0.5;
            } else {
                ax = wa.x() - 0.5;  ay = wa.y() - 0.5;
                bx = wb.x() - 0.5;  by = wb.y() - 0.5;
            }
            oka = !(ax < 1 || ax > sv.w - 2 || ay < 1 || ay > sv.h - 2);
            okb = !(bx < 1 || bx > sv.w - 2 || by < 1 || by > sv.h - 2);
            NccTaps const ta = taps_at(ax, ay), tb = taps_at(bx, by);
            const float *img = sv.image;
            float3_r const am = *reinterpret_cast<const float3_r *>(mv.image
                + ((unsigned)(py + a.dy) * (unsigned)mv.w + (unsigned)(px + a.dx)) * 3u);
            float3_r const bm = *reinterpret_cast<const float3_r *>(mv.image
                + ((unsigned)(py + b.dy) * (unsigned)mv.w + (unsigned)(px + b.dx)) * 3u);
            float3_r const a00 = *reinterpret_cast<const float3_r *>(img + ta.o00);
            float3_r const a10 = *reinterpret_cast<const float3_r *>(img + ta.o10);
            float3_r const a01 = *reinterpret_cast<const float3_r *>(img + ta.o01);
            float3_r const a11 = *reinterpret_cast<const float3_r *>(img + ta.o11);
            float3_r const b00 = *reinterpret_cast<const float3_r *>(img + tb.o00);
            float3_r const b10 = *reinterpret_cast<const float3_r *>(img + tb.o10);
            float3_r const b01 = *reinterpret_cast<const float3_r *>(img + tb.o01);
            float3_r const b11 = *reinterpret_cast<const float3_r *>(img + tb.o11);
            __builtin_amdgcn_sched_barrier(0);
            ma[0] = am.x; ma[1] = am.y; ma[2] = am.z;
            mb[0] = bm.x; mb[1] = bm.y; mb[2] = bm.z;
            sa[0] = a00.x * ta.k00 + a10.x * ta.k10 + a01.x * ta.k01 + a11.x * ta.k11;
            sa[1] = a00.y * ta.k00 + a10.y * ta.k10 + a01.y * ta.k01 + a11.y * ta.k11;
            sa[2] = a00.z * ta.k00 + a10.z * ta.k10 + a01.z * ta.k01 + a11.z * ta.k11;
            sb[0] = b00.x * tb.k00 + b10.x * tb.k10 + b01.x * tb.k01 + b11.x * tb.k11;
            sb[1] = b00.y * tb.k00 + b10.y * tb.k10 + b01.y * tb.k01 + b11.y * tb.k11;
            sb[2] = b00.z * tb.k00 + b10.z * tb.k10 + b01.z * tb.k01 + b11.z * tb.k11;
        };
        if (alive && rgb && A.ncc_pairs != 0) {
            // pass 0 of the loop below, two samples at a time
            int slot = 0;
            for (int i = gl; i < n; i += 2 * G, slot += 2) {
                int const i2 = i + G;
                bool const two = i2 < n;
                float ma[3], sa[3], mb[3], sb[3];
                bool oka, okb;
                pair(i, two ? i2 : i, ma, sa, oka, mb, sb, okb);
                inside = oka && inside;
#pragma unroll
                for (int k = 0; k < NCC_KEEP; ++k)
                    if (slot == k)
                        for (int c = 0; c < 3; ++c) {
                            keep_m[k][c] = ma[c];
                            keep_s[k][c] = sa[c];
                        }
                if (slot >= NCC_KEEP)
                    stash_put(slot, sa);
                for (int c = 0; c < 3; ++c) {
                    sum0[c] += (double)ma[c];
                    sum1[c] += (double)sa[c];
                }
                if (two) {
                    inside = okb && inside;
#pragma unroll
                    for (int k = 0; k < NCC_KEEP; ++k)
                        if (slot + 1 == k)
                            for (int c = 0; c < 3; ++c) {
                                keep_m[k][c] = mb[c];
                                keep_s[k][c] = sb[c];
                            }
                    if (slot + 1 >= NCC_KEEP)
                        stash_put(slot + 1, sb);
                    for (int c = 0; c < 3; ++c) {
                        sum0[c] += (double)mb[c];
                        sum1[c] += (double)sb[c];
                    }
                }
            }
        }
        for (int pass = 0; pass < 2; ++pass) {
            if (alive && inside && !(pass == 0 && rgb && A.ncc_pairs != 0)) {
                int slot = 0;
                for (int i = gl; i < n; i += G, ++slot) {
                    double cm[3], cs[3];
                    if (pass == 0) {
                        // (no early exit when a sample falls outside: the taps are
                        // clamped into the image, the sums of such a patch are never
                        // used (ncc = -1), and a loop without an exit lets the loads
                        // of the next sample start under the arithmetic of this one)
                        inside = colours(i, cm, cs, true) && inside;
#pragma unroll
                        for (int k = 0; k < NCC_KEEP; ++k)
                            if (slot == k)
                                for (int c = 0; c < 3; ++c) {
                                    keep_m[k][c] = (float)cm[c];
                                    keep_s[k][c] = (float)cs[c];
                                }
                        if (slot >= NCC_KEEP) {
                            // (cs[] ARE floats widened: linear_at's results)
                            float const sf[3] = { (float)cs[0], (float)cs[1], (float)cs[2] };
                            stash_put(slot, sf);
                        }
                        for (int c = 0; c < 3; ++c) {
                            sum0[c] += cm[c];
                            sum1[c] += cs[c];
                        }
                    } else {
                        if (slot < NCC_KEEP) {
#pragma unroll
                            for (int k = 0; k < NCC_KEEP; ++k)
                                if (slot == k)
                                    for (int c = 0; c < 3; ++c) {
                                        cm[c] = keep_m[k][c];
                                        cs[c] = keep_s[k][c];
                                    }
                        } else if (slot - NCC_KEEP < A.ncc_stash_slots) {
                            // the neighbour's colour from the stash, the main
                            // view's read again (one load against a warp, a
                            // division and four taps)
                            NccSample const smp = sample_at(i);
                            size_t const at = (size_t)(py + smp.dy) * mv.w + (px + smp.dx);
                            for (int c = 0; c < 3; ++c) {
                                int const cmi = c < mv.c - 1 ? c : mv.c - 1;
                                cm[c] = mv.image[at * mv.c + cmi];
                                cs[c] = ncc_stash[((slot - NCC_KEEP) * 3 + c) * 256 + threadIdx.x];
                            }
                        } else {
                            (void)colours(i, cm, cs, false);
                        }
                        for (int c = 0; c < 3; ++c) {
                            double const a = cm[c] - mean0[c];
                            double const b = cs[c] - mean1[c];
                            n0 += a * a;
                            n1 += b * b;
                            dot += a * b;
                        }
                    }
                }
            }
            if (pass == 0) {
                inside = group_all(inside, G, lane, red);
                SharedDivisor const by_n((double)n, A.exact_divisions == 0);
                double six[6] = { sum0[0], sum0[1], sum0[2], sum1[0], sum1[1], sum1[2] };
                vis_group_sums<6>(six, G, red);
                for (int c = 0; c < 3; ++c) {
                    mean0[c] = by_n.quotient(six[c]);
                    mean1[c] = by_n.quotient(six[3 + c]);
                }
            }
        }
        double three[3] = { n0, n1, dot };
        vis_group_sums<3>(three, G, red);
        n0 = sqrt(three[0]);
        n1 = sqrt(three[1]);
        dot = three[2];
        if (!inside)
            ncc = -1.0;
        else if (n0 + n1 < 0.001 * n)
            ncc = 1.0;
        else
            ncc = dot / (n0 * n1);
    }
    if (alive && gl == 0 && !(ncc < 0))
        atomicOr(&A.vis_out[p], 1u << s);
}

int
launch_visibility(smvs_ctx *ctx, TopoArgs *A)
{
    {
        long long const pixels = (long long)ctx->num_patches * ctx->patchsize * ctx->patchsize;
        hipLaunchKernelGGL(topo_pixel_surface_kernel, dim3((unsigned)((pixels + 255) / 256)),
            dim3(256), 0, ctx->stream, *A);
    }
    int n_max = 0;
    for (int f = 0; f < 32; ++f)
        n_max = std::max(n_max, ctx->topo_ncc_off[f + 1] - ctx->topo_ncc_off[f]);
    int group_override = 0;
    {
        char name[32];
        std::snprintf(name, sizeof(name), "SMVS_VIS_GROUP_%d", ctx->patchsize);
        const char *e = std::getenv(name);
        group_override = e != nullptr ? std::atoi(e) : 0;
    }
    static bool const no_stash = [] {
        const char *e = std::getenv("SMVS_NCC_STASH");
        return e != nullptr && e[0] == '0';
    }();
    VisLaunchShape const shape = vis_launch_shape(ctx->patchsize, A->use_ncc != 0, n_max,
        ctx->topo_ncc_off[32] - ctx->topo_ncc_off[31], group_override, no_stash);
    A->vis_group = shape.group;
    A->ncc_stash_slots = shape.ncc_stash_slots;
    A->lds_depth_doubles = shape.lds_depth_doubles;
    A->lds_tpl_n = shape.lds_tpl_n;
    long long const items = (long long)ctx->num_patches * shape.group;   // (per neighbour: grid.y)
    hipLaunchKernelGGL(topo_visibility_kernel,
        dim3((unsigned)((items + 255) / 256), (unsigned)ctx->n_subs), dim3(256),
        shape.dynamic_lds_bytes, ctx->stream, *A);
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

} // namespace smvs_hip
