// The 8-path SGM aggregation on gfx950: aggregate_sgm_costs of the reference
// (lib/sgm_stereo.cc:429-667) -- the SSE branch with constant penalty2
// (:361-406); on request the branch without SSE, fill_path_cost :310-346 with
// its seeds :626-654 (SMVS_SGM_P2_ADAPTIVE, the ADAPT kernels below) -- as
// sgm_launch_paths for sgm_run_device (sgm.hip).  Which of the four kernel
// families runs is sgm_path_plan.h's rule.
//
// Every path direction is an independent 1-D recurrence along a row, a column
// or a diagonal line of the image, so one wavefront walks one line (lane l
// owns planes 2l, 2l+1; neighbours and the minimum by DPP), with the loads of
// the next pixels issued ahead of the dependent chain.  With an even plane
// count all eight directions run in ONE launch and add into S with atomics on
// packed u16 pairs (integer adds commute: bit-exact); odd plane counts take
// one launch per direction.  Each path reads C once and read-modify-writes S
// once.  With penalty2 <= 255 and planes in fours a lane holds four planes in
// packed 16-bit arithmetic and stores what the path adds as bytes
// (sgm_paths2_kernel; above 128 planes, multiples of 8 up to SGM_MAX_PLANES:
// sgm_paths_wide_kernel, with or without bytes).
#include "dpp.h"
#include "sgm_internal.h"

#include <cstdlib>
#include <type_traits>

namespace smvs_hip {

struct PathArgs {
    const uint8_t *cost;
    uint16_t *sgm;
    int w, h, D;
    int dx, dy;        // direction of travel
    uint32_t p1, p2;
    int first;         // 1: S is written, not accumulated
    int last;          // 1: last path, fuse the winner-takes-all
    uint8_t *delta;    // all-paths kernel, DELTA form: eight [h][w][D] u8 volumes
    size_t vol;        // bytes of one of them
    const uint8_t *img; // ADAPT kernels: the main image at SGM scale, [h][w]
};

// The reference's build without SSE (sgm_stereo.cc:310-346) adapts penalty2 to
// the intensity step between a pixel and its predecessor on the path:
// max(P1 * 3 / 2, P2 / (|I - I'| + 1)) in int.  It is the same for every plane
// of the pixel, i.e. uniform over the lanes that hold a line.
__device__ __forceinline__ uint32_t
adapted_penalty2(uint32_t p1, uint32_t p2, uint32_t i_here, uint32_t i_before)
{
    uint32_t const diff = (i_here > i_before ? i_here - i_before : i_before - i_here) + 1u;
    return max(p1 * 3u / 2u, p2 / diff);
}

// Line geometry shared by all path kernels.  Lines: for a horizontal path the
// rows, for a vertical path the columns, for a diagonal path all diagonals that
// start on the entry row or the entry column.  Seeding follows the reference
// exactly (sgm_stereo.cc:457-464, 511-534, 589-612): the first pixel of a
// line copies C and adds it to S; for a diagonal path the corner pixel that
// lies on both the entry row and the entry column is added twice (every
// entry-column pixel is the start of its own diagonal, so the reference's
// column seeding needs nothing else).
__device__ __forceinline__ bool
path_line(PathArgs const &A, int line, int *x, int *y, int *len, int *extra)
{
    int const w = A.w, h = A.h;
    *extra = 0;
    if (A.dy == 0) {
        if (line >= h)
            return false;
        *y = line;
        *x = A.dx > 0 ? 0 : w - 1;
        *len = w;
    } else if (A.dx == 0) {
        if (line >= w)
            return false;
        *x = line;
        *y = A.dy > 0 ? 0 : h - 1;
        *len = h;
    } else {
        if (line >= w + h - 1)
            return false;
        int const y_entry = A.dy > 0 ? 0 : h - 1;
        int const x_entry = A.dx > 0 ? 0 : w - 1;
        if (line < w) {
            *x = line;
            *y = y_entry;
            if (*x == x_entry)
                *extra = 1;
        } else {
            int const k = line - w + 1;
            *x = x_entry;
            *y = A.dy > 0 ? k : h - 1 - k;
        }
        int const nx = A.dx > 0 ? w - *x : *x + 1;
        int const ny = A.dy > 0 ? h - *y : *y + 1;
        *len = min(nx, ny);
    }
    return true;
}

// One launch per direction (A.dx, A.dy), one wavefront per line of it
// (path_line), two planes per lane with scalar accesses: the odd plane counts.
//
// ADAPT (the build without SSE): penalty2 per step from the image
// (adapted_penalty2, an exact integer division: this kernel serves the odd
// plane counts and is bound by its scalar accesses), and the corner of an
// UPWARD diagonal sweep starts its line with 2 C, not C (:626-654 seed the path
// volumes with `+=`, row loop and column loop both).  No sum wraps inside
// check_sgm_options' range, so the masks below change nothing there.
template <bool ADAPT>
__global__ void __launch_bounds__(64)
sgm_path_kernel(PathArgs A)
{
    int const lane = threadIdx.x;
    int const w = A.w, D = A.D;
    int x0, y0, len0, extra0;
    if (!path_line(A, blockIdx.x, &x0, &y0, &len0, &extra0))
        return;
    int x = x0, y = y0;
    int const len = len0, extra_seed = extra0;

    int const d0 = 2 * lane, d1 = 2 * lane + 1;
    bool const ok0 = d0 < D, ok1 = d1 < D;
    uint32_t const BIG = 0xFFFFu;
    uint32_t prev0 = BIG, prev1 = BIG;
    uint32_t i_before = 0;

    for (int s = 0; s < len; ++s, x += A.dx, y += A.dy) {
        size_t const base = ((size_t)y * w + x) * D;
        uint32_t c0 = ok0 ? A.cost[base + d0] : 0u;
        uint32_t c1 = ok1 ? A.cost[base + d1] : 0u;
        uint32_t l0, l1;
        uint32_t p2 = A.p2;
        if (ADAPT) {
            uint32_t const i_here = A.img[(size_t)y * w + x];
            p2 = adapted_penalty2(A.p1, A.p2, i_here, i_before);
            i_before = i_here;
        }
        if (s == 0) {
            l0 = c0;
            l1 = c1;
        } else {
            uint32_t const mn = wave_min_u32(min(prev0, prev1));
            uint32_t const left = (uint32_t)__shfl_up((int)prev1, 1);
            uint32_t const right = (uint32_t)__shfl_down((int)prev0, 1);
            bool const has_left = lane > 0;
            bool const has_right = lane < 63 && d1 + 1 < D;
            uint32_t const far = (mn + p2) & 0xFFFFu;
            // u16 wrapping arithmetic of the SSE code (_mm_add_epi16)
            uint32_t u0 = prev0;
            u0 = min(u0, has_left ? ((left + A.p1) & 0xFFFFu) : BIG);
            u0 = min(u0, ok1 ? ((prev1 + A.p1) & 0xFFFFu) : BIG);
            u0 = min(u0, far);
            uint32_t u1 = prev1;
            u1 = min(u1, (prev0 + A.p1) & 0xFFFFu);
            u1 = min(u1, has_right ? ((right + A.p1) & 0xFFFFu) : BIG);
            u1 = min(u1, far);
            l0 = (c0 + u0 - mn) & 0xFFFFu;
            l1 = (c1 + u1 - mn) & 0xFFFFu;
        }
        uint32_t add0 = l0, add1 = l1;
        if (s == 0 && extra_seed) {
            add0 = (2 * c0) & 0xFFFFu;
            add1 = (2 * c1) & 0xFFFFu;
            if (ADAPT && A.dy < 0) {
                l0 = add0;
                l1 = add1;
            }
        }
        if (ok0) {
            uint32_t const old = A.first ? 0u : A.sgm[base + d0];
            A.sgm[base + d0] = (uint16_t)(old + add0);
        }
        if (ok1) {
            uint32_t const old = A.first ? 0u : A.sgm[base + d1];
            A.sgm[base + d1] = (uint16_t)(old + add1);
        }
        prev0 = ok0 ? l0 : BIG;
        prev1 = ok1 ? l1 : BIG;
    }
}

// ---- four planes per lane in packed 16-bit arithmetic: what
// sgm_paths2_kernel and sgm_paths_wide_kernel share ----
typedef unsigned short u16x2_r __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t
pk_add(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, (u16x2_r)(__builtin_bit_cast(u16x2_r, a)
        + __builtin_bit_cast(u16x2_r, b)));
}

__device__ __forceinline__ uint32_t
pk_sub(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, (u16x2_r)(__builtin_bit_cast(u16x2_r, a)
        - __builtin_bit_cast(u16x2_r, b)));
}

__device__ __forceinline__ uint32_t
pk_min(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(
        __builtin_bit_cast(u16x2_r, a), __builtin_bit_cast(u16x2_r, b)));
}

// "no such plane" / "lane without planes", per 16-bit half
constexpr uint32_t PK_BIG2 = 0x7FFF7FFFu;

// One step of the recurrence for the lane's four planes, pa = {L'(4 l),
// L'(4 l + 1)} and pb = {L'(4 l + 2), L'(4 l + 3)} as u16 pairs (sgm_stereo.cc
// :310-346): L = C + min(L'(d), L'(d -+ 1) + P1, min L' + p2') - min L'.
// ca, cb: the four cost bytes as pairs; mnmn: {min L', min L'} of the line;
// far = mnmn + {p2', p2'}; pb_prev / pa_next: pb of the lane before, pa of the
// lane after, as they arrive; the v_perm_b32 selectors make of them the two
// neighbour vectors that reach into the adjacent lanes, {plane 3 of the lane
// before, own plane 0} = perm(pa, pb_prev) and {own plane 3, plane 0 of the
// lane after} = perm(pa_next, pb), 0x05040302 -- or, where the caller's line
// ends at this lane and nothing valid arrives, a selector that puts the bytes
// 0x00, 0xff = 0xFF00 there: no such plane.  *ea, *eb: L - C.
//
// Same integers as sgm_all_paths_kernel, hence the same bytes.  Range, with
// Pmax = the largest penalty2 of a step (check_sgm_penalties; <= 255 where the
// kernel stores bytes, by sgm_path_plan(), <= 7808 where it adds into S): a line
// starts with L = C <= 255, or 2 C <= 510 at the doubly seeded corner of an
// upward diagonal in ADAPT (:626-654 seed the path volumes with `+=`; this
// changes pa / pb only, what is stored there is the same C); a step gives
// L = C + u - min L' with min L' <= u <= min L' + p2' (u is a minimum of terms
// >= min L', one of them min L' + p2'), so L <= 255 + Pmax behind the start
// and every sum of a step is <= max(510, 255 + Pmax) + Pmax < 2^15.  The
// sentinel PK_BIG2 = 0x7FFF per half is above every L, and
// 0x7FFF + P1 <= 0x7FFF + 7808 < 2^16 (P1 <= Pmax in both modes); the 0xFF00 of
// a selector occurs with bytes only, where 0xFF00 + P1 <= 0xFFFF since
// P1 <= 255.  Bytes stored: u - min L' <= p2' <= 255; 0 at the first cell of a
// line, C <= 255 at a doubly seeded corner.
__device__ __forceinline__ void
packed_step(uint32_t &pa, uint32_t &pb, uint32_t ca, uint32_t cb, uint32_t mnmn, uint32_t far,
    uint32_t pb_prev, uint32_t pa_next, uint32_t sel_below, uint32_t sel_above, uint32_t p1p1,
    uint32_t *ea, uint32_t *eb)
{
    // neighbouring planes: {3 of the lane before, 0}, {1, 2}, {3, 0 of the lane after}
    uint32_t const below_a = __builtin_amdgcn_perm(pa, pb_prev, sel_below);
    uint32_t const mid = __builtin_amdgcn_alignbit(pb, pa, 16);
    uint32_t const above_b = __builtin_amdgcn_perm(pa_next, pb, sel_above);
    uint32_t const mid1 = pk_add(mid, p1p1);
    uint32_t const ua = pk_min(pk_min(pa, pk_add(below_a, p1p1)), pk_min(mid1, far));
    uint32_t const ub = pk_min(pk_min(pb, mid1), pk_min(pk_add(above_b, p1p1), far));
    *ea = pk_sub(ua, mnmn);
    *eb = pk_sub(ub, mnmn);
    pa = pk_add(ca, *ea);
    pb = pk_add(cb, *eb);
}

// ADAPT, the build without SSE (sgm_stereo.cc:310-346, adapted_penalty2 above):
// penalty2' depends on |I - I'| in [0, 255] only, so the wave builds the 256
// packed values {p2', p2'} once in LDS (1 KiB, four exact integer divisions
// per lane) and a step is one broadcast ds_read_b32 indexed by the difference
// of two image bytes -- both known as soon as the bytes are loaded, which
// happens with the cost words of the chunk AHEAD, so neither the load nor the
// LDS read sits on the dependent chain of the recurrence.  (An exact division
// per step would add ~25 VALU instructions to a step of ~40.)
__device__ __forceinline__ void
fill_p2_table(uint32_t *table, uint32_t p1, uint32_t p2, int lane)
{
    // entry d: |I - I'| = d (one wave per block: the barrier is a wait on LDS)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t const d = (uint32_t)(lane + 64 * j);
        uint32_t const p = max(p1 * 3u / 2u, p2 / (d + 1u));
        table[d] = p | (p << 16);
    }
    __syncthreads();
}

// {p2', p2'} of a step from its image byte and that of the step before: the
// look-ahead of both kernels, iv[k] -> far_*[k].  (A step past the end of a
// line has image byte 0: an entry of the table like any other, and what that
// step computes is never stored.  As one helper over the K steps of a chunk
// the compiler orders the chunk's blocks differently; this form leaves every
// instruction stream as it was.)
__device__ __forceinline__ uint32_t
table_penalty2(const uint32_t *table, uint32_t i_here, uint32_t i_before)
{
    return table[i_here > i_before ? i_here - i_before : i_before - i_here];
}

// ---- two lines per wavefront (round 6; bytes, plane counts that are
// multiples of four up to 128) ----
// sgm_all_paths_kernel spends ~37 vector instructions per step of a line for
// 128 planes -- two per lane, every minimum and sum a 32-bit operation, and a
// quarter of them the minimum over the wave -- and the launch is bound by
// exactly those (profiles/r6_sgm_counters.txt: 54 % issuing, 0.33 of HBM).
// Here a lane holds FOUR planes as two u16 pairs (v_pk_add_u16 / v_pk_min_u16
// work on both halves), so 32 lanes cover a line and a wave walks TWO adjacent
// lines of one direction: the step's instructions (packed_step) are shared by
// both.  What crosses lanes:
//   * the neighbouring planes come by wave_shr:1 / wave_shl:1; lanes 0 and 31 of
//     a half wave are the ends of a line (the lane before / after belongs to
//     the OTHER line of the wave) and take the 0xFF00 selectors;
//   * the minimum over a line is five DPP steps over a half wave (32 lanes)
//     instead of six over a whole one, one readlane per line.
//
// FULL: 128 planes, every lane of a half wave has four (no idle lanes to reset).
// ADAPT: penalty2' from the table (fill_p2_table); the image byte is one
// address per half wave, a broadcast load.
template <int K, bool FULL, bool ADAPT = false>
__global__ void __launch_bounds__(64)
sgm_paths2_kernel(PathArgs A)
{
    __shared__ uint32_t p2_table[ADAPT ? 256 : 1];
    int const w = A.w, h = A.h, D = A.D;
    // block -> (direction, pair of lines), the grid being sgm_grid_line_pairs();
    // the long horizontal lines first
    int b = blockIdx.x;
    int dir = 0;
    for (; dir < 8; ++dir) {
        int const pairs_of_dir = (sgm_dir_lines(dir, w, h) + 1) >> 1;
        if (b < pairs_of_dir)
            break;
        b -= pairs_of_dir;
    }
    if (dir > 7)
        return;
    A.dx = SGM_DIRS[dir][0];
    A.dy = SGM_DIRS[dir][1];

    int const lane = threadIdx.x;
    int const half = lane >> 5, hl = lane & 31;
    if (ADAPT)
        fill_p2_table(p2_table, A.p1, A.p2, lane);
    int x0 = 0, y0 = 0, len = 0, extra_seed = 0;
    bool const has_line = path_line(A, 2 * b + half, &x0, &y0, &len, &extra_seed);
    if (!has_line)
        len = 0;
    bool const upper = half != 0;
    bool const ok = has_line && (FULL || 4 * hl < D);
    int const li = ok ? hl : 0;
    // the line as running pointers, four planes (bytes) per lane
    size_t const o0 = has_line ? (((size_t)y0 * w + x0) * D >> 2) + li : 0;
    ptrdiff_t const step = ((ptrdiff_t)A.dy * w + A.dx) * D / 4;
    const uint32_t *__restrict__ cin = reinterpret_cast<const uint32_t *>(A.cost) + o0;
    uint32_t *__restrict__ e32
        = reinterpret_cast<uint32_t *>(A.delta + (size_t)dir * A.vol) + o0;
    uint32_t const p1p1 = (uint32_t)A.p1 | ((uint32_t)A.p1 << 16);
    uint32_t const p2p2 = (uint32_t)A.p2 | ((uint32_t)A.p2 << 16);
    // ADAPT: the image bytes of the line, one per step
    size_t const io0 = has_line ? (size_t)y0 * w + x0 : 0;
    ptrdiff_t const istep = (ptrdiff_t)A.dy * w + A.dx;
    const uint8_t *__restrict__ iin = ADAPT ? A.img + io0 : nullptr;
    uint32_t i_before = 0;
    // packed_step's selectors: 0xFF00 at the ends of a line, where the lane
    // before / after belongs to the OTHER line of the wave
    uint32_t const sel_below = hl == 0 ? 0x05040d0cu : 0x05040302u;   // perm(pa, pb_prev)
    uint32_t const sel_above = hl == 31 ? 0x0d0c0302u : 0x05040302u;  // perm(pa_next, pb)

    // ---- the first cell of a line: L = C (sgm_stereo.cc:457-464; a corner that
    // is seeded from its row and from its column adds C twice) ----
    uint32_t pa = PK_BIG2, pb = PK_BIG2;     // planes {4 hl, 4 hl + 1}, {4 hl + 2, 4 hl + 3}
    if (has_line) {
        uint32_t const c = *cin;
        uint32_t const ca = __builtin_amdgcn_perm(0u, c, 0x0c010c00u);
        uint32_t const cb = __builtin_amdgcn_perm(0u, c, 0x0c030c02u);
        if (ok) {
            pa = ca;
            pb = cb;
            if (ADAPT && extra_seed && A.dy < 0) {
                pa = pk_add(ca, ca);
                pb = pk_add(cb, cb);
            }
            *e32 = extra_seed ? c : 0u;
        }
        if (ADAPT)
            i_before = *iin;
    }
    cin += step;
    e32 += step;
    if (ADAPT)
        iin += istep;
    // the remaining steps of the two lines as scalars: every "is this step
    // inside my line" below is then a lane mask built by scalar instructions
    int const rest0 = max(__builtin_amdgcn_readlane(len, 0) - 1, 0);
    int const rest1 = max(__builtin_amdgcn_readlane(len, 32) - 1, 0);
    int const rest_max = max(rest0, rest1), rest_min = min(rest0, rest1);
    auto const inside = [&](int r) -> bool {
        return (!upper & (r < rest0)) | (upper & (r < rest1));
    };

    uint32_t c_cur[K], c_next[K], outv[K];
    uint32_t far_cur[K], far_next[K];   // ADAPT: {p2', p2'} of the steps
#pragma unroll
    for (int k = 0; k < K; ++k) {
        c_cur[k] = 0;
        if (inside(k))
            c_cur[k] = cin[(ptrdiff_t)k * step];
    }
    cin += (ptrdiff_t)K * step;
    if (ADAPT) {
        uint32_t iv[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            iv[k] = 0;
            if (inside(k))
                iv[k] = iin[(ptrdiff_t)k * istep];
        }
        iin += (ptrdiff_t)K * istep;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            far_cur[k] = table_penalty2(p2_table, iv[k], i_before);
            i_before = iv[k];
        }
    }
    // one chunk of K steps; FAST: this chunk and the next lie inside both lines
    // (no predicates on the loads and stores)
    auto const chunk = [&](auto fast_tag, int base) {
        constexpr bool FAST = decltype(fast_tag)::value;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            c_next[k] = 0;
            if (FAST || inside(base + K + k))
                c_next[k] = cin[(ptrdiff_t)k * step];
        }
        uint32_t iv[K];
        if (ADAPT) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                iv[k] = 0;
                if (FAST || inside(base + K + k))
                    iv[k] = iin[(ptrdiff_t)k * istep];
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            outv[k] = 0;
            if (FAST || base + k < rest_max) {
                // the four cost bytes as two u16 pairs
                uint32_t const ca = __builtin_amdgcn_perm(0u, c_cur[k], 0x0c010c00u);
                uint32_t const cb = __builtin_amdgcn_perm(0u, c_cur[k], 0x0c030c02u);
                // the minimum over the line: per lane, then over its half wave
                uint32_t m = pk_min(pa, pb);
                m = ~min(m & 0xFFFFu, m >> 16);
                m = max_dpp0<DPP_ROW_SHR1, DPP_ROWS_ALL>(m);
                m = max_dpp0<DPP_ROW_SHR2, DPP_ROWS_ALL>(m);
                m = max_dpp0<DPP_ROW_SHR4, DPP_ROWS_ALL>(m);
                m = max_dpp0<DPP_ROW_SHR8, DPP_ROWS_ALL>(m);
                m = max_dpp0<DPP_ROW_BCAST15, DPP_ROWS_1_3>(m);
                uint32_t const m_lower = ~(uint32_t)__builtin_amdgcn_readlane((int)m, 31);
                uint32_t const m_upper = ~(uint32_t)__builtin_amdgcn_readlane((int)m, 63);
                uint32_t const mm_lower = m_lower | (m_lower << 16);
                uint32_t const mm_upper = m_upper | (m_upper << 16);
                uint32_t const mnmn = upper ? mm_upper : mm_lower;
                uint32_t const far = pk_add(mnmn, ADAPT ? far_cur[k] : p2p2);
                // (the lanes without a source are ends of a line, whose selectors
                // do not look at what arrives)
                uint32_t const pb_prev = dpp_u32<DPP_WAVE_SHR1, DPP_ROWS_ALL, true>(0u, pb);
                uint32_t const pa_next = dpp_u32<DPP_WAVE_SHL1, DPP_ROWS_ALL, true>(0u, pa);
                uint32_t ea, eb;
                packed_step(pa, pb, ca, cb, mnmn, far, pb_prev, pa_next, sel_below, sel_above,
                    p1p1, &ea, &eb);
                outv[k] = __builtin_amdgcn_perm(eb, ea, 0x06040200u);
                if (!FULL && !ok)
                    pa = pb = PK_BIG2;
            }
        }
        if (ADAPT) {
            // the penalties of the chunk ahead
#pragma unroll
            for (int k = 0; k < K; ++k) {
                far_next[k] = table_penalty2(p2_table, iv[k], i_before);
                i_before = iv[k];
            }
        }
        if (FULL && FAST) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                e32[(ptrdiff_t)k * step] = outv[k];
        } else if (ok) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (FAST || inside(base + k))
                    e32[(ptrdiff_t)k * step] = outv[k];
        }
    };
    for (int base = 0; base < rest_max; base += K) {
        if (base + 2 * K <= rest_min)
            chunk(std::true_type(), base);
        else
            chunk(std::false_type(), base);
        cin += (ptrdiff_t)K * step;
        e32 += (ptrdiff_t)K * step;
#pragma unroll
        for (int k = 0; k < K; ++k)
            c_cur[k] = c_next[k];
        if (ADAPT) {
            iin += (ptrdiff_t)K * istep;
#pragma unroll
            for (int k = 0; k < K; ++k)
                far_cur[k] = far_next[k];
        }
    }
}

// All eight path directions in ONE launch.  The recurrences of different
// directions are independent; only their sums meet in S.  Since the sums are
// wrapping integer adds, S is accumulated with device-scope atomic adds on
// the packed u32 (two u16 planes that cannot carry into each other: eight
// paths of at most 255 + P2 plus the seeds stay below 65536), so the result
// is bit-exact for any interleaving.  ~9000 wavefronts instead of <= 1500 per
// launch, and the wall time is the longest line instead of the sum over
// directions.  S must be zeroed first.
//
// DELTA form (penalty2 <= 255): what a path adds to S at a pixel is
// L = C + (u - min_prev) with 0 <= u - min_prev <= P2 (sgm_stereo.cc:310-346:
// u is the minimum of terms that are all >= min_prev, one of them min_prev +
// P2), and C -- or 2 C at a doubly seeded corner -- at the start of a line.
// So every direction stores L - C as ONE BYTE per cell into its own volume
// with plain coalesced stores (each cell lies on exactly one line per
// direction: no atomics, no zero fill) and sgm_sum_wta_kernel forms
// S = 8 C + the eight bytes on the fly: 16 + 9 bytes per cost cell instead of
// 8 x (1 + 4) + 2 with the read-modify-writes of the u16 volume.
//
// ADAPT (the build without SSE): penalty2 per step from the image byte of the
// step and of the step before (adapted_penalty2: an exact integer division on
// values that are uniform over the wave and known a chunk ahead of the
// recurrence; this kernel serves penalty2 > 255 too, which a byte-indexed
// table of packed u16 pairs would serve as well, but the division is off the
// dependent chain here and keeps the fall-back free of LDS).  The corner of an
// upward diagonal sweep starts with L = 2 C (:626-654).  DELTA bytes: as at
// packed_step, u - min L' <= p2' <= 255.  Without DELTA a path adds at
// most max(510, 255 + p2') to a u16 of S (check_sgm_options).
template <int K, bool DELTA, bool ADAPT = false>
__global__ void __launch_bounds__(64)
sgm_all_paths_kernel(PathArgs A)
{
    // block -> (direction, line), the grid being sgm_grid_lines(); the long
    // horizontal lines come first.  (The two horizontal directions by a
    // division, the rest by a walk: sgm_paths2_kernel's single walk over all
    // eight compiles to other instructions here, so this decode keeps its form
    // and takes only its counts from sgm_dir_lines().)
    int const w = A.w, h = A.h, D = A.D;
    int const rows = sgm_dir_lines(0, w, h);   // == sgm_dir_lines(1, w, h)
    int b = blockIdx.x;
    int dir;
    if (b < 2 * rows) {
        dir = b / rows;           // 0: ->, 1: <-
        b -= dir * rows;
    } else {
        b -= 2 * rows;
        // remaining six: (0,1) (1,1) (-1,1) (0,-1) (1,-1) (-1,-1)
        dir = 2;
        for (int k = 2; k < 8; ++k) {
            int const lines_of_dir = sgm_dir_lines(k, w, h);
            if (b < lines_of_dir)
                break;
            b -= lines_of_dir;
            dir += 1;
        }
        if (dir > 7)
            return;
    }
    A.dx = SGM_DIRS[dir][0];
    A.dy = SGM_DIRS[dir][1];

    int const lane = threadIdx.x;
    int x0, y0, len, extra_seed;
    if (!path_line(A, b, &x0, &y0, &len, &extra_seed))
        return;
    int const pairs = D >> 1;
    bool const ok = lane < pairs;
    int const li = ok ? lane : 0;
    // The line as two running pointers (cost in, path bytes / S out): the
    // cell of step s is `step` u16 pairs behind the cell of step s - 1.
    size_t const o0 = (((size_t)y0 * w + x0) * D >> 1) + li;
    ptrdiff_t const step = ((ptrdiff_t)A.dy * w + A.dx) * D / 2;
    const uint16_t *__restrict__ cin = reinterpret_cast<const uint16_t *>(A.cost) + o0;
    uint32_t *__restrict__ s32 = reinterpret_cast<uint32_t *>(A.sgm) + o0;
    uint16_t *__restrict__ e16
        = reinterpret_cast<uint16_t *>(A.delta + (size_t)dir * A.vol) + o0;
    // "no such plane" / "lane without planes": above every path cost
    // (L <= 255 + P2 < 2^15 by check_sgm_options), and BIG + P1 still fits 16
    // bits, so no sum below needs a mask
    uint32_t const BIG = 0x7FFFu;
    uint32_t prev0 = BIG, prev1 = BIG;
    // ADAPT: the image bytes of the line, one per step
    ptrdiff_t const istep = (ptrdiff_t)A.dy * w + A.dx;
    const uint8_t *__restrict__ iin = ADAPT ? A.img + ((size_t)y0 * w + x0) : nullptr;
    uint32_t i_before = 0;

    uint32_t c_cur[K], c_next[K], addv[K];
    uint32_t p2_cur[K], p2_next[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        c_cur[k] = 0;
        if (k < len)
            c_cur[k] = cin[(ptrdiff_t)k * step];
        if (ADAPT) {
            uint32_t const i_here = k < len ? iin[(ptrdiff_t)k * istep] : 0u;
            p2_cur[k] = adapted_penalty2(A.p1, A.p2, i_here, i_before);
            i_before = i_here;
        }
    }
    cin += (ptrdiff_t)K * step;
    if (ADAPT)
        iin += (ptrdiff_t)K * istep;
    for (int base = 0; base < len; base += K) {
        int const n = min(K, len - base);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            c_next[k] = 0;
            if (base + K + k < len)
                c_next[k] = cin[(ptrdiff_t)k * step];
            if (ADAPT) {
                uint32_t const i_here = base + K + k < len ? iin[(ptrdiff_t)k * istep] : 0u;
                p2_next[k] = adapted_penalty2(A.p1, A.p2, i_here, i_before);
                i_before = i_here;
            }
        }
        cin += (ptrdiff_t)K * step;
        if (ADAPT)
            iin += (ptrdiff_t)K * istep;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            addv[k] = 0;
            if (k < n) {
                int const s = base + k;
                uint32_t const c0 = c_cur[k] & 0xFFu, c1 = c_cur[k] >> 8;
                uint32_t e0, e1;     // what the path adds beyond C
                if (s == 0) {
                    // sgm_stereo.cc:457-464: the line starts with L = C; a corner
                    // that is seeded from its row and from its column adds C twice
                    e0 = extra_seed ? c0 : 0u;
                    e1 = extra_seed ? c1 : 0u;
                    prev0 = c0;
                    prev1 = c1;
                    if (ADAPT && extra_seed && A.dy < 0) {
                        prev0 = 2u * c0;
                        prev1 = 2u * c1;
                    }
                } else {
                    // :310-346: L = C + min(L'(d), L'(d -+ 1) + P1, min L' + P2) - min L'
                    uint32_t const mn = wave_min_u32(min(prev0, prev1));
                    uint32_t const left = lane_prev(prev1, BIG);
                    uint32_t const right = lane_next(prev0, BIG);
                    uint32_t const far = mn + (ADAPT ? p2_cur[k] : A.p2);
                    uint32_t const u0 = min(min(prev0, left + A.p1), min(prev1 + A.p1, far));
                    uint32_t const u1 = min(min(prev1, prev0 + A.p1), min(right + A.p1, far));
                    e0 = u0 - mn;
                    e1 = u1 - mn;
                    prev0 = c0 + e0;
                    prev1 = c1 + e1;
                }
                if (DELTA)
                    addv[k] = e0 | (e1 << 8);
                else
                    addv[k] = (c0 + e0) | ((c1 + e1) << 16);
                if (!ok)
                    prev0 = prev1 = BIG;
            }
        }
        if (ok) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (k < n) {
                    if (DELTA)
                        e16[(ptrdiff_t)k * step] = (uint16_t)addv[k];
                    else
                        (void)__hip_atomic_fetch_add(&s32[(ptrdiff_t)k * step], addv[k],
                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
        }
        e16 += (ptrdiff_t)K * step;
        s32 += (ptrdiff_t)K * step;
#pragma unroll
        for (int k = 0; k < K; ++k)
            c_cur[k] = c_next[k];
        if (ADAPT) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                p2_cur[k] = p2_next[k];
        }
    }
}

// ---- one line per wavefront: the plane counts above 128 (multiples of four
// up to SGM_MAX_PLANES = 256; check_sgm_plane_count admits the multiples of
// eight) ----
// packed_step on a whole wave: lane l holds planes 4 l .. 4 l + 3 as two u16
// pairs, 64 lanes cover up to 256 planes, the cost words of the chunk ahead are
// loaded before the recurrence of the current chunk starts.  What differs from
// sgm_paths2_kernel is what crosses lanes:
//   * the neighbouring planes come from lane -+ 1 of the WAVE (wave_shr:1 /
//     wave_shl:1 cross the rows and the 32-lane boundary); only lane 0 and, in
//     FULL, lane 63 have no source.  With DELTA they take the 0xFF00
//     selectors; without, the lane without a source keeps PK_BIG2 as the DPP
//     move's old value;
//   * the minimum of a line runs over 64 lanes (wave_max_dpp0 of the
//     complements: four row shifts, row_bcast:15, row_bcast:31, one readlane).
// A step's instructions serve ONE line here, not two.
//
// FULL: 256 planes, every lane has four (no idle lanes to reset).
// ADAPT: penalty2' from the table (fill_p2_table), read for the chunk ahead.
// DELTA (largest penalty2 <= 255): L - C as one byte per cell into the
// direction's own volume, plain stores.  Without DELTA the lane adds its two
// u16 pairs {L, L} into S with two u32 atomics (sgm_all_paths_kernel's
// argument: no 16-bit half of S carries, check_sgm_penalties).
template <int K, bool FULL, bool ADAPT, bool DELTA>
__global__ void __launch_bounds__(64)
sgm_paths_wide_kernel(PathArgs A)
{
    __shared__ uint32_t p2_table[ADAPT ? 256 : 1];
    int const w = A.w, h = A.h, D = A.D;
    // block -> (direction, line), the grid being sgm_grid_lines(); the long
    // horizontal lines first
    int b = blockIdx.x;
    int dir = 0;
    for (; dir < 8; ++dir) {
        int const lines_of_dir = sgm_dir_lines(dir, w, h);
        if (b < lines_of_dir)
            break;
        b -= lines_of_dir;
    }
    if (dir > 7)
        return;
    A.dx = SGM_DIRS[dir][0];
    A.dy = SGM_DIRS[dir][1];

    int const lane = threadIdx.x;
    if (ADAPT)
        fill_p2_table(p2_table, A.p1, A.p2, lane);
    int x0 = 0, y0 = 0, len = 0, extra_seed = 0;
    if (!path_line(A, b, &x0, &y0, &len, &extra_seed))
        return;
    bool const ok = FULL || 4 * lane < D;
    int const li = ok ? lane : 0;
    // the line as running pointers, four planes (bytes) per lane
    size_t const o0 = (((size_t)y0 * w + x0) * D >> 2) + li;
    ptrdiff_t const step = ((ptrdiff_t)A.dy * w + A.dx) * D / 4;
    const uint32_t *__restrict__ cin = reinterpret_cast<const uint32_t *>(A.cost) + o0;
    uint32_t *__restrict__ e32
        = reinterpret_cast<uint32_t *>(A.delta + (DELTA ? (size_t)dir * A.vol : 0)) + o0;
    // without DELTA: the lane's two u16 pairs of S
    uint32_t *__restrict__ s32 = reinterpret_cast<uint32_t *>(A.sgm) + 2 * o0;
    uint32_t const p1p1 = (uint32_t)A.p1 | ((uint32_t)A.p1 << 16);
    uint32_t const p2p2 = (uint32_t)A.p2 | ((uint32_t)A.p2 << 16);
    // ADAPT: the image bytes of the line, one per step
    ptrdiff_t const istep = (ptrdiff_t)A.dy * w + A.dx;
    const uint8_t *__restrict__ iin = ADAPT ? A.img + ((size_t)y0 * w + x0) : nullptr;
    uint32_t i_before = 0;
    // packed_step's selectors; DELTA: 0xFF00 at lane 0 and lane 63, which have
    // no lane before / after.  (An idle lane after the last one of the line
    // holds PK_BIG2: no selector needed.)
    uint32_t const sel_below = DELTA && lane == 0 ? 0x05040d0cu : 0x05040302u;   // perm(pa, pb_prev)
    uint32_t const sel_above = DELTA && lane == 63 ? 0x0d0c0302u : 0x05040302u;  // perm(pa_next, pb)

    // ---- the first cell of the line: L = C (sgm_stereo.cc:457-464; a corner
    // that is seeded from its row and from its column adds C twice) ----
    uint32_t pa = PK_BIG2, pb = PK_BIG2;     // planes {4 l, 4 l + 1}, {4 l + 2, 4 l + 3}
    {
        uint32_t const c = *cin;
        uint32_t const ca = __builtin_amdgcn_perm(0u, c, 0x0c010c00u);
        uint32_t const cb = __builtin_amdgcn_perm(0u, c, 0x0c030c02u);
        if (ok) {
            pa = ca;
            pb = cb;
            if (ADAPT && extra_seed && A.dy < 0) {
                pa = pk_add(ca, ca);
                pb = pk_add(cb, cb);
            }
            if (DELTA) {
                *e32 = extra_seed ? c : 0u;
            } else {
                (void)__hip_atomic_fetch_add(s32, extra_seed ? pk_add(ca, ca) : ca,
                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                (void)__hip_atomic_fetch_add(s32 + 1, extra_seed ? pk_add(cb, cb) : cb,
                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (ADAPT)
            i_before = *iin;
    }
    cin += step;
    e32 += step;
    s32 += 2 * step;
    if (ADAPT)
        iin += istep;
    // the remaining steps of the line, a scalar
    int const rest = max(__builtin_amdgcn_readfirstlane(len) - 1, 0);

    uint32_t c_cur[K], c_next[K], outa[K], outb[K];
    uint32_t far_cur[K], far_next[K];   // ADAPT: {p2', p2'} of the steps
#pragma unroll
    for (int k = 0; k < K; ++k) {
        c_cur[k] = 0;
        if (k < rest)
            c_cur[k] = cin[(ptrdiff_t)k * step];
    }
    cin += (ptrdiff_t)K * step;
    if (ADAPT) {
        uint32_t iv[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            iv[k] = 0;
            if (k < rest)
                iv[k] = iin[(ptrdiff_t)k * istep];
        }
        iin += (ptrdiff_t)K * istep;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            far_cur[k] = table_penalty2(p2_table, iv[k], i_before);
            i_before = iv[k];
        }
    }
    // one chunk of K steps; FAST: this chunk and the next lie inside the line
    // (no predicates on the loads and stores)
    auto const chunk = [&](auto fast_tag, int base) {
        constexpr bool FAST = decltype(fast_tag)::value;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            c_next[k] = 0;
            if (FAST || base + K + k < rest)
                c_next[k] = cin[(ptrdiff_t)k * step];
        }
        uint32_t iv[K];
        if (ADAPT) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                iv[k] = 0;
                if (FAST || base + K + k < rest)
                    iv[k] = iin[(ptrdiff_t)k * istep];
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            outa[k] = outb[k] = 0;
            if (FAST || base + k < rest) {
                // the four cost bytes as two u16 pairs
                uint32_t const ca = __builtin_amdgcn_perm(0u, c_cur[k], 0x0c010c00u);
                uint32_t const cb = __builtin_amdgcn_perm(0u, c_cur[k], 0x0c030c02u);
                // the minimum over the line: per lane, then over the wave
                uint32_t m = pk_min(pa, pb);
                m = wave_max_dpp0(~min(m & 0xFFFFu, m >> 16));
                uint32_t const mn = ~m;
                uint32_t const mnmn = mn | (mn << 16);
                uint32_t const far = pk_add(mnmn, ADAPT ? far_cur[k] : p2p2);
                uint32_t pb_prev, pa_next;
                if (DELTA) {
                    // (a lane without a source reads 0; its selector does not
                    // look at what arrives)
                    pb_prev = dpp_u32<DPP_WAVE_SHR1, DPP_ROWS_ALL, true>(0u, pb);
                    pa_next = dpp_u32<DPP_WAVE_SHL1, DPP_ROWS_ALL, true>(0u, pa);
                } else {
                    pb_prev = lane_prev(pb, PK_BIG2);
                    pa_next = lane_next(pa, PK_BIG2);
                }
                uint32_t ea, eb;
                packed_step(pa, pb, ca, cb, mnmn, far, pb_prev, pa_next, sel_below, sel_above,
                    p1p1, &ea, &eb);
                if (DELTA) {
                    outa[k] = __builtin_amdgcn_perm(eb, ea, 0x06040200u);
                } else {
                    outa[k] = pa;
                    outb[k] = pb;
                }
                if (!FULL && !ok)
                    pa = pb = PK_BIG2;
            }
        }
        if (ADAPT) {
            // the penalties of the chunk ahead
#pragma unroll
            for (int k = 0; k < K; ++k) {
                far_next[k] = table_penalty2(p2_table, iv[k], i_before);
                i_before = iv[k];
            }
        }
        if (FULL || ok) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (FAST || base + k < rest) {
                    if (DELTA) {
                        e32[(ptrdiff_t)k * step] = outa[k];
                    } else {
                        (void)__hip_atomic_fetch_add(&s32[2 * (ptrdiff_t)k * step], outa[k],
                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        (void)__hip_atomic_fetch_add(&s32[2 * (ptrdiff_t)k * step + 1], outb[k],
                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
        }
    };
    for (int base = 0; base < rest; base += K) {
        if (base + 2 * K <= rest)
            chunk(std::true_type(), base);
        else
            chunk(std::false_type(), base);
        cin += (ptrdiff_t)K * step;
        e32 += (ptrdiff_t)K * step;
        s32 += 2 * (ptrdiff_t)K * step;
#pragma unroll
        for (int k = 0; k < K; ++k)
            c_cur[k] = c_next[k];
        if (ADAPT) {
            iin += (ptrdiff_t)K * istep;
#pragma unroll
            for (int k = 0; k < K; ++k)
                far_cur[k] = far_next[k];
        }
    }
}

// f(std::bool_constant<b>()...) for run-time bools b...: a kernel's template
// arguments from what the plan and the options say
template <typename F>
static void
with_bools(F &&f)
{
    f();
}
template <typename F, typename... Rest>
static void
with_bools(F &&f, bool b, Rest... rest)
{
    if (b)
        with_bools([&](auto... tags) { f(std::true_type(), tags...); }, rest...);
    else
        with_bools([&](auto... tags) { f(std::false_type(), tags...); }, rest...);
}

// (declared in sgm_internal.h)
SgmPathPlan
sgm_path_plan_here(int num_steps, unsigned largest_p2)
{
    // (SMVS_SGM_PATHS=wave: a wave per line, two planes per lane -- rounds 3-5)
    static bool const wave_per_line = [] {
        const char *e = std::getenv("SMVS_SGM_PATHS");
        return e != nullptr && e[0] == 'w';
    }();
    return sgm_path_plan(num_steps, largest_p2, wave_per_line);
}
static_assert(SGM_MAX_PLANES == 256, "sgm_path_plan's `full` of the wide form");

// (declared in sgm_internal.h)
int
sgm_launch_paths(SgmWorkspace &B, SgmPathPlan const &plan, const uint8_t *d_main,
    int w, int h, SgmRunParams const &R)
{
    hipStream_t const stream = B.ws->stream;
    size_t const vol = (size_t)w * h * R.num_steps;
    bool const adapt = R.p2_mode == SMVS_SGM_P2_ADAPTIVE;
    PathArgs P;
    P.cost = B.cost;
    P.sgm = B.sgm;
    P.w = w;
    P.h = h;
    P.D = R.num_steps;
    P.dx = P.dy = 0;
    P.p1 = R.penalty1;
    P.p2 = R.penalty2;
    P.first = 0;
    P.last = 0;
    P.delta = B.delta;
    P.vol = vol;
    P.img = d_main;
    if (plan.zero_s)
        SMVS_HIP_CHECK(hipMemsetAsync(B.sgm, 0, sizeof(uint16_t) * vol, stream));
    {
        SgmKernelTimer timer(B.prof, stream, SMVS_SGM_K_PATHS);
        auto const launch = [&](auto kernel, int blocks) {
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64), 0, stream, P);
        };
        switch (plan.form) {
        case SGM_PATHS_WIDE:
            with_bools([&](auto full, auto adapt_tag, auto delta) {
                launch(sgm_paths_wide_kernel<8, decltype(full)::value, decltype(adapt_tag)::value,
                           decltype(delta)::value>, sgm_grid_lines(w, h));
            }, plan.full, adapt, plan.delta);
            break;
        case SGM_PATHS_PAIRS:
            with_bools([&](auto full, auto adapt_tag) {
                launch(sgm_paths2_kernel<8, decltype(full)::value, decltype(adapt_tag)::value>,
                    sgm_grid_line_pairs(w, h));
            }, plan.full, adapt);
            break;
        case SGM_PATHS_LINES:
            with_bools([&](auto delta, auto adapt_tag) {
                launch(sgm_all_paths_kernel<16, decltype(delta)::value, decltype(adapt_tag)::value>,
                    sgm_grid_lines(w, h));
            }, plan.delta, adapt);
            break;
        case SGM_PATHS_PER_DIRECTION:
            // the first direction writes S, the others add to it
            for (int k = 0; k < 8; ++k) {
                P.dx = SGM_DIRS[k][0];
                P.dy = SGM_DIRS[k][1];
                P.first = k == 0 ? 1 : 0;
                with_bools([&](auto adapt_tag) {
                    launch(sgm_path_kernel<decltype(adapt_tag)::value>, sgm_dir_lines(k, w, h));
                }, adapt);
            }
            break;
        }
    }
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

} // namespace smvs_hip
