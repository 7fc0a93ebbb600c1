// The opt-in plane sweep of a view's SGM front end on gfx950 (not in the
// reference; include/smvs_hip.h, "multi-neighbour plane sweep", has the
// definition): the cost volumes of the main view against n neighbours over the
// main view's planes, folded into one volume, one path aggregation, one winner,
// and the support of the winner among the neighbours.  The census, warp, cost,
// path and WTA kernels are those of a run (sgm.hip, sgm_paths.hip, sgm_wta.hip); the fold and
// the support kernel are here.
#include "sgm_internal.h"

#include <utility>

namespace smvs_hip {

// ------------------------------------------------------------------ the fold
// Two cost bytes of a neighbour travel as the two 16-bit halves of a register,
// so that every operation of the fold is one packed 16-bit instruction for two
// volume cells (v_pk_min_u16, v_pk_max_u16, v_pk_add_u16 and their kin).
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u16x2
pk_min(u16x2 a, u16x2 b)
{
    return __builtin_elementwise_min(a, b);
}
__device__ __forceinline__ u16x2
pk_max(u16x2 a, u16x2 b)
{
    return __builtin_elementwise_max(a, b);
}
__device__ __forceinline__ u16x2
pk_from_u32(uint32_t x)
{
    return __builtin_bit_cast(u16x2, x);
}
// 1 for a cost, 0 for the byte 255
__device__ __forceinline__ u16x2
pk_is_cost(u16x2 v)
{
    u16x2 const all = { 255, 255 }, one = { 1, 1 };
    return pk_min(all - v, one);
}

// Batcher's odd-even merge sort for P = the power of two at or above N, without
// the comparators that touch an index >= N: those slots would hold +infinity,
// every comparator keeps the larger value at the higher index, so they stay
// where they are.  63 comparators at N = 16, 12 at N = 6.
template <int N>
struct SortNet {
    static constexpr int P = N <= 1 ? 1 : N <= 2 ? 2 : N <= 4 ? 4 : N <= 8 ? 8 : 16;
    int a[64], b[64];
    int count = 0;
    constexpr SortNet() : a(), b()
    {
        for (int p = 1; p < P; p *= 2)
            for (int k = p; k >= 1; k /= 2)
                for (int j = k % p; j + k < P; j += 2 * k)
                    for (int i = 0; i < k && i + j + k < P; ++i)
                        if ((i + j) / (2 * p) == (i + j + k) / (2 * p) && i + j + k < N) {
                            a[count] = i + j;
                            b[count] = i + j + k;
                            ++count;
                        }
    }
};
static_assert(SMVS_MAX_SUBS <= 16, "SortNet: at most 16 values");
static_assert(SortNet<16>().count == 63 && SortNet<6>().count == 12 && SortNet<2>().count == 1
        && SortNet<1>().count == 0, "comparators of the odd-even merge sort");

// comparator I of the network: the smaller value to the lower index (the
// indices are constants, v[] stays in registers)
template <int N, size_t I>
__device__ __forceinline__ void
pk_compare_exchange(u16x2 (&v)[N])
{
    constexpr int ia = SortNet<N>().a[I], ib = SortNet<N>().b[I];
    u16x2 const lo = pk_min(v[ia], v[ib]);
    u16x2 const hi = pk_max(v[ia], v[ib]);
    v[ia] = lo;
    v[ib] = hi;
}

template <int N, size_t... I>
__device__ __forceinline__ void
pk_sort(u16x2 (&v)[N], std::index_sequence<I...>)
{
    (pk_compare_exchange<N, I>(v), ...);
}

// The fold of include/smvs_hip.h for two cells at once: v[k] holds the two bytes
// of neighbour k (0 .. 255 in each half).  SELECT: best_k is in 1 .. N - 1, the
// values are sorted (255, no cost, sorts behind every cost) and the first best_k
// are looked at; otherwise all are.  S comes from the sum of the bytes looked at
// less 255 for every one of them that is no cost; all sums stay below 2^16.
// The rounded mean (2 S + k) / (2 k) is floor(x) of x = (2 S + k) / (2 k): the
// quotient is a whole number or at least 1 / 32 away from one, v_rcp_f32 is good
// to 1 ulp and x < 256, so (2 S + k) * rcp(2 k) is within 2^-14 of x and
// truncating it after adding 1 / 64 gives floor(x) for every input.
template <int N, bool SELECT>
__device__ __forceinline__ uint32_t
fold_pair(u16x2 (&v)[N], int best_k, int min_views)
{
    u16x2 m = { 0, 0 };
#pragma unroll
    for (int k = 0; k < N; ++k)
        m += pk_is_cost(v[k]);
    u16x2 sum = { 0, 0 }, keff = m;
    if constexpr (SELECT) {
        pk_sort<N>(v, std::make_index_sequence<(size_t)SortNet<N>().count>());
        keff = u16x2{ 0, 0 };
#pragma unroll
        for (int j = 0; j < N; ++j) {
            // (wave-uniform)
            if (j < best_k) {
                sum += v[j];
                keff += pk_is_cost(v[j]);
            }
        }
        u16x2 const looked = { (unsigned short)best_k, (unsigned short)best_k };
        sum -= (looked - keff) * (unsigned short)255;
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            sum += v[k];
        u16x2 const looked = { (unsigned short)N, (unsigned short)N };
        sum -= (looked - m) * (unsigned short)255;
    }
    uint32_t out = 0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        // (no cost at all: the byte is 255 whatever the quotient)
        int const mm = (int)m[e], kk = max((int)keff[e], 1), ss = (int)sum[e];
        float const x = (float)(2 * ss + kk) * __builtin_amdgcn_rcpf((float)(2 * kk));
        int const c = (int)(x + 0.015625f);
        out |= (uint32_t)(mm < min_views ? 255 : c) << (16 * e);
    }
    return out;
}

// Elementwise on the flat volume: thread i < len / 16 folds 16 cells from one
// 16-byte load per neighbour, the len % 16 threads behind them a byte each.
// `stride`: bytes between two neighbours' volumes, a multiple of 16 wherever
// len >= 16 is folded (the loads are aligned).  N is a template parameter so
// that every array is registers (.private_segment_fixed_size is 0 for all 16).
template <int N, bool SELECT>
__global__ void __launch_bounds__(256)
sgm_fold_kernel(const uint8_t *__restrict__ costs, size_t stride, size_t len,
    uint8_t *__restrict__ out, int best_k, int min_views)
{
    size_t const i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t const nvec = len / 16;
    if (i < nvec) {
        uint4 c[N];
#pragma unroll
        for (int k = 0; k < N; ++k)
            c[k] = reinterpret_cast<const uint4 *>(costs + (size_t)k * stride)[i];
        uint32_t r[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            u16x2 even[N], odd[N];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                uint32_t const x = q == 0 ? c[k].x : q == 1 ? c[k].y : q == 2 ? c[k].z : c[k].w;
                even[k] = pk_from_u32(x & 0x00FF00FFu);          // bytes 0 and 2
                odd[k] = pk_from_u32((x >> 8) & 0x00FF00FFu);    // bytes 1 and 3
            }
            r[q] = fold_pair<N, SELECT>(even, best_k, min_views)
                | (fold_pair<N, SELECT>(odd, best_k, min_views) << 8);
        }
        reinterpret_cast<uint4 *>(out)[i] = make_uint4(r[0], r[1], r[2], r[3]);
        return;
    }
    size_t const o = nvec * 16 + (i - nvec);
    if (o >= len)
        return;
    u16x2 v[N];
#pragma unroll
    for (int k = 0; k < N; ++k)
        v[k] = pk_from_u32((uint32_t)costs[(size_t)k * stride + o]);
    out[o] = (uint8_t)(fold_pair<N, SELECT>(v, best_k, min_views) & 0xFFu);
}

template <int N>
static void
launch_fold_n(const uint8_t *costs, size_t stride, size_t len, uint8_t *out, int n, int best_k,
    int min_views, hipStream_t stream)
{
    if constexpr (N > SMVS_MAX_SUBS)
        return;
    else if (n == N) {
        unsigned const blocks = (unsigned)((len / 16 + len % 16 + 255) / 256);
        // (best_k = 0 and best_k >= n look at every cost: nothing to select)
        if (best_k == 0 || best_k >= n)
            hipLaunchKernelGGL((sgm_fold_kernel<N, false>), dim3(blocks), dim3(256), 0, stream,
                costs, stride, len, out, 0, min_views);
        else if constexpr (N > 1)
            hipLaunchKernelGGL((sgm_fold_kernel<N, true>), dim3(blocks), dim3(256), 0, stream,
                costs, stride, len, out, best_k, min_views);
    } else
        launch_fold_n<N + 1>(costs, stride, len, out, n, best_k, min_views, stream);
}

// the fold of n volumes, under a timer of class SMVS_SGM_K_MERGE
static int
launch_fold(const uint8_t *costs, size_t stride, size_t len, uint8_t *out, int n, int best_k,
    int min_views, SgmProfile *prof, hipStream_t stream)
{
    {
        SgmKernelTimer timer(prof, stream, SMVS_SGM_K_MERGE);
        launch_fold_n<1>(costs, stride, len, out, n, best_k, min_views, stream);
    }
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

// the distance between two neighbours' volumes of `len` bytes
static size_t
fold_stride(size_t len)
{
    return (len + 15) & ~(size_t)15;
}

// --------------------------------------------------------------- the support
// One lane per pixel: the neighbours whose own cost at the winner plane is at
// most support_cost (n byte gathers; 255, no cost, is above every accepted
// support_cost), and no depth below min_support.  argmin stays.
__global__ void __launch_bounds__(256)
sgm_support_kernel(const uint8_t *__restrict__ costs, size_t stride, int n,
    const int32_t *__restrict__ argmin, size_t npix, int D, int support_cost,
    int min_support, uint8_t *__restrict__ support, float *__restrict__ depth)
{
    size_t const p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix)
        return;
    int const i = min(max(argmin[p], 0), D - 1);
    const uint8_t *cell = costs + p * (size_t)D + i;
    int count = 0;
    for (int k = 0; k < n; ++k)
        count += (int)cell[(size_t)k * stride] <= support_cost ? 1 : 0;
    support[p] = (uint8_t)count;
    if (min_support > 0 && count < min_support)
        depth[p] = 0.0f;
}

static const char SGM_NULL_SWEEP_OPTIONS[]
    = "null options (p2_mode, winner, min_views, best_k, support_cost, min_support)";

// (declared in sgm_internal.h)
int
check_sgm_sweep_options(const smvs_sgm_sweep_options *opts, int n_neighbors)
{
    SMVS_REQUIRE(opts != nullptr, SGM_NULL_SWEEP_OPTIONS);
    SMVS_REQUIRE(opts->p2_mode == SMVS_SGM_P2_CONSTANT
            || opts->p2_mode == SMVS_SGM_P2_ADAPTIVE, "unknown penalty2 mode");
    SMVS_REQUIRE(opts->winner == SMVS_SGM_WINNER_PLANE
            || opts->winner == SMVS_SGM_WINNER_SUBPLANE, "unknown winner");
    SMVS_REQUIRE(n_neighbors >= 1 && n_neighbors <= SMVS_MAX_SUBS,
        "n_neighbors must be in [1, SMVS_MAX_SUBS]");
    SMVS_REQUIRE(opts->min_views >= 1 && opts->min_views <= n_neighbors,
        "min_views must be in [1, n_neighbors]");
    SMVS_REQUIRE(opts->best_k >= 0 && opts->best_k <= SMVS_MAX_SUBS,
        "best_k must be in [0, SMVS_MAX_SUBS]");
    SMVS_REQUIRE(opts->support_cost >= 0 && opts->support_cost <= 254,
        "support_cost must be in [0, 254]");
    SMVS_REQUIRE(opts->min_support >= 0 && opts->min_support <= n_neighbors,
        "min_support must be in [0, n_neighbors]");
    return SMVS_OK;
}

// (declared in sgm_internal.h)  The sweep front: main census once; per
// neighbour its image (one at a time through the slots of neighbour 0, as the
// consensus front), warp and cost into volume k; fold into the run's cost
// buffer; paths; WTA; support.
int
sgm_front_sweep(SgmViewSession &S, SgmViewCall const &C)
{
    int rc;
    Workspace &ws = S.ws();
    SgmWorkspace &B = S.B;
    int const n = C.n_neighbors, mw = S.mw, mh = S.mh, num_steps = C.P.num_steps;
    size_t const npix = S.npix;
    size_t const vol = npix * (size_t)num_steps;
    size_t const stride = fold_stride(vol);
    size_t max_out = 0, max_tmp = 0;
    for (int k = 0; k < n; ++k) {
        SgmPreparedSize const Z = sgm_prepared_size(C.neighbors[k].width, C.neighbors[k].height,
            C.neighbor_channels[k], C.halvings);
        max_out = Z.out > max_out ? Z.out : max_out;
        max_tmp = Z.tmp > max_tmp ? Z.tmp : max_tmp;
    }
    // every buffer at its largest size before the first SGM launch (growing one
    // waits for the stream)
    float *d_depth = nullptr;
    uint8_t *d_nbr = nullptr, *d_tmp = nullptr, *d_support = nullptr, *d_vols = nullptr;
    SgmRun R;
    if ((C.runner_up != nullptr && (rc = ws.ensure(WS_RUNNER_UP, npix, &B.runner_up)))
        || (rc = ws.ensure(WS_NBR0, max_out, &d_nbr))
        || (max_tmp != 0 && (rc = ws.ensure(WS_RAW0, max_tmp, &d_tmp)))
        || (rc = ws.ensure(WS_FWD0, npix, &d_depth))
        || (rc = ws.ensure(WS_SUPPORT, npix, &d_support))
        || (rc = ws.ensure(WS_SWEEP, stride * (size_t)n, &d_vols))
        || (rc = sgm_run_plan(B, mw, mh, C.range[0], C.range[1], C.P, &R)))
        return rc;
    sgm_launch_census(B, S.d_main, mw, mh);
    for (int k = 0; k < n; ++k) {
        smvs_sgm_neighbor const &N = C.neighbors[k];
        int pw = 0, ph = 0;
        if ((rc = S.neighbor(k, WS_NBR0, WS_RAW0, &d_nbr, &pw, &ph)) != SMVS_OK
            || (rc = sgm_launch_warp_cost(B, R, mw, mh, d_nbr, pw, ph, N.M_fwd, N.t_fwd,
                    num_steps, d_vols + stride * (size_t)k)) != SMVS_OK)
            return rc;
    }
    if ((rc = launch_fold(d_vols, stride, vol, B.cost, n, C.sweep_opts.best_k,
             C.sweep_opts.min_views, &S.prof, ws.stream)) != SMVS_OK
        || (rc = sgm_run_tail(B, R, S.d_main, mw, mh, C.P, d_depth)) != SMVS_OK)
        return rc;
    {
        SgmKernelTimer timer(&S.prof, ws.stream, SMVS_SGM_K_LR_CHECK);
        hipLaunchKernelGGL(sgm_support_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256),
            0, ws.stream, d_vols, stride, n, B.argmin, npix, num_steps,
            C.sweep_opts.support_cost, C.sweep_opts.min_support, d_support, d_depth);
    }
    SMVS_HIP_CHECK(hipGetLastError());
    return S.finish(d_depth, nullptr, d_support);
}

} // namespace smvs_hip

using namespace smvs_hip;

// One entry fills the record: raw images, the filters, the photo test, the
// refinement sweeps, every output; the one with the photo test is that one with
// the refinement off.  The two with the filters are that one with the photo test
// off (the one at SGM scale has the volumes among its outputs, the raw one has
// not); the two without the filters are those with both filters off.
extern "C" int
smvs_sgm_sweep_for_view_raw_refine(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, const float *range, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_sweep_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, int32_t *argmin, uint8_t *support,
    uint16_t *cost, uint16_t *sgm, uint16_t *runner_up, int n_witness,
    const smvs_sgm_photo_options *photo, float *confidence, uint8_t *views,
    const smvs_sgm_refine_options *refine, float *slant)
{
    smvs_sgm_sweep_options const o = opts != nullptr ? *opts : smvs_sgm_sweep_options{};
    SgmViewCall const C = { .device = device, .main_img = main_img, .w = w, .h = h,
        .channels = channels, .neighbors = neighbors, .neighbor_channels = neighbor_channels,
        .n_neighbors = n_neighbors, .halvings = halvings,
        .P = { num_steps, penalty1, penalty2, o.p2_mode, o.winner }, .sweep = true,
        .sweep_opts = o, .range = range, .filter = filter,
        .null_options = opts != nullptr ? nullptr : SGM_NULL_SWEEP_OPTIONS,
        .depth = depth, .support = support, .argmin = argmin, .cost = cost, .sgm = sgm,
        .runner_up = runner_up, .n_witness = n_witness, .photo = photo,
        .confidence = confidence, .views = views, .refine = refine, .slant = slant };
    return sgm_run_view_call(C);
}

extern "C" int
smvs_sgm_sweep_for_view_raw_photo(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, const float *range, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_sweep_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, int32_t *argmin, uint8_t *support,
    uint16_t *cost, uint16_t *sgm, uint16_t *runner_up, int n_witness,
    const smvs_sgm_photo_options *photo, float *confidence, uint8_t *views)
{
    return smvs_sgm_sweep_for_view_raw_refine(device, main_img, w, h, channels, neighbors,
        neighbor_channels, n_neighbors, halvings, range, num_steps, penalty1, penalty2, opts,
        filter, depth, argmin, support, cost, sgm, runner_up, n_witness, photo, confidence,
        views, &SGM_REFINE_OFF, nullptr);
}

extern "C" int
smvs_sgm_sweep_for_view_filtered(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, const float *range, int num_steps,
    uint16_t penalty1, uint16_t penalty2, const smvs_sgm_sweep_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, int32_t *argmin, uint8_t *support,
    uint16_t *cost, uint16_t *sgm, uint16_t *runner_up)
{
    return smvs_sgm_sweep_for_view_raw_photo(device, main_img, w, h, 1, neighbors,
        SGM_ONE_CHANNEL, n_neighbors, 0, range, num_steps, penalty1, penalty2, opts, filter,
        depth, argmin, support, cost, sgm, runner_up, 0, &SGM_PHOTO_OFF, nullptr, nullptr);
}

extern "C" int
smvs_sgm_sweep_for_view_raw_filtered(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, const float *range, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_sweep_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, uint8_t *support)
{
    return smvs_sgm_sweep_for_view_raw_photo(device, main_img, w, h, channels, neighbors,
        neighbor_channels, n_neighbors, halvings, range, num_steps, penalty1, penalty2, opts,
        filter, depth, nullptr, support, nullptr, nullptr, nullptr, 0, &SGM_PHOTO_OFF, nullptr,
        nullptr);
}

extern "C" int
smvs_sgm_sweep_for_view(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, const float *range, int num_steps,
    uint16_t penalty1, uint16_t penalty2, const smvs_sgm_sweep_options *opts, float *depth,
    int32_t *argmin, uint8_t *support, uint16_t *cost, uint16_t *sgm)
{
    return smvs_sgm_sweep_for_view_filtered(device, main_img, w, h, neighbors, n_neighbors,
        range, num_steps, penalty1, penalty2, opts, &SGM_FILTERS_OFF, depth, argmin, support,
        cost, sgm, nullptr);
}

extern "C" int
smvs_sgm_sweep_for_view_raw(int device, const uint8_t *main_img, int w, int h, int channels,
    const smvs_sgm_neighbor *neighbors, const int *neighbor_channels, int n_neighbors,
    int halvings, const float *range, int num_steps, uint16_t penalty1, uint16_t penalty2,
    const smvs_sgm_sweep_options *opts, float *depth, uint8_t *support)
{
    return smvs_sgm_sweep_for_view_raw_filtered(device, main_img, w, h, channels, neighbors,
        neighbor_channels, n_neighbors, halvings, range, num_steps, penalty1, penalty2, opts,
        &SGM_FILTERS_OFF, depth, support);
}

// the fold kernel alone, on the caller's bytes
extern "C" int
smvs_sgm_fold_costs(int device, const uint8_t *costs, int n_neighbors, size_t len,
    int min_views, int best_k, uint8_t *out)
{
    smvs_sgm_sweep_options const o = { SMVS_SGM_P2_CONSTANT, SMVS_SGM_WINNER_PLANE, min_views,
        best_k, 0, 0 };
    if (int const rc = check_sgm_sweep_options(&o, n_neighbors); rc != SMVS_OK)
        return rc;
    SMVS_REQUIRE(costs && out, "null argument");
    SMVS_REQUIRE(len >= 1 && len <= ((size_t)1 << 32), "len must be in [1, 2^32]");
    int rc;
    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    SgmProfile prof;
    size_t const stride = fold_stride(len);
    uint8_t *d_vols = nullptr, *d_out = nullptr;
    if ((rc = ws.ensure(WS_SWEEP, stride * (size_t)n_neighbors, &d_vols))
        || (rc = ws.ensure(WS_COST, stride, &d_out)))
        return rc;
    for (int k = 0; k < n_neighbors; ++k)
        if ((rc = ws.upload(d_vols + stride * (size_t)k, costs + len * (size_t)k, len)))
            return rc;
    if ((rc = launch_fold(d_vols, stride, len, d_out, n_neighbors, best_k, min_views, &prof,
             ws.stream)) != SMVS_OK
        || (rc = ws.download(out, d_out, len)) != SMVS_OK)
        return rc;
    SMVS_HIP_CHECK(hipStreamSynchronize(ws.stream));
    return SMVS_OK;
}
