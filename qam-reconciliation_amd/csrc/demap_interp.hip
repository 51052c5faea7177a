// demap_interp.hip -- the reference's second demapper ("Formulation 1", noisemapper.pyx:563-620)
// for gfx950: F_Y inverted by interpolation in the tabulated grid (g_inv, :295-307) instead of the
// root search of demap.hip, on the same 64-frame tiles, bound by its dependent index-search loads
// rather than by fp64 VALU.  The grid's arithmetic is grid_interp.hpp's, written once for these
// kernels, the entry that builds the grid and the native CPU check (tests/native/interp_check.cpp).
#include <atomic>
#include <vector>

#include "qamr_internal.hpp"
#include "demap_wave.hpp"
#include "grid_interp.hpp"

namespace qr {

constexpr int kGridMaxCoarse = 4096;  // coarse entries the wave kernel stages in LDS (32 KiB)
std::atomic<int> g_interp_fast{1};
// log2 of the entries per coarse-table segment, read when a grid is created (knob interp_seg,
// clamped to 1..20); a grid too long for kGridMaxCoarse segments of that size takes the next size
// that fits.  Every divergent probe of the grid in HBM costs the CU's vector-memory pipe a cache
// line per lane, a probe of the LDS table far less, so smaller segments are faster until the LDS
// table cuts the occupancy: 16-PAM 13 dB, B = 4096 (29 354 points): 14.6 / 13.2 / 11.8 / 11.7 ms
// at 64 / 32 / 16 / 8 entries, 4-PAM 3 dB (14 009 points) 7.3 / 6.8 / 6.3 / 5.8 ms
// (profiles/interp/README.md); 16 keeps the table under 32 KiB up to 65 536 points.
std::atomic<int> g_interp_seg{4};

// Formulation 1 on 64-frame tiles, indexed as k_demap_wave: lane = frame, one wave per 64-frame
// tile of one symbol row, grid-stride.  Per hypothesis i (ascending, noisemapper.pyx:587-596):
// y_i = g_inv(n, i), one exp(-((y_i - a_j)**2) / 2 sigma^2) (the reference evaluates the same
// expression once per bit k; Cython's pow(x, 2.0) is compiled to x * x), added to N[k] or D[k]
// by the Gray test of i -- wave-uniform, so the sums stay in registers.  glibc's exp and log
// restated (subnormal and zero sums, log(0) = -inf, are reached at high SNR).
template <int BPS, bool FAST>
__global__ void __launch_bounds__(256) k_demap_interp_wave(const DemapTables *__restrict__ tab, const GridView g,
                                                           int B, int ld, int64_t S, const double *__restrict__ n,
                                                           const int64_t *__restrict__ j, double alpha,
                                                           double *__restrict__ lappr) {
    constexpr int M = 1 << BPS;
    __shared__ GlibcExpLog gt;
    extern __shared__ double coarse[];   // FAST: g.nc entries
    stage_glibc_exp_log(&gt, &kGlibcConst);
    if (FAST) {
        for (int c = threadIdx.x; c < g.nc; c += blockDim.x) coarse[c] = g.coarse[c];
        __syncthreads();
    }
    const DemapTables &t = *tab;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t tiles = ld / 64;
    const int64_t items = S * tiles;
    for (int64_t it = (int64_t)blockIdx.x * 4 + w; it < items; it += (int64_t)gridDim.x * 4) {   // wave-uniform
        const int64_t s = it / tiles;
        const int f = (int)(it - s * tiles) * 64 + lane;
        const bool valid = f < B;
        const double nv = valid ? n[s * ld + f] : 0.5;   // padding lanes: a harmless target
        const int64_t jv = valid ? j[s * ld + f] : 0;
        const bool jok = jv >= 0 && jv < M;
        const double aj = t.a[jok ? (int)jv : 0];
        double N[BPS], D[BPS];
#pragma unroll
        for (int k = 0; k < BPS; ++k) { N[k] = 0; D[k] = 0; }
#pragma unroll 1
        for (int i = 0; i < M; ++i) {
            const double y = grid_g_inv<FAST>(t, g, coarse, nv, i);
            const double d = y - aj;
            const double e = g_exp_full(-(d * d) / t.two_s2, gt);
            int mi = i;
#pragma unroll
            for (int k = 0; k < BPS; ++k) {   // noisemapper.pyx:590-596: Gray bit k of i
                if ((mi * (mi + 1)) & 3) D[k] += e;
                else                     N[k] += e;
                mi >>= 1;
            }
        }
#pragma unroll
        for (int k = 0; k < BPS; ++k) {
            const double out = (g_log_full(N[k], gt) - g_log_full(D[k], gt)) * alpha;   // :598-599, x alpha
            if (valid) lappr[(s * BPS + k) * ld + f] = jok ? out : __builtin_nan("");
        }
    }
}

// One lane per element, for the host entry points (any bps): formulation 1 of symbol s into
// lappr[s * bps + k] (noisemapper.pyx:605-620), the coarse table read from HBM.
template <bool FAST>
__global__ void __launch_bounds__(256) k_demap_interp_lane(const DemapTables *__restrict__ tab, const GridView g,
                                                           int64_t S, const double *__restrict__ n,
                                                           const int64_t *__restrict__ j,
                                                           double *__restrict__ lappr) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const DemapTables &t = *tab;
    const int64_t jv = j[s];
    if (jv < 0 || jv >= t.M) {
        for (int k = 0; k < t.bps; ++k) lappr[s * t.bps + k] = __builtin_nan("");
        return;
    }
    grid_demap_symbol<FAST>(
        t, g, g.coarse, n[s], (int)jv, [](double a) { return g_exp_full(a, kGlibcConst); },
        [](double a) { return g_log_full(a, kGlibcConst); }, lappr + s * t.bps);
}

// noisemapper.pyx:391-403 (demap_noise): y_hat[k] = g_inv(n_hat[k], i[k]); an out-of-range i
// gives NaN (the reference indexes sign_config / F_Y_thresholds out of bounds).
template <bool FAST>
__global__ void __launch_bounds__(256) k_g_inv_interp(const DemapTables *__restrict__ tab, const GridView g, int64_t n,
                                                      const double *__restrict__ n_hat,
                                                      const int64_t *__restrict__ idx, double *__restrict__ y_hat) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const DemapTables &t = *tab;
    const int64_t i = idx[k];
    y_hat[k] = (i < 0 || i >= t.M) ? __builtin_nan("") : grid_g_inv<FAST>(t, g, g.coarse, n_hat[k], (int)i);
}

// The grid itself (noisemapper.pyx:143-144): y[i] = grid_point, and F = the cpdef F_Y of it.
__global__ void __launch_bounds__(256) k_grid_build(const DemapTables *__restrict__ tab, int32_t n, double y_low,
                                                    double y_high, double step, double2 *__restrict__ pairs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double y = grid_point(y_low, y_high, step, n, i);
    double2 p;
    p.x = public_F_Y(*tab, y);
    p.y = y;
    pairs[i] = p;
}

GridView grid_view(const qr_demap *dm) {
    const DemapGrid &gr = dm->grid;
    return GridView{gr.d_pairs, gr.d_coarse, gr.n, gr.nc, gr.seg_shift, gr.h_pairs.back().x, gr.h_pairs.back().y};
}

// body (b) of the index search: the table certified nondecreasing and the knob on
bool grid_fast(const qr_demap *dm) { return dm->grid.nondecreasing && g_interp_fast.load() != 0; }

int need_grid(const qr_demap *dm) {
    if (dm->grid.n <= 0) return set_error(QR_EVALUE, "the interpolation grid has not been created (qr_demap_grid_create)");
    return QR_OK;
}

}  // namespace qr

// ===================================================================== C-ABI
using namespace qr;

extern "C" {

int qr_demap_grid_create(qr_demap *dm, double trunkation_threshold, int64_t n_intervals_per_step, double step) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    if (!(trunkation_threshold > 0) || n_intervals_per_step <= 0 || !(step > 0))
        return set_error(QR_EVALUE, "grid: need trunkation_threshold > 0, n_intervals_per_step > 0, step > 0");
    std::lock_guard<std::mutex> lk(dm->scratch.mu);
    DemapGrid &gr = dm->grid;
    if (gr.n > 0 && gr.trunc == trunkation_threshold && gr.nips == n_intervals_per_step && gr.step == step &&
        gr.seg_req == g_interp_seg.load())
        return QR_OK;
    const GridGeometry geo = grid_geometry(dm->h, trunkation_threshold, (double)n_intervals_per_step, step);
    if (!(geo.n_points >= 2 && geo.n_points <= (double)(1 << 26)))
        return set_error(QR_EVALUE, "grid: %g points (need 2 .. 2^26)", geo.n_points);
    const int32_t n = (int32_t)geo.n_points;
    int32_t seg_shift = g_interp_seg.load();
    seg_shift = seg_shift < 1 ? 1 : seg_shift > 20 ? 20 : seg_shift;
    while (((n - 1) >> seg_shift) + 1 > kGridMaxCoarse) ++seg_shift;
    const int32_t nc = ((n - 1) >> seg_shift) + 1;
    DeviceGuard g(dm->device);
    double2 *d_pairs = nullptr;
    double *d_coarse = nullptr;
    std::vector<double2> h((size_t)n);
    std::vector<double> coarse((size_t)nc);
    hipError_t e = hipMalloc((void **)&d_pairs, (size_t)n * sizeof(double2));
    if (e == hipSuccess) e = hipMalloc((void **)&d_coarse, (size_t)nc * sizeof(double));
    if (e == hipSuccess) {
        k_grid_build<<<(unsigned)((n + 255) / 256), 256>>>(dm->d_tables, n, geo.y_low, geo.y_high, geo.lin_step, d_pairs);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(h.data(), d_pairs, (size_t)n * sizeof(double2), hipMemcpyDeviceToHost);
    int nondecreasing = 1;
    if (e == hipSuccess) {
        for (int32_t r = 0; r + 1 < n; ++r)
            if (!(h[r + 1].x >= h[r].x)) nondecreasing = 0;
        for (int32_t c = 0; c < nc; ++c) coarse[c] = h[(size_t)c << seg_shift].x;
        e = hipMemcpy(d_coarse, coarse.data(), (size_t)nc * sizeof(double), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        (void)hipFree(d_pairs);
        (void)hipFree(d_coarse);
        return hip_fail(e, "qr_demap_grid_create", __FILE__, __LINE__);
    }
    (void)hipFree(gr.d_pairs);   // a rebuild with other parameters replaces the tables
    (void)hipFree(gr.d_coarse);
    gr.d_pairs = d_pairs;
    gr.d_coarse = d_coarse;
    gr.h_pairs.swap(h);
    gr.n = n;
    gr.nc = nc;
    gr.seg_shift = seg_shift;
    gr.seg_req = g_interp_seg.load();
    gr.nondecreasing = nondecreasing;
    gr.trunc = trunkation_threshold;
    gr.nips = n_intervals_per_step;
    gr.step = step;
    return QR_OK;
}

int qr_demap_grid_info(const qr_demap *dm, int32_t *n_points, int32_t *nondecreasing) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    if (int rc = need_grid(dm)) return rc;
    if (n_points) *n_points = dm->grid.n;
    if (nondecreasing) *nondecreasing = dm->grid.nondecreasing;
    return QR_OK;
}

int qr_demap_grid_host(const qr_demap *dm, double *y, double *F) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    if (int rc = need_grid(dm)) return rc;
    for (int32_t r = 0; r < dm->grid.n; ++r) {
        if (F) F[r] = dm->grid.h_pairs[r].x;
        if (y) y[r] = dm->grid.h_pairs[r].y;
    }
    return QR_OK;
}

int qr_g_inv_host(const qr_demap *dm, int64_t n, const double *n_hat, const int64_t *i, double *y_hat) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    if (int rc = need_grid(dm)) return rc;
    if (int rc = check_host_arrays(n, n_hat, i, y_hat)) return rc;
    if (n == 0) return QR_OK;
    HostTrip t(dm->scratch, dm->device);
    double *d_n, *d_y;
    int64_t *d_i;
    if (!t.take(&d_n, (size_t)n, &d_i, (size_t)n, &d_y, (size_t)n)) return t.rc;
    t.up(d_n, n_hat, n);
    t.up(d_i, i, n);
    const GridView gv = grid_view(dm);
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (t.ok()) {
        if (grid_fast(dm)) k_g_inv_interp<true><<<grid, 256>>>(dm->d_tables, gv, n, d_n, d_i, d_y);
        else k_g_inv_interp<false><<<grid, 256>>>(dm->d_tables, gv, n, d_n, d_i, d_y);
        t.launched();
    }
    t.down(y_hat, d_y, n);
    return t.rc;
}

int qr_demap_simplified_host(const qr_demap *dm, int64_t S, const double *n, const int64_t *j, double *lappr) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    if (int rc = need_grid(dm)) return rc;
    if (int rc = check_host_arrays(S, n, j, lappr)) return rc;
    if (S == 0) return QR_OK;
    HostTrip t(dm->scratch, dm->device);
    const size_t bps = dm->h.bps;
    double *d_n, *d_l;
    int64_t *d_j;
    if (!t.take(&d_n, (size_t)S, &d_j, (size_t)S, &d_l, S * bps)) return t.rc;
    t.up(d_n, n, S);
    t.up(d_j, j, S);
    const GridView gv = grid_view(dm);
    const unsigned grid = (unsigned)((S + 255) / 256);
    if (t.ok()) {
        ProfScope ps("demap_interp", nullptr);
        if (grid_fast(dm)) k_demap_interp_lane<true><<<grid, 256>>>(dm->d_tables, gv, S, d_n, d_j, d_l);
        else k_demap_interp_lane<false><<<grid, 256>>>(dm->d_tables, gv, S, d_n, d_j, d_l);
        t.launched();
    }
    t.down(lappr, d_l, S * bps);
    return t.rc;
}

int qr_demap_simplified_batch_device(const qr_demap *dm, int32_t B, int32_t ld, int64_t S, const double *n,
                                     const int64_t *j, double alpha, double *lappr, void *stream) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    int rc = check_shape(B, ld, S);
    if (rc) return rc;
    if ((rc = need_grid(dm))) return rc;
    if (dm->h.bps > kDemapWaveMaxBps)
        return set_error(QR_EUNSUPPORTED, "the batched demapper serves bit_per_symbol <= %d (got %d)", kDemapWaveMaxBps,
                         dm->h.bps);
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g(dm->device);
    ProfScope ps("demap_interp", s);
    const GridView gv = grid_view(dm);
    const int64_t items = S * (ld / kWave);
    const unsigned grid = demap_wave_grid(dm->device, (items + 3) / 4);
    const size_t lds = (size_t)gv.nc * sizeof(double);   // body (b)'s coarse table: nc <= kGridMaxCoarse by construction
    const bool fast = grid_fast(dm);
    dispatch_bps(dm->h.bps, [&](auto b) {
        constexpr int BPS = decltype(b)::value;
        if (fast) k_demap_interp_wave<BPS, true><<<grid, 256, lds, s>>>(dm->d_tables, gv, B, ld, S, n, j, alpha, lappr);
        else k_demap_interp_wave<BPS, false><<<grid, 256, 0, s>>>(dm->d_tables, gv, B, ld, S, n, j, alpha, lappr);
    });
    QR_LAUNCH_CHECK();
    return QR_OK;
}

}  // extern "C"
