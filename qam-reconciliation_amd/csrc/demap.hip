// demap.hip -- PAM/BICM soft demapper (Alice side of the softening scheme) and
// the Bob-side producers of its inputs, for gfx950.
//
// Reference: qamreconciliation/noisemapper.pyx (NoiseMapper), alphabet.pyx,
// bicm.pyx, matrix.pyx, utils.pyx, sims/reconciliation.pyx:93-168.
//
// One lane = one (symbol, frame).  The lane runs the reference's per-symbol
// procedure (noisemapper.pyx:450-540) sequentially: for each hypothesis i a
// bracket + bisection inversion of the mixture CDF F_Y (31..40 F_Y
// evaluations of M scipy-exact erf each), then the Gray-labelled N/D sums in
// i order.  This is fp64-VALU bound (bytes are negligible); lanes of a wave
// hold 64 consecutive frames of the same symbol position so the LAPPR stores
// land directly, coalesced, in the decoder's frame-innermost input layout.
//
// The reference's second demapper ("Formulation 1", noisemapper.pyx:563-620) inverts F_Y by
// interpolation in the tabulated grid instead (g_inv, :295-307): k_demap_interp_wave below, on
// the same tiles, bound by its dependent index-search loads rather than by fp64 VALU.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <vector>

#include "qamr_internal.hpp"
#include "host_build.hpp"
#include "mi_math.hpp"
#include "mi_quad.hpp"

namespace qr {

// 1 = Newton-located root + replayed bisection (bit-identical, ~5x fewer erf), 0 = brute force.
std::atomic<int> g_demap_fast{1};
// Demap kernel on 64-frame tiles (knob demap_hyp): 1 (default) = wave-private (k_demap_wave: one
// wave walks all M hypotheses of its 64-frame tile), 0 = one lane per symbol (k_demap).  Measured
// on MI355X, B = 4096: 16-PAM 13 dB 44.2 vs 47.1 ms, 25 dB 52.2 vs 52.8 ms, 4-PAM 13.7 vs 13.8 ms;
// the round-3 hypothesis-parallel kernel (waves split the hypotheses, two workgroup barriers per
// symbol item) took 46.8 / 54.7 / 20.0 ms and was removed.
std::atomic<int> g_demap_hyp{1};

// Occupancy floor of the per-symbol kernel: 5 waves/SIMD (96 VGPRs, 52-84 B spilled) 53.4 / 58.5 ms
// vs 4 waves 55.9 / 62.5 ms (16-PAM at 13 / 25 dB, 4096 frames), 4-PAM 14.5 ms either way.
constexpr int kDemapWaves = 5;
template <bool FAST, int BPS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kDemapWaves, 8))) k_demap(const DemapTables *__restrict__ tab, const MathTables *__restrict__ gmt,
                                               int B, int ld, int64_t S, const double *__restrict__ n,
                                               const int64_t *__restrict__ j, double alpha,
                                               double *__restrict__ lappr) {
    __shared__ MathTables mt;
    __shared__ GlibcTables gt;
    stage_math_tables(&mt, gmt);
    stage_glibc_tables(&gt, &kGlibcConst);
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t s = item / ld;
    const int f = (int)(item - s * ld);
    if (s >= S || f >= B) return;
    const DemapTables &t = *tab;
    const double nv = n[s * ld + f];
    const int64_t jv = j[s * ld + f];
    double out[BPS];
    if (jv < 0 || jv >= (1 << BPS)) {
#pragma unroll
        for (int k = 0; k < BPS; ++k) out[k] = __builtin_nan("");
    } else {
        demap_symbol<FAST, BPS>(t, mt, gt, nv, (int)jv, alpha, out);
    }
#pragma unroll
    for (int k = 0; k < BPS; ++k) lappr[(s * BPS + k) * ld + f] = out[k];
}

// ---------------------------------------------------------------------------
// Root search of the 64-frame-tile demapper (k_demap_wave, below).  The certified closed form
// of the search needs at most one exact F_Y per (frame, hypothesis), for ~2 % of the lanes;
// instead of the wave running a divergent M-erf F_Y whenever any of its lanes needs one, the
// lanes' evaluation points are compacted into LDS (ballot + mbcnt) and the wave evaluates
// their M erf terms with one lane per (point, m), 64 / M points per pass, after which each
// owner sums its M terms in m order (noisemapper.pyx:278-286: the same products, the same
// sequence of additions).
constexpr int kDemapWaveMaxBps = 6;
#if QR_EXPERIMENT_CLOCK
// the in-kernel clock of the wave-private demapper's launches (diagnostic twin only): {cycles,
// ticks, workgroups}, read and cleared by qr_debug_clock_demap
__device__ unsigned long long g_clk_demap[3];
#endif
// LLR-sum loop unroll of k_demap_wave (1 / 16: 50.3 / 57.0 ms vs 46.8 at 4, 16-PAM, round 3)
constexpr int kDemapUnroll = 4;

// rank of this lane among the set lanes of mk below it
__device__ __forceinline__ int lane_rank(uint64_t mk) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
}

__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// g_inv_search_fast (qamr_math.hpp) with the closed form's exact F_Y evaluated by the
// whole wave (see above).  Every lane of the wave must call it (wave-uniform i).
// ey / et: this wave's 64-double LDS buffers (evaluation points, erf terms).
template <int M>
__device__ __forceinline__ double g_inv_search_wave(const DemapTables &t, const MathTables &mt, double n_hat, int i,
                                                    double *ey, double *et, int lane) {
    SearchCmp cmp{&t, search_target(t, n_hat, i), 0.0, 0.0, false};
    cmp.have = newton_root(t, mt, cmp.T, i, cmp.ystar, cmp.W);   // T lies in region i
    double L = 0.0, H = 0.0;
    int need = 0;
    const bool closed = cmp.have && search_closed_prepare(cmp, L, H, need);
    const bool ask = need != 0;
    const uint64_t mk = __ballot(ask);
    bool gt = false;
    if (mk) {  // wave-uniform
        const int cnt = __popcll(mk);
        const int rank = lane_rank(mk);
        if (ask) ey[rank] = (need == 1) ? L : H;
        wave_lds_fence();
        constexpr int P = 64 / M;  // points per pass
        const int sub = lane / M, m = lane % M;
        for (int base = 0; base < cnt; base += P) {   // wave-uniform trip count
            const int item = base + sub;
            if (item < cnt) et[lane] = (0.5 * (1 + cephes_erf((ey[item] - t.a[m]) / t.den))) * t.p[m];
            wave_lds_fence();
            if (ask && rank >= base && rank < base + P) {
                const double *tt = et + (rank - base) * M;
                double F = tt[0];                     // noisemapper.pyx:282-285, m = 0 first
#pragma unroll
                for (int mm = 1; mm < M; ++mm) F += tt[mm];
                gt = F > cmp.T;                       // SearchCmp::exact(y) > 0
            }
            wave_lds_fence();
        }
    }
    if (closed) return search_closed_finish(L, H, need, gt);
    return search_replay(cmp);   // no certified window / outside the closed form (rare): per lane
}

// ---------------------------------------------------------------------------
// Wave-private demapper (knob demap_hyp = 1, the default): ONE wave walks all M hypotheses of its
// own 64-frame tile (lane = frame; the reference's loop over i, noisemapper.pyx:490-530) and
// keeps the Gray-labelled sums N[k] / D[k] of its lanes in a wave-private LDS slice, updated
// in i order (noisemapper.pyx:521-530: per bit the reference's sequence of additions).  No
// workgroup barrier: a wave's search lengths never hold up another wave.  The exact F_Y of the
// closed-form root search is evaluated by the whole wave as in g_inv_search_wave.
// 127 VGPRs, 4 waves/SIMD.  Forced to 5 / 6 waves (96 / 80 VGPRs, 108 / 160 B spilled per lane):
// 16-PAM 44.2-44.3 / 44.6-44.7 ms vs 44.0-44.1, 4-PAM 16.9 / 19.1 ms vs 13.7 (MI355X, B = 4096).
template <int BPS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) k_demap_wave(const DemapTables *__restrict__ tab,
                                                    const MathTables *__restrict__ gmt, int B, int ld, int64_t S,
                                                    const double *__restrict__ n, const int64_t *__restrict__ j,
                                                    double alpha, double *__restrict__ lappr) {
    constexpr int M = 1 << BPS;
#if QR_EXPERIMENT_CLOCK
    ClkScope clk(true, g_clk_demap, nullptr);  // (diagnostic twin only)
#endif
    __shared__ GlibcExpLog gt;
    __shared__ double ey[4][64], et[4][64];
    __shared__ double acc[4][2 * BPS][64];   // per wave: N[k] rows then D[k] rows, lane = frame
    stage_glibc_exp_log(&gt, &kGlibcConst);
    const DemapTables &t = *tab;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double *accw = &acc[w][0][0];
    const int64_t tiles = ld / 64;
    const int64_t items = S * tiles;
    for (int64_t it = (int64_t)blockIdx.x * 4 + w; it < items; it += (int64_t)gridDim.x * 4) {   // wave-uniform
        const int64_t s = it / tiles;
        const int f = (int)(it - s * tiles) * 64 + lane;
        const bool valid = f < B;
        const double nv = valid ? n[s * ld + f] : 0.5;   // padding lanes: a harmless target
        const int64_t jv = valid ? j[s * ld + f] : 0;
        const bool jok = jv >= 0 && jv < M;
        const int jj = jok ? (int)jv : 0;
        const double aj = t.a[jj], pj = t.p[jj];
#pragma unroll
        for (int k = 0; k < 2 * BPS; ++k) accw[k * 64 + lane] = 0.0;
#pragma unroll 1
        for (int i = 0; i < M; ++i) {
            const double y = g_inv_search_wave<M>(t, *gmt, nv, i, ey[w], et[w], lane);
            // noisemapper.pyx:503-515 in the reference's summation order (k < j, p[j], k > j).
            // Straight-line: every lane computes both exponents (e, and e / 2 sigma^2 for k > j;
            // the missing / 2 sigma^2 for k < j is the reference's, noisemapper.pyx:503-507)
            // and selects -- the lanes of a wave hold different j, so a branch around the
            // division ran for nearly every k anyway, plus its exec-mask bookkeeping -- and
            // p[j] is the lane's own, loaded once per tile.
            double sum = 0;
#pragma unroll kDemapUnroll
            for (int k = 0; k < M; ++k) {
                const double ak = t.a[k];
                const double e = (2 * y - ak - aj) * (ak - aj);
                const double ed = div_two_s2(t, e);
                // k == j: the term is p[j] and the exp is not used, but its argument must stay off
                // exp's special cases -- e is 0 there, and one such lane sends the whole wave
                // through the full routine at every k (measured 40.1 -> 46.5 ms)
                const double arg = k < jj ? e : k == jj ? 1.0 : ed;
                const double ex = g_exp_wave(arg, gt);
                const double tk = ex * t.p[k];
                sum += k == jj ? pj : tk;
            }
            const double q = t.dF[i] / sum;
            int mi = i;
#pragma unroll
            for (int k = 0; k < BPS; ++k) {   // noisemapper.pyx:521-530: Gray bit k of i
                double *a = accw + (((mi * (mi + 1)) & 3) ? BPS + k : k) * 64 + lane;
                *a += q;
                mi >>= 1;
            }
        }
#pragma unroll
        for (int k = 0; k < BPS; ++k) {
            const double out = (g_log_full(accw[k * 64 + lane], gt) - g_log_full(accw[(BPS + k) * 64 + lane], gt)) *
                               alpha;   // :534-538, x alpha
            if (valid) lappr[(s * BPS + k) * ld + f] = jok ? out : __builtin_nan("");
        }
    }
}

static bool launch_demap_wave(int bps, unsigned grid, hipStream_t st, const qr_demap *dm, int B, int ld, int64_t S,
                              const double *n, const int64_t *j, double alpha, double *lappr) {
    switch (bps) {
#define QR_DEMAP_WAVE(b) \
        case b: k_demap_wave<b><<<grid, 256, 0, st>>>(dm->d_tables, dm->d_mtab, B, ld, S, n, j, alpha, lappr); return true;
        QR_DEMAP_WAVE(1) QR_DEMAP_WAVE(2) QR_DEMAP_WAVE(3) QR_DEMAP_WAVE(4) QR_DEMAP_WAVE(5) QR_DEMAP_WAVE(6)
#undef QR_DEMAP_WAVE
        default: return false;
    }
}

// workgroups of the grid-stride demap: enough to fill every CU several times over
static unsigned demap_wave_grid(int device, int64_t items) {
    static std::atomic<int> cus[64];
    int cu = (device >= 0 && device < 64) ? cus[device].load() : 0;
    if (cu <= 0) {
        if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cu <= 0)
            cu = 256;
        if (device >= 0 && device < 64) cus[device].store(cu);
    }
    const int64_t want = (int64_t)cu * 16;
    return (unsigned)(items < want ? items : want);
}

template <int BPS>
static void launch_demap(bool fast, unsigned grid, hipStream_t st, const qr_demap *dm, int B, int ld, int64_t S,
                         const double *n, const int64_t *j, double alpha, double *lappr) {
    if (fast) k_demap<true, BPS><<<grid, 256, 0, st>>>(dm->d_tables, dm->d_mtab, B, ld, S, n, j, alpha, lappr);
    else k_demap<false, BPS><<<grid, 256, 0, st>>>(dm->d_tables, dm->d_mtab, B, ld, S, n, j, alpha, lappr);
}

static void launch_demap_bps(int bps, bool fast, unsigned grid, hipStream_t st, const qr_demap *dm, int B, int ld,
                             int64_t S, const double *n, const int64_t *j, double alpha, double *lappr) {
    switch (bps) {
        case 1: launch_demap<1>(fast, grid, st, dm, B, ld, S, n, j, alpha, lappr); break;
        case 2: launch_demap<2>(fast, grid, st, dm, B, ld, S, n, j, alpha, lappr); break;
        case 3: launch_demap<3>(fast, grid, st, dm, B, ld, S, n, j, alpha, lappr); break;
        case 4: launch_demap<4>(fast, grid, st, dm, B, ld, S, n, j, alpha, lappr); break;
        case 5: launch_demap<5>(fast, grid, st, dm, B, ld, S, n, j, alpha, lappr); break;
        case 6: launch_demap<6>(fast, grid, st, dm, B, ld, S, n, j, alpha, lappr); break;
        case 7: launch_demap<7>(fast, grid, st, dm, B, ld, S, n, j, alpha, lappr); break;
        default: launch_demap<8>(fast, grid, st, dm, B, ld, S, n, j, alpha, lappr); break;
    }
}

// Bob: hard decision (noisemapper.pyx:349-359), transformed noise g(y, x_hat)
// (:289-292, :373-388) and Gray bits of x_hat (alphabet.pyx:98-107, bicm.pyx:26-41).
__global__ void __launch_bounds__(256) k_bob(const DemapTables *__restrict__ tab, int B, int ld, int64_t S,
                                             const double *__restrict__ y, int64_t *__restrict__ xhat,
                                             double *__restrict__ nhat, uint8_t *__restrict__ word) {
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t s = item / ld;
    const int f = (int)(item - s * ld);
    if (s >= S || f >= B) return;
    const DemapTables &t = *tab;
    const double yv = y[s * ld + f];
    int i = binsearch_thr(t.thr, t.M + 1, yv);
    if (i == t.M) i = t.M - 1;
    double g;
    if (t.sign[i]) g = (t.Fthr[i + 1] - single_F_Y(t, yv)) / t.dF[i];
    else           g = (single_F_Y(t, yv) - t.Fthr[i]) / t.dF[i];
    xhat[s * ld + f] = i;
    nhat[s * ld + f] = g;
    const int gray = i ^ (i >> 1);
    for (int k = 0; k < t.bps; ++k) word[(s * t.bps + k) * ld + f] = (uint8_t)((gray >> k) & 1);
}

// Direct reconciliation (sims/reconciliation.pyx:25-51, _y_to_lappr_grey): Bob's
// BICM LAPPRs of his own sample y, Gray-labelled log-sums over the alphabet.
// (y - a_i)**2 is evaluated as a product (the reference's pow(x, 2.0)).
__global__ void __launch_bounds__(256) k_direct_lappr(const DemapTables *__restrict__ tab, double two_var, int B,
                                                      int ld, int64_t S, const double *__restrict__ y,
                                                      double *__restrict__ lappr) {
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t s = item / ld;
    const int f = (int)(item - s * ld);
    if (s >= S || f >= B) return;
    const DemapTables &t = *tab;
    const double yv = y[s * ld + f];
    double N[kMaxBps], D[kMaxBps];
#pragma unroll
    for (int k = 0; k < kMaxBps; ++k) { N[k] = 0; D[k] = 0; }
    for (int i = 0; i < t.M; ++i) {
        const double d = yv - t.a[i];
        const double add = g_exp_full(-(d * d) / two_var, kGlibcConst);
        int mi = i;
#pragma unroll
        for (int k = 0; k < kMaxBps; ++k) {
            if (k < t.bps) {
                if ((mi * (mi + 1)) & 3) D[k] += add;
                else                     N[k] += add;
                mi >>= 1;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kMaxBps; ++k)
        if (k < t.bps) lappr[(s * t.bps + k) * ld + f] = g_log_full(N[k], kGlibcConst) - g_log_full(D[k], kGlibcConst);
}

// Hard reverse reconciliation (noisemapper.pyx:423-432, bare_llr): Alice's LAPPRs
// are the table row of her own symbol, table[M][bps] built on the host (:197-220).
__global__ void __launch_bounds__(256) k_bare_llr(const double *__restrict__ table, int M, int bps, int B, int ld,
                                                  int64_t S, const int64_t *__restrict__ x,
                                                  double *__restrict__ lappr) {
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t s = item / ld;
    const int f = (int)(item - s * ld);
    if (s >= S || f >= B) return;
    const int64_t xi = x[s * ld + f];
    const bool ok = xi >= 0 && xi < M;
    for (int k = 0; k < bps; ++k) lappr[(s * bps + k) * ld + f] = ok ? table[xi * bps + k] : __builtin_nan("");
}

// alphabet.pyx:98-107 with the reflected Gray table of bicm.pyx:26-41.
__global__ void __launch_bounds__(256) k_symbols_to_bits(int bps, int B, int ld, int64_t S,
                                                         const int64_t *__restrict__ x, uint8_t *__restrict__ word) {
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t s = item / ld;
    const int f = (int)(item - s * ld);
    if (s >= S || f >= ld) return;
    const int64_t xi = (f < B) ? x[s * ld + f] : 0;
    const int64_t g = xi ^ (xi >> 1);
    for (int k = 0; k < bps; ++k) word[(s * bps + k) * ld + f] = (uint8_t)((g >> k) & 1);
}

// noisemapper.pyx:289-292, :373-388 with a caller-given index (x_hat).
__global__ void __launch_bounds__(256) k_map_noise(const DemapTables *__restrict__ tab, int B, int ld, int64_t S,
                                                   const double *__restrict__ y, const int64_t *__restrict__ idx,
                                                   double *__restrict__ nhat) {
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t s = item / ld;
    const int f = (int)(item - s * ld);
    if (s >= S || f >= B) return;
    const DemapTables &t = *tab;
    const double yv = y[s * ld + f];
    const int64_t i = idx[s * ld + f];
    double g;
    if (i < 0 || i >= t.M) g = __builtin_nan("");
    else if (t.sign[i]) g = (t.Fthr[i + 1] - single_F_Y(t, yv)) / t.dF[i];
    else g = (single_F_Y(t, yv) - t.Fthr[i]) / t.dF[i];
    nhat[s * ld + f] = g;
}

// noisemapper.pyx:310-345 (cpdef g_inv_search) over arrays, i.e. :407-419 (demap_noise_search):
// y_hat[k] = g_inv_search(n_hat[k], i[k], y_accuracy).  At the default accuracy 1e-9 the fast
// certified search runs (bit-identical to the reference's loops: tests/test_demap_replay.py);
// any other accuracy runs the loops verbatim.  An out-of-range i gives NaN (the reference
// indexes sign_config / F_Y_thresholds out of bounds).
__global__ void __launch_bounds__(256) k_g_inv_search(const DemapTables *__restrict__ tab,
                                                      const MathTables *__restrict__ gmt, int64_t n,
                                                      const double *__restrict__ n_hat, const int64_t *__restrict__ idx,
                                                      double y_accuracy, int fast, double *__restrict__ y_hat) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const DemapTables &t = *tab;
    const int64_t i = idx[k];
    double y;
    if (i < 0 || i >= t.M) y = __builtin_nan("");
    else if (fast && y_accuracy == 1e-9) y = g_inv_search_fast(t, *gmt, n_hat[k], (int)i);
    else y = g_inv_search(t, n_hat[k], (int)i, y_accuracy);
    y_hat[k] = y;
}

// noisemapper.pyx:264-275 (cpdef F_Y, uniform weighting).
__global__ void __launch_bounds__(256) k_public_F_Y(const DemapTables *__restrict__ tab, int64_t n,
                                                    const double *__restrict__ y, double *__restrict__ F) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) F[k] = public_F_Y(*tab, y[k]);
}

// ---------------------------------------------------------------------------
// Table-interpolated g_inv (noisemapper.pyx:295-307) and the formulation-1 demapper built on it
// (demap_lappr_simplified, noisemapper.pyx:563-601).
//
// The grid of noisemapper.pyx:135-144 lives in HBM as n {F[r], y[r]} pairs (qr_demap_grid_create):
// y = numpy's linspace(y_low, y_high, n), F = the cpdef F_Y of it (public_F_Y, the uniform
// mixture).  g_inv(n_hat, i) = __interp(F, y, target) (noisemapper.pyx:47-63): the index r of
// __binsearch (:27-44), then a linear interpolation between pairs r and r + 1, which are 32
// contiguous bytes.
//
// Index search, two bodies:
//  (a) grid_binsearch: the reference's recursion, iterated -- the same probes in the same
//      order, so it returns the reference's index on ANY table;
//  (b) grid_interp_fast: "the last r with F[r] <= val (0 when val < F[0])" by bisection of a
//      coarse table (every 16th F by default, in LDS for the wave kernel) and then of the one
//      16-entry segment in HBM (at most 4 steps).  On a nondecreasing table (a) returns exactly
//      that index:
//      a probe sequence of (a) keeps the invariant F[base] <= val (or base = 0) and
//      val < F[base + size] (or base + size = n), it only ever discards entries on the strength
//      of one comparison val < F[k] (everything from k on is > val) or val >= F[k] (everything up
//      to k is <= val), and it stops at an index r with F[r] <= val < F[r + 1], or at the last
//      entry of its range when val exceeds it -- with ties, always the last of the tied run,
//      because val >= F[index + 1] sends it right.  F is a rounded sum of erf terms, so nothing
//      guarantees that it is nondecreasing: qr_demap_grid_create checks it in one pass and (b) is
//      used only when the check passed (and val is not NaN).
//      Knob interp_fast = 0 forces (a).
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

struct GridView {
    const double2 *pairs;   // [n] {F, y}
    const double *coarse;   // [nc] F[c << seg_shift]
    int32_t n, nc, seg_shift;
    double F_last, y_last;  // pairs[n - 1]
};

#if QR_DEBUG_ASSERT
__device__ unsigned long long g_dbg_demap[4];  // {failed checks, first site, first a, first b}
__device__ __noinline__ void dcheck_fail_demap(int site, long long a, long long b) {
    if (atomicAdd(&g_dbg_demap[0], 1ull) == 0ull) {
        g_dbg_demap[1] = (unsigned long long)site;
        g_dbg_demap[2] = (unsigned long long)a;
        g_dbg_demap[3] = (unsigned long long)b;
        printf("qamr debug check %d failed: a=%lld b=%lld (block %u thread %u)\n", site, a, b, blockIdx.x, threadIdx.x);
    }
}
#define QR_DCHECK(ok, site, a, b)                                         \
    do {                                                                  \
        if (!(ok)) dcheck_fail_demap((site), (long long)(a), (long long)(b)); \
    } while (0)
#else
#define QR_DCHECK(ok, site, a, b) ((void)0)
#endif
enum GridDebugSite {
    kDbgGridIndex = 10,    // grid index r outside [0, n), or r + 1 read with r + 1 >= n
    kDbgGridCoarse = 11,   // coarse-table index outside [0, nc)
    kDbgMiSymbol = 12,     // k_mi_terms: the symbol index x used to read a[] / p[] / fw outside [0, M)
    kDbgMiDecision = 13,   // k_mi_terms: Bob's hard decision x_hat outside [0, M)
    kDbgQuadNode = 14,     // k_mi_quad: the rule's node index outside [0, nodes of the rule)
    kDbgQuadSlot = 15,     // k_mi_quad: the wave's LDS value slot outside [0, 64)
    kDbgQuadProblem = 16,  // k_mi_quad: a work item's problem id outside [0, P), or its half count not 1 / 2
};

// noisemapper.pyx:27-44 (__binsearch) over the F of the pairs, iterated: slice = [base, base + size).
__device__ __forceinline__ int grid_binsearch(const GridView &g, double val) {
    int base = 0, size = g.n;
    for (;;) {
        QR_DCHECK(base >= 0 && size >= 1 && base + size <= g.n, kDbgGridIndex, base, size);
        if (size == 1) return base;
        if (val < g.pairs[base].x) return base;
        if (val > g.pairs[base + size - 1].x) return base + size - 1;
        const int index = size / 2 - 1;
        if (val < g.pairs[base + index].x) { size = index; continue; }
        if (val >= g.pairs[base + index + 1].x) { base += index + 1; size -= index + 1; continue; }
        return base + index;
    }
}

// Body (b) with the interpolation: the last r with F[r] <= val (0 when val < F[0]) and
// __interp's result at it; val is not NaN and val < F[n - 1].  coarse: the coarse table (LDS or
// HBM).  The segment's probes load whole pairs, and the last two probes of a bisection are r and
// r + 1 themselves, so the interpolation operands are usually in registers already; only when r
// is the first or r + 1 is past the last entry probed in the segment is a pair loaded again.
__device__ __forceinline__ double grid_interp_fast(const GridView &g, const double *coarse, double val) {
    int a = 0, b = 1;        // the pairs r = a and r + 1 = b ...
    double2 pa, pb;          // ... once loaded
    bool have_a = false, have_b = false;
    if (!(val < coarse[0])) {
        int lo = 0, hi = g.nc;   // coarse[lo] <= val, and hi == nc or coarse[hi] > val
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            QR_DCHECK(mid >= 0 && mid < g.nc, kDbgGridCoarse, mid, g.nc);
            if (coarse[mid] <= val) lo = mid; else hi = mid;
        }
        a = lo << g.seg_shift;   // F[a] <= val; at most seg_shift steps inside the segment
        b = a + (1 << g.seg_shift) < g.n ? a + (1 << g.seg_shift) : g.n;
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            QR_DCHECK(mid >= 0 && mid < g.n, kDbgGridIndex, mid, g.n);
            const double2 p = g.pairs[mid];
            if (p.x <= val) { a = mid; pa = p; have_a = true; }
            else            { b = mid; pb = p; have_b = true; }
        }
    }
    QR_DCHECK(a >= 0 && a < g.n && b == a + 1, kDbgGridIndex, a, b);
    if (a == g.n - 1) return g.y_last;               // noisemapper.pyx:55-56
    if (!have_a) pa = g.pairs[a];
    QR_DCHECK(a + 1 < g.n, kDbgGridIndex, a + 1, g.n);
    if (!have_b) pb = g.pairs[a + 1];
    if (pb.x == pa.x) return pa.y;                   // :58-59
    return pa.y + (pb.y - pa.y) * (val - pa.x) / (pb.x - pa.x);   // :61-63
}

// noisemapper.pyx:295-307 (g_inv) with __interp (:47-63): left to right, unfused.
// grid_g_inv_val: __interp (:47-63) at the target val; grid_g_inv: the target of (n_hat, i) first.
template <bool FAST>
__device__ __forceinline__ double grid_g_inv_val(const GridView &g, const double *coarse, double val) {
    if (val >= g.F_last) return g.y_last;            // :50-51
    if (FAST && val == val) return grid_interp_fast(g, coarse, val);
    const int r = grid_binsearch(g, val);
    QR_DCHECK(r >= 0 && r < g.n, kDbgGridIndex, r, g.n);
    if (r == g.n - 1) return g.y_last;               // :55-56
    QR_DCHECK(r + 1 < g.n, kDbgGridIndex, r + 1, g.n);
    const double2 p0 = g.pairs[r], p1 = g.pairs[r + 1];
    if (p1.x == p0.x) return p0.y;                   // :58-59
    return p0.y + (p1.y - p0.y) * (val - p0.x) / (p1.x - p0.x);   // :61-63
}
template <bool FAST>
__device__ __forceinline__ double grid_g_inv(const DemapTables &t, const GridView &g, const double *coarse,
                                             double n_hat, int i) {
    // the same expression as g_inv_search's (:297-307)
    return grid_g_inv_val<FAST>(g, coarse, search_target(t, n_hat, i));
}

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
    const double nv = n[s], aj = t.a[jv];
    double N[kMaxBps], D[kMaxBps];
#pragma unroll
    for (int k = 0; k < kMaxBps; ++k) { N[k] = 0; D[k] = 0; }
    for (int i = 0; i < t.M; ++i) {
        const double y = grid_g_inv<FAST>(t, g, g.coarse, nv, i);
        const double d = y - aj;
        const double e = g_exp_full(-(d * d) / t.two_s2, kGlibcConst);
        int mi = i;
#pragma unroll
        for (int k = 0; k < kMaxBps; ++k) {
            if (k < t.bps) {
                if ((mi * (mi + 1)) & 3) D[k] += e;
                else                     N[k] += e;
                mi >>= 1;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kMaxBps; ++k)
        if (k < t.bps) lappr[s * t.bps + k] = g_log_full(N[k], kGlibcConst) - g_log_full(D[k], kGlibcConst);
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

// ---------------------------------------------------------------------------
// Monte-Carlo mutual-information estimator (mutual_information.pyx:218-297): the three per-sample
// terms (mi_math.hpp mi_sample_terms, the arithmetic written once) and their sequential block sums.
// The "frame" of the frame-innermost layout is one montecarlo_information call, a block of S
// samples: d_x[S][ld] int64 (Alice's symbol indices), d_y[S][ld] fp64 (Bob's samples), lane = block.
//
// k_mi_terms: one wave per (sample row s, 64-block tile), grid-stride, as k_demap_interp_wave.  A
// lane takes Bob's hard decision x_hat and n = g(y, x_hat) for its own sample (mi_bob = k_bob's
// expressions), then walks the hypotheses k = 0..M-1 uniformly with the interpolated g_inv; at
// k == x_hat the root-searched y_hat is selected instead (no branch: the lanes of a wave hold
// different x_hat).  That one search per sample is g_inv_search_wave with a per-lane hypothesis:
// the routine is documented for a wave-uniform i, but i enters it only through search_target and
// newton_root, both per-lane computations (k_g_inv_search already runs them with a per-lane i);
// the wave-cooperative part -- compaction of the lanes' evaluation points, M erf terms per point,
// the owner's sum in m order -- reads t.a / t.p / t.den and the lane's own target, never i.  What it
// does need is that every lane of the wave calls it, which holds here (padding lanes run a harmless
// sample).  Terms go to d_terms[q][s][ld], q = 0..2; planes of disabled quantities and the padding
// columns are not written; an out-of-range x gives NaN terms for that sample.
struct MiLds {
    double2 ex[128];   // glibc exp table (g_exp_wave / g_exp_full read T.ex)
    double4 e[64];     // glibc log2 table (g_log2_full reads T.e)
};
template <int BPS, bool FAST>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8)))
k_mi_terms(const DemapTables *__restrict__ tab, const MathTables *__restrict__ gmt, const GridView g,
           const double *__restrict__ mi, unsigned which, int B, int ld, int64_t S, const int64_t *__restrict__ x,
           const double *__restrict__ y, double *__restrict__ terms) {
    constexpr int M = 1 << BPS;
    __shared__ MiLds lt;
    __shared__ double ey[4][64], et[4][64];
    extern __shared__ double coarse[];   // FAST: g.nc entries
    for (int i = threadIdx.x; i < 128; i += blockDim.x) lt.ex[i] = kGlibcConst.ex[i];
    for (int i = threadIdx.x; i < 64; i += blockDim.x) lt.e[i] = kGlibcLog2Const.e[i];
    if (FAST)
        for (int c = threadIdx.x; c < g.nc; c += blockDim.x) coarse[c] = g.coarse[c];
    __syncthreads();
    const DemapTables &t = *tab;
    const double *pX = mi, *fw = mi + M;   // qr_demap_mi_tables: p_Xhat[M] then fwrd[M][M]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t tiles = ld / 64;
    const int64_t items = S * tiles;
    for (int64_t it = (int64_t)blockIdx.x * 4 + w; it < items; it += (int64_t)gridDim.x * 4) {   // wave-uniform
        const int64_t s = it / tiles;
        const int f = (int)(it - s * tiles) * 64 + lane;
        const bool valid = f < B;
        const double yv = valid ? y[s * ld + f] : 0.25;   // padding lanes: a harmless sample
        const int64_t xv = valid ? x[s * ld + f] : 0;
        const bool xok = xv >= 0 && xv < M;
        const int xx = xok ? (int)xv : 0;
        int xh;
        double nv;
        mi_bob(t, yv, xh, nv);
        QR_DCHECK(xx >= 0 && xx < M, kDbgMiSymbol, xx, M);
        QR_DCHECK(xh >= 0 && xh < M, kDbgMiDecision, xh, M);
        double ys = 0.0;
        if (which & kMiXNXhat) ys = g_inv_search_wave<M>(t, *gmt, nv, xh, ey[w], et[w], lane);   // wave-uniform branch
        mi_sample_terms(
            t, pX, fw, M, which, xx, xh, yv,
            [&](int k) { const double yi = grid_g_inv<FAST>(t, g, coarse, nv, k); return k == xh ? ys : yi; },
            [&](double a) { return g_exp_wave(a, lt); }, [&](double a) { return g_log2_full(a, lt); },
            [&](int q, double v) { if (valid) terms[((int64_t)q * S + s) * ld + f] = xok ? v : __builtin_nan(""); });
    }
}

// k_mi_sum: the block totals (mutual_information.pyx:245-297).  One lane per (block, quantity): it
// adds (I0, I1) or subtracts (I2) its S terms in sample order from 0.0 and divides by (double)S; a
// disabled quantity is 0.0 / S.  The chain of dependent adds cannot be reordered, so the launch has
// 3 B lanes of parallelism whatever S is: the next kMiSumAhead rows are requested before the current
// kMiSumAhead are added, so the chain does not wait for memory (S = 4096, B = 256: 0.184 ms with 8 rows
// loaded right before their adds, 0.127 ms now; profiles/mi/README.md).
constexpr int kMiSumAhead = 32;
// the chain of one (block, quantity): SUB subtracts (I2, :295), else adds (:259, :269); a template so
// that the dependent chain is one v_add_f64 per sample, not both results and a select
template <bool SUB>
__device__ __forceinline__ double mi_chain(const double *__restrict__ p, int ld, int64_t S) {
    double acc = 0.0;
    double v[kMiSumAhead], nx[kMiSumAhead];
    int64_t s = 0;
    if (S >= kMiSumAhead) {
#pragma unroll
        for (int u = 0; u < kMiSumAhead; ++u) v[u] = p[u * (int64_t)ld];
    }
    for (; s + kMiSumAhead <= S; s += kMiSumAhead) {
        const bool more = s + 2 * kMiSumAhead <= S;   // block-uniform
        if (more) {
#pragma unroll
            for (int u = 0; u < kMiSumAhead; ++u) nx[u] = p[(s + kMiSumAhead + u) * ld];
        }
#pragma unroll
        for (int u = 0; u < kMiSumAhead; ++u) acc = SUB ? acc - v[u] : acc + v[u];
        if (more) {
#pragma unroll
            for (int u = 0; u < kMiSumAhead; ++u) v[u] = nx[u];
        }
    }
    for (; s < S; ++s) acc = SUB ? acc - p[s * ld] : acc + p[s * ld];
    return acc;
}
__global__ void __launch_bounds__(64) k_mi_sum(unsigned which, int B, int ld, int64_t S,
                                               const double *__restrict__ terms, double *__restrict__ info) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    const int q = blockIdx.y;
    if (f >= B) return;
    double acc = 0.0;
    if ((which >> q) & 1u) {
        const double *p = terms + (int64_t)q * S * ld + f;
        acc = q == 2 ? mi_chain<true>(p, ld, S) : mi_chain<false>(p, ld, S);   // block-uniform
    }
    info[(int64_t)q * ld + f] = acc / (double)S;
}

// glibc log2 over an array (qr_log2_host)
__global__ void __launch_bounds__(256) k_log2(int64_t n, const double *__restrict__ x, double *__restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = g_log2_full(x[k], kGlibcLog2Const);
}

// ---------------------------------------------------------------------------
// Quadrature evaluators (mutual_information.pyx:123-148 and :202-208): scipy.integrate.quad over the
// two integrands of mi_math.hpp.  The integrator's decisions are the host's (mi_quad.hpp); the GPU
// evaluates the rules.  A "problem" is one integral, with its own tables: its demapper's
// DemapTables and grid, its p_Xhat (base kind) and its sign configuration as a bit mask (bit i =
// sign_config[i]; it enters the base integrand only through g_inv's target, noisemapper.pyx:297-307).
//
// k_mi_quad: one wavefront per work item, grid-stride.  A work item is a problem and one interval of
// it (round 1: the whole range) or two (afterwards: the halves of the bisected interval).  KIND =
// base: lane l < 21 of a half takes mi_base_arg at node l of the 21-point rule on that half (lanes
// 0..41 for a pair).  KIND = X_Y: lanes 2 q and 2 q + 1 of a half take mi_xy_arg at +T and -T of node q
// of the transformed 15-point rule (lanes 0..59 for a pair).  Each lane computes its abscissa as the
// rule does (gk21_node / gk15i_x, gk15i_T), the values go to the wave's LDS slice, and lane h forms the
// four sums of half h in the rule's order (gk21_sums / gk15i_sums): out[item][h] = {result,
// |(resk - resg) hlgth|, resabs, resasc}; the rest of the error estimate (a pow) is the host's.  With a
// debug pointer the lanes also write their abscissae and values (qr_mi_quad_rule_host).  The
// tables are wave-uniform: the problem id is read through the first lane, so the compiler addresses
// them with scalar loads.  Every lane of the wave runs the integrand (g_exp_wave's common path
// is branch-free); the padding lanes take a harmless point.
struct MiQuadProblem {
    const DemapTables *tab;
    GridView g;
    const double *pX;   // base kind: p_Xhat[M] (device)
    uint64_t sign;      // bit i = sign_config[i]
    int32_t fast;       // body (b) of the grid's index search (the table certified nondecreasing)
};
struct MiQuadWork {
    int32_t prob, nh;   // problem id; intervals of this item: 1 or 2
    double a[2], b[2];
};

template <int BPS, int KIND>
__device__ __forceinline__ double mi_quad_point(const MiQuadProblem &pr, double x, const MiLds &lt) {
    constexpr int M = 1 << BPS;
    const DemapTables &t = *pr.tab;
    auto ex = [&](double v) { return g_exp_wave(v, lt); };
    auto lg = [&](double v) { return g_log2_full(v, lt); };
    if constexpr (KIND == kMiQuadXY) {
        return mi_xy_arg(t, M, x, ex, lg);
    } else {
        double yh[M];   // y_hat of every hypothesis: read M^2 times, M^3 exp between
        const GridView g = pr.g;
#pragma unroll 1
        for (int i = 0; i < M; ++i) {
            // search_target with the problem's configuration
            const double val = ((pr.sign >> i) & 1u) ? t.Fthr[i + 1] - x * t.dF[i] : x * t.dF[i] + t.Fthr[i];
            yh[i] = pr.fast ? grid_g_inv_val<true>(g, g.coarse, val) : grid_g_inv_val<false>(g, g.coarse, val);
        }
        return mi_base_arg(t, pr.pX, M, [&](int i) { return yh[i]; }, ex, lg);
    }
}

__device__ __forceinline__ void stage_mi_lds(MiLds &lt) {
    for (int i = threadIdx.x; i < 128; i += blockDim.x) lt.ex[i] = kGlibcConst.ex[i];
    for (int i = threadIdx.x; i < 64; i += blockDim.x) lt.e[i] = kGlibcLog2Const.e[i];
    __syncthreads();
}

template <int BPS, int KIND>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8)))
k_mi_quad(const MiQuadProblem *__restrict__ probs, int nprob, const MiQuadWork *__restrict__ work, int nwork,
          double *__restrict__ out, double *__restrict__ dbg) {
    constexpr int per = KIND == kMiQuadXY ? 2 * kGk15Nodes : kGk21Nodes;   // lanes per interval: 30 / 21
    __shared__ MiLds lt;
    __shared__ double vals[4][64];
    stage_mi_lds(lt);
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int it = (int)blockIdx.x * 4 + w; it < nwork; it += (int)gridDim.x * 4) {   // wave-uniform
        const int prob = __builtin_amdgcn_readfirstlane(work[it].prob);
        const int nh = __builtin_amdgcn_readfirstlane(work[it].nh);
        QR_DCHECK(prob >= 0 && prob < nprob && (nh == 1 || nh == 2), kDbgQuadProblem, prob, nh);
        const MiQuadProblem &pr = probs[prob >= 0 && prob < nprob ? prob : 0];
        const int h = lane >= per ? 1 : 0;
        const bool valid = lane < per * nh;
        const int k = valid ? lane - h * per : 0;   // node slot within the interval
        QR_DCHECK(k >= 0 && k < per, kDbgQuadNode, k, per);
        const double a = work[it].a[h], b = work[it].b[h];
        double x;
        if constexpr (KIND == kMiQuadXY) {
            const double T = gk15i_T(gk15i_x(a, b, k >> 1));
            x = valid ? ((k & 1) ? -T : T) : 0.0;
        } else {
            x = valid ? gk21_node(a, b, k) : 0.5;
        }
        const double v = mi_quad_point<BPS, KIND>(pr, x, lt);
        QR_DCHECK(lane >= 0 && lane < 64 && w >= 0 && w < 4, kDbgQuadSlot, lane, w);
        vals[w][lane] = v;
        if (dbg && valid) {   // debug: dbg[item][lane] = {abscissa, value}, lanes 0 .. per * nh - 1
            dbg[((size_t)it * 64 + lane) * 2] = x;
            dbg[((size_t)it * 64 + lane) * 2 + 1] = v;
        }
        wave_lds_fence();
        if (lane < 2) {
            double r[4] = {0.0, 0.0, 0.0, 0.0};
            if (lane < nh) {
                const double ra = work[it].a[lane], rb = work[it].b[lane];
                if constexpr (KIND == kMiQuadXY) gk15i_sums(&vals[w][lane * per], ra, rb, r);
                else gk21_sums(&vals[w][lane * per], ra, rb, r);
            }
            double *o = out + ((size_t)it * 2 + lane) * 4;
            o[0] = r[0];
            o[1] = r[1];
            o[2] = r[2];
            o[3] = r[3];
        }
        wave_lds_fence();   // the sums are taken before the next item's values land
    }
}

// The integrand itself over an array (qr_mi_integrand_device / _host): lane = abscissa, whole waves.
template <int BPS, int KIND>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8)))
k_mi_integrand(const MiQuadProblem pr, int64_t n, const double *__restrict__ x, double *__restrict__ f) {
    __shared__ MiLds lt;
    stage_mi_lds(lt);
    for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < n; base += (int64_t)gridDim.x * 256) {
        const int64_t k = base + (threadIdx.x & 63);
        const bool valid = k < n;
        const double v = mi_quad_point<BPS, KIND>(pr, valid ? x[k] : (KIND == kMiQuadXY ? 0.0 : 0.5), lt);
        if (valid) f[k] = v;
    }
}

// The grid itself (noisemapper.pyx:143-144): y[i] as numpy's linspace computes it,
// fl(fl(i * step) + y_low) with the last point set to y_high, and F = the cpdef F_Y of it.
__global__ void __launch_bounds__(256) k_grid_build(const DemapTables *__restrict__ tab, int32_t n, double y_low,
                                                    double y_high, double step, double2 *__restrict__ pairs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double y = (i == n - 1) ? y_high : (double)i * step + y_low;
    double2 p;
    p.x = public_F_Y(*tab, y);
    p.y = y;
    pairs[i] = p;
}

// matrix.pyx:55-60, frame-innermost; one lane = (check, frame).
__global__ void __launch_bounds__(256) k_syndrome(int64_t C, int ld, int B, const int32_t *__restrict__ chk_ptr,
                                                  const int32_t *__restrict__ chk_var,
                                                  const uint8_t *__restrict__ word, uint8_t *__restrict__ synd) {
    const int f = blockIdx.y * blockDim.x + threadIdx.x;
    const int64_t c = blockIdx.x;
    if (c >= C || f >= ld) return;
    uint8_t x = 0;
    if (f < B)
        for (int k = chk_ptr[c]; k < chk_ptr[c + 1]; ++k) x ^= word[(size_t)chk_var[k] * ld + f];
    synd[(size_t)c * ld + f] = x;
}

// utils.pyx:27-40 (lappr >= 0 decides bit 0) over the first K nodes, then the
// per-frame bookkeeping of reconciliation.pyx:149-157.
__global__ void __launch_bounds__(256) k_count_errors(int B, int ld, int64_t K, int64_t kpb,
                                                      const double *__restrict__ fin,
                                                      const uint8_t *__restrict__ word, int32_t *__restrict__ ferr) {
    const int f = blockIdx.y * blockDim.x + threadIdx.x;
    if (f >= B) return;
    const int64_t v0 = (int64_t)blockIdx.x * kpb;
    const int64_t v1 = (v0 + kpb < K) ? v0 + kpb : K;
    int32_t cnt = 0;
    for (int64_t v = v0; v < v1; ++v) {
        const uint8_t w = word[v * ld + f];
        cnt += (fin[v * ld + f] >= 0) ? w : 1 - w;
    }
    if (cnt) atomicAdd(&ferr[f], cnt);
}

__global__ void k_count_finish(int B, const int32_t *__restrict__ ferr, const uint8_t *__restrict__ success,
                               const int32_t *__restrict__ iters, unsigned long long *counters) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long be = 0, fe = 0, su = 0, it = 0, fr = 0;
    if (f < B) {
        be = (unsigned long long)ferr[f];
        fe = ferr[f] ? 1 : 0;
        su = success[f] ? 1 : 0;
        it = success[f] ? (unsigned long long)iters[f] : 0;
        fr = 1;
    }
    // wave-level sums, then one atomic per wave per counter
    for (int off = 32; off > 0; off >>= 1) {
        be += __shfl_down(be, off);
        fe += __shfl_down(fe, off);
        su += __shfl_down(su, off);
        it += __shfl_down(it, off);
        fr += __shfl_down(fr, off);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&counters[0], be);
        atomicAdd(&counters[1], fe);
        atomicAdd(&counters[2], su);
        atomicAdd(&counters[3], it);
        atomicAdd(&counters[4], fr);
    }
}

static int check_shape(int B, int ld, int64_t S) {
    if (B <= 0 || ld < B || ld % kWave) return set_error(QR_EVALUE, "need 0 < B <= ld, ld %% 64 == 0 (B=%d ld=%d)", B, ld);
    if (S <= 0) return set_error(QR_EVALUE, "S must be positive");
    return QR_OK;
}

int demap_batch_device(const qr_demap *dm, int B, int ld, int64_t S, const double *n, const int64_t *j, double alpha,
                       double *lappr, hipStream_t s) {
    int rc = check_shape(B, ld, S);
    if (rc) return rc;
    DeviceGuard g(dm->device);
    ProfScope ps("demap", s);
    const bool fast = g_demap_fast.load() != 0;
    const int hyp = g_demap_hyp.load();
    if (fast && hyp >= 1 && ld % kWave == 0 &&
        dm->h.bps <= kDemapWaveMaxBps) {
        const int64_t items = S * (ld / kWave);
        launch_demap_wave(dm->h.bps, demap_wave_grid(dm->device, (items + 3) / 4), s, dm, B, ld, S, n, j, alpha, lappr);
    } else {
        const int64_t items = S * ld;
        launch_demap_bps(dm->h.bps, fast, (unsigned)((items + 255) / 256), s, dm, B, ld, S, n, j, alpha, lappr);
    }
    QR_LAUNCH_CHECK();
    return QR_OK;
}

static GridView grid_view(const qr_demap *dm) {
    const DemapGrid &gr = dm->grid;
    return GridView{gr.d_pairs, gr.d_coarse, gr.n, gr.nc, gr.seg_shift, gr.h_pairs.back().x, gr.h_pairs.back().y};
}

// body (b) of the index search: the table certified nondecreasing and the knob on
static bool grid_fast(const qr_demap *dm) { return dm->grid.nondecreasing && g_interp_fast.load() != 0; }

template <bool FAST>
static bool launch_demap_interp_wave(int bps, unsigned grid, size_t lds, hipStream_t st, const qr_demap *dm,
                                     const GridView &g, int B, int ld, int64_t S, const double *n, const int64_t *j,
                                     double alpha, double *lappr) {
    switch (bps) {
#define QR_DEMAP_INTERP(b) \
        case b: k_demap_interp_wave<b, FAST><<<grid, 256, lds, st>>>(dm->d_tables, g, B, ld, S, n, j, alpha, lappr); return true;
        QR_DEMAP_INTERP(1) QR_DEMAP_INTERP(2) QR_DEMAP_INTERP(3) QR_DEMAP_INTERP(4) QR_DEMAP_INTERP(5) QR_DEMAP_INTERP(6)
#undef QR_DEMAP_INTERP
        default: return false;
    }
}

int demap_simplified_batch_device(const qr_demap *dm, int B, int ld, int64_t S, const double *n, const int64_t *j,
                                  double alpha, double *lappr, hipStream_t s) {
    int rc = check_shape(B, ld, S);
    if (rc) return rc;
    if (dm->grid.n <= 0) return set_error(QR_EVALUE, "the interpolation grid has not been created (qr_demap_grid_create)");
    if (dm->h.bps > kDemapWaveMaxBps)
        return set_error(QR_EUNSUPPORTED, "the batched demapper serves bit_per_symbol <= %d (got %d)", kDemapWaveMaxBps,
                         dm->h.bps);
    DeviceGuard g(dm->device);
    ProfScope ps("demap_interp", s);
    const GridView gv = grid_view(dm);
    const int64_t items = S * (ld / kWave);
    const unsigned grid = demap_wave_grid(dm->device, (items + 3) / 4);
    if (grid_fast(dm))   // nc <= kGridMaxCoarse by construction
        launch_demap_interp_wave<true>(dm->h.bps, grid, (size_t)gv.nc * sizeof(double), s, dm, gv, B, ld, S, n, j, alpha,
                                       lappr);
    else
        launch_demap_interp_wave<false>(dm->h.bps, grid, 0, s, dm, gv, B, ld, S, n, j, alpha, lappr);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

template <bool FAST>
static bool launch_mi_terms(int bps, unsigned grid, size_t lds, hipStream_t st, const qr_demap *dm, const GridView &g,
                            unsigned which, int B, int ld, int64_t S, const int64_t *x, const double *y, double *terms) {
    switch (bps) {
#define QR_MI_TERMS(b) \
        case b: k_mi_terms<b, FAST><<<grid, 256, lds, st>>>(dm->d_tables, dm->d_mtab, g, dm->d_mi, which, B, ld, S, x, y, terms); return true;
        QR_MI_TERMS(1) QR_MI_TERMS(2) QR_MI_TERMS(3) QR_MI_TERMS(4) QR_MI_TERMS(5) QR_MI_TERMS(6)
#undef QR_MI_TERMS
        default: return false;
    }
}

// the two launches of the estimator on stream s; the checks are the caller's
static int mi_launch(const qr_demap *dm, unsigned which, int B, int ld, int64_t S, const int64_t *x, const double *y,
                     double *info, double *terms, hipStream_t s) {
    const GridView gv = grid_view(dm);
    {
        ProfScope ps("mi_terms", s);
        const int64_t items = S * (ld / kWave);
        const unsigned grid = demap_wave_grid(dm->device, (items + 3) / 4);
        if (grid_fast(dm))   // nc <= kGridMaxCoarse by construction
            launch_mi_terms<true>(dm->h.bps, grid, (size_t)gv.nc * sizeof(double), s, dm, gv, which, B, ld, S, x, y, terms);
        else
            launch_mi_terms<false>(dm->h.bps, grid, 0, s, dm, gv, which, B, ld, S, x, y, terms);
        QR_LAUNCH_CHECK();
    }
    if (info) {
        ProfScope ps("mi_sum", s);
        k_mi_sum<<<dim3((unsigned)(ld / kWave), 3), 64, 0, s>>>(which, B, ld, S, terms, info);
        QR_LAUNCH_CHECK();
    }
    return QR_OK;
}

static int mi_ready(const qr_demap *dm) {
    if (dm->grid.n <= 0) return set_error(QR_EVALUE, "the interpolation grid has not been created (qr_demap_grid_create)");
    if (!dm->d_mi) return set_error(QR_EVALUE, "the mutual-information tables have not been created (qr_demap_mi_tables)");
    return QR_OK;
}

// ---- quadrature evaluators: launches
template <int KIND>
static bool launch_mi_quad(int bps, unsigned grid, hipStream_t st, const MiQuadProblem *probs, int nprob,
                           const MiQuadWork *work, int nwork, double *out, double *dbg = nullptr) {
    switch (bps) {
#define QR_MI_QUAD(b) \
        case b: k_mi_quad<b, KIND><<<grid, 256, 0, st>>>(probs, nprob, work, nwork, out, dbg); return true;
        QR_MI_QUAD(1) QR_MI_QUAD(2) QR_MI_QUAD(3) QR_MI_QUAD(4) QR_MI_QUAD(5) QR_MI_QUAD(6)
#undef QR_MI_QUAD
        default: return false;
    }
}

template <int KIND>
static bool launch_mi_integrand(int bps, unsigned grid, hipStream_t st, const MiQuadProblem &pr, int64_t n,
                                const double *x, double *f) {
    switch (bps) {
#define QR_MI_INTEGRAND(b) \
        case b: k_mi_integrand<b, KIND><<<grid, 256, 0, st>>>(pr, n, x, f); return true;
        QR_MI_INTEGRAND(1) QR_MI_INTEGRAND(2) QR_MI_INTEGRAND(3) QR_MI_INTEGRAND(4) QR_MI_INTEGRAND(5) QR_MI_INTEGRAND(6)
#undef QR_MI_INTEGRAND
        default: return false;
    }
}

static uint64_t sign_mask(const uint8_t *cfg, int M) {
    uint64_t m = 0;
    for (int i = 0; i < M; ++i) m |= (uint64_t)(cfg[i] ? 1u : 0u) << i;
    return m;
}

static MiQuadProblem quad_problem(const qr_demap *dm, const double *d_pX, const uint8_t *cfg) {
    return MiQuadProblem{dm->d_tables, grid_view(dm), d_pX, sign_mask(cfg ? cfg : dm->h.sign, dm->h.M),
                         grid_fast(dm) ? 1 : 0};
}

// the checks every quadrature entry makes of one handle
static int quad_ready(const qr_demap *dm, int kind) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    if (kind != kMiQuadBase && kind != kMiQuadXY) return set_error(QR_EVALUE, "kind must be 0 (base scheme) or 1 (X;Y)");
    if (dm->h.bps > kDemapWaveMaxBps)
        return set_error(QR_EUNSUPPORTED, "the quadrature evaluators serve bit_per_symbol <= %d (got %d)", kDemapWaveMaxBps,
                         dm->h.bps);
    if (dm->grid.n <= 0)   // both kinds (the X;Y integrand does not read it)
        return set_error(QR_EVALUE, "the interpolation grid has not been created (qr_demap_grid_create)");
    return QR_OK;
}

static int mi_integrand_launch(const qr_demap *dm, int kind, int64_t n, const double *d_x, double *d_f, hipStream_t s) {
    const MiQuadProblem pr = quad_problem(dm, dm->d_mi, nullptr);   // p_Xhat: the head of the handle's MI tables
    ProfScope ps("mi_integrand", s);
    const unsigned grid = demap_wave_grid(dm->device, (n + 255) / 256);
    if (kind == kMiQuadBase) launch_mi_integrand<kMiQuadBase>(dm->h.bps, grid, s, pr, n, d_x, d_f);
    else launch_mi_integrand<kMiQuadXY>(dm->h.bps, grid, s, pr, n, d_x, d_f);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

// device memory of one qr_mi_quad_batch call
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
};

// {rounds, launches, work items, host bookkeeping ns, wall ns} of this thread's last qr_mi_quad_batch
static thread_local int64_t g_quad_stats[5];

#if QR_DEBUG_ASSERT
int debug_asserts_demap(unsigned long long h[4]) {
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_dbg_demap), 4 * sizeof(unsigned long long)) != hipSuccess) return QR_EDEVICE;
    const unsigned long long z[4] = {0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_dbg_demap), z, sizeof(z)) != hipSuccess) return QR_EDEVICE;
    return QR_OK;
}
#endif

}  // namespace qr

// ===================================================================== C-ABI
using namespace qr;

extern "C" {

#if QR_EXPERIMENT_CLOCK
// Diagnostic builds only (not in include/qamr.h): out = {sum cycles, sum ticks, workgroups} of the
// wave-private demapper's stamped launches since the last call.
QR_API int qr_debug_clock_demap(int64_t *out) {
    unsigned long long h[3] = {0, 0, 0};
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(qr::g_clk_demap), sizeof(h)) != hipSuccess) return QR_EDEVICE;
    const unsigned long long z[3] = {0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(qr::g_clk_demap), z, sizeof(z)) != hipSuccess) return QR_EDEVICE;
    for (int i = 0; i < 3; ++i) out[i] = (int64_t)h[i];
    return QR_OK;
}
#endif

int qr_demap_create(int32_t bps, const double *constellation, const double *probabilities, const double *thresholds,
                    double noise_var, const uint8_t *sign_config, int32_t device, qr_demap **out) {
    if (!out) return set_error(QR_EVALUE, "null output handle");
    *out = nullptr;
    DemapTables t;  // host_build.hpp (noisemapper.pyx:103-236 + the fast search's tables)
    std::vector<double2> quant;
    std::vector<double> ftab;
    std::string err;
    if (int rc = build_demap_host(bps, constellation, probabilities, thresholds, noise_var, sign_config, t, quant, ftab,
                                  err))
        return set_error(rc, "%s", err.c_str());
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return set_error(QR_EDEVICE, "no HIP device available (libqamr has no CPU fallback)");
    if (device < 0 || device >= ndev) return set_error(QR_EVALUE, "device %d out of range", device);
    qr_demap *dm = new qr_demap();
    dm->h = t;
    std::vector<MathTables> mt(1);
    build_math_tables(&mt[0]);
    dm->device = device;
    dm->scratch.device = device;
    DeviceGuard g(device);
    hipError_t e = hipSuccess;
    if (!quant.empty()) {
        e = hipMalloc((void **)&dm->d_quant, quant.size() * sizeof(double2));
        if (e == hipSuccess)
            e = hipMemcpy(dm->d_quant, quant.data(), quant.size() * sizeof(double2), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && !ftab.empty()) {
        e = hipMalloc((void **)&dm->d_ftab, ftab.size() * sizeof(double));
        if (e == hipSuccess)
            e = hipMemcpy(dm->d_ftab, ftab.data(), ftab.size() * sizeof(double), hipMemcpyHostToDevice);
    }
    t.quant = dm->d_quant;  // device pointers in the device copy
    t.ftab = dm->d_ftab;
    if (e == hipSuccess) e = hipMalloc((void **)&dm->d_mtab, sizeof(MathTables));
    if (e == hipSuccess) e = hipMemcpy(dm->d_mtab, mt.data(), sizeof(MathTables), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&dm->d_tables, sizeof(DemapTables));
    if (e == hipSuccess) e = hipMemcpy(dm->d_tables, &t, sizeof(DemapTables), hipMemcpyHostToDevice);
    t.quant = nullptr;      // the host copy never dereferences them
    t.ftab = nullptr;
    if (e != hipSuccess) {
        (void)hipFree(dm->d_tables);
        (void)hipFree(dm->d_mtab);
        (void)hipFree(dm->d_quant);
        (void)hipFree(dm->d_ftab);
        delete dm;
        return hip_fail(e, "qr_demap_create upload", __FILE__, __LINE__);
    }
    *out = dm;
    return QR_OK;
}

int qr_demap_destroy(qr_demap *dm) {
    if (!dm) return QR_OK;
    {
        DeviceGuard g(dm->device);
        (void)hipFree(dm->d_tables);
        (void)hipFree(dm->d_mtab);
        (void)hipFree(dm->d_quant);
        (void)hipFree(dm->d_ftab);
        (void)hipFree(dm->grid.d_pairs);
        (void)hipFree(dm->grid.d_coarse);
        (void)hipFree(dm->d_mi);
    }
    delete dm;
    return QR_OK;
}

int qr_demap_grid_create(qr_demap *dm, double trunkation_threshold, int64_t n_intervals_per_step, double step) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    if (!(trunkation_threshold > 0) || n_intervals_per_step <= 0 || !(step > 0))
        return set_error(QR_EVALUE, "grid: need trunkation_threshold > 0, n_intervals_per_step > 0, step > 0");
    std::lock_guard<std::mutex> lk(dm->scratch.mu);
    DemapGrid &gr = dm->grid;
    if (gr.n > 0 && gr.trunc == trunkation_threshold && gr.nips == n_intervals_per_step && gr.step == step &&
        gr.seg_req == g_interp_seg.load())
        return QR_OK;
    const DemapTables &t = dm->h;
    const double sigma = sqrt(t.two_s2 / 2);   // noisemapper.pyx:132 (two_s2 / 2 = noise_var, exactly)
    double y_low, y_high;
    if (trunkation_threshold > 1.) {           // :135-137
        y_low = t.a[0] * 10;
        y_high = t.a[t.M - 1] * 10;
    } else {                                   // :138-141
        const double tmp = sqrt(-2. * log(trunkation_threshold)) * sigma;
        y_high = t.a[t.M - 1] + tmp;
        y_low = t.a[0] - tmp;
    }
    const double np = ceil((y_high - y_low) * (double)n_intervals_per_step / step) + 1;   // :142
    if (!(np >= 2 && np <= (double)(1 << 26)))
        return set_error(QR_EVALUE, "grid: %g points (need 2 .. 2^26)", np);
    const int32_t n = (int32_t)np;
    int32_t seg_shift = g_interp_seg.load();
    seg_shift = seg_shift < 1 ? 1 : seg_shift > 20 ? 20 : seg_shift;
    while (((n - 1) >> seg_shift) + 1 > kGridMaxCoarse) ++seg_shift;
    const int32_t nc = ((n - 1) >> seg_shift) + 1;
    const double lin_step = (y_high - y_low) / (double)(n - 1);   // numpy.linspace: delta / div
    DeviceGuard g(dm->device);
    double2 *d_pairs = nullptr;
    double *d_coarse = nullptr;
    std::vector<double2> h((size_t)n);
    std::vector<double> coarse((size_t)nc);
    hipError_t e = hipMalloc((void **)&d_pairs, (size_t)n * sizeof(double2));
    if (e == hipSuccess) e = hipMalloc((void **)&d_coarse, (size_t)nc * sizeof(double));
    if (e == hipSuccess) {
        k_grid_build<<<(unsigned)((n + 255) / 256), 256>>>(dm->d_tables, n, y_low, y_high, lin_step, d_pairs);
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
    if (dm->grid.n <= 0) return set_error(QR_EVALUE, "the interpolation grid has not been created (qr_demap_grid_create)");
    if (n_points) *n_points = dm->grid.n;
    if (nondecreasing) *nondecreasing = dm->grid.nondecreasing;
    return QR_OK;
}

int qr_demap_grid_host(const qr_demap *dm, double *y, double *F) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    if (dm->grid.n <= 0) return set_error(QR_EVALUE, "the interpolation grid has not been created (qr_demap_grid_create)");
    for (int32_t r = 0; r < dm->grid.n; ++r) {
        if (F) F[r] = dm->grid.h_pairs[r].x;
        if (y) y[r] = dm->grid.h_pairs[r].y;
    }
    return QR_OK;
}

int qr_g_inv_host(const qr_demap *dm, int64_t n, const double *n_hat, const int64_t *i, double *y_hat) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    if (dm->grid.n <= 0) return set_error(QR_EVALUE, "the interpolation grid has not been created (qr_demap_grid_create)");
    if (n < 0) return set_error(QR_EVALUE, "negative size");
    if (n == 0) return QR_OK;
    if (!n_hat || !i || !y_hat) return set_error(QR_EVALUE, "null pointer argument");
    DeviceGuard g(dm->device);
    std::lock_guard<std::mutex> lk(dm->scratch.mu);
    double *d_n, *d_y;
    int64_t *d_i;
    if (int rc = dm->scratch.take(&d_n, (size_t)n, &d_i, (size_t)n, &d_y, (size_t)n)) return rc;
    QR_HIP(hipMemcpy(d_n, n_hat, (size_t)n * 8, hipMemcpyHostToDevice));
    QR_HIP(hipMemcpy(d_i, i, (size_t)n * 8, hipMemcpyHostToDevice));
    const GridView gv = grid_view(dm);
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (grid_fast(dm)) k_g_inv_interp<true><<<grid, 256>>>(dm->d_tables, gv, n, d_n, d_i, d_y);
    else k_g_inv_interp<false><<<grid, 256>>>(dm->d_tables, gv, n, d_n, d_i, d_y);
    QR_LAUNCH_CHECK();
    QR_HIP(hipMemcpy(y_hat, d_y, (size_t)n * 8, hipMemcpyDeviceToHost));
    return QR_OK;
}

int qr_demap_simplified_host(const qr_demap *dm, int64_t S, const double *n, const int64_t *j, double *lappr) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    if (dm->grid.n <= 0) return set_error(QR_EVALUE, "the interpolation grid has not been created (qr_demap_grid_create)");
    if (S < 0) return set_error(QR_EVALUE, "negative size");
    if (S == 0) return QR_OK;
    if (!n || !j || !lappr) return set_error(QR_EVALUE, "null pointer argument");
    DeviceGuard g(dm->device);
    std::lock_guard<std::mutex> lk(dm->scratch.mu);
    const int bps = dm->h.bps;
    double *d_n, *d_l;
    int64_t *d_j;
    if (int rc = dm->scratch.take(&d_n, (size_t)S, &d_j, (size_t)S, &d_l, (size_t)S * bps)) return rc;
    QR_HIP(hipMemcpy(d_n, n, (size_t)S * 8, hipMemcpyHostToDevice));
    QR_HIP(hipMemcpy(d_j, j, (size_t)S * 8, hipMemcpyHostToDevice));
    const GridView gv = grid_view(dm);
    const unsigned grid = (unsigned)((S + 255) / 256);
    {
        ProfScope ps("demap_interp", nullptr);
        if (grid_fast(dm)) k_demap_interp_lane<true><<<grid, 256>>>(dm->d_tables, gv, S, d_n, d_j, d_l);
        else k_demap_interp_lane<false><<<grid, 256>>>(dm->d_tables, gv, S, d_n, d_j, d_l);
        QR_LAUNCH_CHECK();
    }
    QR_HIP(hipMemcpy(lappr, d_l, (size_t)S * bps * 8, hipMemcpyDeviceToHost));
    return QR_OK;
}

int qr_demap_simplified_batch_device(const qr_demap *dm, int32_t B, int32_t ld, int64_t S, const double *d_n,
                                     const int64_t *d_j, double alpha, double *d_lappr, void *stream) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    return demap_simplified_batch_device(dm, B, ld, S, d_n, d_j, alpha, d_lappr, (hipStream_t)stream);
}

// ---- Monte-Carlo mutual information (mutual_information.pyx:218-297) ----
int qr_demap_mi_tables(qr_demap *dm, const double *p_xhat, const double *fwrd) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    if (!p_xhat || !fwrd) return set_error(QR_EVALUE, "null pointer argument");
    const size_t M = (size_t)dm->h.M, n = M + M * M;
    std::lock_guard<std::mutex> lk(dm->scratch.mu);
    DeviceGuard g(dm->device);
    if (!dm->d_mi) QR_HIP(hipMalloc((void **)&dm->d_mi, n * sizeof(double)));
    QR_HIP(hipDeviceSynchronize());   // a replacement: no launch that reads the old values is pending
    QR_HIP(hipMemcpy(dm->d_mi, p_xhat, M * sizeof(double), hipMemcpyHostToDevice));
    QR_HIP(hipMemcpy(dm->d_mi + M, fwrd, M * M * sizeof(double), hipMemcpyHostToDevice));
    return QR_OK;
}

int qr_mi_workspace_size(int32_t ld, int64_t S, size_t *bytes) {
    if (!bytes) return set_error(QR_EVALUE, "null output pointer");
    *bytes = 0;
    if (int rc = check_shape(ld > 0 ? ld : 1, ld, S)) return rc;
    *bytes = align_up((size_t)3 * (size_t)S * (size_t)ld * sizeof(double), 256);
    return QR_OK;
}

int qr_mi_montecarlo_device(const qr_demap *dm, uint32_t which_mask, int32_t B, int32_t ld, int64_t S,
                            const int64_t *d_x, const double *d_y, double *d_info, double *d_terms, void *d_workspace,
                            size_t workspace_bytes, void *stream) {
    if (int rc = check_shape(B, ld, S)) return rc;   // S < 1: the reference divides by zero
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    if (which_mask & ~kMiAll) return set_error(QR_EVALUE, "which_mask has bits beyond the three quantities");
    if (!d_x || !d_y || !d_info) return set_error(QR_EVALUE, "null pointer argument");
    if (int rc = mi_ready(dm)) return rc;
    if (dm->h.bps > kDemapWaveMaxBps)
        return set_error(QR_EUNSUPPORTED, "the batched estimator serves bit_per_symbol <= %d (got %d)", kDemapWaveMaxBps,
                         dm->h.bps);
    if (!d_terms) {
        size_t need = 0;
        (void)qr_mi_workspace_size(ld, S, &need);
        if (!d_workspace || workspace_bytes < need)
            return set_error(QR_EVALUE, "workspace too small: %zu bytes, need %zu (qr_mi_workspace_size)", workspace_bytes,
                             need);
        d_terms = (double *)d_workspace;
    }
    DeviceGuard g(dm->device);
    return mi_launch(dm, which_mask, B, ld, S, d_x, d_y, d_info, d_terms, (hipStream_t)stream);
}

// One block from host memory.  The per-sample kernel is elementwise, so the N samples are laid
// along the frame axis as ONE sample row of N "blocks" (S = 1, ld = N rounded up to 64); the
// block's own sums (:245-297) are then taken here, in sample order, on the terms copied back.
int qr_mi_montecarlo_host(const qr_demap *dm, int64_t N, const int64_t *x, const double *y, const uint8_t *which,
                          double *out, double *terms) {
    if (N < 1) return set_error(QR_EVALUE, "N must be positive (the reference divides by N)");
    if (N > (int64_t)1 << 30) return set_error(QR_EVALUE, "N too large for one host block");
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    if (!x || !y || !out) return set_error(QR_EVALUE, "null pointer argument");
    if (int rc = mi_ready(dm)) return rc;
    if (dm->h.bps > kDemapWaveMaxBps)
        return set_error(QR_EUNSUPPORTED, "the estimator serves bit_per_symbol <= %d (got %d)", kDemapWaveMaxBps, dm->h.bps);
    const unsigned mask = which ? (which[0] ? kMiXXhat : 0u) | (which[1] ? kMiXY : 0u) | (which[2] ? kMiXNXhat : 0u) : kMiAll;
    const int ld = (int)align_up((size_t)N, kWave);
    DeviceGuard g(dm->device);
    std::lock_guard<std::mutex> lk(dm->scratch.mu);
    int64_t *d_x;
    double *d_y, *d_t;
    if (int rc = dm->scratch.take(&d_x, (size_t)ld, &d_y, (size_t)ld, &d_t, (size_t)3 * ld)) return rc;
    QR_HIP(hipMemcpy(d_x, x, (size_t)N * 8, hipMemcpyHostToDevice));
    QR_HIP(hipMemcpy(d_y, y, (size_t)N * 8, hipMemcpyHostToDevice));
    if (int rc = mi_launch(dm, mask, (int)N, ld, 1, d_x, d_y, nullptr, d_t, nullptr)) return rc;
    std::vector<double> h((size_t)N);
    for (int q = 0; q < 3; ++q) {
        double acc = 0.0;
        if ((mask >> q) & 1u) {
            QR_HIP(hipMemcpy(h.data(), d_t + (size_t)q * ld, (size_t)N * 8, hipMemcpyDeviceToHost));
            for (int64_t p = 0; p < N; ++p) acc = q == 2 ? acc - h[(size_t)p] : acc + h[(size_t)p];
        } else {
            std::fill(h.begin(), h.end(), 0.0);
        }
        if (terms) memcpy(terms + (size_t)q * N, h.data(), (size_t)N * 8);
        out[q] = acc / (double)N;
    }
    return QR_OK;
}

int qr_log2_host(int64_t n, const double *x, double *out) {
    if (n < 0) return set_error(QR_EVALUE, "negative size");
    if (n == 0) return QR_OK;
    if (!x || !out) return set_error(QR_EVALUE, "null pointer argument");
    double *d_x = nullptr, *d_o = nullptr;
    hipError_t e = hipMalloc((void **)&d_x, (size_t)n * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&d_o, (size_t)n * 8);
    if (e == hipSuccess) e = hipMemcpy(d_x, x, (size_t)n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        k_log2<<<(unsigned)((n + 255) / 256), 256>>>(n, d_x, d_o);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_o, (size_t)n * 8, hipMemcpyDeviceToHost);
    (void)hipFree(d_x);
    (void)hipFree(d_o);
    if (e != hipSuccess) return hip_fail(e, "qr_log2_host", __FILE__, __LINE__);
    return QR_OK;
}

// ---- quadrature evaluators (mutual_information.pyx:43-148, :175-208) ----
int qr_mi_integrand_device(const qr_demap *dm, int32_t kind, int64_t n, const double *d_x, double *d_f, void *stream) {
    if (int rc = quad_ready(dm, kind)) return rc;
    if (n < 0) return set_error(QR_EVALUE, "negative size");
    if (kind == kMiQuadBase && !dm->d_mi)
        return set_error(QR_EVALUE, "the mutual-information tables have not been created (qr_demap_mi_tables)");
    if (n == 0) return QR_OK;
    if (!d_x || !d_f) return set_error(QR_EVALUE, "null pointer argument");
    DeviceGuard g(dm->device);
    return mi_integrand_launch(dm, kind, n, d_x, d_f, (hipStream_t)stream);
}

int qr_mi_integrand_host(const qr_demap *dm, int32_t kind, int64_t n, const double *x, double *f) {
    if (int rc = quad_ready(dm, kind)) return rc;
    if (n < 0) return set_error(QR_EVALUE, "negative size");
    if (kind == kMiQuadBase && !dm->d_mi)
        return set_error(QR_EVALUE, "the mutual-information tables have not been created (qr_demap_mi_tables)");
    if (n == 0) return QR_OK;
    if (!x || !f) return set_error(QR_EVALUE, "null pointer argument");
    DeviceGuard g(dm->device);
    std::lock_guard<std::mutex> lk(dm->scratch.mu);
    double *d_x, *d_f;
    if (int rc = dm->scratch.take(&d_x, (size_t)n, &d_f, (size_t)n)) return rc;
    QR_HIP(hipMemcpy(d_x, x, (size_t)n * 8, hipMemcpyHostToDevice));
    if (int rc = mi_integrand_launch(dm, kind, n, d_x, d_f, nullptr)) return rc;
    QR_HIP(hipMemcpy(f, d_f, (size_t)n * 8, hipMemcpyDeviceToHost));
    return QR_OK;
}

int qr_mi_quad_batch(const qr_demap *const *dms, const double *p_xhat, const uint8_t *sign_cfg, int32_t P, int32_t kind,
                     double epsabs, double epsrel, int32_t limit, double *result, double *abserr, int32_t *neval,
                     int32_t *ier, void *stream) {
    using clk = std::chrono::steady_clock;
    const auto t_begin = clk::now();
    for (int64_t &v : g_quad_stats) v = 0;
    if (P < 0) return set_error(QR_EVALUE, "negative problem count");
    if (limit < 1) return set_error(QR_EVALUE, "limit must be at least 1 (got %d)", limit);
    if (kind != kMiQuadBase && kind != kMiQuadXY) return set_error(QR_EVALUE, "kind must be 0 (base scheme) or 1 (X;Y)");
    if (P == 0) return QR_OK;
    if (!dms || !result || !abserr || !neval || !ier) return set_error(QR_EVALUE, "null pointer argument");
    if (kind == kMiQuadBase && !p_xhat) return set_error(QR_EVALUE, "the base-scheme integrals need p_xhat");
    for (int32_t i = 0; i < P; ++i) {
        if (int rc = quad_ready(dms[i], kind)) return rc;
        if (dms[i]->h.bps != dms[0]->h.bps)
            return set_error(QR_EVALUE, "the handles of one batch must share bit_per_symbol (problem %d has %d, problem 0 %d)",
                             i, dms[i]->h.bps, dms[0]->h.bps);
        if (dms[i]->device != dms[0]->device) return set_error(QR_EVALUE, "the handles of one batch must share a device");
    }
    const int bps = dms[0]->h.bps, M = dms[0]->h.M, device = dms[0]->device;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard g(device);
    DevBuf b_prob, b_px, b_work, b_out;
    QR_HIP(b_prob.alloc((size_t)P * sizeof(MiQuadProblem)));
    QR_HIP(b_px.alloc(kind == kMiQuadBase ? (size_t)P * M * sizeof(double) : 0));
    QR_HIP(b_work.alloc((size_t)P * sizeof(MiQuadWork)));
    QR_HIP(b_out.alloc((size_t)P * 8 * sizeof(double)));
    std::vector<MiQuadProblem> probs((size_t)P);
    for (int32_t i = 0; i < P; ++i)
        probs[(size_t)i] = quad_problem(dms[i], kind == kMiQuadBase ? (const double *)b_px.p + (size_t)i * M : nullptr,
                                        sign_cfg ? sign_cfg + (size_t)i * M : nullptr);
    QR_HIP(hipMemcpyAsync(b_prob.p, probs.data(), (size_t)P * sizeof(MiQuadProblem), hipMemcpyHostToDevice, st));
    if (kind == kMiQuadBase)
        QR_HIP(hipMemcpyAsync(b_px.p, p_xhat, (size_t)P * M * sizeof(double), hipMemcpyHostToDevice, st));
    // both kinds run dqagse on [0, 1]: QAGS on the integral's own range, QAGI (inf = 2) on the transformed one
    std::vector<QuadState> qs((size_t)P);
    std::vector<int32_t> active;
    for (int32_t i = 0; i < P; ++i) {
        qs[(size_t)i].start(0.0, 1.0, epsabs, epsrel, limit, kind == kMiQuadXY);
        if (!qs[(size_t)i].done) active.push_back(i);
    }
    std::vector<MiQuadWork> work;
    std::vector<double> out;
    int64_t host_ns = 0;
    while (!active.empty()) {
        auto t0 = clk::now();
        const int nwork = (int)active.size();
        work.resize((size_t)nwork);
        out.resize((size_t)nwork * 8);
        for (int k = 0; k < nwork; ++k) {
            MiQuadWork &wk = work[(size_t)k];
            wk.prob = active[(size_t)k];
            wk.nh = qs[(size_t)wk.prob].pending(wk.a, wk.b);
            if (wk.nh == 1) { wk.a[1] = wk.a[0]; wk.b[1] = wk.b[0]; }
        }
        host_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(clk::now() - t0).count();
        QR_HIP(hipMemcpyAsync(b_work.p, work.data(), (size_t)nwork * sizeof(MiQuadWork), hipMemcpyHostToDevice, st));
        {
            ProfScope ps("mi_quad", st);
            const unsigned grid = demap_wave_grid(device, (nwork + 3) / 4);
            if (kind == kMiQuadBase)
                launch_mi_quad<kMiQuadBase>(bps, grid, st, (const MiQuadProblem *)b_prob.p, P, (const MiQuadWork *)b_work.p,
                                            nwork, (double *)b_out.p);
            else
                launch_mi_quad<kMiQuadXY>(bps, grid, st, (const MiQuadProblem *)b_prob.p, P, (const MiQuadWork *)b_work.p,
                                          nwork, (double *)b_out.p);
            QR_LAUNCH_CHECK();
        }
        QR_HIP(hipMemcpyAsync(out.data(), b_out.p, (size_t)nwork * 8 * sizeof(double), hipMemcpyDeviceToHost, st));
        QR_HIP(hipStreamSynchronize(st));
        t0 = clk::now();
        size_t keep = 0;
        for (int k = 0; k < nwork; ++k) {
            QuadState &q = qs[(size_t)active[(size_t)k]];
            double *r = &out[(size_t)k * 8];
            quad_rule_tail(r);
            if (work[(size_t)k].nh == 2) quad_rule_tail(r + 4);
            q.feed(r, r + 4);
            if (!q.done) active[keep++] = active[(size_t)k];
        }
        active.resize(keep);
        host_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(clk::now() - t0).count();
        g_quad_stats[0] += 1;
        g_quad_stats[1] += 1;
        g_quad_stats[2] += nwork;
    }
    for (int32_t i = 0; i < P; ++i) {
        const QuadState &q = qs[(size_t)i];
        result[i] = q.result;
        abserr[i] = q.abserr;
        neval[i] = q.neval;
        ier[i] = q.ier;
    }
    g_quad_stats[3] = host_ns;
    g_quad_stats[4] = std::chrono::duration_cast<std::chrono::nanoseconds>(clk::now() - t_begin).count();
    return QR_OK;
}

int qr_mi_quad_rule_host(const qr_demap *dm, const double *p_xhat, const uint8_t *sign_cfg, int32_t kind, int32_t nh,
                          const double *a, const double *b, double *sums, double *nodes) {
    if (int rc = quad_ready(dm, kind)) return rc;
    if (nh != 1 && nh != 2) return set_error(QR_EVALUE, "a work item holds 1 or 2 intervals (got %d)", nh);
    if (!a || !b || !sums) return set_error(QR_EVALUE, "null pointer argument");
    if (kind == kMiQuadBase && !p_xhat) return set_error(QR_EVALUE, "the base-scheme integrand needs p_xhat");
    const int M = dm->h.M, per = kind == kMiQuadXY ? 2 * kGk15Nodes : kGk21Nodes;
    DeviceGuard g(dm->device);
    DevBuf b_prob, b_px, b_work, b_out, b_dbg;
    QR_HIP(b_prob.alloc(sizeof(MiQuadProblem)));
    QR_HIP(b_px.alloc((size_t)M * sizeof(double)));
    QR_HIP(b_work.alloc(sizeof(MiQuadWork)));
    QR_HIP(b_out.alloc(8 * sizeof(double)));
    QR_HIP(b_dbg.alloc(128 * sizeof(double)));
    const MiQuadProblem pr = quad_problem(dm, (const double *)b_px.p, sign_cfg);
    MiQuadWork wk;
    wk.prob = 0;
    wk.nh = nh;
    for (int h = 0; h < 2; ++h) {
        wk.a[h] = a[h < nh ? h : 0];
        wk.b[h] = b[h < nh ? h : 0];
    }
    QR_HIP(hipMemcpy(b_prob.p, &pr, sizeof pr, hipMemcpyHostToDevice));
    if (kind == kMiQuadBase) QR_HIP(hipMemcpy(b_px.p, p_xhat, (size_t)M * sizeof(double), hipMemcpyHostToDevice));
    QR_HIP(hipMemcpy(b_work.p, &wk, sizeof wk, hipMemcpyHostToDevice));
    QR_HIP(hipMemset(b_dbg.p, 0, 128 * sizeof(double)));
    if (kind == kMiQuadBase)
        launch_mi_quad<kMiQuadBase>(dm->h.bps, 1, nullptr, (const MiQuadProblem *)b_prob.p, 1, (const MiQuadWork *)b_work.p, 1,
                                    (double *)b_out.p, (double *)b_dbg.p);
    else
        launch_mi_quad<kMiQuadXY>(dm->h.bps, 1, nullptr, (const MiQuadProblem *)b_prob.p, 1, (const MiQuadWork *)b_work.p, 1,
                                  (double *)b_out.p, (double *)b_dbg.p);
    QR_LAUNCH_CHECK();
    QR_HIP(hipMemcpy(sums, b_out.p, (size_t)nh * 4 * sizeof(double), hipMemcpyDeviceToHost));
    if (nodes) QR_HIP(hipMemcpy(nodes, b_dbg.p, (size_t)nh * per * 2 * sizeof(double), hipMemcpyDeviceToHost));
    return QR_OK;
}

int qr_mi_quad_stats(int64_t *out) {
    if (!out) return set_error(QR_EVALUE, "null output pointer");
    for (int i = 0; i < 5; ++i) out[i] = g_quad_stats[i];
    return QR_OK;
}

int qr_quad_host(qr_quad_fn f, void *user, int32_t kind, double a, double b, double epsabs, double epsrel, int32_t limit,
                 double *result, double *abserr, int32_t *neval, int32_t *ier, int32_t *last) {
    if (!f) return set_error(QR_EVALUE, "null integrand");
    if (kind != kMiQuadBase && kind != kMiQuadXY) return set_error(QR_EVALUE, "kind must be 0 (QAGS on [a, b]) or 1 (QAGI)");
    if (limit < 1) return set_error(QR_EVALUE, "limit must be at least 1 (got %d)", limit);
    QuadState q;
    if (kind == kMiQuadXY) q.start(0.0, 1.0, epsabs, epsrel, limit, true);
    else q.start(a, b, epsabs, epsrel, limit, false);
    while (!q.done) {
        double ia[2], ib[2], r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int nh = q.pending(ia, ib);
        for (int h = 0; h < nh; ++h) {
            if (kind == kMiQuadXY) quad_rule_15i([&](double x) { return f(x, user); }, ia[h], ib[h], r + 4 * h);
            else quad_rule_21([&](double x) { return f(x, user); }, ia[h], ib[h], r + 4 * h);
            quad_rule_tail(r + 4 * h);
        }
        q.feed(r, r + 4);
    }
    if (result) *result = q.result;
    if (abserr) *abserr = q.abserr;
    if (neval) *neval = q.neval;
    if (ier) *ier = q.ier;
    if (last) *last = q.last;
    return QR_OK;
}

int qr_demap_tables(const qr_demap *dm, double *Fthr, double *dF) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    for (int i = 0; i <= dm->h.M; ++i)
        if (Fthr) Fthr[i] = dm->h.Fthr[i];
    for (int i = 0; i < dm->h.M; ++i)
        if (dF) dF[i] = dm->h.dF[i];
    return QR_OK;
}

int qr_demap_batch_device(const qr_demap *dm, int32_t B, int32_t ld, int64_t S, const double *d_n,
                          const int64_t *d_j, double alpha, double *d_lappr, void *stream) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    return demap_batch_device(dm, B, ld, S, d_n, d_j, alpha, d_lappr, (hipStream_t)stream);
}

// One array from host memory: the same kernel with B = ld = 1, i.e. one lane
// per symbol and the interleaved out[s*bps + k] layout of noisemapper.pyx:556.
int qr_demap_host(const qr_demap *dm, int64_t S, const double *n, const int64_t *j, double *lappr) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    if (S <= 0) return QR_OK;
    DeviceGuard g(dm->device);
    std::lock_guard<std::mutex> lk(dm->scratch.mu);
    const int bps = dm->h.bps;
    const size_t a = align_up(S * 8, 256), b = align_up(S * 8, 256), c = align_up(S * bps * 8, 256);
    int rc = dm->scratch.reserve(a + b + c);
    if (rc) return rc;
    char *p = (char *)dm->scratch.ptr;
    double *d_n = (double *)p;
    int64_t *d_j = (int64_t *)(p + a);
    double *d_l = (double *)(p + a + b);
    QR_HIP(hipMemcpy(d_n, n, S * 8, hipMemcpyHostToDevice));
    QR_HIP(hipMemcpy(d_j, j, S * 8, hipMemcpyHostToDevice));
    // ld = 1, B = 1: item = s, f = 0; lappr index (s*bps + k) * 1 + 0 = interleaved output.
    {
        ProfScope ps("demap", nullptr);
        launch_demap_bps(dm->h.bps, g_demap_fast.load() != 0, (unsigned)((S + 255) / 256), nullptr, dm, 1, 1, S, d_n,
                         d_j, 1.0, d_l);
        QR_LAUNCH_CHECK();
    }
    QR_HIP(hipMemcpy(lappr, d_l, S * bps * 8, hipMemcpyDeviceToHost));
    return QR_OK;
}

int qr_g_inv_search_host(const qr_demap *dm, int64_t n, const double *n_hat, const int64_t *i, double y_accuracy,
                         double *y_hat) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    if (n < 0) return set_error(QR_EVALUE, "negative size");
    if (n == 0) return QR_OK;
    if (!n_hat || !i || !y_hat) return set_error(QR_EVALUE, "null pointer argument");
    DeviceGuard g(dm->device);
    std::lock_guard<std::mutex> lk(dm->scratch.mu);
    const size_t a = align_up((size_t)n * 8, 256);
    int rc = dm->scratch.reserve(3 * a);
    if (rc) return rc;
    char *p = (char *)dm->scratch.ptr;
    double *d_n = (double *)p;
    int64_t *d_i = (int64_t *)(p + a);
    double *d_y = (double *)(p + 2 * a);
    QR_HIP(hipMemcpy(d_n, n_hat, (size_t)n * 8, hipMemcpyHostToDevice));
    QR_HIP(hipMemcpy(d_i, i, (size_t)n * 8, hipMemcpyHostToDevice));
    k_g_inv_search<<<(unsigned)((n + 255) / 256), 256>>>(dm->d_tables, dm->d_mtab, n, d_n, d_i, y_accuracy,
                                                         g_demap_fast.load() != 0, d_y);
    QR_LAUNCH_CHECK();
    QR_HIP(hipMemcpy(y_hat, d_y, (size_t)n * 8, hipMemcpyDeviceToHost));
    return QR_OK;
}

int qr_F_Y_host(const qr_demap *dm, int64_t n, const double *y, double *F) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    if (n < 0) return set_error(QR_EVALUE, "negative size");
    if (n == 0) return QR_OK;
    if (!y || !F) return set_error(QR_EVALUE, "null pointer argument");
    DeviceGuard g(dm->device);
    std::lock_guard<std::mutex> lk(dm->scratch.mu);
    const size_t a = align_up((size_t)n * 8, 256);
    int rc = dm->scratch.reserve(2 * a);
    if (rc) return rc;
    char *p = (char *)dm->scratch.ptr;
    double *d_y = (double *)p;
    double *d_F = (double *)(p + a);
    QR_HIP(hipMemcpy(d_y, y, (size_t)n * 8, hipMemcpyHostToDevice));
    k_public_F_Y<<<(unsigned)((n + 255) / 256), 256>>>(dm->d_tables, n, d_y, d_F);
    QR_LAUNCH_CHECK();
    QR_HIP(hipMemcpy(F, d_F, (size_t)n * 8, hipMemcpyDeviceToHost));
    return QR_OK;
}

int qr_bob_map_device(const qr_demap *dm, int32_t B, int32_t ld, int64_t S, const double *d_y, int64_t *d_xhat,
                      double *d_nhat, uint8_t *d_word, void *stream) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    int rc = check_shape(B, ld, S);
    if (rc) return rc;
    DeviceGuard g(dm->device);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("bob", s);
    const int64_t items = S * ld;
    k_bob<<<(unsigned)((items + 255) / 256), 256, 0, s>>>(dm->d_tables, B, ld, S, d_y, d_xhat, d_nhat, d_word);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

int qr_map_noise_device(const qr_demap *dm, int32_t B, int32_t ld, int64_t S, const double *d_y,
                        const int64_t *d_index, double *d_nhat, void *stream) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    int rc = check_shape(B, ld, S);
    if (rc) return rc;
    DeviceGuard g(dm->device);
    hipStream_t s = (hipStream_t)stream;
    const int64_t items = S * ld;
    k_map_noise<<<(unsigned)((items + 255) / 256), 256, 0, s>>>(dm->d_tables, B, ld, S, d_y, d_index, d_nhat);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

int qr_direct_lappr_device(const qr_demap *dm, double two_variance, int32_t B, int32_t ld, int64_t S,
                           const double *d_y, double *d_lappr, void *stream) {
    if (!dm) return set_error(QR_EVALUE, "null demapper");
    int rc = check_shape(B, ld, S);
    if (rc) return rc;
    DeviceGuard g(dm->device);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("direct_lappr", s);
    const int64_t items = S * ld;
    k_direct_lappr<<<(unsigned)((items + 255) / 256), 256, 0, s>>>(dm->d_tables, two_variance, B, ld, S, d_y, d_lappr);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

int qr_bare_llr_device(int32_t bps, const double *d_table, int32_t B, int32_t ld, int64_t S, const int64_t *d_x,
                       double *d_lappr, void *stream) {
    if (bps < 1 || bps > kMaxBps) return set_error(QR_EVALUE, "bit_per_symbol out of range");
    int rc = check_shape(B, ld, S);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t items = S * ld;
    k_bare_llr<<<(unsigned)((items + 255) / 256), 256, 0, s>>>(d_table, 1 << bps, bps, B, ld, S, d_x, d_lappr);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

int qr_symbols_to_bits_device(int32_t bps, int32_t B, int32_t ld, int64_t S, const int64_t *d_x, uint8_t *d_word,
                              void *stream) {
    if (bps < 1 || bps > kMaxBps) return set_error(QR_EVALUE, "bit_per_symbol out of range");
    int rc = check_shape(B, ld, S);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t items = S * ld;
    k_symbols_to_bits<<<(unsigned)((items + 255) / 256), 256, 0, s>>>(bps, B, ld, S, d_x, d_word);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

int qr_syndrome_device(const qr_code *code, int32_t B, int32_t ld, const uint8_t *d_word, uint8_t *d_synd,
                       void *stream) {
    if (!code) return set_error(QR_EVALUE, "null code");
    int rc = check_shape(B, ld, 1);
    if (rc) return rc;
    DeviceGuard g(code->device);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("syndrome", s);
    const int ft = frame_tile(ld);
    dim3 grid((unsigned)code->C, (unsigned)(ld / ft));
    k_syndrome<<<grid, ft, 0, s>>>(code->C, ld, B, code->d_chk_ptr, code->d_chk_var, d_word, d_synd);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

int qr_count_errors_device(int32_t B, int32_t ld, int64_t K, const double *d_final, const uint8_t *d_word,
                           const uint8_t *d_success, const int32_t *d_iters, int32_t *d_frame_errors,
                           int64_t *d_counters, void *stream) {
    int rc = check_shape(B, ld, 1);
    if (rc) return rc;
    if (K < 0) return set_error(QR_EVALUE, "K must be >= 0");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("count", s);
    int32_t *ferr = d_frame_errors;
    QR_HIP(hipMemsetAsync(ferr, 0, (size_t)B * 4, s));
    if (K > 0) {
        const int ft = frame_tile(ld);
        const int64_t kpb = 64;
        dim3 grid((unsigned)((K + kpb - 1) / kpb), (unsigned)(ld / ft));
        k_count_errors<<<grid, ft, 0, s>>>(B, ld, K, kpb, d_final, d_word, ferr);
        QR_LAUNCH_CHECK();
    }
    k_count_finish<<<(B + 255) / 256, 256, 0, s>>>(B, ferr, d_success, d_iters, (unsigned long long *)d_counters);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

}  // extern "C"
