// mi.hip -- the mutual-information estimator and evaluators for gfx950
// (qamreconciliation/mutual_information.pyx): the Monte-Carlo estimator (:218-297) and the
// quad-integrated evaluators (:43-148, :175-208) with their host driver.  The arithmetic is written
// once in mi_math.hpp (sample terms, integrands, quadrature rules), mi_quad.hpp (the integrator's
// decisions) and grid_interp.hpp (the interpolated g_inv); the root search of a sample's own
// hypothesis is demap_wave.hpp's.
#include <algorithm>
#include <chrono>
#include <vector>

#include "qamr_internal.hpp"
#include "demap_wave.hpp"
#include "grid_interp.hpp"
#include "mi_math.hpp"
#include "mi_quad.hpp"

namespace qr {

enum MiDebugSite {         // 10, 11: the grid's (grid_interp.hpp GridDebugSite)
    kDbgMiSymbol = 12,     // k_mi_terms: the symbol index x used to read a[] / p[] / fw outside [0, M)
    kDbgMiDecision = 13,   // k_mi_terms: Bob's hard decision x_hat outside [0, M)
    kDbgQuadNode = 14,     // k_mi_quad: the rule's node index outside [0, nodes of the rule)
    kDbgQuadSlot = 15,     // k_mi_quad: the wave's LDS value slot outside [0, 64)
    kDbgQuadProblem = 16,  // k_mi_quad: a work item's problem id outside [0, P), or its half count not 1 / 2
};

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

// the two launches of the estimator on stream s; the checks are the caller's
static int mi_launch(const qr_demap *dm, unsigned which, int B, int ld, int64_t S, const int64_t *x, const double *y,
                     double *info, double *terms, hipStream_t s) {
    const GridView gv = grid_view(dm);
    {
        ProfScope ps("mi_terms", s);
        const int64_t items = S * (ld / kWave);
        const unsigned grid = demap_wave_grid(dm->device, (items + 3) / 4);
        const size_t lds = (size_t)gv.nc * sizeof(double);   // body (b)'s coarse table: nc <= kGridMaxCoarse by construction
        const bool fast = grid_fast(dm);
        dispatch_bps(dm->h.bps, [&](auto b) {
            constexpr int BPS = decltype(b)::value;
            const auto k = fast ? k_mi_terms<BPS, true> : k_mi_terms<BPS, false>;
            k<<<grid, 256, fast ? lds : 0, s>>>(dm->d_tables, dm->d_mtab, gv, dm->d_mi, which, B, ld, S, x, y, terms);
        });
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
    if (int rc = need_grid(dm)) return rc;
    if (!dm->d_mi) return set_error(QR_EVALUE, "the mutual-information tables have not been created (qr_demap_mi_tables)");
    return QR_OK;
}

// ---- quadrature evaluators: launches
static bool launch_mi_quad(int kind, int bps, unsigned grid, hipStream_t st, const MiQuadProblem *probs, int nprob,
                           const MiQuadWork *work, int nwork, double *out, double *dbg = nullptr) {
    return dispatch_bps(bps, [&](auto b) {
        constexpr int BPS = decltype(b)::value;
        if (kind == kMiQuadBase) k_mi_quad<BPS, kMiQuadBase><<<grid, 256, 0, st>>>(probs, nprob, work, nwork, out, dbg);
        else k_mi_quad<BPS, kMiQuadXY><<<grid, 256, 0, st>>>(probs, nprob, work, nwork, out, dbg);
    });
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
    return need_grid(dm);   // both kinds (the X;Y integrand does not read it)
}

static int mi_integrand_launch(const qr_demap *dm, int kind, int64_t n, const double *d_x, double *d_f, hipStream_t s) {
    const MiQuadProblem pr = quad_problem(dm, dm->d_mi, nullptr);   // p_Xhat: the head of the handle's MI tables
    ProfScope ps("mi_integrand", s);
    const unsigned grid = demap_wave_grid(dm->device, (n + 255) / 256);
    dispatch_bps(dm->h.bps, [&](auto b) {
        constexpr int BPS = decltype(b)::value;
        if (kind == kMiQuadBase) k_mi_integrand<BPS, kMiQuadBase><<<grid, 256, 0, s>>>(pr, n, d_x, d_f);
        else k_mi_integrand<BPS, kMiQuadXY><<<grid, 256, 0, s>>>(pr, n, d_x, d_f);
    });
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

}  // namespace qr

// ===================================================================== C-ABI
using namespace qr;

extern "C" {

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
        if (!ws_aligned(d_workspace)) return set_error(QR_EVALUE, "workspace must be 256-byte aligned");
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
    HostTrip t(dm->scratch, dm->device);
    int64_t *d_x;
    double *d_y, *d_t;
    if (!t.take(&d_x, (size_t)ld, &d_y, (size_t)ld, &d_t, (size_t)3 * ld)) return t.rc;
    t.up(d_x, x, N);
    t.up(d_y, y, N);
    if (t.ok()) t.rc = mi_launch(dm, mask, (int)N, ld, 1, d_x, d_y, nullptr, d_t, nullptr);
    std::vector<double> h((size_t)N);
    for (int q = 0; q < 3 && t.ok(); ++q) {
        double acc = 0.0;
        if ((mask >> q) & 1u) {
            t.down(h.data(), d_t + (size_t)q * ld, N);
            for (int64_t p = 0; p < N; ++p) acc = q == 2 ? acc - h[(size_t)p] : acc + h[(size_t)p];
        } else {
            std::fill(h.begin(), h.end(), 0.0);
        }
        if (terms) memcpy(terms + (size_t)q * N, h.data(), (size_t)N * 8);
        out[q] = acc / (double)N;
    }
    return t.rc;
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
    if (int rc = check_host_arrays(n, x, f)) return rc;
    if (n == 0) return QR_OK;
    HostTrip t(dm->scratch, dm->device);
    double *d_x, *d_f;
    if (!t.take(&d_x, (size_t)n, &d_f, (size_t)n)) return t.rc;
    t.up(d_x, x, n);
    if (t.ok()) t.rc = mi_integrand_launch(dm, kind, n, d_x, d_f, nullptr);
    t.down(f, d_f, n);
    return t.rc;
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
            launch_mi_quad(kind, bps, grid, st, (const MiQuadProblem *)b_prob.p, P, (const MiQuadWork *)b_work.p, nwork,
                           (double *)b_out.p);
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
    launch_mi_quad(kind, dm->h.bps, 1, nullptr, (const MiQuadProblem *)b_prob.p, 1, (const MiQuadWork *)b_work.p, 1,
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

}  // extern "C"
