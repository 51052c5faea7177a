// math_eval.hip -- qr_math_eval_host: the arithmetic primitives of glibc_math.hpp, qamr_math.hpp and
// strict_pack.hpp evaluated ON THE DEVICE over arrays, for tests (tests/test_gpu_device_math.py).
//
// The host harnesses (tests/native/*.cpp) compile those headers for x86; what ships is their gfx950
// compile, which differs: inline assembly (g_add_ki, g_bfi), erfc's exp (g_exp_full instead of libm),
// the wave-level code that exists only on the device (g_exp_wave, h_packed), the table homes and
// GlibcK::pinned().  Each kernel here calls one primitive exactly as a product kernel calls it -- the
// same table type, staged from the same source by the same staging routine, the same GlibcK form --
// and is built into libqamr.so with the product's flags.  include/qamr.h lists the call sites a
// "home" stands for.
#include <memory>

#include "qamr_internal.hpp"
#include "strict_pack.hpp"

namespace qr {

// the LDS block of mi.hip's kernels (MiLds): g_exp_wave reads T.ex only
struct MathEvalMiLds {
    double2 ex[128];
    double4 e[64];
};

constexpr int kMathFnCount = QR_MATH_DIV_TWO_S2 + 1;
constexpr int kMathHomeCount = QR_MATH_HOME_MI + 1;

// One element per lane.  Every lane of a wave runs the primitive (the wave-level ones need that, and
// the product's padding lanes run along too); lanes past n take the harmless argument 1.0, as
// k_demap_wave's padding does, and store nothing.
template <int FN>
struct MathOp {
    template <class TT>
    __device__ __forceinline__ static double run(double x, double y, double z, const TT &T, const GlibcK &K) {
        if constexpr (FN == QR_MATH_EXP) return g_exp(x, T);
        else if constexpr (FN == QR_MATH_EXP_NEG) return g_exp_neg(x, T, K);
        else if constexpr (FN == QR_MATH_EXP_FULL) return g_exp_full(x, T);
        else if constexpr (FN == QR_MATH_EXP_WAVE) return g_exp_wave(x, T);
        else if constexpr (FN == QR_MATH_LOG) return g_log(x, T);
        else if constexpr (FN == QR_MATH_LOG_U) return g_log_u(x, T, K);
        else if constexpr (FN == QR_MATH_LOG_U_SEL) return g_log_u_sel(x, T, K);
        else if constexpr (FN == QR_MATH_LOG_FULL) return g_log_full(x, T);
        else if constexpr (FN == QR_MATH_H_STRICT) return h_strict<false>(x, T, K);
        else if constexpr (FN == QR_MATH_H_STRICT_SEL) return h_strict<true>(x, T, K);
        else if constexpr (FN == QR_MATH_BOX_PLUS) return box_plus_strict_t<false>(x, y, T, K);
        else if constexpr (FN == QR_MATH_BOX_PLUS_SEL) return box_plus_strict_t<true>(x, y, T, K);
        else if constexpr (FN == QR_MATH_ERF) return cephes_erf(x);
        else return div_two_s2_core(y, z, x);
    }
};

template <int FN, int HOME>
__global__ void __launch_bounds__(256) k_math_eval(int64_t n, const double *__restrict__ a, const double *__restrict__ b,
                                                   const double *__restrict__ c, double *__restrict__ out,
                                                   const GlibcTables *__restrict__ gtab) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    const double x = live ? a[i] : 1.0;
    const double y = (live && b) ? b[i] : 1.0;
    const double z = (live && c) ? c[i] : 1.0;
    double r;
    if constexpr (HOME == QR_MATH_HOME_SWEEP) {
        __shared__ GlibcTablesBP tab;
        stage_glibc_tables(&tab, gtab);
        const auto K = GlibcK::pinned();
        r = MathOp<FN>::run(x, y, z, tab, K);
    } else if constexpr (HOME == QR_MATH_HOME_NODE) {
        __shared__ GlibcTables tab;
        stage_glibc_tables(&tab, gtab);
        r = MathOp<FN>::run(x, y, z, tab, GlibcK());
    } else if constexpr (HOME == QR_MATH_HOME_CONST) {
        r = MathOp<FN>::run(x, y, z, kGlibcConst, GlibcK());
    } else if constexpr (HOME == QR_MATH_HOME_EXPLOG) {
        __shared__ GlibcExpLog gt;
        stage_glibc_exp_log(&gt, &kGlibcConst);
        r = MathOp<FN>::run(x, y, z, gt, GlibcK());
    } else if constexpr (HOME == QR_MATH_HOME_DEMAP) {
        __shared__ GlibcTables gt;
        stage_glibc_tables(&gt, &kGlibcConst);
        r = MathOp<FN>::run(x, y, z, gt, GlibcK());
    } else {
        __shared__ MathEvalMiLds lt;
        for (int q = threadIdx.x; q < 128; q += blockDim.x) lt.ex[q] = kGlibcConst.ex[q];
        for (int q = threadIdx.x; q < 64; q += blockDim.x) lt.e[q] = kGlibcLog2Const.e[q];
        __syncthreads();
        r = MathOp<FN>::run(x, y, z, lt, GlibcK());
    }
    if (live) out[i] = r;
}

// h_packed<CL> with NJ arguments per lane, as check_strict_packed calls it from the check sweeps: the
// box-plus tables in LDS, GlibcK::pinned(), one buffer of kPackWaveDoubles per wavefront.  Wave w takes
// the 64 NJ elements from 64 NJ w on; argument j of lane l is element 64 NJ w + 64 j + l (so a test
// lays a wave's near-1 / table mix out per job).  Elements past n are the harmless 1.0.
template <int CL, int NJ>
__global__ void __launch_bounds__(256) k_math_h_packed(int64_t n, const double *__restrict__ a, double *__restrict__ out,
                                                       const GlibcTables *__restrict__ gtab) {
    __shared__ GlibcTablesBP tab;
    __shared__ double hb[4 * kPackWaveDoubles];
    stage_glibc_tables(&tab, gtab);
    const auto K = GlibcK::pinned();
    const int lane = threadIdx.x & 63;
    const int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 * NJ) + lane;
    double t[kPackMaxJobs], h[kPackMaxJobs];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int64_t e = base + 64 * j;
        t[j] = e < n ? a[e] : 1.0;
    }
    h_packed<CL>(t, h, NJ, hb + (threadIdx.x >> 6) * kPackWaveDoubles, tab, K);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int64_t e = base + 64 * j;
        if (e < n) out[e] = h[j];
    }
}

// the homes a primitive is called from in the product (include/qamr.h); bit h = home h
static unsigned math_homes(int fn) {
    constexpr unsigned sweep = 1u << QR_MATH_HOME_SWEEP, node = 1u << QR_MATH_HOME_NODE, cst = 1u << QR_MATH_HOME_CONST,
                       explog = 1u << QR_MATH_HOME_EXPLOG, demap = 1u << QR_MATH_HOME_DEMAP, mi = 1u << QR_MATH_HOME_MI;
    switch (fn) {
    case QR_MATH_EXP: return node | cst;
    case QR_MATH_EXP_NEG: case QR_MATH_LOG_U: case QR_MATH_LOG_U_SEL: case QR_MATH_H_STRICT: case QR_MATH_H_STRICT_SEL:
    case QR_MATH_BOX_PLUS: case QR_MATH_BOX_PLUS_SEL: return sweep | node;
    case QR_MATH_EXP_FULL: case QR_MATH_LOG: case QR_MATH_LOG_FULL: return cst | explog | demap;
    case QR_MATH_EXP_WAVE: return explog | mi;
    case QR_MATH_ERF: case QR_MATH_DIV_TWO_S2: return cst;
    default: return 0;
    }
}

struct MathArgs {
    int64_t n;
    const double *a, *b, *c;
    double *out;
    const GlibcTables *gtab;
};

template <int FN, int HOME>
static void launch_math(const MathArgs &m) {
    k_math_eval<FN, HOME><<<(unsigned)((m.n + 255) / 256), 256>>>(m.n, m.a, m.b, m.c, m.out, m.gtab);
}

template <int FN, int... HOME>
static bool launch_math_homes(int home, const MathArgs &m) {
    return ((home == HOME && (launch_math<FN, HOME>(m), true)) || ...);
}

static bool launch_math_fn(int fn, int home, const MathArgs &m) {
    constexpr int S = QR_MATH_HOME_SWEEP, N = QR_MATH_HOME_NODE, C = QR_MATH_HOME_CONST, E = QR_MATH_HOME_EXPLOG,
                  D = QR_MATH_HOME_DEMAP, M = QR_MATH_HOME_MI;
    switch (fn) {
    case QR_MATH_EXP: return launch_math_homes<QR_MATH_EXP, N, C>(home, m);
    case QR_MATH_EXP_NEG: return launch_math_homes<QR_MATH_EXP_NEG, S, N>(home, m);
    case QR_MATH_EXP_FULL: return launch_math_homes<QR_MATH_EXP_FULL, C, E, D>(home, m);
    case QR_MATH_EXP_WAVE: return launch_math_homes<QR_MATH_EXP_WAVE, E, M>(home, m);
    case QR_MATH_LOG: return launch_math_homes<QR_MATH_LOG, C, E, D>(home, m);
    case QR_MATH_LOG_U: return launch_math_homes<QR_MATH_LOG_U, S, N>(home, m);
    case QR_MATH_LOG_U_SEL: return launch_math_homes<QR_MATH_LOG_U_SEL, S, N>(home, m);
    case QR_MATH_LOG_FULL: return launch_math_homes<QR_MATH_LOG_FULL, C, E, D>(home, m);
    case QR_MATH_H_STRICT: return launch_math_homes<QR_MATH_H_STRICT, S, N>(home, m);
    case QR_MATH_H_STRICT_SEL: return launch_math_homes<QR_MATH_H_STRICT_SEL, S, N>(home, m);
    case QR_MATH_BOX_PLUS: return launch_math_homes<QR_MATH_BOX_PLUS, S, N>(home, m);
    case QR_MATH_BOX_PLUS_SEL: return launch_math_homes<QR_MATH_BOX_PLUS_SEL, S, N>(home, m);
    case QR_MATH_ERF: return launch_math_homes<QR_MATH_ERF, C>(home, m);
    case QR_MATH_DIV_TWO_S2: return launch_math_homes<QR_MATH_DIV_TWO_S2, C>(home, m);
    default: return false;
    }
}

template <int CL, int... NJ>
static bool launch_h_packed_nj(int nj, const MathArgs &m, std::integer_sequence<int, NJ...>) {
    const unsigned grid = (unsigned)((m.n + 256 * (int64_t)nj - 1) / (256 * (int64_t)nj));   // 4 waves x 64 nj elements
    return ((nj == NJ + 1 && (k_math_h_packed<CL, NJ + 1><<<grid, 256>>>(m.n, m.a, m.out, m.gtab), true)) || ...);
}

static bool launch_h_packed(int clamp, int nj, const MathArgs &m) {
    const auto seq = std::make_integer_sequence<int, kPackMaxJobs>{};
    switch (clamp) {
    case kClampNone: return launch_h_packed_nj<kClampNone>(nj, m, seq);
    case kClampFull: return launch_h_packed_nj<kClampFull>(nj, m, seq);
    case kClampFinite: return launch_h_packed_nj<kClampFinite>(nj, m, seq);
    default: return false;
    }
}

}  // namespace qr

using namespace qr;

int qr_math_eval_host(int32_t fn, int32_t variant, int64_t n, const double *a, const double *b, double *out) {
    const bool packed = fn == QR_MATH_H_PACKED;
    if (packed) {
        if (variant < 0 || variant >= 3 * kPackMaxJobs)
            return set_error(QR_EVALUE, "h_packed: variant is clamp * %d + (nj - 1), clamp 0..2, nj 1..%d (got %d)",
                             kPackMaxJobs, kPackMaxJobs, variant);
    } else {
        if (fn < 0 || fn >= kMathFnCount) return set_error(QR_EVALUE, "unknown function %d", fn);
        if (variant < 0 || variant >= kMathHomeCount || !((math_homes(fn) >> variant) & 1u))
            return set_error(QR_EVALUE, "function %d has no call site with table home %d", fn, variant);
    }
    const bool two = fn == QR_MATH_BOX_PLUS || fn == QR_MATH_BOX_PLUS_SEL || fn == QR_MATH_DIV_TWO_S2;
    if (int rc = two ? check_host_arrays(n, a, b, out) : check_host_arrays(n, a, out)) return rc;
    if (n == 0) return QR_OK;
    if (n > (int64_t)1 << 28) return set_error(QR_EVALUE, "n too large for one call");
    // no handle: the scratch of this entry alone, on the caller's current device; never destroyed (a
    // static destructor would call into a HIP runtime that may be gone)
    static Scratch *scratch = new Scratch;
    int device = 0;
    QR_HIP(hipGetDevice(&device));
    HostTrip t(*scratch, device);
    if (scratch->ptr && scratch->device != device) {   // the caller changed device: start over there
        DeviceGuard g(scratch->device);
        (void)hipFree(scratch->ptr);
        scratch->ptr = nullptr;
        scratch->bytes = 0;
    }
    scratch->device = device;
    double *d_a, *d_b, *d_c, *d_o;
    GlibcTables *d_g;
    const size_t nn = (size_t)n;
    if (!t.take(&d_a, nn, &d_b, nn, &d_c, nn, &d_o, nn, &d_g, (size_t)1)) return t.rc;
    // the tables as a code handle holds them: build_glibc_tables on the host, uploaded (qr_code_create)
    auto gt = std::make_unique<GlibcTables>();
    build_glibc_tables(gt.get());
    t.up(d_g, (const GlibcTables *)gt.get(), 1);
    t.up(d_a, a, nn);
    if (two) t.up(d_b, b, nn);
    std::vector<double> inv;
    if (fn == QR_MATH_DIV_TWO_S2) {   // RN(1 / two_s2), as build_demap_host forms DemapTables::inv_two_s2
        inv.resize(nn);
        for (size_t k = 0; k < nn; ++k) inv[k] = 1.0 / b[k];
        t.up(d_c, (const double *)inv.data(), nn);
    }
    if (t.ok()) {
        const MathArgs m{n, d_a, two ? d_b : nullptr, fn == QR_MATH_DIV_TWO_S2 ? d_c : nullptr, d_o, d_g};
        const bool ok = packed ? launch_h_packed(variant / kPackMaxJobs, variant % kPackMaxJobs + 1, m)
                               : launch_math_fn(fn, variant, m);
        if (!ok) return set_error(QR_EINTERNAL, "qr_math_eval_host: no kernel for function %d, variant %d", fn, variant);
        t.launched();
    }
    t.down(out, (const double *)d_o, nn);
    return t.rc;
}
