// density_evolution.hip -- sampled (population) density evolution of a code ensemble on an empirical
// LLR density, for gfx950 (DESIGN.md "Density evolution").  Not a reference interface: the reference
// has no such tool; the definition is this library's (include/qamr.h qr_de_evolve_device) and the
// results are bit-exact against it (tests/de_fixture.py restates it with the oracle's box-plus).
//
// The decoder's own arithmetic applied to random draws from populations of M messages instead of to
// a graph.  All of it IEEE fp64, unfused, the box-plus the reference's (decoder.pyx:41-45).
//
//   rnd(t, phase, j, k, n) = ((z >> 32) * n) >> 32,  z = mix(seed + G * (ctr + 1)),
//   ctr = ((t * 4 + phase) * 2^32 + j) * 512 + k:     a counter-based SplitMix64, so a lane computes any draw
//   c2v(0)[j] = +0.0
//   phase 0, t >= 1:  d = edge_vdeg[rnd(.., 0, Ne)];  s = u[rnd(.., 1, Mu)]
//                     s = s + c2v(t-1)[rnd(.., 2 + k, M)], k = 0 .. d-2;          v2c(t)[j] = s
//   phase 1, t >= 1:  d = edge_cdeg[rnd(.., 0, Ne)];  F = v2c(t)[rnd(.., 2, M)]
//                     F = box_plus(F, v2c(t)[rnd(.., 2 + k, M)]), k = 1 .. d-2;   c2v(t)[j] = F
//   phase 2, t >= 0:  d = node_vdeg[rnd(.., 0, Nv)];  p = u[rnd(.., 1, Mu)]
//                     p = p + c2v(t)[rnd(.., 2 + k, M)], k = 0 .. d-1;            errors[t] += !(p >= 0)
//
// A lane is one sample j; 256-thread workgroups run grid-stride.  The degree is per lane, so a wave
// runs to its largest trip count.  A phase reads one population and writes the other, and the
// kernel boundary orders them: c2v(t) overwrites c2v(t-1) once phase 0 has read it, so the call
// holds two populations and needs no workspace.  The operands of a lane are gathered in blocks of
// kDeBlock (indices first, then the loads, then the dependent chain), so that the random 8-byte
// reads of a population that sits in L2 / the Infinity Cache overlap the arithmetic.
#include <vector>

#include "qamr_internal.hpp"
#include "debug_check.hpp"

// the three degree tables of an ensemble, one byte per entry (degrees are at most 255)
struct qr_de_tables {
    int device = 0;
    int64_t Ne = 0, Nv = 0;
    uint8_t *d_edge_vdeg = nullptr, *d_edge_cdeg = nullptr, *d_node_vdeg = nullptr;
};

namespace qr {

enum DeDebugSite {         // 27..30: decode_layered.hip (decode_dev.hpp DebugSite)
    kDbgDeDegree = 31,     // k_de_var / k_de_check / k_de_post: a degree-table index outside [0, Ne) or [0, Nv)
    kDbgDeChannel = 32,    // k_de_var / k_de_post: a channel index outside [0, Mu)
    kDbgDeMessage = 33,    // k_de_var / k_de_check / k_de_post: a message index outside [0, M)
    kDbgDeSource = 34,     // k_de_population: the source element r * ld + f outside [0, rows * ld)
};

constexpr int kDeBlock = 8;           // operands gathered ahead of the chain that consumes them
constexpr int64_t kDeMaxPop = (int64_t)1 << 30;
constexpr int64_t kDeMaxTable = (int64_t)1 << 31;   // exclusive
constexpr int kDeMaxIter = 10000;
constexpr uint64_t kDeGolden = 0x9E3779B97F4A7C15ull;

__host__ __device__ __forceinline__ uint64_t de_mix(uint64_t x) {
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// the draws of one (t, phase, j): s = seed + G * (ctr(t, phase, j, 0) + 1), and draw k adds G * k
struct DeDraw {
    uint64_t s;
    __host__ __device__ DeDraw(uint64_t seed, int t, int phase, int64_t j)
        : s(seed + kDeGolden * ((((((uint64_t)t * 4 + (uint64_t)phase) << 32) + (uint64_t)j) << 9) + 1)) {}
    // in [0, n), 1 <= n < 2^31
    __host__ __device__ __forceinline__ uint32_t at(int k, uint32_t n) const {
        const uint64_t z = de_mix(s + kDeGolden * (uint64_t)k);
        return (uint32_t)(((z >> 32) * (uint64_t)n) >> 32);
    }
};

struct DeArgs {
    const uint8_t *deg;   // the phase's degree table
    uint32_t n_deg;       // its entries
    const double *u;      // the channel population
    uint32_t Mu;
    const double *src;    // the population the phase reads
    double *dst;          // the population it writes (phase 2: none)
    uint32_t M;
    uint64_t seed;
    int t;
    unsigned long long *errors;   // phase 2: &errors[t]
};

__device__ __forceinline__ int de_degree(const DeArgs &a, const DeDraw &r) {
    const uint32_t i = r.at(0, a.n_deg);
    QR_DCHECK(i < a.n_deg, kDbgDeDegree, i, a.n_deg);
    return a.deg[i];
}

__device__ __forceinline__ double de_channel(const DeArgs &a, const DeDraw &r) {
    const uint32_t i = r.at(1, a.Mu);
    QR_DCHECK(i < a.Mu, kDbgDeChannel, i, a.Mu);
    return a.u[i];
}

__device__ __forceinline__ double de_message(const DeArgs &a, const DeDraw &r, int k) {
    const uint32_t i = r.at(k, a.M);
    QR_DCHECK(i < a.M, kDbgDeMessage, i, a.M);
    return a.src[i];
}

// s + the messages of draws k0 .. k1-1 in ascending k, a block of kDeBlock loads ahead of its adds
__device__ __forceinline__ double de_add_messages(const DeArgs &a, const DeDraw &r, double s, int k0, int k1) {
    for (int kb = k0; kb < k1; kb += kDeBlock) {
        double x[kDeBlock];
#pragma unroll
        for (int i = 0; i < kDeBlock; ++i) x[i] = kb + i < k1 ? de_message(a, r, kb + i) : 0.0;
#pragma unroll
        for (int i = 0; i < kDeBlock; ++i)
            if (kb + i < k1) s = s + x[i];
    }
    return s;
}

// u[r * B + f] = alpha * L[r][f], its sign bit flipped where word[r][f] != 0: the batch as a signed
// population (u > 0: the LAPPR points at the word's bit).  The padding columns [B, ld) are not read.
__global__ void __launch_bounds__(256) k_de_population(int B, int ld, int64_t rows, const double *__restrict__ lappr,
                                                       const uint8_t *__restrict__ word, double alpha,
                                                       double *__restrict__ u) {
    const int64_t n = rows * B;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / B;
        const int64_t e = r * ld + (i - r * B);
        QR_DCHECK(e >= 0 && e < rows * ld, kDbgDeSource, e, rows * ld);
        const uint64_t x = __builtin_bit_cast(uint64_t, alpha * lappr[e]);
        u[i] = __builtin_bit_cast(double, word[e] != 0 ? x ^ 0x8000000000000000ull : x);
    }
}

// phase 0.  FIRST (t == 1): every message is +0.0 and is not read; x + 0.0 once or d - 1 times is
// the same double, so one add stands for them (none at degree 1: -0.0 stays -0.0).
template <bool FIRST>
__global__ void __launch_bounds__(256) k_de_var(DeArgs a) {
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < a.M; j += (int64_t)gridDim.x * 256) {
        const DeDraw r(a.seed, a.t, 0, j);
        const int d = de_degree(a, r);
        double s = de_channel(a, r);
        if constexpr (FIRST) {
            if (d >= 2) s = s + 0.0;
        } else {
            s = de_add_messages(a, r, s, 2, d + 1);   // k = 0 .. d-2 are draws 2 .. d
        }
        a.dst[j] = s;
    }
}

// phase 1: F = the message of draw 2, then box_plus(F, .) over draws 3 .. d (degree 2: a bare copy)
__global__ void __launch_bounds__(256) k_de_check(DeArgs a) {
    __shared__ GlibcTablesBP tab;
    stage_glibc_tables(&tab, &kGlibcConst);
    const auto K = GlibcK::pinned();
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < a.M; j += (int64_t)gridDim.x * 256) {
        const DeDraw r(a.seed, a.t, 1, j);
        const int d = de_degree(a, r);
        double F = de_message(a, r, 2);
        for (int kb = 3; kb <= d; kb += kDeBlock) {
            double x[kDeBlock];
#pragma unroll
            for (int i = 0; i < kDeBlock; ++i) x[i] = kb + i <= d ? de_message(a, r, kb + i) : 0.0;
#pragma unroll
            for (int i = 0; i < kDeBlock; ++i)
                if (kb + i <= d) F = box_plus_strict(F, x[i], tab, K);
        }
        a.dst[j] = F;
    }
}

// phase 2: the decision count_errors_from_lappr makes (p >= 0 is correct, NaN an error), counted by
// a wave ballot, the waves' counts added in LDS and one atomic add on errors[t] per workgroup (integer
// sums are order-free; every add of a launch goes to the one address, so they are kept few: one per
// wave cost 0.15 ms a launch at 16 384 waves).  FIRST (t == 0): every message is +0.0; p + 0.0 and
// p decide alike (-0.0 >= 0 holds), so neither degree nor message is read.
template <bool FIRST>
__global__ void __launch_bounds__(256) k_de_post(DeArgs a) {
    __shared__ unsigned wg;
    if (threadIdx.x == 0) wg = 0;
    __syncthreads();
    unsigned cnt = 0;   // wave-uniform
    for (int64_t b = (int64_t)blockIdx.x * 256; b < a.M; b += (int64_t)gridDim.x * 256) {   // block-uniform
        const int64_t j = b + threadIdx.x;
        bool err = false;
        if (j < a.M) {
            const DeDraw r(a.seed, a.t, 2, j);
            double p = de_channel(a, r);
            if constexpr (!FIRST) p = de_add_messages(a, r, p, 2, de_degree(a, r) + 2);   // k = 0 .. d-1 are draws 2 .. d+1
            err = !(p >= 0.0);
        }
        cnt += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(err));
    }
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&wg, cnt);
    __syncthreads();
    if (threadIdx.x == 0 && wg) atomicAdd(a.errors, (unsigned long long)wg);
}

// ------------------------------------------------------------------ host
static unsigned de_grid(int device, int64_t n) { return demap_wave_grid(device, (n + 255) / 256); }

static int de_check_sizes(int64_t Mu, int64_t M, int32_t T) {
    if (Mu < 1 || Mu >= kDeMaxTable) return set_error(QR_EVALUE, "density evolution: Mu must be in [1, 2^31) (got %lld)", (long long)Mu);
    if (M < 1 || M > kDeMaxPop) return set_error(QR_EVALUE, "density evolution: M must be in [1, 2^30] (got %lld)", (long long)M);
    if (T < 0 || T > kDeMaxIter) return set_error(QR_EVALUE, "density evolution: T must be in [0, %d] (got %d)", kDeMaxIter, T);
    return QR_OK;
}

// degrees in lo..255, one byte each
static int de_pack_degrees(const char *name, const int32_t *deg, int64_t n, int lo, std::vector<uint8_t> &out) {
    out.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (deg[i] < lo || deg[i] > 255)
            return set_error(QR_EVALUE, "density evolution: %s[%lld] = %d outside %d..255", name, (long long)i, deg[i], lo);
        out[(size_t)i] = (uint8_t)deg[i];
    }
    return QR_OK;
}

}  // namespace qr

// ===================================================================== C-ABI
using namespace qr;

extern "C" {

int qr_de_tables_create(int32_t device, int64_t Ne, const int32_t *edge_vdeg, const int32_t *edge_cdeg, int64_t Nv,
                        const int32_t *node_vdeg, qr_de_tables **out) {
    if (!edge_vdeg || !edge_cdeg || !node_vdeg || !out) return set_error(QR_EVALUE, "qr_de_tables_create: null argument");
    *out = nullptr;
    if (Ne < 1 || Ne >= kDeMaxTable || Nv < 1 || Nv >= kDeMaxTable)
        return set_error(QR_EVALUE, "qr_de_tables_create: Ne and Nv must be in [1, 2^31) (Ne=%lld, Nv=%lld)", (long long)Ne,
                         (long long)Nv);
    std::vector<uint8_t> ev, ec, nv;
    if (int rc = de_pack_degrees("edge_vdeg", edge_vdeg, Ne, 1, ev)) return rc;
    if (int rc = de_pack_degrees("edge_cdeg", edge_cdeg, Ne, 2, ec)) return rc;
    if (int rc = de_pack_degrees("node_vdeg", node_vdeg, Nv, 0, nv)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return set_error(QR_EDEVICE, "no HIP device available (libqamr has no CPU fallback)");
    if (device < 0 || device >= ndev) return set_error(QR_EVALUE, "device %d out of range (%d devices)", device, ndev);
    DeviceGuard g(device);
    qr_de_tables *t = new qr_de_tables();
    t->device = device;
    t->Ne = Ne;
    t->Nv = Nv;
    auto up = [](uint8_t **d, const std::vector<uint8_t> &h) {
        return hipMalloc((void **)d, h.size()) == hipSuccess &&
               hipMemcpy(*d, h.data(), h.size(), hipMemcpyHostToDevice) == hipSuccess;
    };
    if (!up(&t->d_edge_vdeg, ev) || !up(&t->d_edge_cdeg, ec) || !up(&t->d_node_vdeg, nv)) {
        (void)hipGetLastError();
        qr_de_tables_destroy(t);
        return set_error(QR_EMEMORY, "qr_de_tables_create: the tables do not fit on device %d", device);
    }
    *out = t;
    return QR_OK;
}

int qr_de_tables_destroy(qr_de_tables *t) {
    if (!t) return QR_OK;
    DeviceGuard g(t->device);
    (void)hipFree(t->d_edge_vdeg);
    (void)hipFree(t->d_edge_cdeg);
    (void)hipFree(t->d_node_vdeg);
    delete t;
    return QR_OK;
}

int qr_de_population_device(int32_t B, int32_t ld, int64_t rows, const double *d_lappr, const uint8_t *d_word,
                            double alpha, double *d_u, void *stream) {
    if (int rc = check_shape(B, ld, rows)) return rc;
    if (rows > (kDeMaxTable - 1) / B) return set_error(QR_EVALUE, "qr_de_population_device: rows * B must be below 2^31");
    if (!(alpha - alpha == 0.0)) return set_error(QR_EVALUE, "qr_de_population_device: alpha is not finite");
    if (!d_lappr || !d_word || !d_u) return set_error(QR_EVALUE, "qr_de_population_device: null pointer argument");
    int device = 0;   // no handle: the caller's current device, as the other handle-free *_device entries
    QR_HIP(hipGetDevice(&device));
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("de_population", s);
    k_de_population<<<de_grid(device, rows * B), 256, 0, s>>>(B, ld, rows, d_lappr, d_word, alpha, d_u);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

int qr_de_evolve_device(const qr_de_tables *tables, int64_t Mu, const double *d_u, int64_t M, int32_t T, uint64_t seed,
                        double *d_v2c, double *d_c2v, int64_t *d_errors, void *stream) {
    if (!tables || !d_u || !d_v2c || !d_c2v || !d_errors) return set_error(QR_EVALUE, "qr_de_evolve_device: null pointer argument");
    if (int rc = de_check_sizes(Mu, M, T)) return rc;
    DeviceGuard dg(tables->device);
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = de_grid(tables->device, M);
    const unsigned pgrid = (grid + 1) / 2;   // the decision: half the workgroups, each ends in an add on the one address
    QR_HIP(hipMemsetAsync(d_c2v, 0, (size_t)M * sizeof(double), s));
    QR_HIP(hipMemsetAsync(d_errors, 0, ((size_t)T + 1) * sizeof(int64_t), s));
    DeArgs a;
    a.u = d_u;
    a.Mu = (uint32_t)Mu;
    a.M = (uint32_t)M;
    a.seed = seed;
    auto post = [&](int t) {
        a.t = t;
        a.deg = tables->d_node_vdeg;
        a.n_deg = (uint32_t)tables->Nv;
        a.src = d_c2v;
        a.dst = nullptr;
        a.errors = (unsigned long long *)(d_errors + t);
        ProfScope ps("de_post", s);
        if (t == 0) k_de_post<true><<<pgrid, 256, 0, s>>>(a);
        else k_de_post<false><<<pgrid, 256, 0, s>>>(a);
    };
    post(0);
    QR_LAUNCH_CHECK();
    for (int t = 1; t <= T; ++t) {
        a.t = t;
        a.errors = nullptr;
        a.n_deg = (uint32_t)tables->Ne;
        {
            a.deg = tables->d_edge_vdeg;
            a.src = d_c2v;
            a.dst = d_v2c;
            ProfScope ps("de_var", s);
            if (t == 1) k_de_var<true><<<grid, 256, 0, s>>>(a);
            else k_de_var<false><<<grid, 256, 0, s>>>(a);
            QR_LAUNCH_CHECK();
        }
        {
            a.deg = tables->d_edge_cdeg;
            a.src = d_v2c;
            a.dst = d_c2v;
            ProfScope ps("de_check", s);
            k_de_check<<<grid, 256, 0, s>>>(a);
            QR_LAUNCH_CHECK();
        }
        post(t);
        QR_LAUNCH_CHECK();
    }
    return QR_OK;
}

// The same from host memory on GPU `device`: the tables uploaded and dropped again, synchronous copies
// around qr_de_evolve_device.  v2c comes down only when T > 0 (the call does not write it otherwise).
int qr_de_evolve_host(int32_t device, int64_t Ne, const int32_t *edge_vdeg, const int32_t *edge_cdeg, int64_t Nv,
                      const int32_t *node_vdeg, int64_t Mu, const double *u, int64_t M, int32_t T, uint64_t seed,
                      double *v2c, double *c2v, int64_t *errors) {
    if (!u || !v2c || !c2v || !errors) return set_error(QR_EVALUE, "qr_de_evolve_host: null pointer argument");
    if (int rc = de_check_sizes(Mu, M, T)) return rc;
    qr_de_tables *tables = nullptr;
    if (int rc = qr_de_tables_create(device, Ne, edge_vdeg, edge_cdeg, Nv, node_vdeg, &tables)) return rc;
    // no handle of its own to keep: the scratch of this entry alone; never destroyed (a static
    // destructor would call into a HIP runtime that may be gone)
    static Scratch *scratch = new Scratch;
    int rc;
    {
        HostTrip t(*scratch, device);
        if (scratch->ptr && scratch->device != device) {   // another device than last time: start over there
            DeviceGuard g(scratch->device);
            (void)hipFree(scratch->ptr);
            scratch->ptr = nullptr;
            scratch->bytes = 0;
        }
        scratch->device = device;
        double *d_u, *d_v2c, *d_c2v;
        int64_t *d_err;
        if (t.take(&d_u, (size_t)Mu, &d_v2c, (size_t)M, &d_c2v, (size_t)M, &d_err, (size_t)T + 1)) {
            t.up(d_u, u, (size_t)Mu);
            if (t.ok()) t.rc = qr_de_evolve_device(tables, Mu, d_u, M, T, seed, d_v2c, d_c2v, d_err, nullptr);
            if (T > 0) t.down(v2c, (const double *)d_v2c, (size_t)M);
            t.down(c2v, (const double *)d_c2v, (size_t)M);
            t.down(errors, (const int64_t *)d_err, (size_t)T + 1);
        }
        rc = t.rc;
    }
    qr_de_tables_destroy(tables);
    return rc;
}

}  // extern "C"
