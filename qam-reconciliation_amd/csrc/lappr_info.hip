// lappr_info.hip -- the information rate the LAPPRs carry to the bit-wise decoder (the BICM
// generalised mutual information, DESIGN.md "LAPPR information rate") for gfx950.  Not a reference
// interface: the reference has no such estimator; the definition below is this project's and the
// results are bit-exact against it (tests/lappr_info_fixture.py evaluates it with libm).
//
//   x = alpha * L, negated when the word's bit is 0;  m = x > 0 ? x : 0.0;
//   t = m * LOG2E + log2(1.0 + exp(-|x|))        (every operation rounded separately, glibc exp / log2)
//   chunk[a][k][q][f] = sum from 0.0, s ascending, of t over the symbols s of chunk q (kInfoChunk symbols)
//   loss[a][k][f]     = sum from 0.0 of the chunks, q ascending
//   total[a][k]       = sum from 0.0 of loss[a][k][f], f = 0 .. B-1 ascending
//   errors[k][f]      = elements whose decided bit (0 iff L >= 0: NaN decides 1, utils.pyx:35-38) differs from the word's
//
// The layout is the decoder's frame-innermost [V, ld], v = s * bps + k: lane = frame, one wave per
// 64-frame tile, so a row read is one coalesced 512 B (LAPPRs) or 64 B (bits) access.
#include "qamr_internal.hpp"
#include "debug_check.hpp"

namespace qr {

enum InfoDebugSite {       // 20..24: npstream.hip (NpDebugSite)
    kDbgInfoRow = 25,      // k_lappr_info: the row v = s * bps + k outside [0, S * bps)
    kDbgInfoSlot = 26,     // k_lappr_info: a chunk sum's workspace slot outside [0, A * bps * chunks)
};

constexpr int kInfoChunk = QR_LAPPR_INFO_CHUNK;
constexpr int kInfoMaxScales = 16;
constexpr int kInfoMaxBps = 8;
constexpr double kInfoLog2e = 1.4426950408889634;

// the scales, as a kernel argument: read through scalar loads at a wave-uniform index
struct InfoScales {
    double v[kInfoMaxScales];
};

struct InfoLds {
    double2 ex[128];   // glibc exp table (g_exp_wave / g_exp_full read T.ex)
    double4 e[64];     // glibc log2 table (g_log2_full reads T.e)
};

// k_lappr_info: one wave per work item (chunk q, level k, 64-frame tile), grid-stride.  A lane walks
// its frame's symbols of the chunk in ascending s; each LAPPR and bit is loaded once and evaluated at
// all A scales.  The A running sums live in the wave's LDS slice acc[w][a][lane] (A is a runtime
// value: a register array indexed by it would go to scratch); a lane reads and writes only its own
// column of the slice, so no fence is needed.  Every lane of the wave runs every term (g_exp_wave
// needs the whole wave); the padding lanes take L = 0.0 and store nothing.  The chunk sums go to
// wloss[a][k][q][ld], the chunk's error counts to werr[k][q][ld].
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8)))
k_lappr_info(int bps, int B, int ld, int64_t S, int A, const InfoScales al, const double *__restrict__ lappr,
             const uint8_t *__restrict__ word, double *__restrict__ wloss, int32_t *__restrict__ werr) {
    __shared__ InfoLds lt;
    __shared__ double acc[4][kInfoMaxScales][64];
    for (int i = threadIdx.x; i < 128; i += blockDim.x) lt.ex[i] = kGlibcConst.ex[i];
    for (int i = threadIdx.x; i < 64; i += blockDim.x) lt.e[i] = kGlibcLog2Const.e[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t tiles = ld / 64;
    const int64_t nq = (S + kInfoChunk - 1) / kInfoChunk;
    const int64_t items = nq * bps * tiles;
    for (int64_t it = (int64_t)blockIdx.x * 4 + w; it < items; it += (int64_t)gridDim.x * 4) {   // wave-uniform
        const int64_t r = it / tiles;
        const int f = (int)(it - r * tiles) * 64 + lane;
        const int64_t q = r / bps;
        const int k = (int)(r - q * bps);
        const bool valid = f < B;
        for (int a = 0; a < A; ++a) acc[w][a][lane] = 0.0;
        int32_t err = 0;
        const int64_t s1 = (q + 1) * kInfoChunk < S ? (q + 1) * kInfoChunk : S;
        for (int64_t s = q * kInfoChunk; s < s1; ++s) {
            const int64_t v = s * bps + k;
            QR_DCHECK(v >= 0 && v < S * bps, kDbgInfoRow, v, S * bps);
            const double L = valid ? lappr[v * ld + f] : 0.0;
            const uint8_t bit = valid ? word[v * ld + f] : (uint8_t)0;
            err += ((L >= 0.0) ? 0 : 1) != bit ? 1 : 0;
#pragma unroll 1
            for (int a = 0; a < A; ++a) {
                double x = al.v[a] * L;
                x = bit == 0 ? -x : x;
                const double m = x > 0.0 ? x : 0.0;
                const double t = m * kInfoLog2e + g_log2_full(1.0 + g_exp_wave(-__builtin_fabs(x), lt), lt);
                acc[w][a][lane] += t;
            }
        }
        if (valid) {
            for (int a = 0; a < A; ++a) {
                const int64_t slot = ((int64_t)a * bps + k) * nq + q;
                QR_DCHECK(slot >= 0 && slot < (int64_t)A * bps * nq, kDbgInfoSlot, slot, (int64_t)A * bps * nq);
                wloss[slot * ld + f] = acc[w][a][lane];
            }
            werr[((int64_t)k * nq + q) * ld + f] = err;
        }
    }
}

// k_lappr_info_total: one workgroup per (plane, level k); plane a < A is scale a, plane A the error
// counts.  Thread t takes the frames t, t + kInfoTotalThreads, ...: it adds the frame's chunks in
// ascending q from 0.0 (0) and writes loss[a][k][f] (errors[k][f]).  The sum over the frames is one
// chain in ascending f: the values of a pass go through LDS and thread 0 adds them in order (the LDS
// reads unrolled ahead of the dependent adds).  Columns [B, ld) are neither read nor written.  The launch has only (A + 1) bps workgroups and every load of a chunk sum is
// a strided, latency-bound read: the workgroups are as wide as they can be (kInfoTotalThreads).
constexpr int kInfoTotalThreads = 1024;
__global__ void __launch_bounds__(kInfoTotalThreads)
k_lappr_info_total(int bps, int B, int ld, int64_t nq, int A, const double *__restrict__ wloss,
                   const int32_t *__restrict__ werr, double *__restrict__ loss, int32_t *__restrict__ errors,
                   double *__restrict__ total, int64_t *__restrict__ total_errors) {
    __shared__ double sh[kInfoTotalThreads];
    __shared__ int32_t she[kInfoTotalThreads];
    const int plane = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    if (plane < A) {   // block-uniform
        const double *src = wloss + ((int64_t)plane * bps + k) * nq * ld;
        double tot = 0.0;
        for (int base = 0; base < B; base += kInfoTotalThreads) {
            const int f = base + tid;
            if (f < B) {
                double v = 0.0;
#pragma unroll 8
                for (int64_t q = 0; q < nq; ++q) v += src[q * ld + f];
                loss[((int64_t)plane * bps + k) * ld + f] = v;
                sh[tid] = v;
            }
            __syncthreads();
            if (tid == 0) {
                const int n = B - base < kInfoTotalThreads ? B - base : kInfoTotalThreads;
#pragma unroll 16
                for (int i = 0; i < n; ++i) tot += sh[i];
            }
            __syncthreads();
        }
        if (tid == 0) total[(int64_t)plane * bps + k] = tot;
    } else {
        const int32_t *src = werr + (int64_t)k * nq * ld;
        int64_t tot = 0;
        for (int base = 0; base < B; base += kInfoTotalThreads) {
            const int f = base + tid;
            if (f < B) {
                int32_t v = 0;
                for (int64_t q = 0; q < nq; ++q) v += src[q * ld + f];
                errors[(int64_t)k * ld + f] = v;
                she[tid] = v;
            }
            __syncthreads();
            if (tid == 0) {
                const int n = B - base < kInfoTotalThreads ? B - base : kInfoTotalThreads;
#pragma unroll 16
                for (int i = 0; i < n; ++i) tot += she[i];
            }
            __syncthreads();
        }
        if (tid == 0) total_errors[k] = tot;
    }
}

static int64_t info_chunks(int64_t S) { return (S + kInfoChunk - 1) / kInfoChunk; }

// the workspace: chunk sums [A][bps][chunks][ld] fp64, then chunk error counts [bps][chunks][ld] int32
static void info_workspace(Cursor &c, int bps, int ld, int64_t S, int A, double **wloss, int32_t **werr) {
    const size_t rows = (size_t)bps * (size_t)info_chunks(S) * (size_t)ld;
    *wloss = c.take<double>((size_t)A * rows);
    *werr = c.take<int32_t>(rows);
}

// bps, ld, S, A of both entries and of the workspace query
static int info_check_shape(int bps, int ld, int64_t S, int A) {
    if (bps < 1 || bps > kInfoMaxBps) return set_error(QR_EVALUE, "bit_per_symbol must be in 1..%d (got %d)", kInfoMaxBps, bps);
    if (A < 1 || A > kInfoMaxScales) return set_error(QR_EVALUE, "the number of scales must be in 1..%d (got %d)", kInfoMaxScales, A);
    if (ld <= 0 || ld % kWave) return set_error(QR_EVALUE, "need ld > 0, ld %% 64 == 0 (ld=%d)", ld);
    if (S < 1) return set_error(QR_EVALUE, "S must be positive");
    if (S > ((int64_t)1 << 40) / ((int64_t)bps * ld)) return set_error(QR_EVALUE, "S * bit_per_symbol * ld too large");
    return QR_OK;
}

static int info_scales(int A, const double *alphas, InfoScales &al) {
    if (!alphas) return set_error(QR_EVALUE, "null pointer argument");
    for (int a = 0; a < kInfoMaxScales; ++a) al.v[a] = 0.0;
    for (int a = 0; a < A; ++a) {
        if (!(alphas[a] - alphas[a] == 0.0)) return set_error(QR_EVALUE, "scale %d is not finite", a);
        al.v[a] = alphas[a];
    }
    return QR_OK;
}

// the two launches on stream s; the checks are the caller's
static int info_launch(int device, int bps, int B, int ld, int64_t S, const double *lappr, const uint8_t *word, int A,
                       const InfoScales &al, double *loss, int32_t *errors, double *total, int64_t *total_errors,
                       void *workspace, hipStream_t s) {
    Cursor c{(uintptr_t)workspace};
    double *wloss;
    int32_t *werr;
    info_workspace(c, bps, ld, S, A, &wloss, &werr);
    const int64_t nq = info_chunks(S);
    {
        ProfScope ps("lappr_info", s);
        const int64_t items = nq * bps * (ld / kWave);
        k_lappr_info<<<demap_wave_grid(device, (items + 3) / 4), 256, 0, s>>>(bps, B, ld, S, A, al, lappr, word, wloss, werr);
        QR_LAUNCH_CHECK();
    }
    {
        ProfScope ps("lappr_info_total", s);
        k_lappr_info_total<<<dim3((unsigned)(A + 1), (unsigned)bps), kInfoTotalThreads, 0, s>>>(bps, B, ld, nq, A, wloss, werr, loss, errors,
                                                                                 total, total_errors);
        QR_LAUNCH_CHECK();
    }
    return QR_OK;
}

}  // namespace qr

// ===================================================================== C-ABI
using namespace qr;

extern "C" {

int qr_lappr_info_workspace_size(int32_t bps, int32_t ld, int64_t S, int32_t A, size_t *bytes) {
    if (!bytes) return set_error(QR_EVALUE, "null output pointer");
    *bytes = 0;
    if (int rc = info_check_shape(bps, ld, S, A)) return rc;
    Cursor c{0};
    double *wloss;
    int32_t *werr;
    info_workspace(c, bps, ld, S, A, &wloss, &werr);
    *bytes = c.off;
    return QR_OK;
}

int qr_lappr_info_device(int32_t bps, int32_t B, int32_t ld, int64_t S, const double *d_lappr, const uint8_t *d_word,
                         int32_t A, const double *alphas, double *d_loss, int32_t *d_errors, double *d_total,
                         int64_t *d_total_errors, void *d_workspace, size_t workspace_bytes, void *stream) {
    if (int rc = info_check_shape(bps, ld, S, A)) return rc;
    if (B < 1 || B > ld) return set_error(QR_EVALUE, "need 0 < B <= ld (B=%d ld=%d)", B, ld);
    InfoScales al;
    if (int rc = info_scales(A, alphas, al)) return rc;
    if (!d_lappr || !d_word || !d_loss || !d_errors || !d_total || !d_total_errors)
        return set_error(QR_EVALUE, "null pointer argument");
    size_t need = 0;
    (void)qr_lappr_info_workspace_size(bps, ld, S, A, &need);
    if (!d_workspace || workspace_bytes < need)
        return set_error(QR_EVALUE, "workspace too small: %zu bytes, need %zu (qr_lappr_info_workspace_size)", workspace_bytes,
                         need);
    if (!ws_aligned(d_workspace)) return set_error(QR_EVALUE, "workspace must be 256-byte aligned");
    int device = 0;   // no handle: the caller's current device, as the other handle-free *_device entries
    QR_HIP(hipGetDevice(&device));
    return info_launch(device, bps, B, ld, S, d_lappr, d_word, A, al, d_loss, d_errors, d_total, d_total_errors, d_workspace,
                       (hipStream_t)stream);
}

// One frame from host memory, interleaved as the reference holds it (v = s * bps + k): that is column
// 0 of the [V, 64] frame-innermost layout, so the arrays go up as they are, the transposes of the
// batch interface put them into that column, and the same two kernels run with B = 1.  With one frame
// total[a][k] = 0.0 + loss[a][k][0] and total_errors[k] = errors[k][0]: those come down.
int qr_lappr_info_host(int32_t device, int32_t bps, int64_t S, const double *lappr, const uint8_t *word, int32_t A,
                       const double *alphas, double *loss, int64_t *errors) {
    if (int rc = info_check_shape(bps, kWave, S, A)) return rc;
    InfoScales al;
    if (int rc = info_scales(A, alphas, al)) return rc;
    if (!lappr || !word || !loss || !errors) return set_error(QR_EVALUE, "null pointer argument");
    if (S * bps > (int64_t)1 << 30) return set_error(QR_EVALUE, "S * bit_per_symbol too large for one host frame");
    int count = 0;
    QR_HIP(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return set_error(QR_EVALUE, "no device %d (%d visible)", device, count);
    // no handle: the scratch of this entry alone; never destroyed (a static destructor would call into
    // a HIP runtime that may be gone)
    static Scratch *scratch = new Scratch;
    HostTrip t(*scratch, device);
    if (scratch->ptr && scratch->device != device) {   // another device than last time: start over there
        DeviceGuard g(scratch->device);
        (void)hipFree(scratch->ptr);
        scratch->ptr = nullptr;
        scratch->bytes = 0;
    }
    scratch->device = device;
    const size_t V = (size_t)S * (size_t)bps;
    size_t ws = 0;
    (void)qr_lappr_info_workspace_size(bps, kWave, S, A, &ws);
    double *d_l, *d_lfi, *d_loss, *d_total;
    uint8_t *d_w, *d_wfi, *d_ws;
    int32_t *d_err;
    int64_t *d_terr;
    if (!t.take(&d_l, V, &d_lfi, V * kWave, &d_w, V, &d_wfi, V * kWave, &d_loss, (size_t)A * bps * kWave, &d_err,
                (size_t)bps * kWave, &d_total, (size_t)A * bps, &d_terr, (size_t)bps, &d_ws, ws))
        return t.rc;
    t.up(d_l, lappr, V);
    t.up(d_w, word, V);
    if (t.ok()) t.rc = launch_transpose_to_fi_f64(1, kWave, (int64_t)V, d_l, d_lfi, nullptr);
    if (t.ok()) t.rc = launch_transpose_to_fi_u8(1, kWave, (int64_t)V, d_w, d_wfi, nullptr);
    if (t.ok())
        t.rc = info_launch(device, bps, 1, kWave, S, d_lfi, d_wfi, A, al, d_loss, d_err, d_total, d_terr, d_ws, nullptr);
    t.down(loss, (const double *)d_total, (size_t)A * bps);
    t.down(errors, (const int64_t *)d_terr, (size_t)bps);
    return t.rc;
}

}  // extern "C"
