// rate_adapt.hip -- rate adaptation of one mother code (puncturing, shortening, blind rounds;
// DESIGN.md "Rate adaptation") for gfx950.  Not a reference interface: the reference has no rate
// adaptation; the definition below is this project's (qamr/rate_adapt.py expand_host is its
// normative statement) and the results are bit-exact against it.
//
//   slot[v] >= 0 : variable v is payload row slot[v]; it takes that row's LAPPR and bit, bit for bit
//   slot[v] <  0 : variable v is filler j = -1 - slot[v] (j < s shortened, else punctured);
//                  bit   = fill[j][f] != 0
//                  known = j < s + max(revealed[f], 0)          (revealed absent: 0)
//                  lappr = known ? (bit ? -L : +L) : +0.0
//
// The layout is the decoder's frame-innermost [rows, ld]: the expand is a row gather, and a row's
// slot is uniform across its frames.
#include "qamr_internal.hpp"
#include "debug_check.hpp"

namespace qr {

enum RaDebugSite {         // 31..34: density_evolution.hip (DeDebugSite)
    kDbgRaOutRow = 35,     // k_rate_adapt_expand: the output row v outside [0, V)
    kDbgRaPayRow = 36,     // k_rate_adapt_expand: a payload row outside [0, n)
    kDbgRaFiller = 37,     // k_rate_adapt_expand: a filler index outside [0, p + s)
    kDbgRaCountRow = 38,   // k_count_errors_rows: a listed row below 0, or its place in the list outside [0, n_rows)
};

constexpr int kRaThreads = 256;
constexpr int kRaPairs = 4;                                // 16-byte LAPPR accesses per lane
constexpr int kRaCols = kRaThreads * 2 * kRaPairs;         // frames per workgroup: 2048
static_assert(kRaCols == kRaThreads * 8, "one 8-byte access of bits per lane covers the same frames");

// bytes of x that are not zero -> 1, the others 0
__device__ inline uint64_t nonzero_bytes(uint64_t x) {
    const uint64_t m = 0x7f7f7f7f7f7f7f7full;
    return ((((x & m) + m) | x) >> 7) & 0x0101010101010101ull;
}

// the first (B - f) of the 8 bytes of x to dst[0..]: the tail of a row that ends inside the access
__device__ inline void store_bytes(uint8_t *dst, uint64_t x, int count) {
    for (int i = 0; i < count; ++i) dst[i] = (uint8_t)(x >> (8 * i));
}

// k_rate_adapt_expand: workgroup (v, c) writes the frames [c * kRaCols, (c + 1) * kRaCols) of row v.
// The row's slot is read at a workgroup-uniform address (one scalar load), so the branch on it is
// uniform.  A lane moves kRaPairs pairs of LAPPRs (16 bytes each, all loads ahead of the stores) and
// 8 frames' bits (one 8-byte access); a pair or an octet that crosses B is stored element by element,
// so columns [B, ld) keep what they hold.  The loads of such a pair or octet stay inside the row:
// ld is a multiple of 64.  Every offset is formed in 64 bits (V * ld * 8 passes 2^31 at N = 64 800,
// ld = 4 096).
__global__ void __launch_bounds__(kRaThreads)
k_rate_adapt_expand(int64_t V, int64_t n, int64_t nfill, int64_t s, const int32_t *__restrict__ slot, int B, int ld,
                    const double *__restrict__ lappr_pay, const uint8_t *__restrict__ word_pay,
                    const uint8_t *__restrict__ fill, const int32_t *__restrict__ revealed, double L,
                    double *__restrict__ lappr, uint8_t *__restrict__ word) {
    const int64_t v = blockIdx.x;
    QR_DCHECK(v >= 0 && v < V, kDbgRaOutRow, v, V);
    const int sl = slot[v];
    const int tid = threadIdx.x;
    const int c0 = (int)blockIdx.y * kRaCols;
    double *__restrict__ dst = lappr + v * (int64_t)ld;
    uint8_t *__restrict__ wdst = word + v * (int64_t)ld;
    const int fb = c0 + tid * 8;   // this lane's 8 frames of bits
    if (sl >= 0) {                 // workgroup-uniform
        QR_DCHECK(sl < n, kDbgRaPayRow, sl, n);
        const double *__restrict__ src = lappr_pay + (int64_t)sl * ld;
        const uint8_t *__restrict__ wsrc = word_pay + (int64_t)sl * ld;
        double2 x[kRaPairs];
#pragma unroll
        for (int u = 0; u < kRaPairs; ++u) {
            const int f = c0 + (u * kRaThreads + tid) * 2;
            if (f < B) x[u] = *reinterpret_cast<const double2 *>(src + f);
        }
        uint64_t bits = 0;
        if (fb < B) bits = *reinterpret_cast<const uint64_t *>(wsrc + fb);
#pragma unroll
        for (int u = 0; u < kRaPairs; ++u) {
            const int f = c0 + (u * kRaThreads + tid) * 2;
            if (f + 1 < B) *reinterpret_cast<double2 *>(dst + f) = x[u];
            else if (f < B) dst[f] = x[u].x;
        }
        if (fb + 7 < B) *reinterpret_cast<uint64_t *>(wdst + fb) = bits;
        else if (fb < B) store_bytes(wdst + fb, bits, B - fb);
    } else {
        const int64_t j = -1 - (int64_t)sl;
        QR_DCHECK(j >= 0 && j < nfill, kDbgRaFiller, j, nfill);
        const uint8_t *__restrict__ fsrc = fill + j * (int64_t)ld;
        const int64_t short_of = j - s;   // known iff max(revealed, 0) > j - s
        uchar2 b[kRaPairs];
        int2 r[kRaPairs];
#pragma unroll
        for (int u = 0; u < kRaPairs; ++u) {
            const int f = c0 + (u * kRaThreads + tid) * 2;
            r[u] = make_int2(0, 0);
            if (f < B) {
                b[u] = *reinterpret_cast<const uchar2 *>(fsrc + f);
                if (revealed) r[u] = make_int2(revealed[f], revealed[f + 1]);
            }
        }
        uint64_t bits = 0;
        if (fb < B) bits = nonzero_bytes(*reinterpret_cast<const uint64_t *>(fsrc + fb));
#pragma unroll
        for (int u = 0; u < kRaPairs; ++u) {
            const int f = c0 + (u * kRaThreads + tid) * 2;
            if (f < B) {
                const int64_t r0 = r[u].x > 0 ? r[u].x : 0, r1 = r[u].y > 0 ? r[u].y : 0;
                double2 o;
                o.x = r0 > short_of ? (b[u].x ? -L : L) : 0.0;
                o.y = r1 > short_of ? (b[u].y ? -L : L) : 0.0;
                if (f + 1 < B) *reinterpret_cast<double2 *>(dst + f) = o;
                else dst[f] = o.x;
            }
        }
        if (fb + 7 < B) *reinterpret_cast<uint64_t *>(wdst + fb) = bits;
        else if (fb < B) store_bytes(wdst + fb, bits, B - fb);
    }
}

// k_count_errors (demap.hip) over the listed rows: utils.pyx:27-40 (lappr >= 0 decides bit 0, so a
// NaN decides 1) at the rows rows[0 .. n_rows), kpb of them per workgroup.  A row's index is read at a
// workgroup-uniform address.
__global__ void __launch_bounds__(256)
k_count_errors_rows(int B, int ld, int64_t n_rows, int64_t kpb, const int32_t *__restrict__ rows,
                    const double *__restrict__ fin, const uint8_t *__restrict__ word, int32_t *__restrict__ ferr) {
    const int f = blockIdx.y * blockDim.x + threadIdx.x;
    if (f >= B) return;
    const int64_t i0 = (int64_t)blockIdx.x * kpb;
    const int64_t i1 = (i0 + kpb < n_rows) ? i0 + kpb : n_rows;
    int32_t cnt = 0;
    for (int64_t i = i0; i < i1; ++i) {
        const int64_t v = rows[i];
        QR_DCHECK(v >= 0 && i >= 0 && i < n_rows, kDbgRaCountRow, v, i);
        const uint8_t w = word[v * ld + f];
        const double x = fin[v * ld + f];
        cnt += (x >= 0) ? w : 1 - w;
    }
    if (cnt) atomicAdd(&ferr[f], cnt);
}

}  // namespace qr

// ===================================================================== C-ABI
using namespace qr;

extern "C" {

int qr_rate_adapt_expand_device(int64_t V, int64_t n, int64_t p, int64_t s, const int32_t *d_slot, int32_t B, int32_t ld,
                                const double *d_lappr_pay, const uint8_t *d_word_pay, const uint8_t *d_fill,
                                const int32_t *d_revealed_or_null, double L, double *d_lappr, uint8_t *d_word,
                                void *stream) {
    if (!d_slot || !d_lappr_pay || !d_word_pay || !d_fill || !d_lappr || !d_word)
        return set_error(QR_EVALUE, "qr_rate_adapt_expand_device: null pointer argument");
    if (int rc = check_shape(B, ld, 1)) return rc;
    if (n < 1 || p < 0 || s < 0 || V > INT32_MAX || n + p + s != V)
        return set_error(QR_EVALUE, "need n >= 1, p >= 0, s >= 0, n + p + s == V < 2^31 (V=%lld n=%lld p=%lld s=%lld)",
                         (long long)V, (long long)n, (long long)p, (long long)s);
    if (!(L - L == 0.0) || !(L > 0.0)) return set_error(QR_EVALUE, "the shortened LAPPR must be finite and positive");
    if ((((uintptr_t)d_lappr_pay | (uintptr_t)d_lappr) & 15) || (((uintptr_t)d_word_pay | (uintptr_t)d_fill | (uintptr_t)d_word) & 7))
        return set_error(QR_EVALUE, "the LAPPR arrays must be 16-byte aligned, the bit arrays 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("rate_adapt_expand", st);
    dim3 grid((unsigned)V, (unsigned)((B + kRaCols - 1) / kRaCols));
    k_rate_adapt_expand<<<grid, kRaThreads, 0, st>>>(V, n, p + s, s, d_slot, B, ld, d_lappr_pay, d_word_pay, d_fill,
                                                     d_revealed_or_null, L, d_lappr, d_word);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

int qr_count_errors_rows_device(int32_t B, int32_t ld, int64_t n_rows, const int32_t *d_rows, const double *d_final,
                                const uint8_t *d_word, const uint8_t *d_success, const int32_t *d_iters,
                                int32_t *d_frame_errors, int64_t *d_counters, void *stream) {
    if (!d_rows || !d_final || !d_word || !d_success || !d_iters || !d_frame_errors || !d_counters)
        return set_error(QR_EVALUE, "qr_count_errors_rows_device: null pointer argument");
    if (int rc = check_shape(B, ld, 1)) return rc;
    if (n_rows < 0) return set_error(QR_EVALUE, "n_rows must be >= 0");
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("count_rows", st);
    QR_HIP(hipMemsetAsync(d_frame_errors, 0, (size_t)B * 4, st));
    if (n_rows > 0) {
        const int ft = frame_tile(ld);
        const int64_t kpb = 64;
        dim3 grid((unsigned)((n_rows + kpb - 1) / kpb), (unsigned)(ld / ft));
        k_count_errors_rows<<<grid, ft, 0, st>>>(B, ld, n_rows, kpb, d_rows, d_final, d_word, d_frame_errors);
        QR_LAUNCH_CHECK();
    }
    return launch_count_finish(B, d_frame_errors, d_success, d_iters, d_counters, st);
}

}  // extern "C"
