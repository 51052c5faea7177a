// binary_channel.hip -- the channel front ends of the code-evaluation simulations
// (sims/sim_decode.py, sims/sim_direct.py, sims/sim_bsc.py): the decoder's input LLRs of a
// binary-input AWGN channel (soft and hard-decided) and of a binary symmetric channel, and the
// `final < 0` error count those scripts use.  Frame-innermost planes [V][ld], one lane per
// (v, f) with f innermost; columns [B, ld) are neither read nor written.
#include "qamr_internal.hpp"

namespace qr {

// numpy.sign of a double: -1, 0, +1; +0.0 for -0.0; a NaN stays a NaN.
__device__ __forceinline__ double np_sign(double x) { return x > 0 ? 1.0 : (x < 0 ? -1.0 : (x == 0 ? 0.0 : x)); }

// sim_decode.py:98-100 (soft): coef * (((-2 w) + 1) + vsqrt * z), coef = 2 alpha / v, and :69-71 (hard):
// coef * sign((1 - 2 w) + vsqrt * z), coef = LLR0.  Every product and sum is rounded on its own
// (-ffp-contract=off); the last product is a multiply in both forms, so inf * 0 and NaN come out as
// IEEE gives them.
template <bool kHard>
__global__ void __launch_bounds__(256) k_biawgn_llr(double coef, double vsqrt, int B, int ld, int64_t V,
                                                    const uint8_t *__restrict__ word, const double *__restrict__ z,
                                                    double *__restrict__ llr) {
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t v = item / ld;
    const int f = (int)(item - v * ld);
    if (v >= V || f >= B) return;
    const double bpsk = word[item] ? -1.0 : 1.0;       // 1 - 2 w, exact
    const double y = bpsk + vsqrt * z[item];
    llr[item] = coef * (kHard ? np_sign(y) : y);
}

// sim_bsc.py:58-61: coef * (1 - 2 (w ^ (u < rber))), coef = log2(1 - rber) - log2(rber).  rx, when
// given, receives the channel output w ^ flip.
__global__ void __launch_bounds__(256) k_bsc_llr(double coef, double rber, int B, int ld, int64_t V,
                                                 const uint8_t *__restrict__ word, const double *__restrict__ u,
                                                 double *__restrict__ llr, uint8_t *__restrict__ rx) {
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t v = item / ld;
    const int f = (int)(item - v * ld);
    if (v >= V || f >= B) return;
    const uint8_t r = (uint8_t)((word[item] ? 1 : 0) ^ (u[item] < rber ? 1 : 0));
    llr[item] = coef * (r ? -1.0 : 1.0);
    if (rx) rx[item] = r;
}

// check_shape plus the bound of a one-dimensional grid of 256-lane workgroups over V * ld items.
static int plane_grid(int B, int ld, int64_t V, unsigned *grid) {
    if (int rc = check_shape(B, ld, V)) return rc;
    const int64_t blocks = (V * ld + 255) / 256;
    if (blocks > 0x7fffffff) return set_error(QR_EVALUE, "V * ld = %lld is too large for one launch", (long long)(V * ld));
    *grid = (unsigned)blocks;
    return QR_OK;
}

}  // namespace qr

using namespace qr;

extern "C" {

int qr_biawgn_llr_device(int32_t hard, double coef, double vsqrt, int32_t B, int32_t ld, int64_t V,
                         const uint8_t *d_word, const double *d_z, double *d_llr, void *stream) {
    if (!d_word || !d_z || !d_llr) return set_error(QR_EVALUE, "qr_biawgn_llr_device: null pointer argument");
    unsigned grid = 0;
    if (int rc = plane_grid(B, ld, V, &grid)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("biawgn_llr", s);
    if (hard) k_biawgn_llr<true><<<grid, 256, 0, s>>>(coef, vsqrt, B, ld, V, d_word, d_z, d_llr);
    else k_biawgn_llr<false><<<grid, 256, 0, s>>>(coef, vsqrt, B, ld, V, d_word, d_z, d_llr);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

int qr_bsc_llr_device(double coef, double rber, int32_t B, int32_t ld, int64_t V, const uint8_t *d_word,
                      const double *d_u, double *d_llr, uint8_t *d_rx_or_null, void *stream) {
    if (!d_word || !d_u || !d_llr) return set_error(QR_EVALUE, "qr_bsc_llr_device: null pointer argument");
    unsigned grid = 0;
    if (int rc = plane_grid(B, ld, V, &grid)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("bsc_llr", s);
    k_bsc_llr<<<grid, 256, 0, s>>>(coef, rber, B, ld, V, d_word, d_u, d_llr, d_rx_or_null);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

int qr_count_errors_neg_device(int32_t B, int32_t ld, int64_t K, const double *d_final, const uint8_t *d_word,
                               const uint8_t *d_success, const int32_t *d_iters, int32_t *d_frame_errors,
                               int64_t *d_counters, void *stream) {
    if (!d_final || !d_word || !d_success || !d_iters || !d_frame_errors || !d_counters)
        return set_error(QR_EVALUE, "qr_count_errors_neg_device: null pointer argument");
    return launch_count_errors(true, B, ld, K, d_final, d_word, d_success, d_iters, d_frame_errors, d_counters,
                               (hipStream_t)stream);
}

}  // extern "C"
