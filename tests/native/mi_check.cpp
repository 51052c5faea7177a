// Host harness of the mutual-information estimator's arithmetic, compiled by tests/test_mi_cpu.py
// with hipcc as host code (once plain, once with the address and undefined-behaviour sanitizers):
//
//   mi_check log2 N          g_log2_full (glibc_math.hpp) against libm's log2, bit for bit, on > 4 N
//                            inputs: log-uniform on [2^-60, 2^60], the near-1 window of e_log2.c and
//                            its edges, [0.5, 2], random bit patterns, subnormals, every special case
//   mi_check sample FILE     mi_sample_terms (mi_math.hpp, the function the kernel calls) fed the
//                            fixture's x, x_hat, y and y_hat[k] (tests/golden/mi.npz, dumped by the
//                            test as raw doubles): terms and the sequential block totals must equal
//                            the fixture's bit for bit; mi_bob must return the fixture's x_hat.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "qamr.h"
#include "glibc_math.hpp"
#include "qamr_math.hpp"
#include "host_build.hpp"
#include "mi_math.hpp"

static uint64_t bits(double x) {
    uint64_t u;
    memcpy(&u, &x, 8);
    return u;
}
static double from_bits(uint64_t u) {
    double x;
    memcpy(&x, &u, 8);
    return x;
}
static bool same(double a, double b) { return bits(a) == bits(b) || (std::isnan(a) && std::isnan(b)); }

struct Count {
    const char *what;
    long n = 0, bad = 0;
    void check(double ref, double got, double arg) {
        ++n;
        if (!same(ref, got)) {
            if (bad < 5) printf("  %s mismatch: arg=%a ref=%a got=%a\n", what, arg, ref, got);
            ++bad;
        }
    }
    long report() const {
        printf("%-12s %10ld inputs, %ld mismatches\n", what, n, bad);
        return bad;
    }
};

static int check_log2(long n) {
    static const qr::GlibcLog2 T = QR_GLIBC_LOG2_INIT;
    std::mt19937_64 g(29);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    Count c{"log2"};
    auto one = [&](double x) { c.check(log2(x), qr::g_log2_full(x, T), x); };
    const double lo = 1.0 - 0x1.5b51p-5, hi = 1.0 + 0x1.6ab2p-5;
    for (long i = 0; i < n; ++i) {
        one(exp2(-60.0 + 120.0 * U(g)));                       // dense on [2^-60, 2^60]
        one(lo - 0x1p-8 + (hi - lo + 0x1p-7) * U(g));          // the near-1 window and a margin
        one(0.5 + 1.5 * U(g));
        one(from_bits(g()));                                   // every exponent, both signs, NaNs
        if ((i & 3) == 0) one(from_bits(g() & 0x000FFFFFFFFFFFFFull));   // subnormals
        if ((i & 3) == 1) one(1.0 + (2 * U(g) - 1) * exp2(-52.0 * U(g)));   // towards 1 from both sides
    }
    for (int k = 0; k <= 64; ++k) {   // the 64 table intervals' edges, at several exponents
        const uint64_t z = 0x3FE6000000000000ull + ((uint64_t)k << 46);
        for (int e : {-1022, -500, -1, 0, 1, 37, 1000})
            for (int64_t d = -2; d <= 2; ++d) one(ldexp(from_bits(z + (uint64_t)d), e));
    }
    const double sp[] = {0.0, -0.0, (double)INFINITY, -(double)INFINITY, std::nan(""), -std::nan(""), 1.0, 2.0, 0.5, -1.0,
                         lo, hi, 0x1p-1022, 0x1p-1074, 0x1.fffffffffffffp1023, 0x0.fffffffffffffp-1022, -0x1p-1074,
                         0x1p-1023, 3.0, 1e-300, 1e300};
    for (double x : sp)
        for (double v : {x, nextafter(x, 0.0), nextafter(x, (double)INFINITY), nextafter(x, -(double)INFINITY)}) one(v);
    const long bad = c.report();
    if (bad) puts("FAIL g_log2_full differs from libm's log2");
    return bad ? 1 : 0;
}

static int check_sample(const char *path) {
    FILE *fp = fopen(path, "rb");
    if (!fp) { printf("FAIL cannot open %s\n", path); return 1; }
    std::vector<double> d;
    double buf[4096];
    size_t got;
    while ((got = fread(buf, 8, 4096, fp)) > 0) d.insert(d.end(), buf, buf + got);
    fclose(fp);
    size_t at = 0;
    auto take = [&](size_t n) {
        if (at + n > d.size()) { puts("FAIL input file too short"); exit(1); }
        const double *p = d.data() + at;
        at += n;
        return p;
    };
    const double *hd = take(4);
    const int bps = (int)hd[0], nblk = (int)hd[1], S = (int)hd[2];
    const double noise_var = hd[3];
    if (bps < 1 || bps > 6 || nblk < 1 || S < 1) { puts("FAIL bad header"); return 1; }
    const int M = 1 << bps;
    const double *a = take(M), *p = take(M), *thr = take(M + 1), *cfgd = take(M), *pX = take(M), *fw = take((size_t)M * M);
    std::vector<uint8_t> cfg(M);
    for (int i = 0; i < M; ++i) cfg[i] = (uint8_t)cfgd[i];
    qr::DemapTables t;
    std::vector<double2> quant;
    std::vector<double> ftab;
    std::string err;
    if (qr::build_demap_host(bps, a, p, thr, noise_var, cfg.data(), t, quant, ftab, err)) {
        printf("FAIL build_demap_host: %s\n", err.c_str());
        return 1;
    }
    t.quant = nullptr;   // the per-sample function reads neither
    t.ftab = nullptr;
    if (bits(t.two_s2) != bits(2.0 * noise_var)) { puts("FAIL two_s2 is not 2.0 * noise_var"); return 1; }
    qr::GlibcTables GT;
    qr::build_glibc_tables(&GT);
    static const qr::GlibcLog2 L2 = QR_GLIBC_LOG2_INIT;
    Count ct{"terms"}, cs{"totals"}, cw{"which"};
    long bad_xhat = 0;
    for (int b = 0; b < nblk; ++b) {
        const double *x = take(S), *xh = take(S), *y = take(S), *yh = take((size_t)S * M), *terms = take((size_t)3 * S),
                     *totals = take(3);
        double I[3] = {0.0, 0.0, 0.0};
        for (int q = 0; q < S; ++q) {
            int xhat;
            double nhat;
            qr::mi_bob(t, y[q], xhat, nhat);
            if (xhat != (int)xh[q]) ++bad_xhat;
            for (unsigned which : {7u, 5u, 2u}) {
                double out[3] = {0.0, 0.0, 0.0};
                bool put[3] = {false, false, false};
                qr::mi_sample_terms(
                    t, pX, fw, M, which, (int)x[q], (int)xh[q], y[q], [&](int k) { return yh[(size_t)q * M + k]; },
                    [&](double v) { return qr::g_exp_full(v, GT); }, [&](double v) { return qr::g_log2_full(v, L2); },
                    [&](int k, double v) { out[k] = v; put[k] = true; });
                for (int k = 0; k < 3; ++k) {
                    const bool on = (which >> k) & 1u;
                    if (which == 7u) ct.check(terms[k * S + q], out[k], y[q]);
                    else cw.check(on ? terms[k * S + q] : 0.0, out[k], y[q]);   // enabled ones unchanged
                    if (put[k] != on) { puts("FAIL a disabled term was put (or an enabled one was not)"); return 1; }
                }
                if (which == 7u) {
                    I[0] += out[0];
                    I[1] += out[1];
                    I[2] -= out[2];
                }
            }
        }
        for (int k = 0; k < 3; ++k) cs.check(totals[k], I[k] / (double)S, (double)b);
    }
    if (at != d.size()) { puts("FAIL trailing data in the input file"); return 1; }
    long bad = ct.report() + cs.report() + cw.report();
    printf("x_hat        %10ld samples, %ld mismatches\n", (long)nblk * S, bad_xhat);
    bad += bad_xhat;
    if (bad) puts("FAIL mi_sample_terms differs from the fixture");
    return bad ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc >= 3 && !strcmp(argv[1], "log2")) return check_log2(atol(argv[2]));
    if (argc >= 3 && !strcmp(argv[1], "sample")) return check_sample(argv[2]);
    puts("usage: mi_check log2 N | mi_check sample FILE");
    return 2;
}
