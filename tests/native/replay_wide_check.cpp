// Host harness, the wide twin of replay_check.cpp: the fast g_inv_search (Newton + replayed
// bisection) must return bit-identical doubles to the brute-force reference search outside the
// uniform 2..16-PAM, -2..40 dB box too.  The tables come from the library's own build_demap_host
// (host_build.hpp), so the regime a configuration lands in (quantile + Taylor table, quantile
// table only, no tables) is the one qr_demap_create would choose, and is printed.
//
//   replay_wide_check <draws per grid configuration> [fixture case dump]
//
// Configurations: every case of the dump (written by tests/test_demap_replay.py from
// tests/golden/demap_wide.npz: "case <bps> <noise_var>" and the lines a / thr / p / sign), then the
// grid bps 1..5 x {uniform, shaped} x {-12, 3, 25, 50, 70, 80} dB with random sign configurations.
// Targets are drawn as in replay_check.cpp, its adversarial draws on the bisection grid included.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "host_build.hpp"

namespace {

struct Totals {
    long draws = 0, mism = 0, fallback = 0;
};

std::mt19937_64 g(24680);
qr::MathTables mt;

// One configuration: `draws` targets, as replay_check.cpp draws them.  "plain" counts the uniform
// draws that are neither an edge target (0 / 1, 1e-12-deep tail) nor adversarial.
void run(const char *label, int bps, const std::vector<double> &a, const std::vector<double> &thr,
         const std::vector<double> &p, double nv, const std::vector<uint8_t> &sign, double snr, long draws,
         Totals &tot) {
    qr::DemapTables t;
    std::vector<double2> quant;
    std::vector<double> ftab;
    std::string err;
    if (qr::build_demap_host(bps, a.data(), p.data(), thr.data(), nv, sign.data(), t, quant, ftab, err) != QR_OK) {
        printf("BUILD FAILED %s bps=%d: %s\n", label, bps, err.c_str());
        ++tot.mism;
        return;
    }
    t.quant = quant.empty() ? nullptr : quant.data();   // host pointers (the library uploads them)
    t.ftab = ftab.empty() ? nullptr : ftab.data();
    const int M = t.M;
    bool uniform = true;
    for (int i = 1; i < M; ++i) uniform = uniform && p[i] == p[0];
    std::uniform_real_distribution<double> U(0.0, 1.0);
    long mism = 0, fallback = 0, plain = 0, plain_fallback = 0;
    for (long d = 0; d < draws; ++d) {
        double n = U(g);
        const int i = (int)(g() % M);
        bool is_plain = true;
        if (d % 97 == 0) { n = (d % 2) ? 0.0 : 1.0; is_plain = false; }
        if (d % 101 == 0) { n = U(g) * 1e-12; is_plain = false; }
        if (d % 3 == 1) {
            // adversarial: the root sits within ~1e-12 of a bisection grid point
            // (lo + j 2^-30), where the window decisions need exact F_Y
            const double l = fmax(t.thr[i], t.a[i] - 3.0), h = fmin(t.thr[i + 1], t.a[i] + 3.0);
            const double y0 = l + U(g) * (h - l);
            const double off[] = {0.0, 1e-15, -1e-15, 1e-13, -1e-13, 3e-12, -3e-12, 1e-11};
            const double yg = ldexp(floor(ldexp(y0, 30)), -30) + off[g() % 8];
            const double T = qr::single_F_Y(t, yg);
            const double na = t.sign[i] ? (t.Fthr[i + 1] - T) / t.dF[i] : (T - t.Fthr[i]) / t.dF[i];
            if (na >= 0.0 && na <= 1.0) { n = na; is_plain = false; }
        }
        const double ref = qr::g_inv_search(t, n, i);
        double ystar, W;
        const bool have = qr::newton_root(t, mt, qr::search_target(t, n, i), i, ystar, W);
        const double fast = qr::g_inv_search_fast(t, mt, n, i);
        if (!have) ++fallback;
        if (is_plain) {
            ++plain;
            if (!have) ++plain_fallback;
        }
        if (memcmp(&ref, &fast, 8) != 0 && !(std::isnan(ref) && std::isnan(fast))) {
            if (mism < 5)
                printf("MISMATCH %s bps=%d snr=%g n=%.17g i=%d ref=%.17g fast=%.17g have=%d W=%g\n", label, bps, snr, n,
                       i, ref, fast, (int)have, have ? W : 0.0);
            ++mism;
        }
    }
    printf("cfg %s bps=%d snr=%.4g uniform=%d quant=%d ftab=%d ftab_n=%d draws=%ld plain=%ld plain_fallbacks=%ld "
           "fallbacks=%ld mismatches=%ld\n", label, bps, snr, (int)uniform, (int)!quant.empty(), (int)!ftab.empty(),
           ftab.empty() ? 0 : t.ftab_n, draws, plain, plain_fallback, fallback, mism);
    fflush(stdout);
    tot.draws += draws;
    tot.mism += mism;
    tot.fallback += fallback;
}

double variance(const std::vector<double> &a, const std::vector<double> &p) {
    double Es = 0;
    for (size_t i = 0; i < a.size(); ++i) Es += p[i] * (a[i] * a[i]);   // alphabet.pyx:66-67
    return Es;
}

bool read_doubles(FILE *f, const char *tag, int n, std::vector<double> &v) {
    char word[32];
    if (fscanf(f, "%31s", word) != 1 || strcmp(word, tag) != 0) return false;
    v.resize(n);
    for (int i = 0; i < n; ++i) {
        char num[64];
        if (fscanf(f, "%63s", num) != 1) return false;
        v[i] = strtod(num, nullptr);   // hexadecimal floats: exact
    }
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    const long draws = argc > 1 ? atol(argv[1]) : 1500;
    qr::build_math_tables(&mt);
    Totals tot;
    if (argc > 2) {
        FILE *f = fopen(argv[2], "r");
        if (!f) { printf("cannot open %s\n", argv[2]); return 2; }
        char word[32];
        int c = 0;
        while (fscanf(f, "%31s", word) == 1) {
            int bps = 0;
            char nvs[64];
            if (strcmp(word, "case") != 0 || fscanf(f, "%d %63s", &bps, nvs) != 2 || bps < 1 || bps > qr::kMaxBps) {
                printf("bad dump at case %d\n", c);
                return 2;
            }
            const int M = 1 << bps;
            const double nv = strtod(nvs, nullptr);
            std::vector<double> a, thr, p, sg;
            if (!read_doubles(f, "a", M, a) || !read_doubles(f, "thr", M + 1, thr) || !read_doubles(f, "p", M, p) ||
                !read_doubles(f, "sign", M, sg)) {
                printf("bad dump at case %d\n", c);
                return 2;
            }
            std::vector<uint8_t> sign(M);
            for (int i = 0; i < M; ++i) sign[i] = (uint8_t)(sg[i] != 0.0);
            const double snr = -10.0 * log10(2.0 * nv / variance(a, p));
            char label[32];
            snprintf(label, sizeof label, "fixture%d", c);
            // without a quantile table (M > 32) both searches are the brute-force loops, M erf per
            // step: fewer draws, what such a case reports is its regime
            run(label, bps, a, thr, p, nv, sign, snr, M > 32 ? std::max(draws * 512 / ((long)M * M), 20L) : draws, tot);
            ++c;
        }
        fclose(f);
    }
    for (int bps = 1; bps <= 5; ++bps) {
        const int M = 1 << bps;
        for (int shaped = 0; shaped < 2; ++shaped) {
            std::vector<double> a(M), thr(M + 1), p(M);
            // p_m ~ exp(-nu (a_m - 1/2)^2): not symmetric, so that 2-PAM is shaped too
            const double nu[] = {0.3, 0.1, 0.05, 0.01, 0.003};
            double sum = 0;
            for (int i = 0; i < M; ++i) {
                a[i] = ((double)i - (double)(M - 1) / 2.0) * 2.0;
                p[i] = shaped ? exp(-nu[bps - 1] * (a[i] - 0.5) * (a[i] - 0.5)) : 1.0 / M;
                sum += p[i];
            }
            if (shaped) {
                // in-order sum exactly 1.0 (F_Y(+inf)): the residual off the largest entry
                int big = 0;
                for (int i = 0; i < M; ++i) { p[i] /= sum; if (p[i] > p[big]) big = i; }
                for (int it = 0; it < 64; ++it) {
                    double s = 0;
                    for (int i = 0; i < M; ++i) s += p[i];
                    if (s == 1.0) break;
                    p[big] -= s - 1.0;
                }
            }
            for (int i = 1; i < M; ++i) thr[i] = a[i] - 1.0;
            thr[0] = a[0] * 100;
            thr[M] = a[M - 1] * 100;
            for (double snr : {-12.0, 3.0, 25.0, 50.0, 70.0, 80.0}) {
                std::vector<uint8_t> sign(M);
                for (int i = 0; i < M; ++i) sign[i] = (uint8_t)(g() & 1);
                const double nv = variance(a, p) * pow(10.0, -snr / 10) / 2;
                run("grid", bps, a, thr, p, nv, sign, snr, draws, tot);
            }
        }
    }
    printf("total draws=%ld mismatches=%ld fallbacks=%ld\n", tot.draws, tot.mism, tot.fallback);
    return tot.mism ? 1 : 0;
}
