// Host harness of the quad-integrated mutual-information evaluators, compiled by
// tests/test_mi_quad_cpu.py with hipcc as host code (once plain, once with the address and
// undefined-behaviour sanitizers).  Input: raw doubles dumped by the test from tests/golden/mi_quad.npz.
//
//   mi_quad_check integrator FILE   the host driver (mi_quad.hpp QuadState over mi_math.hpp's rules, the
//                                   code qr_quad_host and qr_mi_quad_batch run) on the fixture's
//                                   integrator-only records: result and abserr bit-equal to scipy's,
//                                   neval equal, (ier != 0) == warned
//   mi_quad_check case FILE         mi_base_arg / mi_xy_arg (the functions the kernel calls) at the
//                                   fixture's abscissae with host providers -- y_hat by grid_interp.hpp's g_inv
//                                   (the kernels' own) on a host-built grid, the restated glibc exp / log2 -- bit-equal to the
//                                   fixture's values; with the header's flag set, also both integrals
//                                   wholly on the host through the same driver, bit-equal
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "qamr.h"
#include "glibc_math.hpp"
#include "qamr_math.hpp"
#include "host_build.hpp"
#include "grid_interp.hpp"
#include "mi_math.hpp"
#include "mi_quad.hpp"

static uint64_t bits(double x) {
    uint64_t u;
    memcpy(&u, &x, 8);
    return u;
}
static bool same(double a, double b) { return bits(a) == bits(b) || (std::isnan(a) && std::isnan(b)); }

struct Reader {
    std::vector<double> d;
    size_t at = 0;
    explicit Reader(const char *path) {
        FILE *fp = fopen(path, "rb");
        if (!fp) { printf("FAIL cannot open %s\n", path); exit(1); }
        double buf[4096];
        size_t got;
        while ((got = fread(buf, 8, 4096, fp)) > 0) d.insert(d.end(), buf, buf + got);
        fclose(fp);
    }
    const double *take(size_t n) {
        if (at + n > d.size()) { puts("FAIL input file too short"); exit(1); }
        const double *p = d.data() + at;
        at += n;
        return p;
    }
    double one() { return *take(1); }
    bool end() const { return at == d.size(); }
};

struct Outcome {
    double result, abserr;
    int neval, ier, last;
};

template <class F>
static Outcome integrate(F f, bool infinite, double a, double b, double epsabs, double epsrel, int limit) {
    qr::QuadState q;
    if (infinite) q.start(0.0, 1.0, epsabs, epsrel, limit, true);
    else q.start(a, b, epsabs, epsrel, limit, false);
    int feeds = 0;
    while (!q.done) {
        double ia[2], ib[2], r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int nh = q.pending(ia, ib);
        for (int h = 0; h < nh; ++h) {
            if (infinite) qr::quad_rule_15i(f, ia[h], ib[h], r + 4 * h);
            else qr::quad_rule_21(f, ia[h], ib[h], r + 4 * h);
            qr::quad_rule_tail(r + 4 * h);
        }
        q.feed(r, r + 4);
        if (++feeds > limit) { puts("FAIL the driver did not end within `limit` rounds"); exit(1); }
    }
    return Outcome{q.result, q.abserr, q.neval, q.ier, q.last};
}

static long compare(const char *what, const Outcome &o, double I, double abserr, double neval, double warned) {
    const bool ok = same(o.result, I) && same(o.abserr, abserr) && o.neval == (int)neval && (o.ier != 0) == (warned != 0.0);
    if (!ok)
        printf("  %s mismatch: got I=%a abserr=%a neval=%d ier=%d, expected I=%a abserr=%a neval=%d warned=%d\n", what,
               o.result, o.abserr, o.neval, o.ier, I, abserr, (int)neval, (int)warned);
    return ok ? 0 : 1;
}

static int check_integrator(const char *path) {
    Reader in(path);
    const int n = (int)in.one();
    long bad = 0;
    int warned_n = 0;
    for (int r = 0; r < n; ++r) {
        const double *h = in.take(10);   // fn, inf, c, w, limit, eps, result, abserr, neval, warned
        const int fn = (int)h[0];
        const double c = h[2], w = h[3];
        auto f = [&](double x) {
            switch (fn) {
                case 0: return 1.0 / (w * w + (x - c) * (x - c));
                case 1: return sqrt(fabs(x - c));
                case 2: return 1.0 / sqrt(fabs(x - c) + 1e-300);
                default: return (x > c ? 1.0 : 0.0) + x * x;
            }
        };
        const Outcome o = integrate(f, h[1] != 0.0, 0.0, 1.0, h[5], h[5], (int)h[4]);
        char what[64];
        snprintf(what, sizeof what, "record %d (fn %d, inf %d, limit %d)", r, fn, (int)h[1], (int)h[4]);
        bad += compare(what, o, h[6], h[7], h[8], h[9]);
        warned_n += o.ier != 0;
    }
    if (!in.end()) { puts("FAIL trailing data in the input file"); return 1; }
    printf("integrator   %10d records, %ld mismatches, %d with ier != 0\n", n, bad, warned_n);
    if (bad) puts("FAIL the host driver differs from scipy.integrate.quad");
    return bad ? 1 : 0;
}

// The grid of noisemapper.pyx:135-144 on the host, as qr_demap_grid_create builds it (grid_interp.hpp).
static std::vector<double2> build_grid(const qr::DemapTables &t, double trunc, double nips, double step) {
    const qr::GridGeometry geo = qr::grid_geometry(t, trunc, nips, step);
    const int n = (int)geo.n_points;
    std::vector<double2> pairs((size_t)n);
    for (int i = 0; i < n; ++i) {
        pairs[(size_t)i].y = qr::grid_point(geo.y_low, geo.y_high, geo.lin_step, n, i);
        pairs[(size_t)i].x = qr::public_F_Y(t, pairs[(size_t)i].y);
    }
    return pairs;
}

static int check_case(const char *path) {
    Reader in(path);
    const double *hd = in.take(7);   // bps, noise_var, limit, trunkation_threshold, n_intervals_per_step, step, integrals?
    const int bps = (int)hd[0], limit = (int)hd[2];
    const bool integrals = hd[6] != 0.0;
    if (bps < 1 || bps > 6 || limit < 1) { puts("FAIL bad header"); return 1; }
    const int M = 1 << bps;
    const double *a = in.take(M), *p = in.take(M), *thr = in.take(M + 1), *cfgd = in.take(M), *pX = in.take(M);
    std::vector<uint8_t> cfg(M);
    for (int i = 0; i < M; ++i) cfg[i] = (uint8_t)cfgd[i];
    qr::DemapTables t;
    std::vector<double2> quant;
    std::vector<double> ftab;
    std::string err;
    if (qr::build_demap_host(bps, a, p, thr, hd[1], cfg.data(), t, quant, ftab, err)) {
        printf("FAIL build_demap_host: %s\n", err.c_str());
        return 1;
    }
    const std::vector<double2> pairs = build_grid(t, hd[3], hd[4], hd[5]);
    const qr::GridView grid{pairs.data(), nullptr, (int)pairs.size(), 0, 0, pairs.back().x, pairs.back().y};   // body (a): no coarse table
    qr::GlibcTables GT;
    qr::build_glibc_tables(&GT);
    static const qr::GlibcLog2 L2 = QR_GLIBC_LOG2_INIT;
    auto ex = [&](double v) { return qr::g_exp_full(v, GT); };
    auto lg = [&](double v) { return qr::g_log2_full(v, L2); };
    auto base = [&](double n) {
        double yh[64];
        for (int i = 0; i < M; ++i) yh[i] = qr::grid_g_inv<false>(t, grid, nullptr, n, i);
        return qr::mi_base_arg(t, pX, M, [&](int i) { return yh[i]; }, ex, lg);
    };
    auto xy = [&](double y) { return qr::mi_xy_arg(t, M, y, ex, lg); };
    long bad = 0, npts = 0;
    for (int kind = 0; kind < 2; ++kind) {
        const int n = (int)in.one();
        const double *x = in.take((size_t)n), *f = in.take((size_t)n);
        for (int k = 0; k < n; ++k) {
            const double got = kind == 0 ? base(x[k]) : xy(x[k]);
            ++npts;
            if (!same(got, f[k])) {
                if (bad < 5) printf("  %s integrand mismatch at x=%a: ref=%a got=%a\n", kind ? "X_Y" : "base", x[k], f[k], got);
                ++bad;
            }
        }
    }
    printf("integrands   %10ld points, %ld mismatches\n", npts, bad);
    const double *rb = in.take(4), *rx = in.take(4);   // I, abserr, neval, warned
    if (integrals) {
        long badi = compare("base integral", integrate(base, false, 0.0, 1.0, 1.49e-8, 1.49e-8, limit), rb[0], rb[1], rb[2], rb[3]);
        badi += compare("X_Y integral", integrate(xy, true, 0.0, 1.0, 1.49e-8, 1.49e-8, limit), rx[0], rx[1], rx[2], rx[3]);
        printf("integrals    %10d on the host, %ld mismatches\n", 2, badi);
        bad += badi;
    }
    if (!in.end()) { puts("FAIL trailing data in the input file"); return 1; }
    if (bad) puts("FAIL the host evaluation differs from the fixture");
    return bad ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc >= 3 && !strcmp(argv[1], "integrator")) return check_integrator(argv[2]);
    if (argc >= 3 && !strcmp(argv[1], "case")) return check_case(argv[2]);
    puts("usage: mi_quad_check integrator FILE | mi_quad_check case FILE");
    return 2;
}
