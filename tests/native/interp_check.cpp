// Host harness of the interpolation grid (csrc/grid_interp.hpp: the very functions the kernels of
// demap_interp.hip and mi.hip and qr_demap_grid_create run), compiled by
// tests/test_interp_native_cpu.py with hipcc as host code (once plain, once with the address and
// undefined-behaviour sanitizers).  Input: raw doubles dumped by the test from tests/golden/interp.npz.
//
//   interp_check case IN OUT    one fixture case: builds the grid (grid_geometry, grid_point,
//                               public_F_Y) and writes y[n] then F[n] to OUT for the test to hash;
//                               grid_g_inv with both index-search bodies against the fixture's g_inv
//                               values, grid_demap_symbol with both against its formulation-1
//                               LAPPRs, bit for bit (NaN matches NaN)
//   interp_check property SEED  seeded tables of every length 2..70, ties and decreasing runs
//                               included: grid_binsearch returns binsearch_thr's index; on the
//                               nondecreasing ones body (b) returns body (a)'s result bit for bit
//                               at coarse-table segment sizes 2..16
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "qamr.h"
#include "glibc_math.hpp"
#include "qamr_math.hpp"
#include "host_build.hpp"
#include "grid_interp.hpp"

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

// a table with its coarse table, as qr_demap_grid_create lays them out
struct HostTable {
    std::vector<double2> pairs;
    std::vector<double> coarse;
    qr::GridView view(int seg_shift) {
        const int n = (int)pairs.size(), nc = ((n - 1) >> seg_shift) + 1;
        coarse.resize((size_t)nc);
        for (int c = 0; c < nc; ++c) coarse[(size_t)c] = pairs[(size_t)c << seg_shift].x;
        return qr::GridView{pairs.data(), coarse.data(), n, nc, seg_shift, pairs.back().x, pairs.back().y};
    }
    bool nondecreasing() const {
        for (size_t r = 0; r + 1 < pairs.size(); ++r)
            if (!(pairs[r + 1].x >= pairs[r].x)) return false;
        return true;
    }
};

static int check_case(const char *in_path, const char *out_path) {
    Reader in(in_path);
    const double *hd = in.take(5);   // bps, noise_var, trunkation_threshold, n_intervals_per_step, step
    const int bps = (int)hd[0];
    if (bps < 1 || bps > qr::kMaxBps) { puts("FAIL bad header"); return 1; }
    const int M = 1 << bps;
    const double *a = in.take(M), *p = in.take(M), *thr = in.take(M + 1), *cfgd = in.take(M);
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
    const qr::GridGeometry geo = qr::grid_geometry(t, hd[2], hd[3], hd[4]);
    if (!(geo.n_points >= 2 && geo.n_points <= (double)(1 << 26))) { puts("FAIL point count out of range"); return 1; }
    const int n = (int)geo.n_points;
    HostTable tb;
    tb.pairs.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        const double y = qr::grid_point(geo.y_low, geo.y_high, geo.lin_step, n, i);
        tb.pairs[(size_t)i].x = qr::public_F_Y(t, y);
        tb.pairs[(size_t)i].y = y;
    }
    FILE *fo = fopen(out_path, "wb");
    if (!fo) { printf("FAIL cannot write %s\n", out_path); return 1; }
    for (int i = 0; i < n; ++i) fwrite(&tb.pairs[(size_t)i].y, 8, 1, fo);
    for (int i = 0; i < n; ++i) fwrite(&tb.pairs[(size_t)i].x, 8, 1, fo);
    fclose(fo);
    const bool nd = tb.nondecreasing();
    printf("grid         %10d points, nondecreasing %d\n", n, (int)nd);
    if (!nd) { puts("FAIL the table decreases somewhere: body (b) does not apply"); return 1; }
    const qr::GridView g = tb.view(4);   // 16 entries per segment, the default

    long bad = 0, cnt = 0;
    const int n3 = (int)in.one();
    const double *n300 = in.take((size_t)n3), *ginv = in.take((size_t)M * n3);
    for (int i = 0; i < M; ++i)
        for (int q = 0; q < n3; ++q) {
            const double ref = ginv[(size_t)i * n3 + q];
            const double ga = qr::grid_g_inv<false>(t, g, g.coarse, n300[q], i);
            const double gb = qr::grid_g_inv<true>(t, g, g.coarse, n300[q], i);
            cnt += 2;
            if (!same(ga, ref) || !same(gb, ref)) {
                if (bad < 5) printf("  g_inv mismatch at n_hat=%a i=%d: ref=%a (a)=%a (b)=%a\n", n300[q], i, ref, ga, gb);
                bad += !same(ga, ref) + !same(gb, ref);
            }
        }
    printf("g_inv        %10ld values, %ld mismatches\n", cnt, bad);

    qr::GlibcTables GT;
    qr::build_glibc_tables(&GT);
    auto ex = [&](double v) { return qr::g_exp_full(v, GT); };
    auto lg = [&](double v) { return qr::g_log_full(v, GT); };
    long badl = 0, cntl = 0;
    const int n2 = (int)in.one();
    const double *n2000 = in.take((size_t)n2), *j2000 = in.take((size_t)n2), *la = in.take((size_t)n2 * bps);
    for (int s = 0; s < n2; ++s) {
        const int j = (int)j2000[s];
        if (j < 0 || j >= M) { puts("FAIL symbol index out of range in the input"); return 1; }
        double oa[qr::kMaxBps], ob[qr::kMaxBps];
        qr::grid_demap_symbol<false>(t, g, g.coarse, n2000[s], j, ex, lg, oa);
        qr::grid_demap_symbol<true>(t, g, g.coarse, n2000[s], j, ex, lg, ob);
        for (int k = 0; k < bps; ++k) {
            const double ref = la[(size_t)s * bps + k];
            cntl += 2;
            if (!same(oa[k], ref) || !same(ob[k], ref)) {
                if (badl < 5) printf("  formulation-1 mismatch at s=%d k=%d: ref=%a (a)=%a (b)=%a\n", s, k, ref, oa[k], ob[k]);
                badl += !same(oa[k], ref) + !same(ob[k], ref);
            }
        }
    }
    printf("formulation1 %10ld values, %ld mismatches\n", cntl, badl);
    if (!in.end()) { puts("FAIL trailing data in the input file"); return 1; }
    if (bad || badl) puts("FAIL the host evaluation differs from the fixture");
    return bad || badl ? 1 : 0;
}

static int check_property(unsigned long seed) {
    std::mt19937_64 rng(seed);
    auto uni = [&]() { return (double)(rng() >> 11) * 0x1p-53; };
    const double nan = std::numeric_limits<double>::quiet_NaN();
    long tables = 0, idx = 0, bad_idx = 0, val = 0, bad_val = 0;
    for (int n = 2; n <= 70; ++n)
        for (int kind = 0; kind < 6; ++kind) {
            // kind 0..2: nondecreasing (strictly increasing / with tied runs / mostly ties);
            // kind 3..5: any order (decreasing runs, ties among them)
            HostTable tb;
            tb.pairs.resize((size_t)n);
            double F = uni() - 0.5;
            for (int r = 0; r < n; ++r) {
                const double u = uni();
                if (kind == 0) F += 0.01 + u;
                else if (kind == 1) F += u < 0.4 ? 0.0 : u;
                else if (kind == 2) F += u < 0.85 ? 0.0 : 1.0;
                else if (kind == 3) F += u - 0.5;
                else if (kind == 4) F += u < 0.3 ? 0.0 : u < 0.6 ? -0.25 : 0.5;
                else F -= u < 0.2 ? 0.0 : u;
                tb.pairs[(size_t)r].x = F;
                tb.pairs[(size_t)r].y = 3.0 * r + uni();
            }
            if (kind >= 3 && tb.nondecreasing()) tb.pairs[(size_t)n - 1].x = tb.pairs[(size_t)n - 2].x - 1.0;
            ++tables;
            const bool nd = tb.nondecreasing();
            if (nd != (kind < 3)) { puts("FAIL the generator's table kinds"); return 1; }
            std::vector<double> Fs((size_t)n), targets;
            double lo = tb.pairs[0].x, hi = lo;
            for (int r = 0; r < n; ++r) {
                Fs[(size_t)r] = tb.pairs[(size_t)r].x;
                lo = std::fmin(lo, Fs[(size_t)r]);
                hi = std::fmax(hi, Fs[(size_t)r]);
                targets.push_back(Fs[(size_t)r]);
                targets.push_back(std::nextafter(Fs[(size_t)r], -HUGE_VAL));
                targets.push_back(std::nextafter(Fs[(size_t)r], HUGE_VAL));
                if (r) targets.push_back(0.5 * (Fs[(size_t)r - 1] + Fs[(size_t)r]));
            }
            const double inf = std::numeric_limits<double>::infinity();
            for (double v : {lo - 1.0, hi + 1.0, -inf, inf, Fs[0] - 1.0, Fs[(size_t)n - 1] + 1.0, nan}) targets.push_back(v);
            for (int k = 0; k < 8; ++k) targets.push_back(lo + (hi - lo) * uni());
            for (int seg = 1; seg <= 4; ++seg) {
                const qr::GridView g = tb.view(seg);
                for (double v : targets) {
                    if (seg == 1) {
                        ++idx;
                        const int want = qr::binsearch_thr(Fs.data(), n, v), got = qr::grid_binsearch(g, v);
                        if (want != got) {
                            if (bad_idx++ < 5) printf("  index mismatch: n=%d kind=%d val=%a binsearch_thr=%d grid_binsearch=%d\n", n, kind, v, want, got);
                        }
                    }
                    const double ra = qr::grid_g_inv_val<false>(g, g.coarse, v);   // NaN: body (a) only
                    if (!nd || v != v) continue;
                    ++val;
                    const double rb = qr::grid_g_inv_val<true>(g, g.coarse, v);
                    if (!same(ra, rb)) {
                        if (bad_val++ < 5) printf("  body mismatch: n=%d kind=%d seg_shift=%d val=%a (a)=%a (b)=%a\n", n, kind, seg, v, ra, rb);
                    }
                }
            }
        }
    printf("property     %10ld tables, %ld index comparisons, %ld mismatches; %ld body comparisons, %ld mismatches\n", tables,
           idx, bad_idx, val, bad_val);
    if (bad_idx || bad_val) puts("FAIL the index search bodies disagree");
    return bad_idx || bad_val ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc >= 4 && !strcmp(argv[1], "case")) return check_case(argv[2], argv[3]);
    if (argc >= 3 && !strcmp(argv[1], "property")) return check_property(strtoul(argv[2], nullptr, 10));
    puts("usage: interp_check case IN OUT | interp_check property SEED");
    return 2;
}
