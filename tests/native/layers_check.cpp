// The layers of the layered decode schedule (host_build.hpp build_layers) under AddressSanitizer +
// UndefinedBehaviorSanitizer (tests/test_layered_cpu.py builds this stand-alone program with
// -Xarch_host -fsanitize=address,undefined and -fno-sanitize-recover).
//
//   layers_check FILE...      each FILE: "E" then E lines "vid cid" (edge e = line e)
//
// For every edge list: no two checks of a layer share a variable; every check's layer is the
// smallest one free of its variables among the checks before it (first-fit in ascending check id);
// the (layer, degree) segments come in schedule order, their lists are ascending, of their degree
// and layer, and cover every check exactly once; the repeat flag is set exactly for the checks
// that hold a variable more than once.  Prints "NAME: layers=L sizes=a,b,..." per code.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "host_build.hpp"

using namespace qr;

static int fails = 0;
#define EXPECT(c, ...)                    \
    do {                                  \
        if (!(c)) {                       \
            printf("FAIL: " __VA_ARGS__); \
            printf("\n");                 \
            ++fails;                      \
        }                                 \
    } while (0)

static bool read_edges(const char *path, std::vector<int64_t> &vid, std::vector<int64_t> &cid) {
    FILE *f = fopen(path, "r");
    if (!f) return false;
    long long E = 0;
    bool ok = fscanf(f, "%lld", &E) == 1 && E > 0;
    for (long long e = 0; ok && e < E; ++e) {
        long long v, c;
        ok = fscanf(f, "%lld %lld", &v, &c) == 2;
        vid.push_back(v);
        cid.push_back(c);
    }
    fclose(f);
    return ok;
}

static void check_layers(const char *name, const std::vector<int64_t> &vid, const std::vector<int64_t> &cid) {
    TannerCsr t;
    std::string err;
    const int rc = build_tanner_csr(vid.data(), cid.data(), (int64_t)vid.size(), (int64_t)cid.size(), t, err);
    EXPECT(rc == QR_OK, "%s: build_tanner_csr: %s", name, err.c_str());
    if (rc != QR_OK) return;
    Layers L;
    build_layers(t, L);
    const int64_t C = t.C;
    EXPECT((int64_t)L.layer_of.size() == C && (int64_t)L.repeat.size() == C && (int64_t)L.checks.size() == C,
           "%s: array sizes", name);
    if ((int64_t)L.layer_of.size() != C || (int64_t)L.repeat.size() != C || (int64_t)L.checks.size() != C) return;
    // first-fit, restated with sets: vars[l] = the variables of the checks placed in layer l so far
    std::vector<std::set<int32_t>> vars;
    for (int64_t c = 0; c < C; ++c) {
        std::set<int32_t> mine;
        bool rep = false;
        for (int32_t k = t.chk_ptr[c]; k < t.chk_ptr[c + 1]; ++k) rep |= !mine.insert(t.chk_var[(size_t)k]).second;
        EXPECT((L.repeat[(size_t)c] != 0) == rep, "%s: check %lld repeat flag %d", name, (long long)c, L.repeat[(size_t)c]);
        const int32_t l = L.layer_of[(size_t)c];
        EXPECT(l >= 0 && l < L.n_layers, "%s: check %lld in layer %d of %d", name, (long long)c, l, L.n_layers);
        if (l < 0 || l >= L.n_layers) continue;
        auto shares = [&](int32_t layer) {
            if (layer >= (int32_t)vars.size()) return false;
            for (int32_t v : mine)
                if (vars[(size_t)layer].count(v)) return true;
            return false;
        };
        EXPECT(!shares(l), "%s: check %lld shares a variable with its layer %d", name, (long long)c, l);
        for (int32_t lower = 0; lower < l; ++lower)
            EXPECT(shares(lower), "%s: check %lld is in layer %d but layer %d is free", name, (long long)c, l, lower);
        if (l >= (int32_t)vars.size()) vars.resize((size_t)l + 1);
        vars[(size_t)l].insert(mine.begin(), mine.end());
    }
    EXPECT((int32_t)vars.size() == L.n_layers, "%s: %zu layers in use, n_layers %d", name, vars.size(), L.n_layers);
    // the segments: schedule order, ascending lists, every check once
    std::vector<char> seen((size_t)C, 0);
    int64_t off = 0;
    int32_t last_layer = -1, last_deg = -1;
    for (const LayerSeg &g : L.segs) {
        EXPECT(g.n > 0 && g.off == off && g.off + g.n <= C, "%s: segment (%d, %d) at %lld + %lld", name, g.layer, g.degree,
               (long long)g.off, (long long)g.n);
        EXPECT(g.layer > last_layer || (g.layer == last_layer && g.degree > last_deg), "%s: segment (%d, %d) out of order",
               name, g.layer, g.degree);
        last_layer = g.layer;
        last_deg = g.degree;
        if (g.off != off || g.n <= 0 || g.off + g.n > C) break;
        for (int64_t j = 0; j < g.n; ++j) {
            const int32_t c = L.checks[(size_t)(g.off + j)];
            EXPECT(c >= 0 && c < C, "%s: segment (%d, %d) lists check %d", name, g.layer, g.degree, c);
            if (c < 0 || c >= C) continue;
            EXPECT(!seen[(size_t)c], "%s: check %d listed twice", name, c);
            seen[(size_t)c] = 1;
            EXPECT(L.layer_of[(size_t)c] == g.layer && t.chk_ptr[(size_t)c + 1] - t.chk_ptr[(size_t)c] == g.degree,
                   "%s: check %d in segment (%d, %d)", name, c, g.layer, g.degree);
            EXPECT(j == 0 || c > L.checks[(size_t)(g.off + j - 1)], "%s: segment (%d, %d) not ascending", name, g.layer,
                   g.degree);
        }
        off += g.n;
    }
    EXPECT(off == C, "%s: the segments hold %lld of %lld checks", name, (long long)off, (long long)C);
    std::vector<int64_t> sizes((size_t)L.n_layers, 0);
    for (int64_t c = 0; c < C; ++c) sizes[(size_t)L.layer_of[(size_t)c]]++;
    printf("%s: layers=%d sizes=", name, L.n_layers);
    for (size_t l = 0; l < sizes.size(); ++l) printf("%s%lld", l ? "," : "", (long long)sizes[l]);
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 2) {
        printf("usage: layers_check FILE...\n");
        return 2;
    }
    for (int a = 1; a < argc; ++a) {
        std::vector<int64_t> vid, cid;
        if (!read_edges(argv[a], vid, cid)) {
            printf("FAIL: cannot read %s\n", argv[a]);
            ++fails;
            continue;
        }
        check_layers(argv[a], vid, cid);
    }
    if (fails) {
        printf("layers_check: %d failures\n", fails);
        return 1;
    }
    printf("layers_check ok: %d codes\n", argc - 1);
    return 0;
}
