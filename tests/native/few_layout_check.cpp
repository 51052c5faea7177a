// The message-slot layout of the node-parallel decodes (host_build.hpp build_few_layout) under
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_few_cpu.py builds this stand-alone
// program with -Xarch_host -fsanitize=address,undefined and -fno-sanitize-recover).
//
//   few_layout_check FILE...      each FILE: "E" then E lines "vid cid" (edge e = line e)
//
// For every edge list: the classes are the check degrees in ascending order with consecutive
// bases; the slots base_k + i n_k + j of all (check, edge position) pairs form a bijection with
// the edges; every variable's slot list names its own edges in ascending edge id; a single-class
// code gives i C + c.
#include <cstdio>
#include <cstdlib>
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

static void check_layout(const char *name, const std::vector<int64_t> &vid, const std::vector<int64_t> &cid) {
    TannerCsr t;
    std::string err;
    const int rc = build_tanner_csr(vid.data(), cid.data(), (int64_t)vid.size(), (int64_t)cid.size(), t, err);
    EXPECT(rc == QR_OK, "%s: build_tanner_csr: %s", name, err.c_str());
    if (rc != QR_OK) return;
    FewLayout L;
    build_few_layout(t, L);
    const int64_t E = t.E;
    EXPECT((int64_t)L.var_slot.size() == E, "%s: %zu slots for %lld edges", name, L.var_slot.size(), (long long)E);
    // classes: ascending degree, every check in one, consecutive bases
    int64_t base = 0, checks = 0;
    int32_t last = 0;
    for (const FewClass &k : L.classes) {
        EXPECT(k.degree > last && k.degree < (int)t.by_deg.size() && k.n == (int64_t)t.by_deg[k.degree].size() && k.n > 0,
               "%s: class of degree %d with %lld checks", name, k.degree, (long long)k.n);
        EXPECT(k.base == base, "%s: class of degree %d starts at %lld, not %lld", name, k.degree, (long long)k.base,
               (long long)base);
        last = k.degree;
        base += k.n * k.degree;
        checks += k.n;
    }
    EXPECT(base == E && checks == t.C, "%s: the classes hold %lld edges, %lld checks", name, (long long)base,
           (long long)checks);
    // the slots of all (check, edge position) pairs <-> the edges
    std::vector<int32_t> edge_of_slot((size_t)E, -1);
    for (const FewClass &k : L.classes) {
        for (int64_t j = 0; j < k.n; ++j) {
            const int32_t c = t.by_deg[k.degree][(size_t)j];
            EXPECT(j == 0 || c > t.by_deg[k.degree][(size_t)j - 1], "%s: class %d not in ascending check id", name, k.degree);
            for (int i = 0; i < k.degree; ++i) {
                const int64_t s = k.base + (int64_t)i * k.n + j;
                EXPECT(s >= 0 && s < E, "%s: slot %lld outside [0, E)", name, (long long)s);
                if (s < 0 || s >= E) continue;
                EXPECT(edge_of_slot[(size_t)s] < 0, "%s: slot %lld taken twice", name, (long long)s);
                edge_of_slot[(size_t)s] = t.chk_edge[(size_t)(t.chk_ptr[c] + i)];
            }
        }
    }
    std::vector<char> seen((size_t)E, 0);
    for (int64_t s = 0; s < E; ++s) {
        const int32_t e = edge_of_slot[(size_t)s];
        EXPECT(e >= 0 && e < E && !seen[(size_t)e], "%s: slot %lld holds edge %d", name, (long long)s, e);
        if (e >= 0 && e < E) seen[(size_t)e] = 1;
    }
    // per variable: its own edges, ascending edge id, each by its slot
    for (int64_t v = 0; v < t.V; ++v) {
        for (int32_t k = t.var_ptr[v]; k < t.var_ptr[v + 1]; ++k) {
            const int32_t s = L.var_slot[(size_t)k];
            EXPECT(s >= 0 && s < E, "%s: variable %lld lists slot %d", name, (long long)v, s);
            if (s < 0 || s >= E) continue;
            const int32_t e = edge_of_slot[(size_t)s];
            EXPECT(e == t.var_edge[(size_t)k] && vid[(size_t)e] == v, "%s: variable %lld entry %d: slot %d holds edge %d",
                   name, (long long)v, k, s, e);
            EXPECT(k == t.var_ptr[v] || e > edge_of_slot[(size_t)L.var_slot[(size_t)k - 1]],
                   "%s: variable %lld not in ascending edge id", name, (long long)v);
        }
    }
    // one class: edge position i of check c at i C + c
    if (L.classes.size() == 1) {
        for (int64_t c = 0; c < t.C; ++c)
            for (int32_t p = t.chk_ptr[c]; p < t.chk_ptr[c + 1]; ++p) {
                const int32_t e = t.chk_edge[(size_t)p];
                EXPECT(edge_of_slot[(size_t)((p - t.chk_ptr[c]) * t.C + c)] == e, "%s: check %lld position %d", name,
                       (long long)c, p - t.chk_ptr[c]);
            }
    }
    printf("%s: V=%lld C=%lld E=%lld classes=%zu\n", name, (long long)t.V, (long long)t.C, (long long)E, L.classes.size());
}

int main(int argc, char **argv) {
    if (argc < 2) {
        printf("usage: few_layout_check FILE...\n");
        return 2;
    }
    for (int a = 1; a < argc; ++a) {
        std::vector<int64_t> vid, cid;
        if (!read_edges(argv[a], vid, cid)) {
            printf("FAIL: cannot read %s\n", argv[a]);
            ++fails;
            continue;
        }
        check_layout(argv[a], vid, cid);
    }
    if (fails) {
        printf("few_layout_check: %d failures\n", fails);
        return 1;
    }
    printf("few_layout_check ok: %d codes\n", argc - 1);
    return 0;
}
