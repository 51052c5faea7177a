// host_build.hpp -- the host-side construction steps of libqamr, free of HIP runtime
// calls so that they also build and run in a sanitizer harness
// (tests/native/host_asan_check.cpp, tests/test_sanitizers.py):
//
//   build_tanner_csr   Decoder.__cinit__ / __build_table (decoder.pyx:60-146): O(E) stable
//                      counting sort of the edge list into int32 CSR per check and per
//                      variable (ascending edge id), checks grouped by degree;
//   build_few_layout   the message slots of the node-parallel decodes (frame-resident, few-frame);
//   build_layers       the first-fit layers of the layered decode schedule and their check lists;
//   build_demap_host   NoiseMapper.__cinit__ tables (noisemapper.pyx:103-236) plus the
//                      Newton-start and Taylor tables of the fast root search.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "qamr.h"
#include "qamr_math.hpp"

namespace qr {

struct TannerCsr {
    int64_t E = 0, V = 0, C = 0;
    int32_t max_dc = 0, max_dv = 0;
    std::vector<int32_t> chk_ptr, chk_edge, chk_var, var_ptr, var_edge;
    std::vector<std::vector<int32_t>> by_deg;  // check ids per degree, ascending
};

// Returns QR_OK or an error code with `err` set (the messages of the reference where it
// has one: decoder.pyx:96-97 "Sizes don't match").
inline int build_tanner_csr(const int64_t *e_to_v, const int64_t *e_to_c, int64_t nv, int64_t nc, TannerCsr &t,
                            std::string &err) {
    auto fail = [&](int code, const char *fmt, long long a = 0, long long b = 0) {
        char buf[256];
        snprintf(buf, sizeof buf, fmt, a, b);
        err = buf;
        return code;
    };
    if (nv != nc) return fail(QR_EVALUE, "Sizes don't match");
    const int64_t E = nv;
    if (E <= 0) return fail(QR_EVALUE, "empty edge list");
    if (!e_to_v || !e_to_c) return fail(QR_EVALUE, "null edge list");
    if (E >= (int64_t)1 << 31) return fail(QR_EUNSUPPORTED, "more than 2^31-1 edges");
    int64_t V = 0, C = 0;
    for (int64_t e = 0; e < E; ++e) {
        if (e_to_v[e] < 0 || e_to_c[e] < 0) return fail(QR_EVALUE, "negative node id at edge %lld", e);
        if (e_to_v[e] >= ((int64_t)1 << 31) - 1 || e_to_c[e] >= ((int64_t)1 << 31) - 1)
            return fail(QR_EUNSUPPORTED, "node ids exceed int32 (edge %lld)", e);
        V = std::max(V, e_to_v[e] + 1);
        C = std::max(C, e_to_c[e] + 1);
    }
    t.E = E;
    t.V = V;
    t.C = C;
    // Stable counting sort by node id == the ascending scan of __build_table (decoder.pyx:69-87).
    t.chk_ptr.assign(C + 1, 0);
    t.var_ptr.assign(V + 1, 0);
    t.chk_edge.resize(E);
    t.chk_var.resize(E);
    t.var_edge.resize(E);
    for (int64_t e = 0; e < E; ++e) {
        t.chk_ptr[e_to_c[e] + 1]++;
        t.var_ptr[e_to_v[e] + 1]++;
    }
    for (int64_t i = 0; i < C; ++i) t.chk_ptr[i + 1] += t.chk_ptr[i];
    for (int64_t i = 0; i < V; ++i) t.var_ptr[i + 1] += t.var_ptr[i];
    {
        std::vector<int32_t> fc(t.chk_ptr.begin(), t.chk_ptr.end() - 1), fv(t.var_ptr.begin(), t.var_ptr.end() - 1);
        for (int64_t e = 0; e < E; ++e) {
            const int32_t kc = fc[e_to_c[e]]++;
            t.chk_edge[kc] = (int32_t)e;
            t.chk_var[kc] = (int32_t)e_to_v[e];  // c_to_v (decoder.pyx:128-129)
            t.var_edge[fv[e_to_v[e]]++] = (int32_t)e;
        }
    }
    t.max_dc = t.max_dv = 0;
    t.by_deg.clear();
    for (int64_t c = 0; c < C; ++c) {
        const int32_t d = t.chk_ptr[c + 1] - t.chk_ptr[c];
        if (d < 2)
            return fail(QR_EVALUE,
                        "check node %lld has degree %lld; degree < 2 is undefined behaviour in the reference "
                        "(decoder.pyx:135-141) and is rejected",
                        c, d);
        t.max_dc = std::max(t.max_dc, d);
        if ((int)t.by_deg.size() <= d) t.by_deg.resize(d + 1);
        t.by_deg[d].push_back((int32_t)c);
    }
    for (int64_t v = 0; v < V; ++v) t.max_dv = std::max(t.max_dv, t.var_ptr[v + 1] - t.var_ptr[v]);
    return QR_OK;
}

// Message slots of the node-parallel decodes (decode_small.hip: k_resident's LDS messages; decode_few.hip: the
// few-frame schedule's frame-major msg[f][slot]).  The check classes are the non-empty degrees of
// by_deg in ascending order; edge position i of the j-th check of class k (n_k checks, the ids of
// by_deg in ascending order) lives at slot base_k + i n_k + j, base_k = the edges of the classes
// before k: the lanes of a check sweep (consecutive checks of one class) touch consecutive
// doubles for each i.  var_slot lists every variable's slots in ascending edge id, indexed by
// var_ptr like var_edge.  A single-class code gives i C + c.  O(E), no HIP call.
struct FewClass {
    int32_t degree;
    int64_t n, base;
};
struct FewLayout {
    std::vector<FewClass> classes;
    std::vector<int32_t> var_slot;
};
inline void build_few_layout(const TannerCsr &t, FewLayout &L) {
    L.classes.clear();
    std::vector<int32_t> slot_of_edge((size_t)t.E);
    int64_t base = 0;
    for (size_t d = 0; d < t.by_deg.size(); ++d) {
        const int64_t n = (int64_t)t.by_deg[d].size();
        if (!n) continue;
        for (int64_t j = 0; j < n; ++j) {
            const int32_t b = t.chk_ptr[(size_t)t.by_deg[d][(size_t)j]];
            for (int64_t i = 0; i < (int64_t)d; ++i)
                slot_of_edge[(size_t)t.chk_edge[(size_t)(b + i)]] = (int32_t)(base + i * n + j);
        }
        L.classes.push_back(FewClass{(int32_t)d, n, base});
        base += n * (int64_t)d;
    }
    L.var_slot.resize((size_t)t.E);
    for (int64_t k = 0; k < t.E; ++k) L.var_slot[(size_t)k] = slot_of_edge[(size_t)t.var_edge[(size_t)k]];
}

// The layers of the layered (serial-check) decode schedule (decode_layered.hip), first-fit in
// ascending check id: layer_of[c] is the smallest l >= 0 such that no check c' < c of layer l
// shares a variable with c, so the checks of one layer touch disjoint posteriors and may run in
// any order.  The schedule order is (layer_of[c], c).  segs lists every non-empty (layer, check
// degree) in that order (ascending degree within a layer); its checks are checks[off, off + n),
// ascending.  repeat[c] = 1 iff check c holds a variable more than once (parallel edges): its
// second edge reads the posterior its first edge has just written.
// used[l] marks the variables of layer l, so a check costs its degree per layer tried:
// O(E layers) time, V bytes per layer.  No HIP call.
struct LayerSeg {
    int32_t layer, degree;
    int64_t off, n;
};
struct Layers {
    int32_t n_layers = 0;
    std::vector<int32_t> layer_of;  // [C]
    std::vector<uint8_t> repeat;    // [C]
    std::vector<int32_t> checks;    // [C], by (layer, degree, check id)
    std::vector<LayerSeg> segs;
};
inline void build_layers(const TannerCsr &t, Layers &L) {
    const size_t C = (size_t)t.C;
    L.n_layers = 0;
    L.layer_of.assign(C, 0);
    L.repeat.assign(C, 0);
    L.checks.clear();
    L.segs.clear();
    std::vector<std::vector<uint8_t>> used;
    std::vector<int32_t> vs;
    for (size_t c = 0; c < C; ++c) {
        const int32_t b = t.chk_ptr[c], e = t.chk_ptr[c + 1];
        vs.assign(t.chk_var.begin() + b, t.chk_var.begin() + e);
        std::sort(vs.begin(), vs.end());
        L.repeat[c] = std::adjacent_find(vs.begin(), vs.end()) != vs.end();
        size_t l = 0;
        for (;; ++l) {
            if (l == used.size()) used.emplace_back((size_t)t.V, (uint8_t)0);
            bool free_layer = true;
            for (int32_t k = b; k < e && free_layer; ++k) free_layer = !used[l][(size_t)t.chk_var[(size_t)k]];
            if (free_layer) break;
        }
        for (int32_t k = b; k < e; ++k) used[l][(size_t)t.chk_var[(size_t)k]] = 1;
        L.layer_of[c] = (int32_t)l;
    }
    L.n_layers = (int32_t)used.size();
    // (layer, degree) -> its checks, ascending: a counting sort over the ascending check ids
    const size_t nd = t.by_deg.size();
    std::vector<int64_t> cnt((size_t)L.n_layers * nd + 1, 0);
    auto key = [&](size_t c) { return (size_t)L.layer_of[c] * nd + (size_t)(t.chk_ptr[c + 1] - t.chk_ptr[c]); };
    for (size_t c = 0; c < C; ++c) cnt[key(c) + 1]++;
    for (size_t k = 0; k + 1 < cnt.size(); ++k) {
        if (cnt[k + 1]) L.segs.push_back(LayerSeg{(int32_t)(k / nd), (int32_t)(k % nd), cnt[k], cnt[k + 1]});
        cnt[k + 1] += cnt[k];
    }
    L.checks.resize(C);
    for (size_t c = 0; c < C; ++c) L.checks[(size_t)cnt[key(c)]++] = (int32_t)c;
}

// NoiseMapper tables on the host (noisemapper.pyx:103-236) and the fast root search's
// Newton-start (quant) and Taylor (ftab) tables; quant/ftab stay empty where the brute
// search is used.  t.quant / t.ftab are left null (device pointers are set on upload).
inline int build_demap_host(int32_t bps, const double *constellation, const double *probabilities,
                            const double *thresholds, double noise_var, const uint8_t *sign_config, DemapTables &t,
                            std::vector<double2> &quant, std::vector<double> &ftab, std::string &err) {
    if (bps < 1 || bps > kMaxBps) {
        err = "bit_per_symbol must be in [1, " + std::to_string(kMaxBps) + "], got " + std::to_string(bps);
        return QR_EVALUE;
    }
    if (!(noise_var > 0)) {  // noisemapper.pyx:111-112
        err = "noise variance must be strictly positive";
        return QR_EVALUE;
    }
    if (!constellation || !thresholds) {
        err = "null constellation/thresholds";
        return QR_EVALUE;
    }
    memset(&t, 0, sizeof t);
    const int M = 1 << bps;
    t.M = M;
    t.bps = bps;
    for (int i = 0; i < M; ++i) {
        t.a[i] = constellation[i];
        t.p[i] = probabilities ? probabilities[i] : 1.0 / M;  // alphabet.pyx:46-47
        t.sign[i] = sign_config ? sign_config[i] : 0;       // noisemapper.pyx:115-116
    }
    for (int i = 0; i <= M; ++i) t.thr[i] = thresholds[i];
    const double sigma = sqrt(noise_var);                     // noisemapper.pyx:132
    t.den = sqrt(2.0) * sigma;                                // __sqrt2 * sigma (:24, :67)
    t.two_s2 = 2 * noise_var;                                 // :469
    t.inv_two_s2 = 1.0 / t.two_s2;                            // div_two_s2
    t.mi_norm = sqrt(2.0 * 3.141592653589793) * sigma;        // mutual_information.pyx:198 (np.pi)
    t.Fthr[0] = 0;                                            // :149-153
    t.Fthr[M] = 1;
    for (int i = 1; i < M; ++i) t.Fthr[i] = single_F_Y(t, t.thr[i]);
    for (int i = 0; i < M; ++i) t.dF[i] = t.Fthr[i + 1] - t.Fthr[i];  // :159-162
    t.inv_den = 1.0 / t.den;
    for (int i = 0; i < M; ++i) t.inv_dF[i] = 1.0 / t.dF[i];          // Newton start only
    t.amin = t.amax = t.a[0];
    for (int i = 1; i < M; ++i) {
        t.amin = fmin(t.amin, t.a[i]);
        t.amax = fmax(t.amax, t.a[i]);
    }
    // Newton start table (qamr_math.hpp, build_quantiles): M * kQStride * M exact F_Y
    // bisections; beyond 32-PAM its cost grows as M^2 and the brute search is used.
    quant.clear();
    ftab.clear();
    if (M <= 32) {
        quant.resize((size_t)M * kQStride);
        build_quantiles(t, quant.data());
    }
    // Taylor table of F_Y for the Newton evaluation (qamr_math.hpp, build_ftab)
    double ftab_w = 0;
    if (!quant.empty() && build_ftab(t, ftab, t.ftab_n, t.ftab_lo, ftab_w, t.ftab_err)) {
        t.ftab_inv_w = 1.0 / ftab_w;
        t.ftab_h = ftab_w / 2;
        t.ftab_inv_h = 2.0 / ftab_w;
    } else {
        ftab.clear();
    }
    t.quant = nullptr;
    t.ftab = nullptr;
    return QR_OK;
}

}  // namespace qr
