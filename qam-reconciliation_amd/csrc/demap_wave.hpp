// demap_wave.hpp -- what the 64-frame-tile kernels of demap.hip (k_demap_wave) and mi.hip
// (k_mi_terms, k_mi_quad) share: the wave-cooperative root search and the dispatch of a runtime
// bit_per_symbol to their templates.  Device-side: included by .hip files only.
#pragma once
#include "qamr_internal.hpp"
#include "qamr_math.hpp"

namespace qr {

// ---------------------------------------------------------------------------
// Root search of the 64-frame-tile demapper (k_demap_wave, demap.hip).  The certified closed form
// of the search needs at most one exact F_Y per (frame, hypothesis), for ~2 % of the lanes;
// instead of the wave running a divergent M-erf F_Y whenever any of its lanes needs one, the
// lanes' evaluation points are compacted into LDS (ballot + mbcnt) and the wave evaluates
// their M erf terms with one lane per (point, m), 64 / M points per pass, after which each
// owner sums its M terms in m order (noisemapper.pyx:278-286: the same products, the same
// sequence of additions).
constexpr int kDemapWaveMaxBps = 6;

// bps in 1..MAX -> f(std::integral_constant<int, bps>), the value as a compile-time constant;
// false (and no call) outside the range.  Host code.
template <int MAX = kDemapWaveMaxBps, class F>
inline bool dispatch_bps(int bps, F f) {
    return dispatch_int_seq<1>(bps, f, std::make_integer_sequence<int, MAX>{});
}

// rank of this lane among the set lanes of mk below it
__device__ __forceinline__ int lane_rank(uint64_t mk) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
}

__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// g_inv_search_fast (qamr_math.hpp) with the closed form's exact F_Y evaluated by the
// whole wave (see above).  Every lane of the wave must call it (wave-uniform i).
// ey / et: this wave's 64-double LDS buffers (evaluation points, erf terms).
template <int M>
__device__ __forceinline__ double g_inv_search_wave(const DemapTables &t, const MathTables &mt, double n_hat, int i,
                                                    double *ey, double *et, int lane) {
    SearchCmp cmp{&t, search_target(t, n_hat, i), 0.0, 0.0, false};
    cmp.have = newton_root(t, mt, cmp.T, i, cmp.ystar, cmp.W);   // T lies in region i
    double L = 0.0, H = 0.0;
    int need = 0;
    const bool closed = cmp.have && search_closed_prepare(cmp, L, H, need);
    const bool ask = need != 0;
    const uint64_t mk = __ballot(ask);
    bool gt = false;
    if (mk) {  // wave-uniform
        const int cnt = __popcll(mk);
        const int rank = lane_rank(mk);
        if (ask) ey[rank] = (need == 1) ? L : H;
        wave_lds_fence();
        constexpr int P = 64 / M;  // points per pass
        const int sub = lane / M, m = lane % M;
        for (int base = 0; base < cnt; base += P) {   // wave-uniform trip count
            const int item = base + sub;
            if (item < cnt) et[lane] = (0.5 * (1 + cephes_erf((ey[item] - t.a[m]) / t.den))) * t.p[m];
            wave_lds_fence();
            if (ask && rank >= base && rank < base + P) {
                const double *tt = et + (rank - base) * M;
                double F = tt[0];                     // noisemapper.pyx:282-285, m = 0 first
#pragma unroll
                for (int mm = 1; mm < M; ++mm) F += tt[mm];
                gt = F > cmp.T;                       // SearchCmp::exact(y) > 0
            }
            wave_lds_fence();
        }
    }
    if (closed) return search_closed_finish(L, H, need, gt);
    return search_replay(cmp);   // no certified window / outside the closed form (rare): per lane
}

}  // namespace qr
