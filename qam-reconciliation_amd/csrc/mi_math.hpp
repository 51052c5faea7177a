// mi_math.hpp -- per-sample arithmetic of the Monte-Carlo mutual-information estimator
// (mutual_information.pyx:218-297, montecarlo_information), written once: the gfx950 kernel
// (demap.hip k_mi_terms) and the host check (tests/native/mi_check.cpp) both call
// mi_sample_terms below, with their own providers of y_hat, exp and log2.
//
// Per sample (x = Alice's symbol index, y = Bob's sample, x_hat = his hard decision,
// n = g(y, x_hat) his transformed noise), with a[] the constellation, p[] its probabilities,
// tv = 2.0 * noise_var (DemapTables::two_s2, the same double), dF = delta_F_Y,
// fw = fwrd_transition_probability, pX = p_Xhat:
//   t0 = log2(pX[x_hat] / fw[x][x_hat])                                              (:259)
//   t1 = log2(p[x] + sum_{k != x} p[k] exp(((2 y - a[k]) - a[x]) (a[k] - a[x]) / tv))   (:264-269)
//   t2 = log2(((sum_{k != x_hat} dF[k] / mix(g_inv(n, k))) * (mix(g_inv_search(n, x_hat)) / dF[x_hat])
//             + 1) * pX[x_hat])                                                      (:274-290)
//        mix(v) = p[x] + sum_{m != x} p[m] exp(((2 v - a[x]) - a[m]) (a[m] - a[x]) / tv)
// every sum in ascending index order, every operation rounded separately (no FMA), exp and log2
// glibc's on their full domains (overflow to inf and underflow are part of the result).  The
// block totals (:245-297) add t0 and t1 and subtract t2 in sample order, then divide by N.
#pragma once
#include "qamr_math.hpp"

namespace qr {

enum MiWhich : unsigned { kMiXXhat = 1u, kMiXY = 2u, kMiXNXhat = 4u, kMiAll = 7u };

// Bob's side of one sample, as k_bob (demap.hip) computes it: the hard decision
// (noisemapper.pyx:349-359) and the transformed noise g(y, x_hat) (:289-292, :373-388).
QR_HD void mi_bob(const DemapTables &t, double y, int &x_hat, double &n_hat) {
    int i = binsearch_thr(t.thr, t.M + 1, y);
    if (i == t.M) i = t.M - 1;
    if (t.sign[i]) n_hat = (t.Fthr[i + 1] - single_F_Y(t, y)) / t.dF[i];
    else           n_hat = (single_F_Y(t, y) - t.Fthr[i]) / t.dF[i];
    x_hat = i;
}

// p[x] + sum over m != x, m ascending, of p[m] exp(e_m / tv).  Y_FIRST: the operand order of
// :268 (I(X;Y): (2 v - a[m]) - a[x]); otherwise that of :282 / :288 ((2 v - a[x]) - a[m]).
// Straight-line: at m == x the term is skipped by a select, and the exp (whose result is not
// used there) gets an argument off its special cases -- e is 0 at m == x, and one such lane would
// send a whole wavefront through exp's full routine (g_exp_wave; demap.hip k_demap_wave).  The
// division by tv is div_two_s2: the correctly rounded quotient, i.e. the IEEE division's bits.
template <bool Y_FIRST, class EX>
QR_HD double mi_mix(const DemapTables &t, int M, int x, double ax, double px, double v, EX ex) {
    double tmp = px;
    const double v2 = 2 * v;
#pragma unroll 4
    for (int m = 0; m < M; ++m) {
        const double am = t.a[m];
        const double d = Y_FIRST ? (v2 - am) - ax : (v2 - ax) - am;
        const double e = div_two_s2(t, d * (am - ax));
        const double term = t.p[m] * ex(m == x ? 1.0 : e);
        tmp = m == x ? tmp : tmp + term;
    }
    return tmp;
}

// The three terms of one sample, each handed to put(q, value) as soon as it is complete (the
// kernel stores it at once instead of holding it through the next term's loops); a term whose bit
// of `which` is clear is not computed and not put.  x and x_hat in [0, M).  pX[M], fw[M * M]
// row-major fw[x][x_hat].  yhat(k): y_hat of hypothesis k -- g_inv(n, k) for k != x_hat,
// g_inv_search(n, x_hat) at k == x_hat; ex / lg2: glibc's exp and log2.
template <class YH, class EX, class L2, class PUT>
QR_HD void mi_sample_terms(const DemapTables &t, const double *pX, const double *fw, int M, unsigned which, int x,
                           int x_hat, double y, YH yhat, EX ex, L2 lg2, PUT put) {
    const double ax = t.a[x], px = t.p[x];
    if (which & kMiXXhat) put(0, lg2(pX[x_hat] / fw[x * M + x_hat]));
    if (which & kMiXY) put(1, lg2(mi_mix<true>(t, M, x, ax, px, y, ex)));
    if (which & kMiXNXhat) {
        double acc = 0.0, own = 0.0;
#pragma unroll 1
        for (int k = 0; k < M; ++k) {   // :276-283 (k != x_hat) and :285-289 (k == x_hat) in one walk
            const double tmp = mi_mix<false>(t, M, x, ax, px, yhat(k), ex);
            const double q = t.dF[k] / tmp;
            acc = k == x_hat ? acc : acc + q;
            own = k == x_hat ? tmp : own;
        }
        acc *= own / t.dF[x_hat];
        acc += 1;
        acc *= pX[x_hat];
        put(2, lg2(acc));
    }
}

}  // namespace qr
