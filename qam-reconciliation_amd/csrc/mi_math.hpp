// mi_math.hpp -- per-sample arithmetic of the Monte-Carlo mutual-information estimator
// (mutual_information.pyx:218-297, montecarlo_information), written once: the gfx950 kernel
// (mi.hip k_mi_terms) and the host check (tests/native/mi_check.cpp) both call
// mi_sample_terms below, with their own providers of y_hat, exp and log2.  The integrands of the
// quad-integrated evaluators (:43-119, :175-199) and the Gauss-Kronrod rules follow further down.
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

// ---------------------------------------------------------------------------------------------
// The quad-integrated evaluators (mutual_information.pyx:43-119 and :175-199): the two integrands,
// written once for the gfx950 kernel (mi.hip k_mi_quad / k_mi_integrand) and the host check
// (tests/native/mi_quad_check.cpp), and the two Gauss-Kronrod rules QUADPACK applies to them
// (dqk21 on [0, 1], dqk15i on (-inf, inf)), split into "abscissa of node k" (one lane each) and "the
// rule's four sums in the rule's order" (one lane per interval).  Every operation is rounded on its
// own; exp and log2 are the providers' (glibc's, restated).

// mutual_information_base_scheme_arg (:43-119) at n, given yhat(i) = g_inv(n, i), the interpolated one.
// f[i][j] = dF[i] / (p[j] + sum_{k != j} p[k] exp(((-((2.0 yhat_i - a[j]) - a[k])) (a[j] - a[k])) / tv)),
// fN[j] = sum_i f[i][j] from 0.0; res walks j, and within it i: v = f[i][j] p[j], res += v log2(v / pX[i])
// where v > 0; then v = p[j] fN[j], res -= v log2(v) where v > 0.  The reference fills f first and walks
// it afterwards; f[i][j] enters nothing but fN[j] and res's j-th stretch, both in ascending i, so one walk
// (j outer, i inner) performs the same operations on the same operands in the same order without the
// M x M array.  The k == j term is skipped by a select, its exp kept off exp's special cases (mi_mix).
template <class YH, class EX, class L2>
QR_HD double mi_base_arg(const DemapTables &t, const double *pX, int M, YH yhat, EX ex, L2 lg2) {
    double res = 0.0;
#pragma unroll 1
    for (int j = 0; j < M; ++j) {
        const double aj = t.a[j], pj = t.p[j];
        double fN = 0.0;
#pragma unroll 1
        for (int i = 0; i < M; ++i) {
            const double y2 = 2.0 * yhat(i);
            double tt = pj;
#pragma unroll 4
            for (int k = 0; k < M; ++k) {
                const double ak = t.a[k];
                const double e = div_two_s2(t, (-((y2 - aj) - ak)) * (aj - ak));
                const double term = t.p[k] * ex(k == j ? 1.0 : e);
                tt = k == j ? tt : tt + term;
            }
            const double f = t.dF[i] / tt;
            fN += f;
            const double v = f * pj;
            const bool on = v > 0.0;
            const double add = v * lg2(on ? v / pX[i] : 1.0);
            res = on ? res + add : res;
        }
        const double v = pj * fN;
        const bool on = v > 0.0;
        const double sub = v * lg2(on ? v : 1.0);
        res = on ? res - sub : res;
    }
    return res;
}

// mutual_information_X_Y_int_arg (:175-199) at y.  t2 = (p[j] exp((-(y - a[j]) (y - a[j])) / tv)) log2(t),
// t = mi_mix<true> (the operand order of :186 / :191 is :268's); a NaN t2 (0 * inf, where the mixture's
// exp overflowed) is skipped, an infinite one is not: both are the reference's result.  mi_norm =
// sqrt(2.0 pi) * noise_sigma (:198), a constant of the table.
template <class EX, class L2>
QR_HD double mi_xy_arg(const DemapTables &t, int M, double y, EX ex, L2 lg2) {
    double res = 0.0;
#pragma unroll 1
    for (int j = 0; j < M; ++j) {
        const double aj = t.a[j], pj = t.p[j];
        const double tt = mi_mix<true>(t, M, j, aj, pj, y, ex);
        const double d = y - aj;
        const double t2 = (pj * ex(div_two_s2(t, (-d) * d))) * lg2(tt);
        res = t2 != t2 ? res : res - t2;
    }
    return res / t.mi_norm;
}

enum MiQuadKind : int { kMiQuadBase = 0, kMiQuadXY = 1 };

// ---- dqk21 on [a, b].  Node k: 0 the centre, k = 1..10 centr - hlgth xgk[k], k = 11..20
// centr + hlgth xgk[k - 10] (xgk 1-based as in QUADPACK).
constexpr int kGk21Nodes = 21;
QR_HD double gk21_node(double a, double b, int k) {
    constexpr double xgk[11] = {0.0,
                                .995657163025808080735527280689003, .973906528517171720077964012084452,
                                .930157491355708226001207180059508, .865063366688984510732096688423493,
                                .780817726586416897063717578345042, .679409568299024406234327365114874,
                                .562757134668604683339000099272694, .433395394129247190799265943165784,
                                .294392862701460198131126603103866, .148874338981631210884826001129720};
    const double centr = 0.5 * (a + b), hlgth = 0.5 * (b - a);
    const double absc = hlgth * xgk[k <= 10 ? k : k - 10];
    return k == 0 ? centr : k <= 10 ? centr - absc : centr + absc;
}

// The rule's sums over the node values v[21] in dqk21's order: out = {result, |(resk - resg) hlgth|,
// resabs, resasc}; the error estimate's pow(., 1.5) step is the host's (mi_quad.hpp quad_rule_tail).
QR_HD void gk21_sums(const double *v, double a, double b, double out[4]) {
    constexpr double wgk[12] = {0.0,
                                .011694638867371874278064396062192, .032558162307964727478818972459390,
                                .054755896574351996031381300244580, .075039674810919952767043140916190,
                                .093125454583697605535065465083366, .109387158802297641899210590325805,
                                .123491976262065851077958109585166, .134709217311473325928054001771707,
                                .142775938577060080797094273138717, .147739104901338491374841515972068,
                                .149445554002916905664936468389821};
    constexpr double wg[6] = {0.0,
                              .066671344308688137593568809893332, .149451349150580593145776339657697,
                              .219086362515982043995534934228163, .269266719309996355091226921569469,
                              .295524224714752870173815619188769};
    const double hlgth = 0.5 * (b - a), dhlgth = fabs(hlgth);
    const double fc = v[0];
    double resg = 0.0, resk = wgk[11] * fc, resabs = fabs(resk);
    for (int j = 1; j <= 5; ++j) {
        const int tw = 2 * j;
        const double f1 = v[tw], f2 = v[10 + tw], fs = f1 + f2;
        resg += wg[j] * fs;
        resk += wgk[tw] * fs;
        resabs += wgk[tw] * (fabs(f1) + fabs(f2));
    }
    for (int j = 1; j <= 5; ++j) {
        const int tw = 2 * j - 1;
        const double f1 = v[tw], f2 = v[10 + tw], fs = f1 + f2;
        resk += wgk[tw] * fs;
        resabs += wgk[tw] * (fabs(f1) + fabs(f2));
    }
    const double reskh = resk * 0.5;
    double resasc = wgk[11] * fabs(fc - reskh);
    for (int j = 1; j <= 10; ++j) resasc += wgk[j] * (fabs(v[j] - reskh) + fabs(v[10 + j] - reskh));
    out[0] = resk * hlgth;
    out[1] = fabs((resk - resg) * hlgth);
    out[2] = resabs * dhlgth;
    out[3] = resasc * dhlgth;
}

// ---- dqk15i for (-inf, inf) (inf = 2: boun = 0, dinf = 1) on t in [a, b] within (0, 1].  Node q: 0
// the centre, q = 1..7 x = centr - hlgth xgk[q], q = 8..14 x = centr + hlgth xgk[q - 7]; the
// integrand is taken at +T and -T, T = 0 + 1 (1 - x) / x.
constexpr int kGk15Nodes = 15;
QR_HD double gk15i_x(double a, double b, int q) {
    constexpr double xgk[8] = {0.0,
                               .991455371120812639206854697526329, .949107912342758524526189684047851,
                               .864864423359769072789712788640926, .741531185599394439863864773280788,
                               .586087235467691130294144838258730, .405845151377397166906606412076961,
                               .207784955007898467600689403773245};
    const double centr = 0.5 * (a + b), hlgth = 0.5 * (b - a);
    const double absc = hlgth * xgk[q <= 7 ? q : q - 7];
    return q == 0 ? centr : q <= 7 ? centr - absc : centr + absc;
}
QR_HD double gk15i_T(double x) { return 0.0 + (1.0 * (1.0 - x)) / x; }

// v[2 q + s]: the integrand at +T (s = 0) and -T (s = 1) of node q.
QR_HD void gk15i_sums(const double *v, double a, double b, double out[4]) {
    constexpr double wgk[9] = {0.0,
                               .022935322010529224963732008058970, .063092092629978553290700663189204,
                               .104790010322250183839876322541518, .140653259715525918745189590510238,
                               .169004726639267902826583426598550, .190350578064785409913256402421014,
                               .204432940075298892414161999234649, .209482141084727828012999174891714};
    constexpr double wg[9] = {0.0, 0.0, .129484966168869693270611432679082, 0.0, .279705391489276667901467771423780,
                              0.0, .381830050505118944950369775488975, 0.0, .417959183673469387755102040816327};
    const double centr = 0.5 * (a + b), hlgth = 0.5 * (b - a);
    const double fc = ((v[0] + v[1]) / centr) / centr;
    double resg = wg[8] * fc, resk = wgk[8] * fc, resabs = fabs(resk);
    double fv1[8], fv2[8];
    for (int j = 1; j <= 7; ++j) {
        const double x1 = gk15i_x(a, b, j), x2 = gk15i_x(a, b, 7 + j);
        double f1 = v[2 * j] + v[2 * j + 1], f2 = v[2 * (7 + j)] + v[2 * (7 + j) + 1];
        f1 = (f1 / x1) / x1;
        f2 = (f2 / x2) / x2;
        fv1[j] = f1;
        fv2[j] = f2;
        const double fs = f1 + f2;
        resg += wg[j] * fs;
        resk += wgk[j] * fs;
        resabs += wgk[j] * (fabs(f1) + fabs(f2));
    }
    const double reskh = resk * 0.5;
    double resasc = wgk[8] * fabs(fc - reskh);
    for (int j = 1; j <= 7; ++j) resasc += wgk[j] * (fabs(fv1[j] - reskh) + fabs(fv2[j] - reskh));
    out[0] = resk * hlgth;
    out[1] = fabs((resk - resg) * hlgth);
    out[2] = resabs * hlgth;
    out[3] = resasc * hlgth;
}

// The two rules over a callable, evaluated one point after the other in QUADPACK's sequence (the
// centre, then the pairs of the even and of the odd nodes; dqk15i: f(T1), f(T2), f(-T1), f(-T2)): what
// the kernel's lanes do at once.  For the host driver over a callback and the host check.
template <class F>
QR_HD void quad_rule_21(F f, double a, double b, double out[4]) {
    double v[kGk21Nodes];
    v[0] = f(gk21_node(a, b, 0));
    for (int s = 0; s < 2; ++s)
        for (int j = 1; j <= 5; ++j) {
            const int tw = s == 0 ? 2 * j : 2 * j - 1;
            v[tw] = f(gk21_node(a, b, tw));
            v[10 + tw] = f(gk21_node(a, b, 10 + tw));
        }
    gk21_sums(v, a, b, out);
}
template <class F>
QR_HD void quad_rule_15i(F f, double a, double b, double out[4]) {
    double v[2 * kGk15Nodes];
    const double Tc = gk15i_T(gk15i_x(a, b, 0));
    v[0] = f(Tc);
    v[1] = f(-Tc);
    for (int j = 1; j <= 7; ++j) {
        const double T1 = gk15i_T(gk15i_x(a, b, j)), T2 = gk15i_T(gk15i_x(a, b, 7 + j));
        v[2 * j] = f(T1);
        v[2 * (7 + j)] = f(T2);
        v[2 * j + 1] = f(-T1);
        v[2 * (7 + j) + 1] = f(-T2);
    }
    gk15i_sums(v, a, b, out);
}

}  // namespace qr
