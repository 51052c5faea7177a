// mi_quad.hpp -- the adaptive integrator behind scipy.integrate.quad, as the reference calls it
// (mutual_information.pyx:146, :205): QUADPACK's QAGS on a finite interval (dqagse with the 21-point
// Gauss-Kronrod rule dqk21) and QAGI on (-inf, inf) (dqagie with inf = 2: the same driver on [0, 1]
// with the transformed 15-point rule dqk15i), restated operation by operation in plain double
// arithmetic: dqagse, dqelg (the epsilon algorithm), dqpsrt (the error-ordered list) and the tail of
// the rules' error estimate.  Plain C++, no HIP call: the stand-alone host check compiles it too.
//
// The driver is a state machine that is fed rule results instead of calling the integrand: the rule
// of the whole interval first, then per bisection the rules of the two halves.  QuadState::pending
// names the interval(s) to evaluate next, QuadState::feed takes their {result, abserr, resabs,
// resasc} (after quad_rule_tail) and advances by one bisection: the round-off tests, dqpsrt, the
// extrapolation bookkeeping and dqelg, then termination.  It ends after at most `limit` feeds.  The
// batched GPU driver (mi.hip qr_mi_quad_batch) runs one state per integral and evaluates the
// pending intervals of all unfinished ones in one launch per round; qr_quad_host runs one state over a
// C callback.  Both are synchronous (a round's launch depends on the host's decisions of the round
// before), so neither can be captured into a graph.  The per-integral bookkeeping is O(limit) per
// round and runs on the calling thread.
//
// Arrays are 1-based as in QUADPACK.  max / min are written as the comparisons they are, so that a
// NaN operand (an integral that is -inf) takes the same side everywhere.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <vector>

namespace qr {

constexpr double kQuadEpmach = 2.220446049250313e-16;   // 2^-52 (d1mach(4))
constexpr double kQuadUflow = 2.2250738585072014e-308;  // d1mach(1)
constexpr double kQuadOflow = DBL_MAX;                  // d1mach(2)

inline double quad_max(double a, double b) { return b > a ? b : a; }
inline double quad_min(double a, double b) { return b < a ? b : a; }

// The end of dqk21 / dqk15i: r = {result, |(resk - resg) hlgth|, resabs, resasc} -> r[1] = abserr.
// pow is the host libm's.
inline void quad_rule_tail(double r[4]) {
    double abserr = r[1];
    const double resabs = r[2], resasc = r[3];
    if (resasc != 0.0 && abserr != 0.0) abserr = resasc * quad_min(1.0, pow(200.0 * abserr / resasc, 1.5));
    if (resabs > kQuadUflow / (50.0 * kQuadEpmach)) abserr = quad_max((kQuadEpmach * 50.0) * resabs, abserr);
    r[1] = abserr;
}

struct QuadState {
    // ---- the call
    double a = 0, b = 0, epsabs = 0, epsrel = 0;
    int limit = 0;
    bool infinite = false;   // QAGI: neval = 2 (30 last - 15) instead of 42 last - 21
    // ---- the outcome (valid once done)
    bool done = false;
    double result = 0, abserr = 0;
    int neval = 0, ier = 0, last = 0;
    // ---- dqagse's state
    std::vector<double> alist, blist, rlist, elist;
    std::vector<int> iord;
    double rlist2[55], res3la[4];
    int ierro = 0, maxerr = 0, nrmax = 0, nres = 0, numrl2 = 0, ktmin = 0, ksgn = 0, iroff1 = 0, iroff2 = 0, iroff3 = 0;
    bool extrap = false, noext = false, first = true;
    double errmax = 0, area = 0, errsum = 0, errbnd = 0, small = 0, erlarg = 0, ertest = 0, correc = 0, defabs = 0;
    double a1 = 0, b1 = 0, a2 = 0, b2 = 0, erlast = 0;

    // limit >= 1.  QUADPACK's own refusal (ier = 6: epsabs <= 0 and epsrel < max(50 epmach, 0.5e-28))
    // ends the integral at once with result = abserr = 0, neval = last = 0.
    void start(double a_, double b_, double epsabs_, double epsrel_, int limit_, bool infinite_) {
        a = a_;
        b = b_;
        epsabs = epsabs_;
        epsrel = epsrel_;
        limit = limit_;
        infinite = infinite_;
        done = false;
        first = true;
        ier = ierro = 0;
        alist.assign(limit + 2, 0.0);
        blist.assign(limit + 2, 0.0);
        rlist.assign(limit + 2, 0.0);
        elist.assign(limit + 2, 0.0);
        iord.assign(limit + 2, 0);
        for (double &v : rlist2) v = 0.0;
        for (double &v : res3la) v = 0.0;
        alist[1] = a;
        blist[1] = b;
        if (epsabs <= 0.0 && epsrel < quad_max(50.0 * kQuadEpmach, 0.5e-28)) {
            result = abserr = 0.0;
            neval = last = 0;
            ier = 6;
            done = true;
        }
    }

    // The intervals whose rule results the next feed() takes: 1 (the whole interval) or 2 (the halves).
    int pending(double ia[2], double ib[2]) const {
        if (first) {
            ia[0] = a;
            ib[0] = b;
            return 1;
        }
        ia[0] = a1;
        ib[0] = b1;
        ia[1] = a2;
        ib[1] = b2;
        return 2;
    }

    void feed(const double r1[4], const double r2[4]) {
        if (first) {
            first = false;
            feed_first(r1);
        } else {
            int go = 0;
            if (!body(r1, r2, go)) {
                next();
                return;
            }
            finish(go);
        }
    }

private:
    void close() {
        if (ier > 2) ier -= 1;
        neval = infinite ? 2 * (30 * last - 15) : 42 * last - 21;
        done = true;
    }

    void feed_first(const double r[4]) {
        result = r[0];
        abserr = r[1];
        defabs = r[2];
        const double resabs = r[3];
        const double dres = fabs(result);
        errbnd = quad_max(epsabs, epsrel * dres);
        last = 1;
        rlist[1] = result;
        elist[1] = abserr;
        iord[1] = 1;
        if (abserr <= 100.0 * kQuadEpmach * defabs && abserr > errbnd) ier = 2;
        if (limit == 1) ier = 1;
        if (ier != 0 || (abserr <= errbnd && abserr != resabs) || abserr == 0.0) {
            close();
            return;
        }
        rlist2[1] = result;
        errmax = abserr;
        maxerr = 1;
        area = result;
        errsum = abserr;
        abserr = kQuadOflow;
        nrmax = 1;
        nres = 0;
        numrl2 = 2;
        ktmin = 0;
        extrap = noext = false;
        iroff1 = iroff2 = iroff3 = 0;
        ksgn = -1;
        if (dres >= (1.0 - 50.0 * kQuadEpmach) * defabs) ksgn = 1;
        small = erlarg = ertest = correc = 0.0;
        next();
    }

    // the head of `do 90 last = 2, limit`: bisect the interval with the largest error estimate
    void next() {
        last += 1;
        if (last > limit) {
            last = limit;
            finish(100);
            return;
        }
        a1 = alist[maxerr];
        b1 = 0.5 * (alist[maxerr] + blist[maxerr]);
        a2 = b1;
        b2 = blist[maxerr];
        erlast = errmax;
    }

    // One pass of the loop body after the two rules; true = leave the loop to label `go` (100 / 115).
    bool body(const double r1[4], const double r2[4], int &go) {
        const double area1 = r1[0], error1 = r1[1], defab1 = r1[3];
        const double area2 = r2[0], error2 = r2[1], defab2 = r2[3];
        const double area12 = area1 + area2, erro12 = error1 + error2;
        errsum = errsum + erro12 - errmax;
        area = area + area12 - rlist[maxerr];
        if (!(defab1 == error1 || defab2 == error2)) {
            if (!(fabs(rlist[maxerr] - area12) > 1e-5 * fabs(area12) || erro12 < 0.99 * errmax)) {
                if (extrap) iroff2 += 1;
                else iroff1 += 1;
            }
            if (last > 10 && erro12 > errmax) iroff3 += 1;
        }
        rlist[maxerr] = area1;
        rlist[last] = area2;
        errbnd = quad_max(epsabs, epsrel * fabs(area));
        if (iroff1 + iroff2 >= 10 || iroff3 >= 20) ier = 2;
        if (iroff2 >= 5) ierro = 3;
        if (last == limit) ier = 1;
        if (quad_max(fabs(a1), fabs(b2)) <= (1.0 + 100.0 * kQuadEpmach) * (fabs(a2) + 1000.0 * kQuadUflow)) ier = 4;
        if (error2 > error1) {
            alist[maxerr] = a2;
            alist[last] = a1;
            blist[last] = b1;
            rlist[maxerr] = area2;
            rlist[last] = area1;
            elist[maxerr] = error2;
            elist[last] = error1;
        } else {
            alist[last] = a2;
            blist[maxerr] = b1;
            blist[last] = b2;
            elist[maxerr] = error1;
            elist[last] = error2;
        }
        qpsrt();
        if (errsum <= errbnd) { go = 115; return true; }
        if (ier != 0) { go = 100; return true; }
        if (last == 2) {
            small = fabs(b - a) * 0.375;
            erlarg = errsum;
            ertest = errbnd;
            rlist2[2] = area;
            return false;
        }
        if (noext) return false;
        erlarg -= erlast;
        if (fabs(b1 - a1) > small) erlarg += erro12;
        if (!extrap) {
            if (fabs(blist[maxerr] - alist[maxerr]) > small) return false;
            extrap = true;
            nrmax = 2;
        }
        if (!(ierro == 3 || erlarg <= ertest)) {
            const int idd = nrmax;
            int jupbnd = last;
            if (last > 2 + limit / 2) jupbnd = limit + 3 - last;
            for (int k = idd; k <= jupbnd; ++k) {
                maxerr = iord[nrmax];
                errmax = elist[maxerr];
                if (fabs(blist[maxerr] - alist[maxerr]) > small) return false;
                nrmax += 1;
            }
        }
        numrl2 += 1;
        rlist2[numrl2] = area;
        double reseps, abseps;
        qelg(reseps, abseps);
        ktmin += 1;
        if (ktmin > 5 && abserr < 1e-3 * errsum) ier = 5;
        if (abseps < abserr) {
            ktmin = 0;
            abserr = abseps;
            result = reseps;
            correc = erlarg;
            ertest = quad_max(epsabs, epsrel * fabs(reseps));
            if (abserr <= ertest) { go = 100; return true; }
        }
        if (numrl2 == 1) noext = true;
        if (ier == 5) { go = 100; return true; }
        maxerr = iord[1];
        errmax = elist[maxerr];
        nrmax = 1;
        extrap = false;
        small *= 0.5;
        erlarg = errsum;
        return false;
    }

    // labels 100 .. 130 of dqagse
    void finish(int go) {
        if (go == 100) {
            bool g115 = false, g110 = false;
            if (abserr == kQuadOflow) {
                g115 = true;
            } else if (ier + ierro == 0) {
                g110 = true;
            } else {
                if (ierro == 3) abserr += correc;
                if (ier == 0) ier = 3;
                if (result != 0.0 && area != 0.0) {
                    if (abserr / fabs(result) > errsum / fabs(area)) g115 = true;
                    else g110 = true;
                } else {
                    if (abserr > errsum) g115 = true;
                    else if (area == 0.0) g110 = false;
                    else g110 = true;
                }
            }
            if (!g115 && g110) {
                if (ksgn == -1 && quad_max(fabs(result), fabs(area)) <= defabs * 0.01) {
                } else if (0.01 > result / area || result / area > 100.0 || errsum > fabs(area)) {
                    ier = 6;
                }
            }
            if (g115) go = 115;
        }
        if (go == 115) {
            result = 0.0;
            for (int k = 1; k <= last; ++k) result += rlist[k];
            abserr = errsum;
        }
        close();
    }

    // dqpsrt: keep iord ordered by decreasing error estimate; sets maxerr, errmax, nrmax
    void qpsrt() {
        if (last <= 2) {
            iord[1] = 1;
            iord[2] = 2;
            maxerr = iord[nrmax];
            errmax = elist[maxerr];
            return;
        }
        const double emax = elist[maxerr];
        if (nrmax != 1) {
            const int ido = nrmax - 1;
            for (int q = 0; q < ido; ++q) {
                const int isucc = iord[nrmax - 1];
                if (emax <= elist[isucc]) break;
                iord[nrmax] = isucc;
                nrmax -= 1;
            }
        }
        int jupbn = last;
        if (last > limit / 2 + 2) jupbn = limit + 3 - last;
        const double errmin = elist[last];
        const int jbnd = jupbn - 1, ibeg = nrmax + 1;
        bool found = false;
        int i = ibeg;
        if (ibeg <= jbnd) {
            for (i = ibeg; i <= jbnd; ++i) {
                const int isucc = iord[i];
                if (emax >= elist[isucc]) { found = true; break; }
                iord[i - 1] = isucc;
            }
        }
        if (!found) {
            iord[jbnd] = maxerr;
            iord[jupbn] = last;
        } else {
            iord[i - 1] = maxerr;
            int k = jbnd;
            bool placed = false;
            for (int j = i; j <= jbnd; ++j) {
                const int isucc = iord[k];
                if (errmin < elist[isucc]) { iord[k + 1] = last; placed = true; break; }
                iord[k + 1] = isucc;
                k -= 1;
            }
            if (!placed) iord[i] = last;
        }
        maxerr = iord[nrmax];
        errmax = elist[maxerr];
    }

    // dqelg on rlist2 / res3la: updates numrl2 (n) and nres
    void qelg(double &res_out, double &abserr_out) {
        double *eps = rlist2;
        int n = numrl2;
        nres += 1;
        double abse = kQuadOflow, res_ = eps[n];
        if (n >= 3) {
            const int limexp = 50;
            eps[n + 2] = eps[n];
            const int newelm = (n - 1) / 2;
            eps[n] = kQuadOflow;
            const int num = n;
            int k1 = n;
            for (int i = 1; i <= newelm; ++i) {
                const int k2 = k1 - 1, k3 = k1 - 2;
                double res = eps[k1 + 2];
                const double e0 = eps[k3], e1 = eps[k2], e2 = res;
                const double e1abs = fabs(e1), delta2 = e2 - e1, err2 = fabs(delta2);
                const double tol2 = quad_max(fabs(e2), e1abs) * kQuadEpmach;
                const double delta3 = e1 - e0, err3 = fabs(delta3);
                const double tol3 = quad_max(e1abs, fabs(e0)) * kQuadEpmach;
                if (!(err2 > tol2 || err3 > tol3)) {   // convergence: e0, e1, e2 equal within machine accuracy
                    res_ = res;
                    abse = err2 + err3;
                    abse = quad_max(abse, 5.0 * kQuadEpmach * fabs(res_));
                    numrl2 = n;
                    res_out = res_;
                    abserr_out = abse;
                    return;
                }
                const double e3 = eps[k1];
                eps[k1] = e1;
                const double delta1 = e1 - e3, err1 = fabs(delta1);
                const double tol1 = quad_max(e1abs, fabs(e3)) * kQuadEpmach;
                if (err1 <= tol1 || err2 <= tol2 || err3 <= tol3) { n = i + i - 1; break; }
                const double ss = 1.0 / delta1 + 1.0 / delta2 - 1.0 / delta3;
                const double epsinf = fabs(ss * e1);
                if (!(epsinf > 1e-4)) { n = i + i - 1; break; }
                res = e1 + 1.0 / ss;
                eps[k1] = res;
                k1 -= 2;
                const double error = err2 + fabs(res - e2) + err3;
                if (error > abse) continue;
                abse = error;
                res_ = res;
            }
            if (n == limexp) n = 2 * (limexp / 2) - 1;
            int ib = 1;
            if ((num / 2) * 2 == num) ib = 2;
            const int ie = newelm + 1;
            for (int i = 1; i <= ie; ++i) {
                const int ib2 = ib + 2;
                eps[ib] = eps[ib2];
                ib = ib2;
            }
            if (num != n) {
                int indx = num - n + 1;
                for (int i = 1; i <= n; ++i) {
                    eps[i] = eps[indx];
                    indx += 1;
                }
            }
            if (nres >= 4) {
                abse = fabs(res_ - res3la[3]) + fabs(res_ - res3la[2]) + fabs(res_ - res3la[1]);
                res3la[1] = res3la[2];
                res3la[2] = res3la[3];
                res3la[3] = res_;
            } else {
                res3la[nres] = res_;
                abse = kQuadOflow;
            }
        }
        abse = quad_max(abse, 5.0 * kQuadEpmach * fabs(res_));
        numrl2 = n;
        res_out = res_;
        abserr_out = abse;
    }
};

}  // namespace qr
