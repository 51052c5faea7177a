// grid_interp.hpp -- the interpolation grid of NoiseMapper.g_inv, written once for the gfx950
// kernels (demap_interp.hip, mi.hip), the host entry that builds it (qr_demap_grid_create) and the
// native CPU checks (tests/native/interp_check.cpp, mi_quad_check.cpp).
//
// Table-interpolated g_inv (noisemapper.pyx:295-307) and the formulation-1 demapper built on it
// (demap_lappr_simplified, noisemapper.pyx:563-601).
//
// The grid of noisemapper.pyx:135-144 lives in HBM as n {F[r], y[r]} pairs (qr_demap_grid_create):
// y = numpy's linspace(y_low, y_high, n), F = the cpdef F_Y of it (public_F_Y, the uniform
// mixture).  g_inv(n_hat, i) = __interp(F, y, target) (noisemapper.pyx:47-63): the index r of
// __binsearch (:27-44), then a linear interpolation between pairs r and r + 1, which are 32
// contiguous bytes.
//
// Index search, two bodies:
//  (a) grid_binsearch: the reference's recursion, iterated -- the same probes in the same
//      order, so it returns the reference's index on ANY table;
//  (b) grid_interp_fast: "the last r with F[r] <= val (0 when val < F[0])" by bisection of a
//      coarse table (every 16th F by default, in LDS for the wave kernel) and then of the one
//      16-entry segment in HBM (at most 4 steps).  On a nondecreasing table (a) returns exactly
//      that index:
//      a probe sequence of (a) keeps the invariant F[base] <= val (or base = 0) and
//      val < F[base + size] (or base + size = n), it only ever discards entries on the strength
//      of one comparison val < F[k] (everything from k on is > val) or val >= F[k] (everything up
//      to k is <= val), and it stops at an index r with F[r] <= val < F[r + 1], or at the last
//      entry of its range when val exceeds it -- with ties, always the last of the tied run,
//      because val >= F[index + 1] sends it right.  F is a rounded sum of erf terms, so nothing
//      guarantees that it is nondecreasing: qr_demap_grid_create checks it in one pass and (b) is
//      used only when the check passed (and val is not NaN).
//      Knob interp_fast = 0 forces (a).
#pragma once
#include <cmath>

#include "debug_check.hpp"
#include "qamr_math.hpp"

namespace qr {

struct GridView {
    const double2 *pairs;   // [n] {F, y}
    const double *coarse;   // [nc] F[c << seg_shift]
    int32_t n, nc, seg_shift;
    double F_last, y_last;  // pairs[n - 1]
};

enum GridDebugSite {
    kDbgGridIndex = 10,    // grid index r outside [0, n), or r + 1 read with r + 1 >= n
    kDbgGridCoarse = 11,   // coarse-table index outside [0, nc)
};

// The grid's geometry (noisemapper.pyx:132-144): the range, the point count of :142 as a double
// (the caller bounds it before it becomes an index) and the step of numpy's linspace, delta / div.
struct GridGeometry {
    double y_low, y_high, n_points, lin_step;
};
inline GridGeometry grid_geometry(const DemapTables &t, double trunkation_threshold, double n_intervals_per_step,
                                  double step) {
    const double sigma = sqrt(t.two_s2 / 2);   // noisemapper.pyx:132 (two_s2 / 2 = noise_var, exactly)
    GridGeometry g;
    if (trunkation_threshold > 1.) {           // :135-137
        g.y_low = t.a[0] * 10;
        g.y_high = t.a[t.M - 1] * 10;
    } else {                                   // :138-141
        const double tmp = sqrt(-2. * log(trunkation_threshold)) * sigma;
        g.y_high = t.a[t.M - 1] + tmp;
        g.y_low = t.a[0] - tmp;
    }
    g.n_points = ceil((g.y_high - g.y_low) * n_intervals_per_step / step) + 1;   // :142
    g.lin_step = (g.y_high - g.y_low) / (g.n_points - 1);
    return g;
}
// y[i] of the n-point grid (noisemapper.pyx:143) as numpy's linspace computes it:
// fl(fl(i * step) + y_low) with the last point set to y_high.
QR_HD double grid_point(double y_low, double y_high, double lin_step, int n, int i) {
    return (i == n - 1) ? y_high : (double)i * lin_step + y_low;
}

// noisemapper.pyx:27-44 (__binsearch) over the F of the pairs, iterated: slice = [base, base + size).
QR_HD int grid_binsearch(const GridView &g, double val) {
    int base = 0, size = g.n;
    for (;;) {
        QR_DCHECK(base >= 0 && size >= 1 && base + size <= g.n, kDbgGridIndex, base, size);
        if (size == 1) return base;
        if (val < g.pairs[base].x) return base;
        if (val > g.pairs[base + size - 1].x) return base + size - 1;
        const int index = size / 2 - 1;
        if (val < g.pairs[base + index].x) { size = index; continue; }
        if (val >= g.pairs[base + index + 1].x) { base += index + 1; size -= index + 1; continue; }
        return base + index;
    }
}

// Body (b) with the interpolation: the last r with F[r] <= val (0 when val < F[0]) and
// __interp's result at it; val is not NaN and val < F[n - 1].  coarse: the coarse table (LDS or
// HBM).  The segment's probes load whole pairs, and the last two probes of a bisection are r and
// r + 1 themselves, so the interpolation operands are usually in registers already; only when r
// is the first or r + 1 is past the last entry probed in the segment is a pair loaded again.
// (That is why __interp's tail stands here a second time: through one function shared with body
// (a), the compiler orders the segment loop's selects differently in every FAST kernel.)
QR_HD double grid_interp_fast(const GridView &g, const double *coarse, double val) {
    int a = 0, b = 1;        // the pairs r = a and r + 1 = b ...
    double2 pa, pb;          // ... once loaded
    bool have_a = false, have_b = false;
    if (!(val < coarse[0])) {
        int lo = 0, hi = g.nc;   // coarse[lo] <= val, and hi == nc or coarse[hi] > val
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            QR_DCHECK(mid >= 0 && mid < g.nc, kDbgGridCoarse, mid, g.nc);
            if (coarse[mid] <= val) lo = mid; else hi = mid;
        }
        a = lo << g.seg_shift;   // F[a] <= val; at most seg_shift steps inside the segment
        b = a + (1 << g.seg_shift) < g.n ? a + (1 << g.seg_shift) : g.n;
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            QR_DCHECK(mid >= 0 && mid < g.n, kDbgGridIndex, mid, g.n);
            const double2 p = g.pairs[mid];
            if (p.x <= val) { a = mid; pa = p; have_a = true; }
            else            { b = mid; pb = p; have_b = true; }
        }
    }
    QR_DCHECK(a >= 0 && a < g.n && b == a + 1, kDbgGridIndex, a, b);
    if (a == g.n - 1) return g.y_last;               // noisemapper.pyx:55-56
    if (!have_a) pa = g.pairs[a];
    QR_DCHECK(a + 1 < g.n, kDbgGridIndex, a + 1, g.n);
    if (!have_b) pb = g.pairs[a + 1];
    if (pb.x == pa.x) return pa.y;                   // :58-59
    return pa.y + (pb.y - pa.y) * (val - pa.x) / (pb.x - pa.x);   // :61-63
}

// noisemapper.pyx:295-307 (g_inv) with __interp (:47-63): left to right, unfused.
// grid_g_inv_val: __interp (:47-63) at the target val; grid_g_inv: the target of (n_hat, i) first.
template <bool FAST>
QR_HD double grid_g_inv_val(const GridView &g, const double *coarse, double val) {
    if (val >= g.F_last) return g.y_last;            // :50-51
    if (FAST && val == val) return grid_interp_fast(g, coarse, val);
    const int r = grid_binsearch(g, val);
    QR_DCHECK(r >= 0 && r < g.n, kDbgGridIndex, r, g.n);
    if (r == g.n - 1) return g.y_last;               // :55-56
    QR_DCHECK(r + 1 < g.n, kDbgGridIndex, r + 1, g.n);
    const double2 p0 = g.pairs[r], p1 = g.pairs[r + 1];
    if (p1.x == p0.x) return p0.y;                   // :58-59
    return p0.y + (p1.y - p0.y) * (val - p0.x) / (p1.x - p0.x);   // :61-63
}
template <bool FAST>
QR_HD double grid_g_inv(const DemapTables &t, const GridView &g, const double *coarse, double n_hat, int i) {
    // the same expression as g_inv_search's (:297-307)
    return grid_g_inv_val<FAST>(g, coarse, search_target(t, n_hat, i));
}

// Formulation 1 of one symbol, any bps (noisemapper.pyx:605-620): per hypothesis i (ascending,
// :587-596) y_i = g_inv(n, i) and one exp(-((y_i - a_j)**2) / 2 sigma^2) (the reference evaluates
// the same expression once per bit k; Cython's pow(x, 2.0) is compiled to x * x), added to N[k] or
// D[k] by the Gray test of i; out[k] = log N[k] - log D[k], k < bps.  0 <= j < M.  ex / lg: glibc's
// exp and log restated (subnormal and zero sums, log(0) = -inf, are reached at high SNR).
template <bool FAST, class Exp, class Log>
QR_HD void grid_demap_symbol(const DemapTables &t, const GridView &g, const double *coarse, double n, int j, Exp ex,
                             Log lg, double *out) {
    const double aj = t.a[j];
    double N[kMaxBps], D[kMaxBps];
#pragma unroll
    for (int k = 0; k < kMaxBps; ++k) { N[k] = 0; D[k] = 0; }
    for (int i = 0; i < t.M; ++i) {
        const double y = grid_g_inv<FAST>(t, g, coarse, n, i);
        const double d = y - aj;
        const double e = ex(-(d * d) / t.two_s2);
        int mi = i;
#pragma unroll
        for (int k = 0; k < kMaxBps; ++k) {
            if (k < t.bps) {
                if ((mi * (mi + 1)) & 3) D[k] += e;
                else                     N[k] += e;
                mi >>= 1;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kMaxBps; ++k)
        if (k < t.bps) out[k] = lg(N[k]) - lg(D[k]);
}

}  // namespace qr
