"""Generate tests/golden/mi_quad.npz: the quad-integrated mutual-information evaluators
(qamreconciliation/mutual_information.pyx: mutual_information_base_scheme_arg :43-119,
mutual_information_base_scheme :123-148, mutual_information_X_Y_int_arg :175-199,
mutual_information_X_Y :202-208) and integrator-only records of scipy.integrate.quad.

Run where the reference build is available, as tests/golden/make_golden_mi.py:

    make -C oracle ref
    PYTHONPATH=oracle/_ref python3 tests/golden/make_golden_mi_quad.py

When this file was written the reference build (oracle/Makefile `ref`) did not compile mutual_information.pyx
(it does now: make_golden_wide_interp_mi.retro_check asserts that the compiled mutual_information_base_scheme /
mutual_information_X_Y return the 18 integrals of cases 1..9 stored here, bit for bit), so every value the
module takes from its NoiseMapper and PAMAlphabet is taken from the compiled reference here too -- g_inv,
delta_F_Y, probabilities, constellation, noise_var, noise_sigma, and fwrd_transition_probability for
P_xhat -- and only the two integrands (:43-119, :175-199) are restated below, in plain Python floats
(IEEE doubles, one rounding per operation, the reference's operation order) with the c_exp / c_log2
helpers of make_golden_mi.py (math.exp / math.log2, i.e. libm's, as the module's
`from libc.math cimport exp, log2`).  The integrals are scipy.integrate.quad(..., full_output=1) over
those restated integrands: the reference's own call (:146, :205), with its default tolerances and limit
unless the case says otherwise.  THE RESTATED INTEGRANDS ARE THE ONE PART OF THE FIXTURE NOT EXECUTED BY
THE REFERENCE ITSELF (a scratch build of mutual_information.pyx, made with the `ref` recipe, returned the 18
integrals of cases 1..9 stored here bit for bit).  The configuration lists of sims/sim_mutual_information_compare_signs.py:33-62 are
restated likewise (that script has no importable function).  Only data is stored, no reference source.

Cases (numbered 1..10 as in CASES; prefix "c<c>_"), noise_var = Es 10^(-snr/10) / 2, alternating sign
configuration unless stated:

  n_cases
  per case: bps, noise_var, cfg [M], probs [M], p_Xhat [M], limit
            base_I, base_abserr, base_neval, base_last, base_warned      quad(base_arg, 0, 1)
            xy_I, xy_abserr, xy_neval, xy_last, xy_warned                quad(X_Y_int_arg, -inf, inf)
            base_x [<= 66], base_f                                       the first 64 abscissae quad visited,
            xy_x [<= 67], xy_f                                           then {0, 1} / {0, +-1e3 sigma}; values
  integrator-only records (24): ig_fn (0: 1/(w^2+(x-c)^2), 1: sqrt|x-c|, 2: 1/sqrt(|x-c|+1e-300),
            3: step(x > c) + x^2), ig_inf (0: [0, 1], 1: (-inf, inf)), ig_c, ig_w, ig_limit, ig_eps
            (epsabs = epsrel), ig_result, ig_abserr, ig_neval, ig_last, ig_warned
  cfg2 [10][4], cfg3 [136][8]: the configuration lists of compare_signs at bps 2 and 3
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
from scipy.integrate import quad

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_mi import NoiseMapper, PAMAlphabet, c_div, c_exp, c_log2, p_xhat  # noqa: E402
from make_golden import alternating, noise_var  # noqa: E402

N_ABSC = 64

# c -> (bps, snr_dB, all-zero configuration?, probabilities, limit)
CASES = {
    1: (1, 5.0, False, None, 50),
    2: (1, 15.0, False, None, 50),
    3: (2, 4.0, False, (0.1, 0.4, 0.3, 0.2), 50),
    4: (2, 15.0, False, None, 50),
    5: (2, 20.0, False, None, 50),
    6: (3, 20.0, False, None, 50),
    7: (4, 13.0, False, None, 50),
    8: (4, 25.0, False, None, 50),
    9: (2, 4.0, True, None, 50),
    10: (2, 5.0, False, None, 5),   # the limit is reached: ier = 1
}


def base_arg(n, nm, M, a, p, dF, pX, tv):
    """mutual_information.pyx:43-119"""
    f = [[0.0] * M for _ in range(M)]
    for i in range(M):
        y_hat = float(nm.g_inv(n, i))
        for j in range(M):
            t = p[j]
            for k in range(j):
                t += p[k] * c_exp(-(2.0 * y_hat - a[j] - a[k]) * (a[j] - a[k]) / tv)
            for k in range(j + 1, M):
                t += p[k] * c_exp(-(2.0 * y_hat - a[j] - a[k]) * (a[j] - a[k]) / tv)
            f[i][j] = c_div(dF[i], t)
    fN = [0.0] * M
    for j in range(M):
        fN[j] = 0.0
        for i in range(M):
            fN[j] += f[i][j]
    res = 0.0
    for j in range(M):
        for i in range(M):
            v = f[i][j] * p[j]
            if v > 0.0:
                res += v * c_log2(c_div(v, pX[i]))
        v = p[j] * fN[j]
        if v > 0.0:
            res -= v * c_log2(v)
    return res


SQRT2PI = math.sqrt(2.0 * np.pi)


def xy_arg(y, M, a, p, tv, sigma):
    """mutual_information.pyx:175-199"""
    res = 0.0
    for j in range(M):
        t = p[j]
        for k in range(j):
            t += p[k] * c_exp((2 * y - a[k] - a[j]) * (a[k] - a[j]) / tv)
        for k in range(j + 1, M):
            t += p[k] * c_exp((2 * y - a[k] - a[j]) * (a[k] - a[j]) / tv)
        t2 = p[j] * c_exp(-(y - a[j]) * (y - a[j]) / tv) * c_log2(t)
        if not t2 != t2:
            res -= t2
    res /= SQRT2PI * sigma
    return res


def run_quad(f, lo, hi, extra, **kw):
    xs, fs = [], []

    def logged(x):
        v = f(x)
        if len(xs) < N_ABSC:
            xs.append(x)
            fs.append(v)
        return v

    ret = quad(logged, lo, hi, full_output=1, **kw)
    for x in extra:
        xs.append(x)
        fs.append(f(x))
    return (ret[0], ret[1], int(ret[2]["neval"]), int(ret[2]["last"]), int(len(ret) > 3)), np.array(xs), np.array(fs)


def gen_case(out, c):
    bps, snr, base, probs, limit = CASES[c]
    pa = PAMAlphabet(bps, 2.0) if probs is None else PAMAlphabet(bps, 2.0, np.array(probs))
    M = pa.order
    nv = float(noise_var(pa, snr))
    cfg = np.zeros(M, np.uint8) if base else alternating(M)
    nm = NoiseMapper(pa, nv, cfg)
    a = [float(v) for v in nm.constellation]
    p = [float(v) for v in nm.probabilities]
    dF = [float(v) for v in nm.delta_F_Y]
    fw = [[float(v) for v in row] for row in np.asarray(nm.fwrd_transition_probability)]
    tv = 2.0 * float(nm.noise_var)
    sigma = float(nm.noise_sigma)
    pX = p_xhat(M, p, fw)
    kw = {} if limit == 50 else {"limit": limit}
    b, bx, bf = run_quad(lambda n: base_arg(n, nm, M, a, p, dF, pX, tv), 0, 1, (0.0, 1.0), **kw)
    x, xx, xf = run_quad(lambda y: xy_arg(y, M, a, p, tv, sigma), -np.inf, np.inf, (0.0, 1e3 * sigma, -1e3 * sigma), **kw)
    k = f"c{c}_"
    out.update({k + "bps": bps, k + "noise_var": nv, k + "cfg": cfg, k + "probs": np.asarray(pa.probabilities),
                k + "p_Xhat": np.array(pX), k + "limit": limit, k + "base_x": bx, k + "base_f": bf, k + "xy_x": xx,
                k + "xy_f": xf})
    for name, r in (("base", b), ("xy", x)):
        for field, v in zip(("I", "abserr", "neval", "last", "warned"), r):
            out[k + name + "_" + field] = v
    print(f"  case {c}: {M}-PAM {snr} dB limit={limit} base={b} xy={x}", flush=True)
    return b, x


INTEGRANDS = (
    lambda x, c, w: 1.0 / (w * w + (x - c) * (x - c)),
    lambda x, c, w: math.sqrt(abs(x - c)),
    lambda x, c, w: 1.0 / math.sqrt(abs(x - c) + 1e-300),
    lambda x, c, w: (1.0 if x > c else 0.0) + x * x,
)
CW = ((0.3, 0.01), (0.5, 1e-4), (0.7071067811865476, 0.25))
LIMITS = (1, 3, 5, 50)
EPS = (1.49e-8, 1e-12)


def gen_integrator(out):
    rec = {n: [] for n in ("fn", "inf", "c", "w", "limit", "eps", "result", "abserr", "neval", "last", "warned")}
    r = 0
    for fn in range(4):
        for inf in (0, 1):
            for (c, w) in CW:
                limit, eps = LIMITS[(r + fn) % 4], EPS[(r // 3) % 2]
                lo, hi = (-np.inf, np.inf) if inf else (0, 1)
                ret = quad(INTEGRANDS[fn], lo, hi, args=(c, w), full_output=1, epsabs=eps, epsrel=eps, limit=limit)
                for n, v in zip(rec, (fn, inf, c, w, limit, eps, ret[0], ret[1], ret[2]["neval"], ret[2]["last"],
                                      int(len(ret) > 3))):
                    rec[n].append(v)
                r += 1
    assert r == 24 and set(rec["limit"]) == set(LIMITS) and set(rec["eps"]) == set(EPS)
    assert 0 < sum(rec["warned"]) < 24
    for n, v in rec.items():
        out["ig_" + n] = np.array(v, np.float64 if n in ("c", "w", "eps", "result", "abserr") else np.int32)
    print(f"  integrator records: {sum(rec['warned'])} of 24 warn, neval {min(rec['neval'])}..{max(rec['neval'])}")


def config_list(bps):
    """sims/sim_mutual_information_compare_signs.py:30-62 (the bit count of reverse_flip_bits is M)."""
    M = 1 << bps

    def reverse_flip_bits(n):
        res = 0
        for k in range(M):
            res += (((n >> k) & 0b1) ^ 0b1) << (M - 1 - k)
        return res

    cfgs = [[(c >> i) & 1 for i in range(M)] for c in range(1 << M) if reverse_flip_bits(c) >= c]
    assert len(cfgs) == (1 << ((M >> 1) - 1)) * ((1 << (M >> 1)) + 1)   # :60
    return np.array(cfgs, np.uint8)


if __name__ == "__main__":
    out = {"n_cases": len(CASES)}
    res = {c: gen_case(out, c) for c in CASES}
    base = [res[c][0] for c in CASES]
    xy = [res[c][1] for c in CASES]
    # conditions on the reference's own values, not measurements of the code under test
    assert any(b[2] == 21 for b in base), "no base integral ends after the first rule"
    assert any(b[2] >= 700 for b in base), "no base integral takes >= 700 evaluations"
    assert any(b[4] for b in base + xy), "no integral warns"
    assert res[10][0][4] == 1 and res[10][0][3] == 5, "the limit=5 case does not reach its limit"
    assert sum(1 for v in xy if v[0] == -math.inf) >= 2, "fewer than two X_Y integrals are -inf"
    assert all(math.isfinite(b[0]) for b in base) and all(math.isfinite(v[0]) or v[0] == -math.inf for v in xy)
    gen_integrator(out)
    out["cfg2"], out["cfg3"] = config_list(2), config_list(3)
    assert out["cfg2"].shape == (10, 4) and out["cfg3"].shape == (136, 8)
    path = os.path.join(HERE, "mi_quad.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"[golden] mi_quad.npz: {size} bytes", flush=True)
    assert size < os.path.getsize(os.path.join(HERE, "interp.npz"))
