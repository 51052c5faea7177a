"""Inputs and references of the device-primitive tests (tests/test_gpu_device_math.py, qr_math_eval_host)
and of the direct-reconciliation LAPPR tests.

* ``FN`` / ``HOME`` / ``HOMES`` / ``device_eval``: the ids of include/qamr.h, the table homes each function
  accepts, and one call of the entry.
* ``ref_exp`` / ``ref_log`` / ``ref_h`` / ``ref_box_plus`` / ``ref_erf`` / ``ref_div``: the references, element by
  element: libm through Python's ``math`` (numpy's vectorised exp / log are other routines), the oracle's C
  restatement for the box-plus and erf, numpy's IEEE division.
* ``*_inputs``: seeded input sets, drawn where tests/native/glibc_math_check.cpp and division_check.cpp draw
  theirs, about 2e5 elements each.  ``exp_wave_inputs`` and ``h_packed_inputs`` lay theirs out by wavefront and
  return the layout with them, so that the CPU tests can check it.
* ``y_to_lappr_grey``: sims/reconciliation.pyx:25-51 restated with ``math.exp`` / ``math.log``; ``lappr_cases``
  and ``lappr_samples`` describe tests/golden/llr_sources_wide.npz (make_golden_llr_wide.py).
"""
import functools
import math

import numpy as np

FN = dict(exp=0, exp_neg=1, exp_full=2, exp_wave=3, log=4, log_u=5, log_u_sel=6, log_full=7, h_strict=8,
          h_strict_sel=9, box_plus=10, box_plus_sel=11, erf=12, div_two_s2=13, h_packed=14)
HOME = dict(sweep=0, node=1, const=2, explog=3, demap=4, mi=5)
_BP = ("sweep", "node")
_FULL = ("const", "explog", "demap")
HOMES = dict(exp=("node", "const"), exp_neg=_BP, exp_full=_FULL, exp_wave=("explog", "mi"), log=_FULL, log_u=_BP,
             log_u_sel=_BP, log_full=_FULL, h_strict=_BP, h_strict_sel=_BP, box_plus=_BP, box_plus_sel=_BP,
             erf=("const",), div_two_s2=("const",))
CLAMP = dict(none=0, full=1, finite=2)
PACK_MAX_JOBS = 8

INF, NAN = math.inf, math.nan
LN2 = float.fromhex("0x1.62e42fefa39efp-1")
NEAR1_LO = 1.0 - 2.0 ** -4                       # e_log.c's near-1 window [1 - 2^-4, 1 + 0x1.09p-4)
NEAR1_HI = 1.0 + float.fromhex("0x1.09p-4")
DBL_MAX, DBL_MIN, DBL_TRUE_MIN = 1.7976931348623157e308, 2.2250738585072014e-308, 5e-324
# tests/native/glibc_math_check.cpp:155-157
FULL_SPECIALS = (0.0, -0.0, INF, -INF, NAN, 709.78, 709.79, -708.4, -745.1, -745.2, -1e5, 1e5, 512.0, -512.0, 1023.9,
                 -1023.9, 1024.0, -1024.0, DBL_TRUE_MIN, -DBL_TRUE_MIN, 1.0, DBL_MIN, DBL_MAX, -1.0)


def device_eval(fn, variant, a, b=None):
    """qr_math_eval_host on float64 arrays -> the output array (pre-filled with a sentinel)."""
    from qamr import _lib

    a = np.ascontiguousarray(a, np.float64)
    out = np.full(a.shape, -7.25)
    bp = None
    if b is not None:
        b = np.ascontiguousarray(b, np.float64)
        assert b.shape == a.shape
        bp = _lib.ptr(b)
    _lib.check(_lib.load().qr_math_eval_host(FN[fn] if isinstance(fn, str) else fn,
                                             HOME[variant] if isinstance(variant, str) else variant, a.size,
                                             _lib.ptr(a), bp, _lib.ptr(out)), "qr_math_eval_host")
    return out


# ------------------------------------------------------------------ references
def _exp1(v):
    try:
        return math.exp(v)
    except OverflowError:
        return INF


def _log1(v):
    if v != v or v < 0:
        return NAN
    if v == 0:
        return -INF
    return math.log(v)


def ref_exp(x):
    """libm's exp per element; overflow -> inf."""
    return np.array([_exp1(v) for v in np.asarray(x, np.float64).tolist()])


def ref_log(x):
    """libm's log per element; 0 -> -inf, negative or NaN -> NaN."""
    return np.array([_log1(v) for v in np.asarray(x, np.float64).tolist()])


def ref_h(t):
    """log(1.0 + exp(-|t|)) as the reference's box-plus evaluates it (decoder.pyx:41-45)."""
    return np.array([math.log(1.0 + math.exp(-abs(v))) for v in np.asarray(t, np.float64).tolist()])


def ref_box_plus(a, b):
    import oracle as O

    return np.array([O.box_plus(u, v) for u, v in zip(np.asarray(a).tolist(), np.asarray(b).tolist())])


def ref_erf(x):
    import oracle as O

    return O.erf(np.asarray(x, np.float64))


def ref_div(x, b):
    """IEEE x / b, except that a zero dividend of either sign gives +0 (division_check.cpp documents it)."""
    x, b = np.asarray(x, np.float64), np.asarray(b, np.float64)
    q = x / b
    q[x == 0.0] = 0.0
    return q


# ------------------------------------------------------------------ input sets
def neighbours(x):
    """x with both nextafter neighbours of every element."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):   # DBL_MAX's neighbour is inf
        return np.concatenate([x, np.nextafter(x, -INF), np.nextafter(x, INF)])


def _bits(rng, n):
    return rng.integers(0, 1 << 64, n, dtype=np.uint64).view(np.float64)


def _signs(rng, n):
    return np.where(rng.integers(0, 2, n) == 1, -1.0, 1.0)


def _boundaries():
    """The 128 * 40 interval boundaries k ln2 / 128 of exp's table, k = -5120..0, with their neighbours."""
    return neighbours(np.arange(-128 * 40, 1) * LN2 / 128.0)


@functools.lru_cache(None)
def exp_inputs():
    """g_exp's domain: |x| < 512, NaN."""
    rng = np.random.default_rng(1101)
    x = np.concatenate([
        -40.0 * rng.random(70000), _signs(rng, 70000) * 2.0 ** rng.uniform(-60, 9, 70000), _boundaries(),
        rng.uniform(-512, 512, 30000),
        neighbours([0.0, -0.0, 2.0 ** -54, -2.0 ** -54, 2.0 ** -55, -DBL_TRUE_MIN, DBL_TRUE_MIN, -40.0, 1.0, -1.0]),
        [np.nextafter(512.0, 0.0), np.nextafter(-512.0, 0.0), NAN, -NAN]])
    assert (np.isnan(x) | (np.abs(x) < 512)).all()
    return x


@functools.lru_cache(None)
def exp_neg_inputs():
    """g_exp_neg's domain: [-37.51, 0], -0.0, tiny and subnormal negatives, NaN."""
    rng = np.random.default_rng(1102)
    b = _boundaries()
    x = np.concatenate([
        -37.51 * rng.random(95000), -(2.0 ** rng.uniform(-1074, 5.2, 95000)), b[(b >= -37.51) & (b <= 0)],
        [0.0, -0.0, -2.0 ** -54, -2.0 ** -55, -DBL_TRUE_MIN, -DBL_MIN, -37.5, np.nextafter(-37.5, 0), np.nextafter(-37.5, -INF),
         -37.51, float.fromhex("-0x1.2c00000000000p+5"), NAN, -NAN]])
    assert (np.isnan(x) | ((x >= -37.51) & (x <= 0))).all()
    return x


@functools.lru_cache(None)
def exp_full_inputs():
    """Every double: the box-plus domain, log-uniform magnitudes up to 2^10, the interval boundaries, [-760, 760]
    (overflow, underflow, subnormal results, the rescaled 512 <= |x| < 1024), random bit patterns, the specials."""
    rng = np.random.default_rng(1103)
    return np.concatenate([
        -40.0 * rng.random(40000), _signs(rng, 40000) * 2.0 ** rng.uniform(-60, 10, 40000), _boundaries(),
        rng.uniform(-760, 760, 50000), _bits(rng, 40000), rng.uniform(-40, 40, 10000), neighbours(FULL_SPECIALS)])


def exp_special(x):
    """g_exp_wave's special lanes: |x| outside [2^-54, 512) or not finite."""
    x = np.asarray(x, np.float64)
    return ~((np.abs(x) >= 2.0 ** -54) & (np.abs(x) < 512))


# one special of each kind: |x| < 2^-54, 512 <= |x| < 1024 (rescaled: overflowing, large, subnormal and
# underflowing results), |x| >= 1024, +-inf, NaN
WAVE_SPECIALS = (2.0 ** -60, -2.0 ** -60, 0.0, -0.0, DBL_TRUE_MIN, 600.0, -600.0, 709.5, 710.0, -708.5, -720.0, -744.0, -746.0, 1023.9,
                 -1023.9, 512.0, -512.0, 1024.0, -1024.0, 1e5, -1e5, DBL_MAX, -DBL_MAX, INF, -INF, NAN, -NAN)
WAVE_LANES = (0, 31, 32, 63)


@functools.lru_cache(None)
def exp_wave_inputs():
    """-> (x, layout): x laid out by wavefront (wave w = x[64 w : 64 w + 64]); layout = dict of
    none (waves without a special lane), one ((wave, lane, value) of the waves with exactly one), all (waves of
    special lanes only), mixed (the rest, exp_full_inputs shuffled), and the last, partial wave's length."""
    rng = np.random.default_rng(1104)
    waves, layout = [], dict(none=[], one=[], all=[], mixed=[])

    def plain(n=64):
        return _signs(rng, n) * np.where(rng.random(n) < 0.5, rng.uniform(2.0 ** -54, 512, n), 2.0 ** rng.uniform(-54, 9, n))

    for _ in range(200):
        layout["none"].append(len(waves))
        waves.append(plain())
    for v in WAVE_SPECIALS:
        for lane in WAVE_LANES:
            w = plain()
            w[lane] = v
            layout["one"].append((len(waves), lane, v))
            waves.append(w)
    pool = np.array(WAVE_SPECIALS)
    for _ in range(40):
        layout["all"].append(len(waves))
        waves.append(rng.choice(pool, 64))
    for kind in range(len(WAVE_SPECIALS)):   # and each kind alone on all 64 lanes
        layout["all"].append(len(waves))
        waves.append(np.full(64, WAVE_SPECIALS[kind]))
    full = rng.permutation(exp_full_inputs())
    full = full[:full.size // 64 * 64].reshape(-1, 64)
    for w in full:
        layout["mixed"].append(len(waves))
        waves.append(w)
    tail = plain(37)     # the partial wave: one special lane among 37
    tail[36] = -720.0
    layout["tail"] = 37
    return np.concatenate(waves + [tail]), layout


def _log_u_core(rng, n):
    t = np.concatenate([40.0 * rng.random(n), 4.0 * rng.random(n)])
    return np.concatenate([1.0 + np.array([math.exp(-v) for v in t.tolist()]), 1.0 + rng.random(n)])


@functools.lru_cache(None)
def log_u_inputs():
    """g_log_u / g_log_u_sel: [1, 2] and NaN -- u = 1 + exp(-t), uniform, the near-1 branch's range, the bounds."""
    rng = np.random.default_rng(1105)
    x = np.concatenate([
        _log_u_core(rng, 50000), rng.uniform(1.0, NEAR1_HI + 0.002, 40000),
        [1.0, 2.0, np.nextafter(1.0, 2.0), np.nextafter(2.0, 1.0), NEAR1_HI, np.nextafter(NEAR1_HI, 1.0), np.nextafter(NEAR1_HI, 2.0),
         1.0 + 2.0 ** -52, 1.0 + 2.0 ** -30, 1.5, NAN, -NAN]])
    assert (np.isnan(x) | ((x >= 1) & (x <= 2))).all()
    return x


@functools.lru_cache(None)
def log_inputs():
    """g_log: positive normals -- the box-plus domain, [1, 2], the near-1 window [0.9375, 1.0645] with its two
    boundary constants and their neighbours, random normals."""
    rng = np.random.default_rng(1106)
    normals = ((rng.integers(0, 1 << 52, 50000, dtype=np.uint64)) | (rng.integers(1, 2047, 50000, dtype=np.uint64) << np.uint64(52)))
    x = np.concatenate([
        _log_u_core(rng, 35000), 0.9375 + 0.127 * rng.random(40000), normals.view(np.float64),
        neighbours([NEAR1_LO, NEAR1_HI, 1.0, 2.0, 0.5]), [DBL_MIN, DBL_MAX, np.nextafter(DBL_MIN, 1.0)]])
    assert ((x >= DBL_MIN) & (x <= DBL_MAX)).all()
    return x


@functools.lru_cache(None)
def log_full_inputs():
    """Every double: log_inputs, subnormals, log-uniform 2^-1074..2^1024, random bit patterns, 0, -0, +-inf, NaN,
    negatives."""
    rng = np.random.default_rng(1107)
    return np.concatenate([
        log_inputs()[::2], rng.integers(1, 1 << 52, 25000, dtype=np.uint64).view(np.float64),
        2.0 ** rng.uniform(-1074, 1024, 40000), 0.9 + 0.2 * rng.random(20000), _bits(rng, 30000),
        neighbours(FULL_SPECIALS), neighbours([NEAR1_LO, NEAR1_HI, 2.0, 0.5]), [-DBL_MAX, -DBL_MIN, -2.5, -NAN]])


H_SPECIALS = (0.0, -0.0, 36.0, 36.7, 36.75, 37.0, 37.5, np.nextafter(37.5, 0), np.nextafter(37.5, 40), 40.0, 41.0, 700.0,
              1e300, INF, -INF, NAN, -NAN, -37.5, -700.0, -1e300)


@functools.lru_cache(None)
def h_inputs():
    """h_strict: any t, +-inf, NaN -- glibc_math_check.cpp's three ranges, both signs, the clamp region."""
    rng = np.random.default_rng(1108)
    t = np.concatenate([45.0 * rng.random(65000), 3.0 * rng.random(65000), 2.0 ** rng.uniform(-60, 6, 65000)])
    t[::3] = -t[::3]
    return np.concatenate([t, H_SPECIALS])


BOX_SPECIALS = (0.0, -0.0, 1.5, -2.25, 40.0, INF, -INF, NAN)


@functools.lru_cache(None)
def box_plus_inputs():
    """-> (a, b): glibc_math_check.cpp:121-136 -- random operands of both signs and mixed magnitudes with
    b = -a, b = a, a = 0 and b = -0 sprinkled in, then the 8 x 8 grid of specials."""
    rng = np.random.default_rng(1109)
    n = 190000
    sc = np.array([1e-9, 1e-3, 0.3, 2.0, 8.0, 30.0, 200.0, 1e6])
    a = (2 * rng.random(n) - 1) * sc[rng.integers(0, 8, n)]
    b = (2 * rng.random(n) - 1) * sc[rng.integers(0, 8, n)]
    i = np.arange(n)
    b = np.where((i & 63) == 1, -a, b)
    b = np.where((i & 63) == 2, a, b)
    a = np.where((i & 127) == 3, 0.0, a)
    b = np.where((i & 127) == 4, -0.0, b)
    ga, gb = np.meshgrid(BOX_SPECIALS, BOX_SPECIALS, indexing="ij")
    return np.concatenate([a, ga.ravel()]), np.concatenate([b, gb.ravel()])


SQRT_MAXLOG = math.sqrt(7.09782712893383996732E2)   # erfc's exp underflow bound, |x| = 26.64...


@functools.lru_cache(None)
def erf_inputs():
    """cephes_erf: every double -- dense around its branch points |x| = 1 (erf / 1 - erfc), 8 (erfc's two
    rationals) and sqrt(MAXLOG) (erfc = 0 beyond), with the nearest 400 doubles on either side of each, the
    ranges between, tiny and subnormal x, +-0, +-inf, NaN, random bit patterns."""
    rng = np.random.default_rng(1110)
    parts = []
    for c, w in ((1.0, 0.05), (8.0, 0.05), (SQRT_MAXLOG, 0.05)):
        near = np.array([c]).view(np.int64)[0] + np.arange(-400, 401)
        parts += [near.view(np.float64), rng.uniform(c - w, c + w, 15000)]
    pos = np.concatenate(parts + [rng.uniform(0, 30, 30000), 2.0 ** rng.uniform(-1074, 0, 15000),
                                  rng.integers(1, 1 << 52, 5000, dtype=np.uint64).view(np.float64),
                                  [1.0, 8.0, SQRT_MAXLOG, 26.0, 27.0, 38.6, 1e300, DBL_MAX, DBL_MIN, DBL_TRUE_MIN]])
    return np.concatenate([pos, -pos, _bits(rng, 20000), [0.0, -0.0, INF, -INF, NAN, -NAN]])


@functools.lru_cache(None)
def div_inputs():
    """-> (x, b): division_check.cpp -- b = 2 sigma^2 log-uniform over 2^-20..2^13 with x log-uniform, random
    significands near 1 and integer-valued; quotients with significands just below 2 and just above 1 for the
    configured 2 sigma^2 of 2..16-PAM at 0..40 dB and for random b; the grid of simple values."""
    rng = np.random.default_rng(1111)
    n = 45000
    b = 2.0 ** rng.uniform(-20, 13, n)
    x1 = _signs(rng, n) * 2.0 ** rng.uniform(-60, 14, n)
    x2 = (rng.integers(0, 1 << 52, n, dtype=np.uint64) | (rng.integers(1011, 1035, n, dtype=np.uint64) << np.uint64(52))).view(np.float64)
    x3 = rng.integers(-10000, 10001, n).astype(np.float64)
    xs, bs = [x1, x2, x3], [b, b, b]
    cfg = [Es * 10.0 ** (-0.5 * d / 10.0) for Es in (1.0, 5.0, 21.0, 85.0) for d in range(81)]
    for bb in np.concatenate([cfg, 2.0 ** rng.uniform(-20, 13, 200)]).tolist():
        k = np.arange(1, 25)
        e = rng.integers(-20, 20, 24)
        q = np.concatenate([np.ldexp(2.0 - k * 2.0 ** -52, e), np.ldexp(1.0 + k * 2.0 ** -52, e)])
        x = q * bb
        x = np.concatenate([x, np.nextafter(x, 0.0), np.nextafter(x, 1e300), -x])
        xs.append(x)
        bs.append(np.full(x.size, bb))
    gb, gx = np.meshgrid([1.0, 2.0, 0.5, 3.0, float.fromhex("0x1.fffffffffffffp+0"), float.fromhex("0x1.0000000000001p+0"), 1e-6, 1e4],
                         [0.0, -0.0, 1.0, -1.0, float.fromhex("0x1.fffffffffffffp+0"), 1e4, -1e4, 3.0, 7.0], indexing="ij")
    return np.concatenate(xs + [gx.ravel()]), np.concatenate(bs + [gb.ravel()])


# ------------------------------------------------------------------ h_packed
H_NEAR_T = 2.738   # t above it: u = 1 + exp(-t) < 1 + 0x1.09p-4, the near-1 branch of log


def h_near(t):
    """g_log_u's branch for h's argument, as h_packed ranks it: True = the near-1 polynomial (NaN: table)."""
    return np.array([1.0 + math.exp(-min(abs(v), 800.0)) < NEAR1_HI for v in np.asarray(t, np.float64).tolist()])


# the extra arguments a clamp mode's contract admits (strict_pack.hpp): kClampNone every |t| < 700, kClampFinite
# every finite t, kClampFull anything
_PACK_COMMON = (0.0, -0.0, 37.5, np.nextafter(37.5, 0), np.nextafter(37.5, 40), -37.5, 36.75, 41.0, 100.0, 699.0, -699.0)
PACK_SPECIALS = dict(none=_PACK_COMMON, finite=_PACK_COMMON + (700.0, -700.0, 1e300, -1e300, DBL_MAX),
                     full=_PACK_COMMON + (700.0, 1e300, -1e300, INF, -INF, NAN, -NAN))


def pack_counts(nj):
    return sorted({c for c in (0, 1, 63, 64, 65, 64 * nj) if c <= 64 * nj})


@functools.lru_cache(None)
def h_packed_inputs(nj, clamp):
    """-> (t, nN): the arguments of h_packed with nj per lane, wave w = t[64 nj w : 64 nj (w + 1)] with argument j
    of lane l at 64 j + l, and the near-1 count nN each whole wave was built to have (the table count is
    64 nj - nN).  Waves: all near-1, all table path, mixed at random, every count of pack_counts(nj) as nN and
    as nT, waves carrying the clamp mode's specials, and a last, partial wave."""
    rng = np.random.default_rng(1200 + 10 * nj + CLAMP[clamp])
    W = 64 * nj

    def near(n):
        return _signs(rng, n) * rng.uniform(2.75, 45.0 if clamp != "none" else 37.0, n)

    def table(n):
        return _signs(rng, n) * np.where(rng.random(n) < 0.8, rng.uniform(0, 2.72, n), 2.0 ** rng.uniform(-60, 1, n))

    def wave(n_near):
        w = np.concatenate([near(n_near), table(W - n_near)])
        return rng.permutation(w)

    counts = [W] * 6 + [0] * 6 + [int(c) for c in rng.integers(0, W + 1, 24)]
    for c in pack_counts(nj):
        counts += [c, W - c]
    waves = [wave(c) for c in counts]
    sp = np.array(PACK_SPECIALS[clamp])
    for _ in range(4):
        w = wave(int(rng.integers(0, W + 1)))
        at = rng.choice(W, sp.size, replace=False)
        w[at] = sp
        waves.append(w)
        counts.append(int(h_near(w).sum()))
    tail = wave(W // 2)[:W - 27]   # n is no multiple of 64: the last wave's last job lacks 27 lanes
    return np.concatenate(waves + [tail]), np.array(counts)


# ------------------------------------------------------------------ direct-reconciliation LAPPRs
def y_to_lappr_grey(y, constellation, bps, two_var):
    """sims/reconciliation.pyx:25-51 (_y_to_lappr_grey over an array): Gray-labelled log-sums over the alphabet
    with libm's exp and log (math.exp / math.log per element), the square as a product, log(0) = -inf,
    overflow -> inf.  The subtraction, product, division and the sums are numpy's elementwise IEEE operations
    over the samples, taken in the reference's order (i ascending).  -> [S * bps]."""
    y = np.asarray(y, np.float64)
    N, D = np.zeros((bps, y.size)), np.zeros((bps, y.size))
    with np.errstate(all="ignore"):
        for i, ai in enumerate(np.asarray(constellation, np.float64).tolist()):
            d = y - ai
            add = ref_exp(-(d * d) / two_var)
            mi = i
            for l in range(bps):
                if (mi * (mi + 1)) & 3:
                    D[l] += add
                else:
                    N[l] += add
                mi >>= 1
        return np.ascontiguousarray((ref_log(N.ravel()) - ref_log(D.ravel())).reshape(bps, y.size).T).ravel()


# tests/golden/llr_sources_wide.npz: (bits per symbol, shaping nu or None (p_m ~ exp(-nu a_m^2)), SNR dB)
LAPPR_WIDE_CASES = ((3, None, 0.0), (3, None, 40.0), (5, None, 3.0), (5, None, 45.0), (6, None, 6.0), (6, None, 50.0),
                    (8, None, 10.0), (8, None, 60.0), (4, 0.02, 2.0), (4, 0.02, 42.0))


def lappr_samples(constellation, thresholds, two_var, seed):
    """The channel samples of one fixture case: every constellation point and finite threshold with both
    neighbours, +-0, samples beyond either end of the constellation where the sums are subnormal (the nearest
    exponent -(d^2) / two_var in (-745, -708)), where exactly one exponential survives (+-inf LAPPRs) and where
    none does (NaN), typical samples, +-1e300, +-inf and NaN."""
    rng = np.random.default_rng(seed)
    a = np.asarray(constellation, np.float64)
    th = np.asarray(thresholds, np.float64)
    th = th[np.abs(th) <= 2 * np.abs(a).max()]
    u = np.concatenate([rng.uniform(708.5, 744.4, 12), [700.0, 720.0, 740.0, 744.0, 745.0, 746.0, 760.0, 800.0, 2000.0]])
    off = np.sqrt(u * two_var)
    typical = rng.choice(a, 48) + math.sqrt(two_var / 2) * rng.standard_normal(48)
    return np.concatenate([neighbours(a), neighbours(th), [0.0, -0.0], a[-1] + off, a[0] - off, typical,
                           [1e300, -1e300, INF, -INF, NAN]])
