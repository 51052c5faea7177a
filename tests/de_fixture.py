"""The restatement of the sampled density evolution (include/qamr.h "sampled density evolution", DESIGN.md
"Density evolution"): the reference of tests/test_de_cpu.py, tests/test_gpu_density_evolution.py and its debug
rerun.

The random indices are the definition's counter-based draws in numpy uint64 (wrapping), one vector over the
samples j per draw k; the adds are Python float adds in the stated order; the box-plus is the oracle's
(``oracle.box_plus``, the reference's decoder.pyx:41-45 with glibc's exp / log -- numpy's own are others).
Every case is computed once (lru_cache) and its arrays are read-only.
"""
import functools
import math

import numpy as np

INF, NAN = math.inf, math.nan
PAD = -7.25          # the value of output cells that must stay untouched
PAD_ERRORS = -7
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_MASK = (1 << 64) - 1


# ------------------------------------------------------------------ random indices
def rnd(seed, t, phase, j, k, n):
    """The definition, in Python integers."""
    def mix(x):
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _MASK
        return x ^ (x >> 31)

    ctr = (((t * 4 + phase) << 32) + j) * 512 + k
    z = mix((seed + 0x9E3779B97F4A7C15 * (ctr + 1)) & _MASK)
    return ((z >> 32) * n) >> 32


def z_of(seed, ctr):
    """z of a raw counter (uint64 array) -> uint64 array."""
    x = np.uint64(seed) + GOLDEN * (np.asarray(ctr, np.uint64) + np.uint64(1))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def rnd_vec(seed, t, phase, j, k, n):
    """rnd for an array of samples j -> int64 array."""
    j = np.asarray(j, np.uint64)
    ctr = (np.full(j.shape, (t * 4 + phase) << 32, np.uint64) + j) * np.uint64(512) + np.uint64(k)
    return (((z_of(seed, ctr) >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


# ------------------------------------------------------------------ the evolution
def _gather_indices(seed, t, phase, J, count, M):
    """[count][M] message indices of draws k = 2 .. 2 + count - 1."""
    return [rnd_vec(seed, t, phase, J, 2 + k, M).tolist() for k in range(count)]


def evolve(u, edge_vdeg, edge_cdeg, node_vdeg, M, T, seed):
    """-> (errors int64 [T + 1], v2c: list over t = 0..T of float64 [M] (entry 0 is None), c2v: the same, entry
    0 all +0.0): every iteration's populations, so one run serves every T' <= T."""
    import oracle as O

    u = np.asarray(u, np.float64).tolist()
    ev, ec, nv = (np.asarray(a, np.int64) for a in (edge_vdeg, edge_cdeg, node_vdeg))
    assert ev.size == ec.size
    Mu, Ne, Nv = len(u), ev.size, nv.size
    J = np.arange(M, dtype=np.uint64)
    box_plus = O.box_plus

    def post(t, c2v):
        d = nv[rnd_vec(seed, t, 2, J, 0, Nv)].tolist()
        iu = rnd_vec(seed, t, 2, J, 1, Mu).tolist()
        idx = _gather_indices(seed, t, 2, J, max(d), M)
        n = 0
        for j in range(M):
            p = u[iu[j]]
            for k in range(d[j]):
                p = p + c2v[idx[k][j]]
            n += 0 if p >= 0 else 1
        return n

    c2v = [0.0] * M
    errors = [post(0, c2v)]
    v2c_t, c2v_t = [None], [np.array(c2v)]
    for t in range(1, T + 1):
        d = ev[rnd_vec(seed, t, 0, J, 0, Ne)].tolist()
        iu = rnd_vec(seed, t, 0, J, 1, Mu).tolist()
        idx = _gather_indices(seed, t, 0, J, max(d) - 1, M)
        v2c = [0.0] * M
        for j in range(M):
            s = u[iu[j]]
            for k in range(d[j] - 1):
                s = s + c2v[idx[k][j]]
            v2c[j] = s
        d = ec[rnd_vec(seed, t, 1, J, 0, Ne)].tolist()
        idx = _gather_indices(seed, t, 1, J, max(d) - 1, M)   # k = 0 .. d-2 are draws 2 .. d
        new = [0.0] * M
        for j in range(M):
            F = v2c[idx[0][j]]
            for k in range(1, d[j] - 1):
                F = box_plus(F, v2c[idx[k][j]])
            new[j] = F
        c2v = new
        errors.append(post(t, c2v))
        v2c_t.append(np.array(v2c))
        c2v_t.append(np.array(c2v))
    for a in v2c_t[1:] + c2v_t:
        a.setflags(write=False)
    e = np.array(errors, np.int64)
    e.setflags(write=False)
    return e, v2c_t, c2v_t


def at(ref, T):
    """(errors [T + 1], v2c(T) or None, c2v(T)) of a longer run."""
    errors, v2c_t, c2v_t = ref
    return errors[:T + 1], v2c_t[T], c2v_t[T]


def _ro(a):
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------ inputs
def biawgn(sigma, n, seed):
    """n signed BIAWGN LLRs of the all-correct word: 2 / sigma^2 + (2 / sigma) N(0, 1)."""
    return _ro(2.0 / sigma ** 2 + (2.0 / sigma) * np.random.default_rng(seed).standard_normal(n))


def regular_tables(dv=3, dc=6, Ne=3024, Nv=1008):
    return (_ro(np.full(Ne, dv, np.int32)), _ro(np.full(Ne, dc, np.int32)), _ro(np.full(Nv, dv, np.int32)))


def mixed_tables(vdegs, cdegs, ndegs, n, seed):
    """Tables of n entries drawn from the given degrees, each degree present."""
    rng = np.random.default_rng(seed)

    def pick(vals):
        vals = np.asarray(vals, np.int32)
        a = vals[rng.integers(0, vals.size, n)]
        a[:vals.size] = vals
        return _ro(rng.permutation(a))

    return pick(vdegs), pick(cdegs), pick(ndegs)


# A: the (3, 6) ensemble on 1 000 BIAWGN draws at sigma = 0.80 (Mu != M)
A_SIZES = (1, 64, 100, 4096)
A_ITERS = (0, 1, 2, 8)
A_SEED = 7


def a_inputs():
    return biawgn(0.80, 1000, 5), regular_tables()


@functools.lru_cache(None)
def a_ref(M):
    u, tables = a_inputs()
    return evolve(u, *tables, M, max(A_ITERS), A_SEED)


# B: degrees that diverge inside one wave
B_M, B_T, B_SEED = 256, 3, 11
B_VDEG, B_CDEG, B_NDEG = (1, 2, 3, 13, 255), (2, 3, 7, 30, 255), (0, 1, 2, 3, 13, 255)
B_HIGH_RATE_CDEG = (22, 27)


@functools.lru_cache(None)
def b_inputs(high_rate=False):
    u = biawgn(0.80, 777, 6)
    if high_rate:
        return u, mixed_tables((3,), B_HIGH_RATE_CDEG, (3,), 40, 13)
    return u, mixed_tables(B_VDEG, B_CDEG, B_NDEG, 48, 12)


@functools.lru_cache(None)
def b_ref(high_rate=False):
    u, tables = b_inputs(high_rate)
    return evolve(u, *tables, B_M, B_T, B_SEED)


# C: special values planted in u.  Degree-1 variables and degree-2 checks hand a value on untouched (a
# -0.0 stays -0.0), isolated variables decide on the channel value alone.
C_M, C_T, C_SEED = 128, 3, 17


@functools.lru_cache(None)
def c_inputs():
    import math_fixture as MF

    specials = (INF, -INF, NAN, 0.0, -0.0, 5e-324, -5e-324, 1e-310) + tuple(MF.BOX_SPECIALS) + tuple(MF.H_SPECIALS) + \
        tuple(MF.FULL_SPECIALS)
    u = np.array(biawgn(0.80, 256, 8))
    pos = np.random.default_rng(9).permutation(256)[:len(specials)]
    u[pos] = specials
    return _ro(u), mixed_tables((1, 2, 3), (2, 3, 6), (0, 1, 3), 24, 14), len(specials)


@functools.lru_cache(None)
def c_ref():
    u, tables, _ = c_inputs()
    return evolve(u, *tables, C_M, C_T, C_SEED)


# D: the signed population of a batch (the GPU test draws it), evolved
D_M, D_T, D_SEED = 4096, 4, 23


def signed_population(lappr, word, alpha):
    """lappr float64 [rows, B], word uint8 [rows, B] (the frames' columns) -> u [rows * B] by numpy: one
    rounding, then the sign bit."""
    x = np.ascontiguousarray(np.float64(alpha) * np.asarray(lappr, np.float64))
    bits = x.view(np.uint64) ^ (np.asarray(word).astype(np.uint64) != 0).astype(np.uint64) << np.uint64(63)
    return bits.view(np.float64).ravel()
