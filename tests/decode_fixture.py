"""Knobs, launch counters, frames, cases and the device round trip shared by the decoder's GPU
tests (tests/test_gpu_*.py) and tests/few_fixture.py; pinned on the CPU by
tests/test_decode_fixture_cpu.py.  Every case is computed once, shared and never modified.

* ``knobs`` / ``profiled``: the one place where tuning knobs are saved, set and restored and the
  profiling counters switched on and off; ``launches`` / ``assert_path``: which decode path ran.
* ``draw_frames`` / ``plant_special`` / ``make_case`` / ``oracle_of``: frames of a code, and the
  oracle's decodes of them per max_iterations.
* ``to_device`` / ``decode_and_compare``: the frame-innermost upload, and one decode into a padded
  output compared with the oracle.
* ``running`` / ``predict_repack`` / ``assert_repack_counts`` / ``assert_repack_inputs``: the
  repacks the device must decide, from the oracle's (success, iterations) alone.
* the small codes of tests/test_gpu_repack_small_codes.py (``CODES``, ``small_code``,
  ``small_case``) and the regular (3, D) codes of tests/test_gpu_degree_matrix.py (``v_of``,
  ``sigma_of``, ``case_of``); ``deal_sockets`` / ``scattered_code``: graph builders.
"""
import contextlib
import functools

import numpy as np

from conftest import assert_bit_exact

import oracle as O

LD = 512
H = LD // 2   # columns per range of the two-stream schedule
MI = 30
PAD = 7.0
NEVER = ((0, 0), (H, H))   # repack_stats of a decode that never repacked
SPECIAL5 = [np.inf, -np.inf, -0.0, 0.0, np.nan]


# ------------------------------------------------------------------ knobs and counters
@contextlib.contextmanager
def knobs(defaults=None, **values):
    """Set tuning knobs for the body; the values they had come back on exit, exception or not.
    ``defaults`` (knob -> the library's default) is asserted first; then every knob of it is set,
    to its value in ``values`` or else to its default, so a run never inherits a knob."""
    from qamr import _lib

    want = {**(defaults or {}), **values}
    for k, v in (defaults or {}).items():
        assert _lib.tune_get(k) == v, f"default {k}={v} changed: update this test"
    saved = {k: _lib.tune_get(k) for k in want}
    try:
        for k, v in want.items():
            _lib.tune_set(k, v)
        yield
    finally:
        for k, v in saved.items():
            _lib.tune_set(k, v)


@contextlib.contextmanager
def profiled():
    """The profiling counters count the launches of the body, from zero."""
    from qamr import _lib

    _lib.profile_enable(True)
    _lib.profile_reset()
    try:
        yield
    finally:
        _lib.profile_enable(False)


def launches(D):
    """Launch counts of the frame-parallel decode paths of check degree D (inside ``profiled``)."""
    from qamr import _lib

    return {k: _lib.profile_query(f"{k}_d{D}")[1] for k in ("resident", "iter", "check", "check1")}


def assert_path(path, mi, n, iter_launches):
    """The launches that ran, by their profile names; ``iter_launches``: the iter_dD launches of
    the one-launch-per-iteration path, (max_iterations + 1) per stream.  The frame-parallel
    schedules name their first check sweep check1_dD and the sweeps of iterations 2.. check_dD."""
    if path == "resident":
        assert n == dict(resident=1, iter=0, check=0, check1=0), n
    elif path == "iter":
        assert n == dict(resident=0, iter=iter_launches, check=0, check1=0), n
    else:
        assert path == "check"
        assert n["check1"] > 0 and n["iter"] == 0 and n["resident"] == 0, n
        assert n["check"] > 0 or mi == 1, n   # max_iterations = 1: the first sweep is the only one


# ------------------------------------------------------------------ frames and cases
def draw_frames(orc, rng, n, sigma):
    """(llr, synd, word, sig) of n frames: words, then per-frame noise sigma ~ U(*sigma), then
    the noise (the sigma ranges of every case were conditioned on draws in this order)."""
    V = orc.vnum
    word = rng.integers(0, 2, (n, V)).astype(np.uint8)
    synd = np.stack([orc.eval_syndrome(w) for w in word])
    sig = rng.uniform(*sigma, n)[:, None]
    llr = 2 / sig ** 2 * ((1 - 2.0 * word) + sig * rng.standard_normal((n, V)))
    return llr, synd, word, sig


def plant_special(llr, word, sig, h):
    """Frames 0..3 and h..h+3 become exact codewords ((1, 0) in both ranges: they stop at
    iteration 0); frames 8 and 300 carry inf, -inf, -0.0, 0.0, NaN, which clears the batch's
    finite flag."""
    cw = np.r_[0:4, h:h + 4]
    llr[cw] = 2 / sig[cw] ** 2 * (1 - 2.0 * word[cw])
    for f in (8, 300):
        llr[f, :5] = SPECIAL5


def make_case(vid, cid, n, sigma, seed, plant=None):
    """n frames from default_rng(seed), read-only, and an empty cache of the oracle's decodes per
    max_iterations; ``plant(orc, llr, word, sig)`` may change the LAPPRs first, what it returns
    is kept as ``planted``."""
    orc = O.OracleCode(vid, cid)
    llr, synd, word, sig = draw_frames(orc, np.random.default_rng(seed), n, sigma)
    planted = plant(orc, llr, word, sig) if plant else ()
    for a in (llr, synd, word, sig):
        a.setflags(write=False)
    return dict(vid=vid, cid=cid, orc=orc, llr=llr, synd=synd, word=word, sig=sig, ref={}, planted=planted)


def oracle_of(case, mi):
    """(success, iterations, final LAPPRs) of the oracle at max_iterations = mi, read-only."""
    if mi not in case["ref"]:
        ref = case["orc"].decode_batch(case["llr"], case["synd"], mi)
        for a in ref:
            a.setflags(write=False)
        case["ref"][mi] = ref
    return case["ref"][mi]


def _variant_case(vid, cid, sigma, seed, variant):
    """LD frames; ``clean``: all LAPPRs finite, ``special``: plant_special."""
    assert variant in ("clean", "special")
    special = variant == "special"
    case = make_case(vid, cid, LD, sigma, seed,
                     plant=(lambda orc, llr, word, sig: plant_special(llr, word, sig, H)) if special else None)
    assert np.isfinite(case["llr"]).all() == (not special)
    return case


# ------------------------------------------------------------------ device round trip
def to_device(case, B, ld):
    """The first B frames, frame-innermost in [rows, ld] device tensors with zero padding."""
    import torch

    V, C = case["orc"].vnum, case["orc"].cnum
    L = torch.zeros((V, ld), dtype=torch.float64, device="cuda")
    L[:, :B] = torch.from_numpy(case["llr"][:B].T.copy()).cuda()
    S = torch.zeros((C, ld), dtype=torch.uint8, device="cuda")
    S[:, :B] = torch.from_numpy(case["synd"][:B].T.copy()).cuda()
    return L, S


def decode_and_compare(dec, L, S, B, mi, ref, tag, pad=PAD):
    """One decode into a final_fi filled with pad: all B frames equal the oracle's, the padding
    columns [B, ld) keep the caller's value."""
    import torch

    s2, i2, f2 = ref
    fin = torch.full(tuple(L.shape), pad, dtype=torch.float64, device="cuda")
    _, succ, its = dec.decode_device(L, S, B, mi, final_fi=fin)
    torch.cuda.synchronize()
    assert np.array_equal(succ.cpu().numpy(), s2[:B]), tag
    assert np.array_equal(its.cpu().numpy(), i2[:B]), tag
    assert_bit_exact(fin[:, :B].cpu().numpy().T, f2[:B])
    assert bool((fin[:, B:] == pad).all()), tag


# ------------------------------------------------------------------ repack prediction
def running(succ, its, B, t):
    """Frames of each range still running after the status update of iteration t."""
    run = ~((succ[:B] != 0) & (its[:B] <= t))
    return int(run[:H].sum()), int(run[H:].sum())


def predict_repack(succ, its, B, mi, pct=80):
    """((repacks 0, repacks 1), (width 0, width 1)) the device must end with: the decision point
    before a range's variable sweep t < mi reads the count its status launch of iteration t - 1
    wrote, and repacks to max(64, count rounded up to 64) when the count is at most pct % of the
    width and that is narrower (decode_repack.hip repack_go)."""
    reps, ws = [], []
    for k in range(2):
        w, rep = H, 0
        for t in range(1, mi):
            cnt = running(succ, its, B, t - 1)[k]
            if w > 64 and cnt > 0 and cnt * 100 <= w * pct:
                wn = max(64, -(-cnt // 64) * 64)
                if wn < w:
                    w, rep = wn, rep + 1
        reps.append(rep)
        ws.append(w)
    return tuple(reps), tuple(ws)


def assert_repack_counts(case, B, mi):
    """Conditions on the frames, from the oracle alone (before any GPU output): each range's
    running count reaches 80 % of its width before the last decision point, the frames stop at
    >= 5 distinct iterations, and both ranges are predicted to repack and end narrower than H.
    Returns the prediction."""
    succ, its, _ = oracle_of(case, mi)
    counts = np.array([running(succ, its, B, t) for t in range(mi - 1)])
    assert (counts.min(axis=0) <= 0.8 * H).all(), counts.min(axis=0)   # both ranges reach the threshold
    iters_ok = np.unique(its[:B][succ[:B] != 0])
    assert 0 < succ[:B].sum() and iters_ok.size >= 5, iters_ok        # frames stop at many iterations
    reps, widths = predict_repack(succ, its, B, mi)
    assert min(reps) >= 1 and max(widths) < H, (reps, widths)          # so both ranges must repack
    return reps, widths


def assert_repack_inputs(V, classes, case, B, mi):
    """The graph has V variables of degree 3 and the check classes (degree, number of checks),
    none above degree 16; then assert_repack_counts."""
    deg = np.bincount(case["cid"])
    assert set(np.unique(deg)) == {d for d, _ in classes} and deg.max() <= 16, np.unique(deg)
    for d, n in classes:
        assert int((deg == d).sum()) == n
    assert np.array_equal(np.bincount(case["vid"]), np.full(V, 3))
    return assert_repack_counts(case, B, mi)


# ------------------------------------------------------------------ the repack file's small codes
# check classes as (degree, number of checks); the degrees sum to 3 V
CODES = {
    "reg7": (770, [(7, 330)]),
    "reg11": (704, [(11, 192)]),
    "reg12": (768, [(12, 192)]),
    "reg16": (768, [(16, 144)]),
    "side12": (768, [(6, 344), (12, 20)]),           # 2064 + 240 edges
    "half7_13": (768, [(7, 162), (13, 90)]),         # 1134 + 1170
    "mix12_16_5": (768, [(12, 88), (16, 63), (5, 48)]),  # 1056 + 1008 + 240
}
SEEDS = {"reg7": 7, "reg11": 11, "reg12": 12, "reg16": 16, "side12": 112, "half7_13": 713, "mix12_16_5": 1216}
# per-frame noise sigma ~ U(lo, hi): (0.35, 0.6) unless the code then converges within a few
# iterations (picked on the CPU, from the oracle alone: frames stop at many different iterations,
# a few run to the last sweep, and both ranges end at most 64 columns wide)
SIGMA = {"reg7": (0.5, 0.8), "side12": (0.5, 0.8), "half7_13": (0.4, 0.7)}

# knob sets of the repack runs at max_iterations = 30 (values not named: the defaults below)
REPACK_DEFAULTS = dict(split=3, compact=1, repack=1, repack_pct=80, repack_grid=128, side=1, nt=1, check_tail=4,
                       split_min_blocks=1024, resident=1)
REPACK_RUNS = [
    dict(split_min_blocks=0),
    dict(split_min_blocks=0, repack=0),
    dict(split_min_blocks=0, repack_pct=50, repack_grid=7),
    dict(split_min_blocks=0, side=0),
    dict(split_min_blocks=0, compact=0),
    dict(split_min_blocks=0, nt=0, check_tail=0),
    dict(split=1),   # lock-step (run_flat; the one-launch-per-iteration schedule for reg7)
]


def small_code(name):
    """(vid, cid): sockets repeat(arange(V), 3) shuffled by default_rng(seed), dealt check-major
    (parallel edges kept, as codes.regular_code); the classes' checks in a shuffled order."""
    from qamr import codes

    V, classes = CODES[name]
    if len(classes) == 1:
        return codes.regular_code(V, 3, classes[0][0], SEEDS[name])
    rng = np.random.default_rng(SEEDS[name])
    s = np.repeat(np.arange(V), 3)
    rng.shuffle(s)
    degs = np.concatenate([np.full(n, d) for d, n in classes])
    rng.shuffle(degs)
    assert degs.sum() == s.size
    return s.astype(np.int64), np.repeat(np.arange(degs.size), degs).astype(np.int64)


@functools.lru_cache(maxsize=None)
def small_case(name, variant):
    """The 512 frames of (code of CODES, variant)."""
    return _variant_case(*small_code(name), SIGMA.get(name, (0.35, 0.6)), 1000 + SEEDS[name], variant)


# ------------------------------------------------------------------ the degree matrix's codes
def v_of(D):
    """The first V >= 768 with 3 V % D == 0."""
    V = 768
    while 3 * V % D:
        V += 1
    return V


def sigma_of(D):
    """Per-frame noise sigma ~ U(lo, hi), picked on the CPU from the oracle alone: both ranges
    repack and end 64 columns wide, at least 5 distinct stop iterations."""
    return {2: (1.2, 2.0), 3: (0.9, 1.5), 4: (0.7, 1.1)}.get(D, (0.5, 0.8) if D <= 8 else (0.35, 0.6))


@functools.lru_cache(maxsize=None)
def case_of(D, variant):
    """The 512 frames of (regular (3, D) code of V = v_of(D), variant)."""
    from qamr import codes

    V = v_of(D)
    case = _variant_case(*codes.regular_code(V, 3, D, seed=100 + D), sigma_of(D), 1000 + D, variant)
    assert case["orc"].vnum == V and case["orc"].cnum == 3 * V // D
    return case


# ------------------------------------------------------------------ graph builders
def deal_sockets(dv, dc, rng):
    """(vid, cid): variable v has dv[v] sockets; the sockets are shuffled and dealt dc per check
    (parallel edges kept), those left over dropped."""
    sockets = np.repeat(np.arange(len(dv)), dv)
    M = sockets.size // dc
    sockets = sockets[rng.permutation(sockets.size)][:M * dc]
    return sockets.astype(np.int64), np.repeat(np.arange(M), dc).astype(np.int64)


def scattered_code(rng, deg, V):
    """(vid, cid): check c has degree deg[c]; the sockets are every variable once and
    integers(0, V) for the rest, shuffled (every variable used, parallel edges kept)."""
    deg = np.asarray(deg)
    sockets = np.concatenate([np.arange(V), rng.integers(0, V, int(deg.sum()) - V)])
    rng.shuffle(sockets)
    return sockets.astype(np.int64), np.repeat(np.arange(deg.size), deg).astype(np.int64)
