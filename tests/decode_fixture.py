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
  ``sigma_of``, ``case_of``), which tests/test_gpu_high_degrees.py extends to ``HIGH_DEGREES`` and
  the high-degree mixed code (``himix_code``, ``himix_case``, ``assert_high_conditions``;
  ``check_block``: the checks per workgroup of a sweep, for the ragged last workgroup);
  ``deal_sockets`` / ``hub_code`` / ``scattered_code``: graph builders.
* ``golden_cases`` / ``frame_digests`` / ``input_digest`` / ``GoldenDegrees`` /
  ``assert_golden_records``: the cases whose decodes by the compiled reference are recorded in
  tests/golden/decoder_degrees.npz, the one digest definition, and the fixture's reader.
"""
import contextlib
import functools
import hashlib

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
    columns [B, ld) keep the caller's value.  Returns the device's (success, iterations, final
    LAPPRs [B, V]) on the host."""
    import torch

    s2, i2, f2 = ref
    fin = torch.full(tuple(L.shape), pad, dtype=torch.float64, device="cuda")
    _, succ, its = dec.decode_device(L, S, B, mi, final_fi=fin)
    torch.cuda.synchronize()
    got = succ.cpu().numpy(), its.cpu().numpy(), fin[:, :B].cpu().numpy().T
    assert np.array_equal(got[0], s2[:B]), tag
    assert np.array_equal(got[1], i2[:B]), tag
    assert_bit_exact(got[2], f2[:B])
    assert bool((fin[:, B:] == pad).all()), tag
    return got


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
    repack and end 64 columns wide, at least 5 distinct stop iterations.  D > 16 (the
    runtime-degree kernel; lock-step, no repack): (0.25, 0.5), which meets assert_high_conditions;
    seen at 30 iterations, special variant (D: successes of 512, distinct stop iterations >= 1):
    17: 507, 10   18: 508, 9   22: 507, 17   27: 488, 18   30: 464, 17   33: 464, 16
    65: 350, 15   100: 314, 16   255: 224, 8."""
    if D > 16:
        return (0.25, 0.5)
    return {2: (1.2, 2.0), 3: (0.9, 1.5), 4: (0.7, 1.1)}.get(D, (0.5, 0.8) if D <= 8 else (0.35, 0.6))


@functools.lru_cache(maxsize=None)
def case_of(D, variant):
    """The 512 frames of (regular (3, D) code of V = v_of(D), variant)."""
    from qamr import codes

    V = v_of(D)
    case = _variant_case(*codes.regular_code(V, 3, D, seed=100 + D), sigma_of(D), 1000 + D, variant)
    assert case["orc"].vnum == V and case["orc"].cnum == 3 * V // D
    return case


# ------------------------------------------------------------------ check degrees above 16
# the runtime-degree kernel (decoder.hip k_check_generic): just past the templated range (17, 18),
# the long DVB-S2 codes' degrees (18, 22, 27, 30), more than a wavefront (65), the largest (255)
HIGH_DEGREES = (17, 18, 22, 27, 30, 33, 65, 100, 255)
PLANTED = tuple(np.r_[0:4, H:H + 4, 8, 300].tolist())   # plant_special(h = H): codewords, special values

# the high-degree mixed code: a packed class (7), a templated unpacked one (12) and three runtime
# ones; a class of 65 checks (a wavefront plus one lane) and one of a single check; parallel
# edges, every sixth variable isolated, variable 0 a hub of degree 70 (as few_fixture.mixed_code)
HIMIX_V = 702
HIMIX_CLASSES = [(7, 40), (12, 20), (17, 65), (30, 13), (64, 1)]
HIMIX_HUB_DEGREE = 70
HIMIX_SEED = 1730
# per-frame noise sigma ~ U(lo, hi) of its frames, picked on the CPU from the oracle alone so that
# assert_high_conditions holds; seen at 30 iterations (variant: successes of 512, distinct stop
# iterations >= 1, frames running after iteration 29):
#   (0.25, 0.5)  special: 508,  6,   4   clean: 510,  7,   2   (few late stops)
#   (0.35, 0.6)  special: 481, 22,  32   clean: 482, 22,  31   <- chosen
#   (0.4, 0.7)   special: 329, 23, 183   clean: 330, 23, 182
HIMIX_SIGMA = (0.35, 0.6)


def himix_code():
    return hub_code(HIMIX_V, HIMIX_CLASSES, HIMIX_HUB_DEGREE, HIMIX_SEED)


@functools.lru_cache(maxsize=None)
def himix_case(variant):
    """The 512 frames of (high-degree mixed code, variant).  plant_special's five values land on
    the hub (variable 0), an isolated variable (2) and three ordinary ones."""
    vid, cid = himix_code()
    case = _variant_case(vid, cid, HIMIX_SIGMA, 1000 + HIMIX_SEED, variant)
    assert case["orc"].vnum == HIMIX_V and case["orc"].cnum == sum(n for _, n in HIMIX_CLASSES)
    return case


def high_case(key, variant):
    """case_of(D, variant) for a degree of HIGH_DEGREES, himix_case(variant) for "mix"."""
    return himix_case(variant) if key == "mix" else case_of(key, variant)


def high_classes(key):
    """The check classes (degree, number of checks) of high_case(key, .)."""
    return list(HIMIX_CLASSES) if key == "mix" else [(key, 3 * v_of(key) // key)]


def check_block(ncols, n, check_ft=128, check_per=16, min_blocks=2048):
    """(frame tile, checks per workgroup) of a check sweep over ncols frames of a class of n checks,
    restated from decoder.hip make_geom: the tile is the largest of 256, 128, 64 that is at most
    check_ft and divides ncols, a workgroup's 256 threads hold nsub = 256 / tile checks side by
    side and per in a row; min_blocks > 0 lowers per, down to 1, while the launch has fewer
    workgroups.  A class whose n is no multiple of per * nsub ends in a ragged workgroup."""
    ft = 256
    while ft > 64 and (ft > check_ft or ncols % ft):
        ft //= 2
    nsub, per = 256 // ft, max(1, check_per)
    if n > 0 and min_blocks > 0:
        per = max(1, min(per, n * (ncols // ft) // (min_blocks * nsub)))
    return ft, per * nsub


def assert_high_conditions(case, variant):
    """Conditions on the frames of a high-degree case, from the oracle alone (before any GPU
    output), at 30 iterations: some frames succeed and some fail, the successful ones stop at
    >= 5 distinct iterations >= 1, the planted codewords stop at (1, 0), and at most 384 frames
    still run after iteration 29, so at least one 128-column tile goes idle while the
    active-frame lists are live.  Returns (successes, distinct stop iterations, still running)."""
    succ, its, _ = oracle_of(case, MI)
    n = int((succ != 0).sum())
    assert 0 < n < LD, n
    stops = np.unique(its[(succ != 0) & (its >= 1)])
    assert stops.size >= 5, stops
    if variant == "special":
        cw = np.array(PLANTED[:8])
        assert (succ[cw] == 1).all() and (its[cw] == 0).all(), (succ[cw], its[cw])
    left = sum(running(succ, its, LD, MI - 1))
    assert left <= 384, left
    return n, int(stops.size), left


# ------------------------------------------------------------------ the reference's own records
# tests/golden/decoder_degrees.npz (tests/golden/make_golden_degrees.py): what the compiled
# reference's Decoder.decode returned for the frames of these cases, as digests
GOLDEN_MIS = (1, 2, 3, MI)
CANON_NAN = 0x7FF8000000000000


def _canon_bytes(a):
    """The doubles' little-endian int64 view with every NaN replaced by CANON_NAN, as bytes."""
    a = np.ascontiguousarray(a, np.float64)
    bits = a.view(np.int64).copy()
    bits[np.isnan(a)] = CANON_NAN
    return bits.astype("<i8").tobytes()


def frame_digests(final):
    """[n, 8] uint8: per frame (row) the 8-byte BLAKE2b digest of its canonical bytes."""
    final = np.ascontiguousarray(final, np.float64)
    assert final.ndim == 2
    return np.array([np.frombuffer(hashlib.blake2b(_canon_bytes(r), digest_size=8).digest(), np.uint8) for r in final],
                    np.uint8).reshape(len(final), 8)


def input_digest(llr, synd):
    """[8] uint8: the digest of a case's inputs (shapes, canonical LAPPRs, syndromes)."""
    h = hashlib.blake2b(digest_size=8)
    h.update(np.array(llr.shape + synd.shape, "<i8").tobytes())
    h.update(_canon_bytes(llr))
    h.update(np.ascontiguousarray(synd, np.uint8).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def golden_cases():
    """name -> function returning the case, in the fixture's order: the degree matrix's and the
    high degrees' cases, the repack file's small codes (special variant), the few-frame mixed
    code, the high-degree mixed code."""
    import few_fixture

    cases = {}
    for D in tuple(range(2, 17)) + HIGH_DEGREES:
        for variant in ("clean", "special"):
            cases[f"deg{D}-{variant}"] = functools.partial(case_of, D, variant)
    for name in CODES:
        cases[f"small-{name}-special"] = functools.partial(small_case, name, "special")
    cases["few-mixed"] = few_fixture.mixed_case
    for variant in ("clean", "special"):
        cases[f"himix-{variant}"] = functools.partial(himix_case, variant)
    return cases


def golden_frames(n, mi):
    """The frames of an n-frame case recorded at max_iterations = mi: all at 30; at 1, 2, 3 the
    first 64 and every planted frame."""
    if mi == MI:
        return np.arange(n)
    return np.array(sorted(set(range(min(n, 64))) | {f for f in PLANTED if f < n}))


def golden_full_frames(n):
    """The frames whose final LAPPRs at 30 iterations are recorded in full: the two that carry
    special values and frame 12 (a 5-frame case: all)."""
    return np.array([f for f in (8, 300, 12) if f < n] if n > 12 else range(n))


class GoldenDegrees:
    """Reader of tests/golden/decoder_degrees.npz: per case name the input digest, per
    max_iterations of GOLDEN_MIS (frames, success, iterations, digests), and the full frames."""

    def __init__(self, z):
        self.names = [str(s) for s in z["names"]]
        self.z = {k: z[k] for k in z.files}
        self.at = {s: k for k, s in enumerate(self.names)}

    def _part(self, key, name):
        off = self.z[key + "_off"]
        k = self.at[name]
        return slice(int(off[k]), int(off[k + 1]))

    def n_frames(self, name):
        return int(self.z["n_frames"][self.at[name]])

    def input_digest(self, name):
        return self.z["input_digest"][self.at[name]]

    def records(self, name, mi):
        """(frames, success, iterations, digests [n, 8]) the reference returned at mi."""
        p = self._part(f"mi{mi}", name)
        frames = golden_frames(self.n_frames(name), mi)
        assert p.stop - p.start == frames.size
        return frames, self.z[f"mi{mi}_success"][p], self.z[f"mi{mi}_iters"][p], self.z[f"mi{mi}_digest"][p]

    def full(self, name):
        """(frames, final LAPPRs [k, V]) at 30 iterations."""
        frames = golden_full_frames(self.n_frames(name))
        p = self._part("full", name)
        return frames, self.z["full"][p].reshape(frames.size, -1)


def assert_golden_inputs(gold, name, case):
    """The fixture was recorded on exactly these frames (detects generator drift first)."""
    assert gold.n_frames(name) == case["llr"].shape[0], name
    assert np.array_equal(gold.input_digest(name), input_digest(case["llr"], case["synd"])), \
        f"{name}: the inputs differ from those tests/golden/make_golden_degrees.py recorded"


def assert_golden_records(gold, name, mi, succ, its, final, tag=None):
    """success, iterations and per-frame digests of final ([n, V], all frames of the case) equal
    the reference's records at mi; the first differing frame is named."""
    frames, s, i, d = gold.records(name, mi)
    tag = tag or (name, mi)
    assert np.array_equal(np.asarray(succ)[frames], s), (tag, "success", frames[np.asarray(succ)[frames] != s][:8])
    assert np.array_equal(np.asarray(its)[frames], i), (tag, "iterations", frames[np.asarray(its)[frames] != i][:8])
    bad = (frame_digests(np.asarray(final)[frames]) != d).any(axis=1)
    assert not bad.any(), (tag, f"{int(bad.sum())} frames' final LAPPRs differ from the reference's; first",
                           frames[bad][:8])


# ------------------------------------------------------------------ graph builders
def deal_sockets(dv, dc, rng):
    """(vid, cid): variable v has dv[v] sockets; the sockets are shuffled and dealt dc per check
    (parallel edges kept), those left over dropped."""
    sockets = np.repeat(np.arange(len(dv)), dv)
    M = sockets.size // dc
    sockets = sockets[rng.permutation(sockets.size)][:M * dc]
    return sockets.astype(np.int64), np.repeat(np.arange(M), dc).astype(np.int64)


def hub_code(V, classes, hub_degree, seed):
    """(vid, cid): variable 0 is a hub of hub_degree sockets, every sixth variable (v % 6 == 2) is
    isolated, every other one has 3 or 4 sockets; the sockets are shuffled by default_rng(seed)
    and dealt check-major (parallel edges kept) to the checks of ``classes`` ((degree, number of
    checks)) in a shuffled order."""
    rng = np.random.default_rng(seed)
    E = sum(d * n for d, n in classes)
    conn = np.array([v for v in range(1, V) if v % 6 != 2])
    extra = E - hub_degree - 3 * conn.size
    assert 0 <= extra <= conn.size
    deg = np.full(conn.size, 3)
    deg[rng.permutation(conn.size)[:extra]] = 4
    s = np.concatenate([np.zeros(hub_degree, np.int64), np.repeat(conn, deg)])
    rng.shuffle(s)
    degs = np.concatenate([np.full(n, d) for d, n in classes])
    rng.shuffle(degs)
    assert degs.sum() == s.size == E
    return s.astype(np.int64), np.repeat(np.arange(degs.size), degs).astype(np.int64)


def scattered_code(rng, deg, V):
    """(vid, cid): check c has degree deg[c]; the sockets are every variable once and
    integers(0, V) for the rest, shuffled (every variable used, parallel edges kept)."""
    deg = np.asarray(deg)
    sockets = np.concatenate([np.arange(V), rng.integers(0, V, int(deg.sum()) - V)])
    rng.shuffle(sockets)
    return sockets.astype(np.int64), np.repeat(np.arange(deg.size), deg).astype(np.int64)
