"""Check degrees 2..16 in every decode schedule, in both clamp variants.

The decoder (decoder.hip, decode_small.hip) instantiates its check update per degree: ``k_check<D>`` for D = 2..16 (the
frame-parallel sweep of the lock-step and two-stream schedules, with the repack's transition
mapping), and ``check_narrow<D>``, ``k_iter<D>`` and ``k_resident<D>`` for D = 2..10
(kPackMaxDeg); the packed update's rounds (strict_pack.hpp) are laid out at compile time from D,
so every D is its own code.  Here one regular (3, D) code of V ~ 770 per degree decodes 512 frames
(ld = 512) in each schedule that can run it:

1. two-stream (``split_min_blocks = 0``, ``resident = 0``) with the device-decided repack, its
   transition sweeps and, for D <= 10, the narrow sweeps;
2. two-stream with ``repack = 0``; 3. with ``compact = 0``;
4. lock-step frame-parallel (``split = 1``, ``fused_iter = 0``, ``resident = 0``);
5. D <= 10: one launch per iteration (``resident = 0``, ``split = 1``; ``iter_streams`` 2, 1);
6. D <= 10: frame-resident, default knobs.

Every frame of every run is compared with the oracle (oracle/qamr_oracle.c): success flag,
iteration count, final LAPPRs bit for bit, padding columns untouched.  Which path ran is read from
the profiling counters (the launches are named ``resident_dD``, ``iter_dD``, ``check1_dD``,
``check_dD``), in the same run whose outputs are compared.  The inputs are conditioned on the CPU
as in tests/test_gpu_repack_small_codes.py.
"""
import functools
from unittest import mock

import numpy as np
import pytest

from conftest import assert_bit_exact

import oracle as O
import test_gpu_repack_small_codes as R
from test_gpu_repack_small_codes import _assert_inputs, _predict

pytestmark = pytest.mark.gpu

LD = 512
MI = 30
PAD = 7.0
NEVER = ((0, 0), (LD // 2, LD // 2))
DEGREES = tuple(range(2, 17))
PACK_MAX = 10   # decode_dev.hpp kPackMaxDeg: narrow sweeps, k_iter and k_resident exist up to here


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


# the knobs the runs touch and their defaults (every run sets all of them; restored in a finally)
DEFAULTS = dict(split=3, compact=1, repack=1, split_min_blocks=1024, resident=1, fused_iter=1, iter_streams=2)
# run -> (knobs, path, max_iterations); "path" names the launches that must have run
TWO_STREAM = dict(split_min_blocks=0, resident=0)
LOCKSTEP = dict(split=1, fused_iter=0, resident=0)
ITER = dict(split=1, resident=0)


def runs_of(D):
    runs = [("two-stream", TWO_STREAM, "check", (1, 2, 3, MI)),
            ("repack off", dict(TWO_STREAM, repack=0), "check", (MI,)),
            ("lists off", dict(TWO_STREAM, compact=0), "check", (MI,)),
            ("lock-step", LOCKSTEP, "check", (1, 2, 3, MI))]
    if D <= PACK_MAX:
        runs += [("iter x2", dict(ITER, iter_streams=2), "iter", (MI,)),
                 ("iter x1", dict(ITER, iter_streams=1), "iter", (MI,)),
                 ("resident", {}, "resident", (1, 2, 3, MI))]
    return runs


@functools.lru_cache(maxsize=None)
def case_of(D, variant):
    """The 512 frames of (D, variant), drawn as _case of the repack file draws them, and a cache
    of the oracle's decodes per max_iterations; computed once, shared, never modified."""
    from qamr import codes

    V = v_of(D)
    vid, cid = codes.regular_code(V, 3, D, seed=100 + D)
    orc = O.OracleCode(vid, cid)
    assert orc.vnum == V and orc.cnum == 3 * V // D
    rng = np.random.default_rng(1000 + D)
    word = rng.integers(0, 2, (LD, V)).astype(np.uint8)
    synd = np.stack([orc.eval_syndrome(w) for w in word])
    sig = rng.uniform(*sigma_of(D), LD)[:, None]
    llr = 2 / sig ** 2 * ((1 - 2.0 * word) + sig * rng.standard_normal((LD, V)))
    if variant == "special":
        cw = np.r_[0:4, LD // 2:LD // 2 + 4]
        llr[cw] = 2 / sig[cw] ** 2 * (1 - 2.0 * word[cw])   # exact codewords: (1, 0) in both ranges
        for f in (8, 300):
            llr[f, :5] = [np.inf, -np.inf, -0.0, 0.0, np.nan]  # clears the batch's finite flag
    else:
        assert variant == "clean" and np.isfinite(llr).all()
    llr.setflags(write=False)
    synd.setflags(write=False)
    return dict(vid=vid, cid=cid, orc=orc, llr=llr, synd=synd, ref={})


def oracle_of(case, mi):
    if mi not in case["ref"]:
        ref = case["orc"].decode_batch(case["llr"], case["synd"], mi)
        for a in ref:
            a.setflags(write=False)
        case["ref"][mi] = ref
    return case["ref"][mi]


def assert_inputs(D, case):
    """Conditions on the inputs, from the graph and the oracle alone (before any GPU output):
    those of the repack file's _assert_inputs (each range's running count reaches 80 % of its
    width, >= 5 distinct stop iterations, both ranges are predicted to repack and end narrower
    than 256) and, for a packed degree, a predicted final width of 64 in at least one range, so
    check_narrow<D> must run."""
    V = v_of(D)
    name = f"matrix{D}"
    with mock.patch.dict(R.CODES, {name: (V, [(D, 3 * V // D)])}):
        reps, widths = _assert_inputs(name, case, LD)
    if D <= PACK_MAX:
        assert min(widths) == 64, widths
    return reps, widths


def launches(D):
    from qamr import _lib

    return {k: _lib.profile_query(f"{k}_d{D}")[1] for k in ("resident", "iter", "check", "check1")}


def assert_path(D, path, mi, knobs, n):
    """The launches that ran, by their profile names.  The frame-parallel schedules name their
    first check sweep check1_dD and the sweeps of iterations 2.. check_dD."""
    if path == "resident":
        assert n["resident"] == 1 and n["iter"] == 0 and n["check"] == 0 and n["check1"] == 0, n
    elif path == "iter":
        assert n["iter"] == (mi + 1) * knobs["iter_streams"] and n["resident"] == 0, n
        assert n["check"] == 0 and n["check1"] == 0, n
    else:
        assert path == "check"
        assert n["check1"] > 0 and n["iter"] == 0 and n["resident"] == 0, n
        assert n["check"] > 0 or mi == 1, n   # max_iterations = 1: the first sweep is the only one


def decode_and_compare(dec, L, S, B, mi, ref, tag):
    """One decode into a final_fi filled with PAD: all B frames equal the oracle's, the padding
    columns [B, ld) keep the caller's value."""
    import torch

    s2, i2, f2 = ref
    fin = torch.full(tuple(L.shape), PAD, dtype=torch.float64, device="cuda")
    _, succ, its = dec.decode_device(L, S, B, mi, final_fi=fin)
    torch.cuda.synchronize()
    assert np.array_equal(succ.cpu().numpy(), s2[:B]), tag
    assert np.array_equal(its.cpu().numpy(), i2[:B]), tag
    assert_bit_exact(fin[:, :B].cpu().numpy().T, f2[:B])
    assert bool((fin[:, B:] == PAD).all()), tag


def to_device(case, B, ld):
    import torch

    V, C = case["orc"].vnum, case["orc"].cnum
    L = torch.zeros((V, ld), dtype=torch.float64, device="cuda")
    L[:, :B] = torch.from_numpy(case["llr"][:B].T.copy()).cuda()
    S = torch.zeros((C, ld), dtype=torch.uint8, device="cuda")
    S[:, :B] = torch.from_numpy(case["synd"][:B].T.copy()).cuda()
    return L, S


@pytest.mark.parametrize("variant", ["clean", "special"])
@pytest.mark.parametrize("D", DEGREES)
def test_degree_matrix_vs_oracle(gpu, D, variant):
    """``clean``: all LAPPRs finite (the finite flag set: the one-instruction clamp).  ``special``:
    frames 0..3 and 256..259 are codewords (stop at iteration 0), frames 8 and 300 carry inf, -inf,
    -0.0, 0.0, NaN (flag clear: the NaN-preserving clamp).  The two-stream run's repack stats equal
    the prediction from the oracle's counts at every max_iterations; with the repack or the lists
    off they are "never"."""
    import qamr
    from qamr import _lib

    case = case_of(D, variant)
    assert_inputs(D, case)
    for k, v in DEFAULTS.items():
        assert _lib.tune_get(k) == v, f"default {k}={v} changed: update this test"
    dec = qamr.Decoder(case["vid"], case["cid"])
    assert dec.max_check_degree == D
    L, S = to_device(case, LD, LD)
    try:
        for label, knobs, path, mis in runs_of(D):
            for k, v in DEFAULTS.items():
                _lib.tune_set(k, knobs.get(k, v))
            for mi in mis:
                tag = (D, variant, label, mi)
                ref = oracle_of(case, mi)
                _lib.profile_enable(True)
                _lib.profile_reset()
                decode_and_compare(dec, L, S, LD, mi, ref, tag)
                n = launches(D)
                _lib.profile_enable(False)
                print(tag, n)
                assert_path(D, path, mi, {**DEFAULTS, **knobs}, n)
                if label == "two-stream":
                    stats, want = dec.repack_stats(LD, mi), _predict(ref[0], ref[1], LD, mi)
                    print(tag, "repack stats", stats, "predicted", want)
                    assert stats == want, (tag, stats, want)
                elif label in ("repack off", "lists off"):
                    assert dec.repack_stats(LD, mi) == NEVER, tag
    finally:
        _lib.profile_enable(False)
        for k, v in DEFAULTS.items():
            _lib.tune_set(k, v)
