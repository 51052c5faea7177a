"""The column repack of the two-stream schedule on small codes with check degrees 11..16.

The repack tests of tests/test_gpu_timed_schedule.py all run the N=64800 DVB-S2-profile code
(check degrees 7 and one 6); the tests of other degrees run B = 70 (ld = 128), which never takes
``run_split2`` (it needs ld % 512 == 0).  Here V ~ 768 codes of variable degree 3 run at B <= 512
(ld = 512, two ranges of 256 columns) with knob ``split_min_blocks = 0``, so every decode takes
``run_split2`` with the device-decided repack (k_repack_rows), its transition sweeps (the first
variable and check sweep after a repack read the messages at the frames' old columns of the old
column set) and the narrow sweeps, on

* one unpacked class: ``reg11``, ``reg12``, ``reg16`` (degree > kPackMaxDeg = 10: the unpacked
  strict update, no narrow check sweep);
* ``side12``: ~90 % of the edges in degree-6 checks, ~10 % in degree-12 checks, which therefore
  run as the side class on the variable stream;
* ``half7_13``: half the edges in degree 7 (packed, narrow sweeps), half in degree 13, both in
  the main check sweep;
* ``mix12_16_5``: 45 % / 45 % / 10 % of the edges in degrees 12 / 16 / 5;
* the control ``reg7`` (knob ``resident = 0``): the packed path at the same shape.

Every frame of every run is compared with the oracle (oracle/qamr_oracle.c): success flag,
iteration count and final LAPPRs bit for bit.  The inputs are conditioned on the CPU: from the
oracle's (success, iterations) alone each range's running-frame count drops to at most 80 % of
its 256 columns before the last decision point, and the repacks the device must then decide
(``_predict``: the rule of decode_repack.hip repack_go applied to the oracle's counts) are compared
with ``Decoder.repack_stats``.
"""
import functools

import numpy as np
import pytest

from conftest import assert_bit_exact

import oracle as O

pytestmark = pytest.mark.gpu

LD = 512
H = LD // 2   # columns per range of the two-stream schedule
MI = 30

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

# knob sets of the runs at max_iterations = 30 (values not named: the defaults below)
DEFAULTS = dict(split=3, compact=1, repack=1, repack_pct=80, repack_grid=128, side=1, nt=1, check_tail=4,
                split_min_blocks=1024, resident=1)
RUNS = [
    dict(split_min_blocks=0),
    dict(split_min_blocks=0, repack=0),
    dict(split_min_blocks=0, repack_pct=50, repack_grid=7),
    dict(split_min_blocks=0, side=0),
    dict(split_min_blocks=0, compact=0),
    dict(split_min_blocks=0, nt=0, check_tail=0),
    dict(split=1),   # lock-step (run_flat; the one-launch-per-iteration schedule for reg7)
]
NEVER = ((0, 0), (H, H))


def _graph(name):
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
def _case(name, variant):
    """The 512 frames of (code, variant) and a cache of the oracle's decodes per max_iterations;
    computed once, shared by every test that uses the case, never modified."""
    vid, cid = _graph(name)
    orc = O.OracleCode(vid, cid)
    V = orc.vnum
    rng = np.random.default_rng(1000 + SEEDS[name])
    word = rng.integers(0, 2, (LD, V)).astype(np.uint8)
    synd = np.stack([orc.eval_syndrome(w) for w in word])
    sig = rng.uniform(*SIGMA.get(name, (0.35, 0.6)), LD)[:, None]
    llr = 2 / sig ** 2 * ((1 - 2.0 * word) + sig * rng.standard_normal((LD, V)))
    if variant == "special":
        cw = np.r_[0:4, H:H + 4]
        llr[cw] = 2 / sig[cw] ** 2 * (1 - 2.0 * word[cw])   # exact codewords: (1, 0) in both ranges
        for f in (8, 300):
            llr[f, :5] = [np.inf, -np.inf, -0.0, 0.0, np.nan]  # clears the batch's finite flag
    else:
        assert variant == "clean" and np.isfinite(llr).all()
    llr.setflags(write=False)
    synd.setflags(write=False)
    return dict(vid=vid, cid=cid, orc=orc, llr=llr, synd=synd, ref={})


def _oracle(case, mi):
    if mi not in case["ref"]:
        s, i, f = case["orc"].decode_batch(case["llr"], case["synd"], mi)
        for a in (s, i, f):
            a.setflags(write=False)
        case["ref"][mi] = (s, i, f)
    return case["ref"][mi]


def _running(succ, its, B, t):
    """Frames of each range still running after the status update of iteration t."""
    run = ~((succ[:B] != 0) & (its[:B] <= t))
    return int(run[:H].sum()), int(run[H:].sum())


def _predict(succ, its, B, mi, pct=80):
    """((repacks 0, repacks 1), (width 0, width 1)) the device must end with: the decision point
    before a range's variable sweep t < mi reads the count its status launch of iteration t - 1
    wrote, and repacks to max(64, count rounded up to 64) when the count is at most pct % of the
    width and that is narrower (decode_repack.hip repack_go)."""
    reps, ws = [], []
    for k in range(2):
        w, rep = H, 0
        for t in range(1, mi):
            cnt = _running(succ, its, B, t - 1)[k]
            if w > 64 and cnt > 0 and cnt * 100 <= w * pct:
                wn = max(64, -(-cnt // 64) * 64)
                if wn < w:
                    w, rep = wn, rep + 1
        reps.append(rep)
        ws.append(w)
    return tuple(reps), tuple(ws)


def _assert_inputs(name, case, B):
    """Conditions on the inputs, from the graph and the oracle alone (before any GPU output)."""
    V, classes = CODES[name]
    deg = np.bincount(case["cid"])
    assert set(np.unique(deg)) == {d for d, _ in classes} and deg.max() <= 16, np.unique(deg)
    for d, n in classes:
        assert int((deg == d).sum()) == n
    assert np.array_equal(np.bincount(case["vid"]), np.full(V, 3))
    succ, its, _ = _oracle(case, MI)
    counts = np.array([_running(succ, its, B, t) for t in range(MI - 1)])
    assert (counts.min(axis=0) <= 0.8 * H).all(), counts.min(axis=0)   # both ranges reach the threshold
    iters_ok = np.unique(its[:B][succ[:B] != 0])
    assert 0 < succ[:B].sum() and iters_ok.size >= 5, iters_ok        # frames stop at many iterations
    reps, widths = _predict(succ, its, B, MI)
    assert min(reps) >= 1 and max(widths) < H, (reps, widths)          # so both ranges must repack
    return reps, widths


def _decode_runs(name, variant, B):
    import torch
    import qamr
    from qamr import _lib

    case = _case(name, variant)
    want = _assert_inputs(name, case, B)
    for k, v in DEFAULTS.items():
        assert _lib.tune_get(k) == v, f"default {k}={v} changed: update this test"
    dec = qamr.Decoder(case["vid"], case["cid"])
    V, C = dec.vnum, dec.cnum
    L = torch.zeros((V, LD), dtype=torch.float64, device="cuda")
    L[:, :B] = torch.from_numpy(case["llr"][:B].T.copy()).cuda()
    S = torch.zeros((C, LD), dtype=torch.uint8, device="cuda")
    S[:, :B] = torch.from_numpy(case["synd"][:B].T.copy()).cuda()
    base = dict(resident=0) if name == "reg7" else {}
    try:
        for mi in (1, 2, 3, MI):
            s2, i2, f2 = _oracle(case, mi)
            for r, knobs in enumerate(RUNS if mi == MI else (RUNS[0], RUNS[6])):
                for k, v in DEFAULTS.items():
                    _lib.tune_set(k, {**base, **knobs}.get(k, v))
                fin = torch.full((V, LD), 7.0, dtype=torch.float64, device="cuda")
                _, succ, its = dec.decode_device(L, S, B, mi, final_fi=fin)
                torch.cuda.synchronize()
                stats = dec.repack_stats(LD, mi)
                tag = (name, variant, B, mi, knobs)
                print(tag, "repack stats", stats)
                assert np.array_equal(succ.cpu().numpy(), s2[:B]), tag
                assert np.array_equal(its.cpu().numpy(), i2[:B]), tag
                assert_bit_exact(fin[:, :B].cpu().numpy().T, f2[:B])
                assert bool((fin[:, B:] == 7.0).all()), tag   # padding columns untouched
                if mi != MI:
                    continue
                if r == 0:
                    print(tag, "predicted", want)
                    (rep0, rep1), (w0, w1) = stats
                    assert rep0 >= 1 and rep1 >= 1, stats        # each range repacked
                    assert w0 < H and w1 < H, stats              # and ended narrower
                    last = _running(s2, i2, B, mi - 2)           # count at the last decision point
                    if min(last) <= 64:   # the narrow sweeps ran (beside the unpacked classes)
                        assert min(w0, w1) <= 64, (stats, last)
                    assert stats == want, (stats, want)
                elif r in (1, 4, 6):
                    assert stats == NEVER, (tag, stats)          # repack off / no lists / lock-step
    finally:
        for k, v in DEFAULTS.items():
            _lib.tune_set(k, v)


@pytest.mark.parametrize("variant", ["clean", "special"])
@pytest.mark.parametrize("name", list(CODES))
def test_repack_small_codes_vs_oracle(gpu, name, variant):
    """B = 512, max_iterations 1, 2, 3 (default knobs with split_min_blocks = 0, and lock-step)
    and 30 (the seven knob sets of RUNS): all 512 frames equal the oracle's in every run; at 30
    with the default knobs both ranges repacked, ended narrower than 256 columns and exactly as
    the oracle's counts predict; with the repack or the lists off, and in lock-step, never.
    ``clean``: all LAPPRs finite (the finite flag set: packed classes run the one-instruction
    clamp).  ``special``: frames 0..3 and 256..259 are codewords (stop at iteration 0), frames 8
    and 300 carry inf, -inf, -0.0, 0.0, NaN (flag clear: the NaN-preserving clamp)."""
    _decode_runs(name, variant, LD)


@pytest.mark.parametrize("B", [450, 257])
@pytest.mark.parametrize("name", ["reg12", "side12"])
def test_repack_small_codes_ragged_batch(gpu, name, B):
    """The first B frames of the clean case in ld = 512: range 1 starts with 194 live columns of
    256 (below the threshold before any frame stops) or holds a single frame; the same runs and
    assertions, and the padding columns [B, ld) of the output keep the caller's values (the
    decode's first variable sweep used to copy the input's padding columns into them)."""
    _decode_runs(name, "clean", B)


def test_repack_small_code_graph_replay(gpu):
    """reg12, clean, max_iterations = 30, captured into a HIP graph on a side stream and
    replayed (as test_repack_decode_is_asynchronous_and_capturable does for the DVB-S2 code):
    the replay equals the oracle on all frames and the device repacked inside the graph."""
    import torch
    import qamr
    from qamr import _lib

    case = _case("reg12", "clean")
    want = _assert_inputs("reg12", case, LD)
    s2, i2, f2 = _oracle(case, MI)
    dec = qamr.Decoder(case["vid"], case["cid"])
    L = torch.from_numpy(case["llr"].T.copy()).cuda()
    S = torch.from_numpy(case["synd"].T.copy()).cuda()
    saved = _lib.tune_get("split_min_blocks")
    try:
        _lib.tune_set("split_min_blocks", 0)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            dec.decode_device(L, S, LD, MI)  # warm-up: allocates this stream's workspace
        torch.cuda.synchronize()
        fin = torch.full_like(L, np.nan)
        succ = torch.zeros(LD, dtype=torch.uint8, device="cuda")
        its = torch.zeros(LD, dtype=torch.int32, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            dec.decode_device(L, S, LD, MI, fin, succ, its)
        g.replay()
        torch.cuda.synchronize()
        stats = dec.repack_stats(LD, MI, stream=s)
    finally:
        _lib.tune_set("split_min_blocks", saved)
    assert np.array_equal(succ.cpu().numpy(), s2) and np.array_equal(its.cpu().numpy(), i2)
    assert_bit_exact(fin.cpu().numpy().T, f2)
    assert min(stats[0]) >= 1 and stats == want, (stats, want)
