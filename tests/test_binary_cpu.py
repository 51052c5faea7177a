"""CPU tests of the binary-channel code evaluation (qamr.sim_binary, qamr.sim_decode / sim_direct /
sim_bsc, csrc/binary_channel.hip's entry points): the CLIs' arguments and CSV headers, the keyword
check, the C-ABI's symbols and argument checks, the fixture, the oracle decoder on the fixture, and
the generalised stopping rule against plain sequential loops, single process and gloo world 2."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from binary_fixture import (FRAMES, K, MAXITER, N, biawgn_script_loop, bsc_script_loop, cases, fixture,
                            result_tuple, sequential)
from conftest import GOLDEN, assert_bit_exact

import oracle as O

NEW_SYMBOLS = ("qr_biawgn_llr_device", "qr_bsc_llr_device", "qr_count_errors_neg_device")


# ------------------------------------------------------------------------ CLIs
def test_parser_defaults():
    from qamr import sim_bsc, sim_decode, sim_direct

    for mod in (sim_decode, sim_direct):
        a = mod.build_parser().parse_args(["code.csv"])
        assert (a.edgefile, a.out, a.maxiter, a.minerr, a.simloops, a.snr, a.nsnr, a.alpha, a.hard, a.first_row) == \
            ("code.csv", "out.csv", 30, 20, 30, [0, 5], 11, 1.0, False, True)
        assert (a.batch, a.seed) == (4096, 0)
        a = mod.build_parser().parse_args(["c.csv", "--hard", "--first_row", "--snr", "-1", "2.5", "--alpha", "0.7"])
        assert a.hard is True and a.first_row is True and a.snr == [-1.0, 2.5] and a.alpha == 0.7
    a = sim_bsc.build_parser().parse_args(["code.csv"])
    assert (a.edgefile, a.out, a.maxiter, a.minerr, a.simloops, a.rber, a.rpoints, a.first_row, a.batch, a.seed) == \
        ("code.csv", "out.csv", 30, 20, 30, [0.01, 0.04], 31, True, 4096, 0)


@pytest.mark.parametrize("argv", [[], ["c.csv", "--maxiter", "x"], ["c.csv", "--snr", "1"], ["c.csv", "--nsnr", "1.5"],
                                  ["c.csv", "--rber", "0.1", "0.2"], ["c.csv", "--nope"]])
def test_decode_parsers_reject(argv):
    from qamr import sim_decode, sim_direct

    for mod in (sim_decode, sim_direct):
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(argv)


@pytest.mark.parametrize("argv", [[], ["c.csv", "--rber", "0.1"], ["c.csv", "--rpoints", "many"], ["c.csv", "--hard"],
                                  ["c.csv", "--snr", "0", "5"], ["c.csv", "--alpha", "1.0"]])
def test_bsc_parser_rejects(argv):
    from qamr import sim_bsc

    with pytest.raises(SystemExit):
        sim_bsc.build_parser().parse_args(argv)


def test_cli_columns_channels_and_csv(monkeypatch, tmp_path):
    """Each main hands its own column name, channel and points to the shared sweep, and the CSV
    writer lays rows out as pandas' to_csv does."""
    from qamr import sim_bsc, sim_decode, sim_direct

    seen = []

    def fake(args, channel, points, column):
        seen.append((channel, [float(p) for p in points], column))
        return []

    monkeypatch.setattr(sim_decode, "sweep", fake)
    monkeypatch.setattr(sim_bsc, "sweep", fake)
    sim_decode.main(["c.csv", "--snr", "1", "2", "--nsnr", "3"])
    sim_direct.main(["c.csv", "--snr", "1", "2", "--nsnr", "2", "--hard"])
    sim_bsc.main(["c.csv", "--rber", "0.02", "0.04", "--rpoints", "3"])
    assert seen[0] == ("biawgn", [1.0, 1.5, 2.0], "EbN0dB")
    assert seen[1] == ("biawgn_hard", [1.0, 2.0], "EsN0dB")
    assert seen[2][0] == "bsc" and seen[2][2] == "f" and np.allclose(seen[2][1], [0.02, 0.03, 0.04])
    for column in ("EbN0dB", "EsN0dB", "f"):
        p = tmp_path / f"{column}.csv"
        sim_decode.write_csv(str(p), column, [(0.5, 0.25, 0.125, 3.5), (1.0, 0.0, 0.0, 2.0)])
        assert p.read_text().splitlines() == [f",{column},ber,fer,iters", "0,0.5,0.25,0.125,3.5", "1,1.0,0.0,0.0,2.0"]


def test_channels_and_keyword_rejected_before_any_device():
    from qamr import sim_binary

    assert sim_binary.CHANNELS == ("biawgn", "biawgn_hard", "bsc")
    for bad in ("awgn", "hard", "BSC", "", None):
        with pytest.raises(ValueError):
            sim_binary.BinaryChannelSimulator(None, bad)      # no decoder is ever looked at


def test_stop_rule_factories():
    from qamr import sim_binary
    from qamr.sim import StopRule

    assert sim_binary.biawgn_stop_rule(30, 20) == StopRule(0, 20, 2)      # wc > 1.5
    assert sim_binary.biawgn_stop_rule(16, 100) == StopRule(0, 100, 1)    # wc > 0.8
    assert sim_binary.biawgn_stop_rule(40, 5) == StopRule(0, 5, 3)        # wc > 2.0
    assert sim_binary.bsc_stop_rule(30, 20) == StopRule(0, 21, 20)        # it > 20: index >= 20
    assert sim_binary.bsc_stop_rule(5000, 20) == StopRule(0, 21, 50)
    assert sim_binary.bsc_stop_rule(16, 20, 2) == StopRule(0, 21, 2)


def test_host_coefficients_match_the_fixture():
    from qamr import sim_binary

    for c in cases():
        if c.channel == "bsc":
            assert sim_binary.bsc_coefficient(c.point) == c.coef
        else:
            coef, vsqrt = sim_binary.biawgn_coefficients(c.point, c.alpha, c.channel == "biawgn_hard")
            assert (coef, vsqrt) == (c.coef, c.vsqrt)
    g = fixture()
    for p, x in enumerate(g["edge_pts"]):
        for h in (0, 1):
            assert sim_binary.biawgn_coefficients(float(x), 1.0, bool(h)) == (g["edge_coef"][p, h], g["edge_vsqrt"][p])
    assert np.isinf(sim_binary.biawgn_coefficients(30.0, 1.0, True)[0])


# ----------------------------------------------------------------------- C-ABI
def test_new_symbols_and_argument_checks():
    import qamr
    from qamr import _lib

    L = qamr.load()
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(L, s), s
    a = np.zeros(64 * 8, np.float64)
    p = _lib.ptr(a)       # never dereferenced: every call below is refused before a launch
    EV = _lib.QR_EVALUE
    assert L.qr_biawgn_llr_device(0, 1.0, 1.0, 16, 64, 8, None, p, p, None) == EV
    assert L.qr_biawgn_llr_device(1, 1.0, 1.0, 16, 64, 8, p, None, p, None) == EV
    assert L.qr_biawgn_llr_device(0, 1.0, 1.0, 16, 64, 8, p, p, None, None) == EV
    assert L.qr_bsc_llr_device(1.0, 0.1, 16, 64, 8, None, p, p, None, None) == EV
    assert L.qr_bsc_llr_device(1.0, 0.1, 16, 64, 8, p, None, p, None, None) == EV
    assert L.qr_bsc_llr_device(1.0, 0.1, 16, 64, 8, p, p, None, p, None) == EV
    for k in range(6):
        args = [p] * 6
        args[k] = None
        assert L.qr_count_errors_neg_device(16, 64, 8, *args, None) == EV
    for B, ld, V in ((65, 64, 8), (0, 64, 8), (16, 96, 8), (16, 64, 0), (16, 64, -3)):
        assert L.qr_biawgn_llr_device(0, 1.0, 1.0, B, ld, V, p, p, p, None) == EV
        assert L.qr_bsc_llr_device(1.0, 0.1, B, ld, V, p, p, p, None, None) == EV
    for B, ld, Kk in ((65, 64, 8), (0, 64, 8), (16, 96, 8), (16, 64, -1)):
        assert L.qr_count_errors_neg_device(B, ld, Kk, p, p, p, p, p, p, None) == EV


# --------------------------------------------------------------------- fixture
def test_fixture_is_well_formed():
    g = fixture()
    cs = cases()
    assert [(c.channel, c.point, c.alpha) for c in cs] == [
        ("biawgn", -1.5, 1.0), ("biawgn", -0.5, 1.0), ("biawgn", -1.5, 0.7), ("biawgn_hard", 0.0, 1.0),
        ("biawgn_hard", 1.0, 1.0), ("bsc", 0.07, 1.0), ("bsc", 0.04, 1.0)]
    for c in cs:
        assert c.word.shape == (FRAMES, N) and c.noise.shape == (FRAMES, N) and c.synd.shape == (FRAMES, N - K)
        assert c.llr.shape == c.final.shape == (4, N) and c.llr.dtype == np.float64
        assert c.success.shape == c.iters.shape == c.err_k.shape == c.err_n.shape == (FRAMES,)
        assert set(np.unique(c.word)) <= {0, 1} and np.all(c.err_k <= c.err_n)
        if c.channel == "bsc":
            assert np.all((c.noise >= 0) & (c.noise < 1))
        # the stored errors are the `final < 0` rule against the word, over K and over N bits
        bits = (c.final < 0).astype(np.uint8) ^ c.word[:4]
        assert np.array_equal(bits[:, :K].sum(1), c.err_k[:4]) and np.array_equal(bits.sum(1), c.err_n[:4])
        # numpy's form of the formula from the stored inputs is the stored llr, bit for bit
        assert_bit_exact(c.numpy_llr()[:4], c.llr)
    # the harder point of each channel has at least 3 failed and 3 successful frames
    for c in (cs[0], cs[3], cs[5]):
        assert 3 <= int(c.success.sum()) <= FRAMES - 3, (c.channel, int(c.success.sum()))
    # at least one stored stop is decided by the index bound and one by the error count
    by_index = by_count = 0
    for c in cs:
        run = np.cumsum(c.errors)
        for a, cnt in zip(c.loop_args, c.loop_counts):
            if cnt[4] == a[0]:
                continue
            need = a[1] + 1 if c.channel == "bsc" else a[1]
            first = int(np.argmax(run >= need))
            assert first <= cnt[4] - 1
            by_index += first < cnt[4] - 1
            by_count += first == cnt[4] - 1
    assert by_index >= 1 and by_count >= 1, (by_index, by_count)
    # edge planes: LLR0 is finite at the first point and inf at 30 dB, where a zero sum gives NaN
    assert np.isfinite(g["edge_coef"][0]).all() and np.isinf(g["edge_coef"][1, 1]) and g["edge_pts"][1] == 30.0
    z = g["edge_z"]
    for v in (0.0, 1e-300, -1e-300, 1.0, -1.0, 1e300, -1e300, np.inf, -np.inf):
        assert np.count_nonzero(z == v) == 2, v
    assert np.count_nonzero(np.isnan(z)) == 2
    assert np.isnan(g["edge_llr"][1, 1][~np.isnan(z)]).any()       # inf * 0
    assert (g["edge_llr"][0, 1][~np.isnan(z)] == 0).any()          # sign(0) = 0 at the finite point
    r = float(g["bsc_edge_r"])
    assert set(g["bsc_edge_u"]) == {0.0, r, np.nextafter(r, 0), np.nextafter(r, 1), 1 - 2.0 ** -53}
    assert np.array_equal(g["bsc_edge_rx"], g["bsc_edge_w"] ^ (g["bsc_edge_u"] < r))
    assert os.path.getsize(os.path.join(GOLDEN, "binary_channel.npz")) <= os.path.getsize(
        os.path.join(GOLDEN, "interp.npz"))


@pytest.fixture(scope="module")
def oracle_code():
    from qamr import codes

    return O.OracleCode(*codes.regular_code(N))


@pytest.mark.parametrize("c", range(7))
def test_oracle_decoder_reproduces_the_fixture(oracle_code, c):
    case = cases()[c]
    for f in range(FRAMES):
        assert np.array_equal(case.synd[f], oracle_code.eval_syndrome(case.word[f]))
    s, i, fin = oracle_code.decode_batch(case.llr, case.synd[:4], MAXITER)
    assert np.array_equal(s, case.success[:4]) and np.array_equal(i, case.iters[:4])
    assert_bit_exact(fin, case.final)
    # the other frames' llr is not stored: numpy's form of it (checked above on the first 4)
    s, i, fin = oracle_code.decode_batch(case.numpy_llr(), case.synd, MAXITER)
    assert np.array_equal(s, case.success) and np.array_equal(i, case.iters)
    bits = (fin < 0).astype(np.uint8) ^ case.word
    assert np.array_equal(bits[:, :K].sum(1), case.err_k) and np.array_equal(bits.sum(1), case.err_n)


# ------------------------------------------------------------------- stop rule
def _case_rule(case, args):
    from qamr import sim_binary

    if case.channel == "bsc":
        return sim_binary.bsc_stop_rule(int(args[0]), int(args[1]), None if args[2] < 0 else int(args[2]))
    return sim_binary.biawgn_stop_rule(int(args[0]), int(args[1]))


@pytest.mark.parametrize("c", range(7))
def test_stop_rule_gives_the_stored_tuples(c):
    case = cases()[c]
    per = [(int(case.errors[f]), int(case.success[f]), int(case.iters[f])) for f in range(FRAMES)]
    for args, cnt, tup in zip(case.loop_args, case.loop_counts, case.loop_tuple):
        got = sequential(_case_rule(case, args), per, int(args[0]))
        assert got == cnt.tolist(), (args, got, cnt)
        assert result_tuple(case.point, got, case.count_bits)[1:] == tuple(tup)
        # and the script's loop, written out with its own inequalities, agrees
        if case.channel == "bsc":
            assert bsc_script_loop(per, int(args[0]), int(args[1]), None if args[2] < 0 else int(args[2])) == got
        else:
            assert biawgn_script_loop(per, int(args[0]), int(args[1])) == got


def _frame_synth(g):
    """Synthetic per-frame results of global frame g: (bit errors, success, iterations)."""
    ferr = (g * 2654435761 % 97 + 1) if (g * 7919) % 5 == 0 else 0
    return ferr, int(g % 3 != 0), 1 + g % 29


# (kind, batch per rank, loops, minerr, bsc index bound)
RULE_CASES = [
    ("biawgn", 16, 1000, 900, None),     # the error count decides, at the last frame of the third batch
    ("biawgn", 10, 1000, 944, None),     # the count is exactly 944 after frame 95: >= stops there, inside a batch
    ("bsc", 10, 1000, 944, None),        # strict >: only at the next frame in error
    ("biawgn", 16, 1000, 1, None),       # the index bound decides (wc > 50), inside the second batch
    ("biawgn", 5, 37, 10 ** 9, None),    # never stops: ragged last batch
    ("bsc", 7, 3000, 0, None),           # the bound niters // 100 = 30 decides
    ("bsc", 4, 16, 20, 2),               # the fixture's bound of 2
    ("biawgn", 4, 60, 60, None),
]


def _rule(kind, loops, minerr, bound):
    from qamr import sim_binary

    return sim_binary.bsc_stop_rule(loops, minerr, bound) if kind == "bsc" else sim_binary.biawgn_stop_rule(loops, minerr)


def _rule_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank))
    from qamr import dist
    from qamr.sim import run_frames, shard_counters

    dist.init("gloo")
    res = []
    for kind, batch, loops, minerr, bound in RULE_CASES:
        def fn(bidx, start, B, batch=batch):
            g0 = bidx * batch * world + start
            rows = [_frame_synth(g) for g in range(g0, g0 + B)]
            ferr = torch.tensor([r[0] for r in rows], dtype=torch.int32)
            succ = torch.tensor([r[1] for r in rows], dtype=torch.uint8)
            its = torch.tensor([r[2] for r in rows], dtype=torch.int32)
            return ferr, succ, its, shard_counters(ferr, succ, its, B)
        res.append(run_frames(fn, batch, loops, minerr, rule=_rule(kind, loops, minerr, bound)))
    dist.barrier()
    dist.finalize()
    q.put((rank, res))


def test_run_frames_world2_new_rules():
    """run_frames with the two new rules at world size 2 over gloo with stub frames: every rank
    returns the sequential loop's counters, the stop falling inside a batch."""
    world = 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_rule_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = dict(q.get(timeout=300) for _ in ps)
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    inside = 0
    for c, (kind, batch, loops, minerr, bound) in enumerate(RULE_CASES):
        per = [_frame_synth(w) for w in range(loops)]
        exp = bsc_script_loop(per, loops, minerr, bound) if kind == "bsc" else biawgn_script_loop(per, loops, minerr)
        assert exp == sequential(_rule(kind, loops, minerr, bound), per, loops)
        for r in range(world):
            assert res[r][c] == exp, (c, r, res[r][c], exp)
        inside += exp[4] < loops and exp[4] % (batch * world) != 0
    assert inside >= 5


def test_run_frames_without_a_rule_is_unchanged():
    """No rule given: reconciliation.pyx:159-161 on the frame-error count, as before."""
    from qamr.sim import StopRule, run_frames, shard_counters

    def fn(bidx, start, B):
        rows = [_frame_synth(g) for g in range(bidx * 16 + start, bidx * 16 + start + B)]
        ferr = torch.tensor([r[0] for r in rows], dtype=torch.int32)
        succ = torch.tensor([r[1] for r in rows], dtype=torch.uint8)
        its = torch.tensor([r[2] for r in rows], dtype=torch.int32)
        return ferr, succ, its, shard_counters(ferr, succ, its, B)

    for loops, fmin in ((1000, 30), (100, 10 ** 6), (20, 0), (500, 12)):
        be = fe = su = it = 0
        for w in range(loops):
            e, s, i = _frame_synth(w)
            be, fe, su, it = be + e, fe + (e > 0), su + s, it + (i if s else 0)
            if fe >= fmin and w > loops / 20:
                break
        got = run_frames(fn, 16, loops, fmin)
        assert got == [be, fe, su, it, w + 1]
        assert got == run_frames(fn, 16, loops, fmin, rule=StopRule(1, fmin, int(np.floor(loops / 20)) + 1))
