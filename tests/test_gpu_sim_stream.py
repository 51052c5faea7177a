"""The simulations on numpy's stream (stream="numpy") against the reference's own results
(tests/golden/sim_stream.npz, tests/golden/make_golden_sim_stream.py): after np.random.seed(s) the
returned tuple is the reference's, float for float, and numpy's global stream is left where the
reference leaves it."""
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden

import oracle as O

pytestmark = pytest.mark.gpu

G = golden("sim_stream.npz")
CASES = list(range(int(G["n_cases"])))


def case(c):
    k = f"c{c}_"
    return {n: G[k + n][()] for n in ("code", "bps", "mode", "snr", "seed", "maxiter", "loops", "ferr_min", "tuple",
                                      "pos", "has_gauss", "gauss", "key_sha256", "frames")}


def load_code(name):
    from qamr import codes

    if name == "reg1008":
        return codes.regular_code(1008)
    return codes.load_edge_csv(os.path.join(GOLDEN, "hamming_7-4.csv"))


def simulator(r, **kw):
    import qamr
    from qamr.sim import Simulator

    vid, cid = load_code(str(r["code"]))
    dec = qamr.Decoder(vid, cid)
    return Simulator(dec, int(r["bps"]), str(r["mode"]), int(r["maxiter"]), batch=64, **kw), (vid, cid)


@pytest.mark.parametrize("c", CASES)
def test_reference_tuple_and_state(gpu, c):
    r = case(c)
    sim, _ = simulator(r, stream="numpy")
    np.random.seed(int(r["seed"]))
    got = sim.run_snr(float(r["snr"]), int(r["loops"]), int(r["ferr_min"]))
    ref = tuple(float(v) for v in r["tuple"])
    assert got == ref, (got, ref, int(r["frames"]))
    st = np.random.get_state()
    assert st[2] == int(r["pos"]) and st[3] == int(r["has_gauss"])
    assert np.float64(st[4]).view(np.int64) == np.float64(r["gauss"]).view(np.int64)
    digest = np.frombuffer(hashlib.sha256(np.ascontiguousarray(st[1], "<u4").tobytes()).digest(), np.uint8)
    assert np.array_equal(digest, r["key_sha256"]), "key"


def test_hook_frames_are_the_host_replay(gpu):
    """Every frame the hook sees (case 0: an early stop inside the first batch of 64) has the word and
    the syndrome of the host's replay of reconciliation.pyx:129-139 on numpy's stream: the batch holds
    the frames the sequential loop would have drawn, in its order."""
    import torch

    r = case(0)
    assert str(r["mode"]) == "softening"
    sim, (vid, cid) = simulator(r, stream="numpy")
    seen = []

    def hook(bidx, lappr, synd, word, B):
        torch.cuda.synchronize()
        seen.append((word[:, :B].cpu().numpy().T.copy(), synd[:, :B].cpu().numpy().T.copy()))

    np.random.seed(int(r["seed"]))
    got = sim.run_snr(float(r["snr"]), int(r["loops"]), int(r["ferr_min"]), hook=hook)
    assert got == tuple(float(v) for v in r["tuple"])
    W = np.concatenate([w for w, _ in seen])
    Sy = np.concatenate([s for _, s in seen])
    assert W.shape[0] >= int(r["frames"])
    Es = sim.pa.variance
    N0 = Es * (10 ** (-float(r["snr"]) / 10)) / 2
    onm = O.OracleNoiseMapper(int(r["bps"]), 2.0, N0, sim.cfg)
    orc = O.OracleCode(vid, cid)
    sigma = np.sqrt(N0)
    p = np.asarray(sim.pa.probabilities, np.float64)
    np.random.seed(int(r["seed"]))
    for f in range(W.shape[0]):
        x = np.random.choice(p.size, size=sim.S, p=p)
        y = onm.constellation[x] + sigma * np.random.randn(sim.S)
        word = onm.symbols_to_bits(onm.hard_decide_index(y))
        assert np.array_equal(W[f], word), f
        assert np.array_equal(Sy[f], np.asarray(orc.eval_syndrome(word), np.uint8)), f


def test_default_stream_is_torch(gpu):
    """stream="torch" is the default and draws what it drew before the keyword existed: the default
    and the explicit form return the same tuple for a seed, and neither touches numpy's stream."""
    r = case(0)
    np.random.seed(5)
    before = np.random.get_state()
    a, _ = simulator(r)
    b, _ = simulator(r, stream="torch")
    ta = a.run_snr(float(r["snr"]), 100, 7, seed=4)
    tb = b.run_snr(float(r["snr"]), 100, 7, seed=4)
    assert ta == tb
    after = np.random.get_state()
    assert after[2] == before[2] and np.array_equal(after[1], before[1])
