"""CPU test: the demapper's fast root search (Newton + replayed bisection,
qamr_math.hpp::g_inv_search_fast) is bit-identical to the reference search
(noisemapper.pyx:310-345 restated as qamr_math.hpp::g_inv_search), compiled
for the host with hipcc over random targets, orders, SNRs and sign configs."""
import re

import numpy as np

from conftest import golden

from native_check import build, run


def test_fast_search_bit_identical(tmp_path):
    out = run(build(tmp_path, "replay_check.cpp"), "120000", timeout=300)
    assert "mismatches=0" in out
    # the fast path itself must be exercised: Newton certifies ~91 % of these draws (the rest
    # are the edge targets n = 0 / 1, 1e-12-deep tails and -2 dB spreads: brute force)
    m = re.search(r"draws=(\d+) mismatches=\d+ fallbacks=(\d+)", out)
    assert m and int(m.group(2)) < 0.15 * int(m.group(1)), out


def _dump_wide_cases(path):
    """The constructor arguments of every demap_wide.npz case as text for replay_wide_check
    (hexadecimal floats: exact), with the alphabet tables of qamr.PAMAlphabet."""
    from qamr import PAMAlphabet

    g = golden("demap_wide.npz")
    hexes = lambda v: " ".join(float(x).hex() for x in np.asarray(v, np.float64))
    with open(path, "w") as f:
        for c in range(int(g["n_cases"])):
            k = f"c{c}_"
            pa = PAMAlphabet(int(g[k + "bps"]), 2.0, g[k + "probs"])
            f.write(f"case {pa.bit_per_symbol} {float(g[k + 'noise_var']).hex()}\n")
            f.write(f"a {hexes(pa.constellation)}\nthr {hexes(pa.thresholds)}\np {hexes(pa.probabilities)}\n"
                    f"sign {hexes(g[k + 'cfg'])}\n")
    return int(g["n_cases"])


def test_fast_search_bit_identical_wide(tmp_path):
    """replay_wide_check: g_inv_search_fast == g_inv_search on tables from the library's own
    build_demap_host, for every demap_wide.npz case and the grid bps 1..5 x {uniform, shaped} x
    {-12, 3, 25, 50, 70, 80} dB; the fixture cases reach all three regimes of the root search."""
    exe = build(tmp_path, "replay_wide_check.cpp")
    n_cases = _dump_wide_cases(str(tmp_path / "cases.txt"))
    out = run(exe, "1500", str(tmp_path / "cases.txt"), timeout=900)
    rows = [dict(label=m.group(1), **{k: float(v) for k, v in re.findall(r"(\w+)=([-\d.e+]+)", m.group(2))})
            for m in re.finditer(r"^cfg (\S+) (.*)$", out, re.M)]
    assert len(rows) == n_cases + 5 * 2 * 6, out[-4000:]
    assert re.search(r"^total draws=\d+ mismatches=0 ", out, re.M), out[-4000:]
    assert all(r["mismatches"] == 0 for r in rows)
    # the three regimes build_demap_host chooses between, each met by a fixture case (the GPU
    # tests of tests/test_gpu_demap_wide.py run those cases)
    fixture = [r for r in rows if r["label"].startswith("fixture")]
    assert len(fixture) == n_cases
    regimes = {(int(r["quant"]), int(r["ftab"])) for r in fixture}
    assert {(1, 1), (1, 0), (0, 0)} <= regimes, regimes
    assert (0, 1) not in {(int(r["quant"]), int(r["ftab"])) for r in rows}
    # the fast path itself must be exercised: in both table regimes Newton certifies a majority of
    # the plain draws (uniform n_hat; not the edge targets 0 / 1, the 1e-12-deep tails or the
    # adversarial targets on the bisection grid) of EVERY configuration.  Observed: none of the 980
    # plain draws fell back, in any of the 60 grid and 11 fixture configurations with tables; the
    # fallbacks are the edge targets (~1 %) and, from 25 dB upward, the adversarial targets that
    # land where F_Y is flat in double (up to a third of all draws at 50..85 dB).
    for r in rows:
        if r["quant"]:
            assert r["plain"] > 0 and r["plain_fallbacks"] < 0.5 * r["plain"], r


def test_llr_exponent_division_bit_identical(tmp_path):
    """qamr_math.hpp::div_two_s2 (reciprocal + FMA correction) == IEEE x / (2 sigma^2)."""
    assert "mismatches=0" in run(build(tmp_path, "division_check.cpp"), "20000000", timeout=300)
