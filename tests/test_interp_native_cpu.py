"""CPU check of the interpolation grid's arithmetic (csrc/grid_interp.hpp): tests/native/interp_check.cpp
runs the very functions the kernels of demap_interp.hip and mi.hip and qr_demap_grid_create run --
grid_geometry / grid_point, grid_binsearch, grid_interp_fast, grid_g_inv, grid_demap_symbol -- as host code
against the reference's outputs in tests/golden/interp.npz, bit for bit, once plain and once under the
address and undefined-behaviour sanitizers.  No GPU."""
import numpy as np
import pytest

from conftest import assert_bit_exact, golden

from mapper_fixture import alphabet, sha
from native_check import build, run

N_CASES = 11


@pytest.fixture(scope="module")
def fx():
    g = golden("interp.npz")
    assert int(g["n_cases"]) == N_CASES
    return g


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    return build(tmp_path_factory.mktemp("interp_check_" + request.param), "interp_check.cpp",
                 sanitize=request.param == "sanitized")


def dump_case(fx, c, path):
    """The raw input of `interp_check case`: every n300 point x every hypothesis, every n2000 / j2000 symbol."""
    k = f"c{c}_"
    pa = alphabet(fx, k)
    bps, M = pa.bit_per_symbol, pa.order
    assert fx[k + "ginv"].shape == (M, fx["n300"].size) and fx[k + "la"].size == fx["n2000"].size * bps
    parts = [[bps, float(fx[k + "noise_var"]), float(fx[k + "trunc"]), float(fx[k + "nips"]), 2.0],
             pa.constellation, pa.probabilities, pa.thresholds, fx[k + "cfg"],
             [fx["n300"].size], fx["n300"], fx[k + "ginv"],
             [fx["n2000"].size], fx["n2000"], fx[k + "j2000"], fx[k + "la"]]
    np.concatenate([np.asarray(p, np.float64).ravel() for p in parts]).tofile(path)
    return bps, M


@pytest.mark.parametrize("c", range(N_CASES))
def test_grid_g_inv_and_formulation1_vs_reference(fx, exe, tmp_path, c):
    """The grid (n_points, end values, digests of y and F; nondecreasing), g_inv on the 309 n300 points x every
    hypothesis and formulation 1 on the 2008 n2000 / j2000 symbols, each with both index-search bodies, equal
    the reference's bit for bit (NaN matches NaN)."""
    k = f"c{c}_"
    src, out = str(tmp_path / "case.bin"), str(tmp_path / "grid.bin")
    bps, M = dump_case(fx, c, src)
    txt = run(exe, "case", src, out)
    n = int(fx[k + "n_points"])
    grid = np.fromfile(out, np.float64)
    assert grid.size == 2 * n
    y, F = grid[:n], grid[n:]
    assert f"{n} points, nondecreasing 1" in txt and not (np.diff(F) < 0).any()
    assert_bit_exact(y[[0, -1]], fx[k + "y_ends"])
    assert_bit_exact(F[[0, -1]], fx[k + "F_ends"])
    assert sha(y) == str(fx[k + "y_sha"])
    assert sha(F) == str(fx[k + "F_sha"])
    assert f"{2 * M * 309} values, 0 mismatches" in txt.split("g_inv")[1].splitlines()[0]
    assert f"{2 * 2008 * bps} values, 0 mismatches" in txt.split("formulation1")[1].splitlines()[0]


def test_index_search_bodies_agree_on_seeded_tables(exe):
    """Tables of every length 2..70 (ties and decreasing runs included): grid_binsearch returns binsearch_thr's
    index at table values, their neighbours, midpoints, values outside both ends and NaN; on the nondecreasing
    tables body (b) returns body (a)'s result bit for bit at seg_shift 1..4."""
    txt = run(exe, "property", "20240611")
    line = [ln for ln in txt.splitlines() if ln.startswith("property")][0].split()
    tables, idx, bad_idx, val, bad_val = (int(line[i]) for i in (1, 3, 6, 8, 11))
    assert tables == 69 * 6 and idx > 10 * tables and val > 10 * tables
    assert bad_idx == 0 and bad_val == 0
