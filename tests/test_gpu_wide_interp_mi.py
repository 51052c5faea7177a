"""The interpolation grid, the table-interpolated g_inv, the formulation-1 demapper, the Monte-Carlo estimator
and the quad-integrated evaluators on the GPU at 32- and 64-PAM (and a shaped 8-PAM), against the compiled
reference's own outputs (tests/golden/wide_interp_mi.npz, written by tests/golden/make_golden_wide_interp_mi.py):
shaped alphabets, sign configurations that set mask bits 32..63, grids of 41 201 to 519 862 points (coarse-table
segments of 16, 32, 64 and 128 entries), and the under- and overflow of 64-PAM at 40 dB.  Every comparison is bit
for bit (conftest.assert_bit_exact: infinities compare as bits, NaN matches NaN).  Only the fixture is read."""
import numpy as np
import pytest

from conftest import assert_bit_exact, golden

from debug_rerun import rerun_on_debug_build
from decode_fixture import knobs
from mapper_fixture import (FIXTURE, ORDER21, ORDER30, block_expected, expected_terms, mapper, mc_inputs, quad_expected,
                            run_device, sha, to_dev)

pytestmark = pytest.mark.gpu

CASES = list(range(1, 8))
MC_CASES = [1, 2, 3, 4, 5, 7]
QUAD_CASES = [1, 2, 3, 4, 5]
B, S, LD = 70, 11, 128
STRIDE = 997


@pytest.fixture(scope="module")
def fx():
    g = golden("wide_interp_mi.npz")
    assert int(g["n_cases"]) == 7 and int(g["B"]) == B and int(g["S"]) == S
    return g


_NM = {}


def make_nm(g, k, cfg=FIXTURE):
    """-> (PAMAlphabet, NoiseMapper), one per case for the whole module (its grid is built once); cfg replaces
    the case's sign configuration (a mapper of its own, cached likewise)."""
    return mapper(g, f"w{k}_", cfg, cache=_NM)


# ----------------------------------------------------------------------- grid
@pytest.mark.parametrize("k", CASES)
def test_grid_and_tables_match_reference(gpu, fx, k):
    """n_points and the nondecreasing flag, the digests, both ends and every 997th entry of y_range / F_Y_values as
    the device built them (k_grid_build's fl(fl(i * step) + y_low) against numpy's linspace at i up to 519 861, a
    32- or 64-term erf sum per point), the host properties, F_Y_thresholds / delta_F_Y, P_xhat and the digest of
    fwrd_transition_probability."""
    from qamr.mutual_information import P_xhat, mutual_information_X_Xhat

    pa, nm = make_nm(fx, k)
    key = f"w{k}_"
    n = int(fx[key + "n_points"])
    assert nm.grid_info() == (n, True)
    y, F = nm.grid_tables()
    assert y.size == n and F.size == n
    for got, t in ((y, "y"), (F, "F")):
        assert_bit_exact(got[:64], fx[key + t + "_head"])
        assert_bit_exact(got[-64:], fx[key + t + "_tail"])
        assert_bit_exact(got[::STRIDE], fx[key + t + "_stride"])
        assert sha(got) == str(fx[key + t + "_sha"])
    assert not (np.diff(F) < 0).any()
    assert sha(nm.y_range) == str(fx[key + "y_sha"]) and sha(nm.F_Y_values) == str(fx[key + "F_sha"])
    assert_bit_exact(nm.F_Y_thresholds, fx[key + "Fthr"])
    assert_bit_exact(nm.delta_F_Y, fx[key + "dF"])
    pX = P_xhat(nm)
    assert_bit_exact(pX, fx[key + "p_Xhat"])
    assert sha(nm.fwrd_transition_probability) == str(fx[key + "fwrd_sha"])
    assert_bit_exact([mutual_information_X_Xhat(nm, pX)], [fx[key + "I_X_Xhat"]])
    assert nm.grid_info() == (n, True)   # a second creation with the same parameters changes nothing


# ------------------------------------------------- g_inv and formulation 1, host entries
@pytest.mark.parametrize("fast", [1, 0])
@pytest.mark.parametrize("k", CASES)
def test_g_inv_and_formulation1_vs_reference(gpu, fx, k, fast):
    """demap_noise on 100 seeded n_hat, the edge values and NaN against every i, and
    demap_lappr_simplified_array on 500 seeded (n, j) and the edge values, with both index searches; an
    out-of-range i gives NaN."""
    pa, nm = make_nm(fx, k)
    key = f"w{k}_"
    M, bps = nm.order, nm.bit_per_symbol
    n109, ginv = fx[key + "n109"], fx[key + "ginv"]
    assert ginv.shape == (M, n109.size)
    n508, j508, la = fx[key + "n508"], fx[key + "j508"].astype(np.int64), fx[key + "la"]
    with knobs(interp_fast=fast):
        got = nm.demap_noise(np.tile(n109, M), np.repeat(np.arange(M, dtype=np.int64), n109.size))
        assert_bit_exact(got.reshape(M, n109.size), ginv)
        assert_bit_exact([nm.g_inv(n109[7], M - 1)], [ginv[M - 1, 7]])
        assert np.isnan(nm.demap_noise(np.array([0.5, 0.5]), np.array([-1, M], np.int64))).all()
        assert_bit_exact(nm.demap_lappr_simplified_array(n508, j508), la)
        for s in (3, 501, 506):
            assert_bit_exact(nm.demap_lappr_simplified(n508[s], j508[s]), la[s * bps:(s + 1) * bps])
    if k == 7:   # the case exists to put exp's zeros and log(0) on the path
        assert np.isposinf(la).any() and np.isneginf(la).any()


# ------------------------------------------------------ formulation 1, device block
@pytest.mark.parametrize("k", CASES)
def test_device_block_vs_reference(gpu, fx, k):
    """demap_simplified_device on the [S=6][B=70] block at ld = 128: the decoder's layout, both index searches,
    alpha as one fp64 multiply, untouched padding columns."""
    import torch

    pa, nm = make_nm(fx, k)
    key = f"w{k}_"
    bps, Sq, ld = nm.bit_per_symbol, 6, 128
    exp = block_expected(fx[key + "blk_la"], Sq, B, bps)
    n_fi = to_dev(fx[key + "blk_n"], ld, torch.float64)
    j_fi = to_dev(fx[key + "blk_j"].astype(np.int64), ld, torch.int64)
    for fast in (1, 0):
        with knobs(interp_fast=fast):
            for alpha in (1.0, 0.7):
                out = torch.full((Sq * bps, ld), float("nan"), dtype=torch.float64, device="cuda")
                ret = nm.demap_simplified_device(n_fi, j_fi, B, alpha, out=out)
                torch.cuda.synchronize()
                assert ret.data_ptr() == out.data_ptr()
                got = out.cpu().numpy()
                assert_bit_exact(got[:, :B], exp if alpha == 1.0 else exp * 0.7)
                assert np.isnan(got[:, B:]).all()


# ---------------------------------------------------------------- Monte-Carlo
@pytest.mark.parametrize("k", MC_CASES)
def test_montecarlo_blocks_vs_reference(gpu, fx, k):
    """montecarlo_information_device at B = 70, ld = 128, S = 11 (two tiles, the second with 6 valid lanes): the
    terms, and the totals the compiled montecarlo_information returned; padding columns are not written; the same
    at B = 1, ld = 64; and montecarlo_information under the stored seeds of blocks 0 and 69."""
    from qamr.mutual_information import P_xhat, montecarlo_information

    pa, nm = make_nm(fx, k)
    key = f"w{k}_"
    pX = P_xhat(nm)
    assert_bit_exact(pX, fx[key + "p_Xhat"])
    x, y = mc_inputs(fx, key, LD)
    info, terms = run_device(nm, pX, x, y, B, LD)
    assert_bit_exact(terms[:, :, :B], expected_terms(fx, key))
    assert_bit_exact(info[:, :B], fx[key + "totals"].T)
    assert np.isnan(terms[:, :, B:]).all() and np.isnan(info[:, B:]).all()
    x1, y1 = mc_inputs(fx, key, 64, 1)
    info1, terms1 = run_device(nm, pX, x1, y1, 1, 64)
    assert_bit_exact(terms1[:, :, :1], expected_terms(fx, key, 1))
    assert_bit_exact(info1[:, 0], fx[key + "totals"][0])
    assert np.isnan(terms1[:, :, 1:]).all() and np.isnan(info1[:, 1:]).all()
    for f in (0, 69):
        np.random.seed(9000 + 100 * k + f)
        t = np.full((3, S), np.nan)
        got = montecarlo_information(pa, nm, pX, S, _terms=t)
        assert_bit_exact(got, fx[key + "totals"][f])
        assert_bit_exact(t, fx[key + "terms"][:, f, :])
    if k == 7:   # exp overflows to inf (and underflows to 0) on this case's path
        assert int(fx[key + "n_overflow"]) > 0


def test_montecarlo_64pam_reference_search_and_which_masks(gpu, fx):
    """Case 2 (64-PAM, a configuration with bits on both sides of index 32) with the reference's own index search
    (interp_fast = 0), and each single-bit `which` mask: a disabled quantity is exactly 0.0 / N and its term plane
    is not written, the enabled one is unchanged."""
    from qamr.mutual_information import P_xhat

    k = 2
    pa, nm = make_nm(fx, k)
    key = f"w{k}_"
    pX = P_xhat(nm)
    x, y = mc_inputs(fx, key, LD)
    exp_t, exp_i = expected_terms(fx, key), fx[key + "totals"].T
    with knobs(interp_fast=0):
        info, terms = run_device(nm, pX, x, y, B, LD)
        assert_bit_exact(terms[:, :, :B], exp_t)
        assert_bit_exact(info[:, :B], exp_i)
    for on in range(3):
        which = [int(q == on) for q in range(3)]
        info, terms = run_device(nm, pX, x, y, B, LD, which)
        for q in range(3):
            if which[q]:
                assert_bit_exact(terms[q, :, :B], exp_t[q])
                assert_bit_exact(info[q, :B], exp_i[q])
            else:
                assert np.isnan(terms[q]).all()
                assert_bit_exact(info[q, :B], np.full(B, 0.0 / S))
                assert not np.signbit(info[q, :B]).any()
        assert np.isnan(info[:, B:]).all()


# ----------------------------------------------------------------- quadrature
@pytest.mark.parametrize("k", QUAD_CASES)
def test_integrands_and_rule_nodes_vs_reference(gpu, fx, k):
    """Both integrands at the first 42 abscissae quad visited (the compiled reference's values); one work item of
    k_mi_quad on [0, 1]: the lanes' abscissae and values in QUADPACK's evaluation order are the first 21 / 30
    stored points, and where quad stopped after the first rule the rule's result is the integral."""
    from qamr.mutual_information import (P_xhat, mutual_information_base_scheme_arg, mutual_information_base_scheme_arg_array,
                                         mutual_information_X_Y_int_arg, mutual_information_X_Y_int_arg_array, quad_rule)

    pa, nm = make_nm(fx, k)
    key = f"w{k}_"
    pX = P_xhat(nm)
    assert_bit_exact(pX, fx[key + "p_Xhat"])
    assert_bit_exact(mutual_information_base_scheme_arg_array(fx[key + "base_x"], nm, pX), fx[key + "base_f"])
    assert_bit_exact(mutual_information_X_Y_int_arg_array(fx[key + "xy_x"], nm), fx[key + "xy_f"])
    assert_bit_exact([mutual_information_base_scheme_arg(float(fx[key + "base_x"][3]), nm, pX)], [fx[key + "base_f"][3]])
    assert_bit_exact([mutual_information_X_Y_int_arg(float(fx[key + "xy_x"][-1]), nm)], [fx[key + "xy_f"][-1]])
    sums, nodes = quad_rule("base", nm, 0.0, 1.0, pX)
    assert sums.shape == (1, 4) and nodes.shape == (1, 21, 2)
    assert_bit_exact(nodes[0, ORDER21, 0], fx[key + "base_x"][:21])
    assert_bit_exact(nodes[0, ORDER21, 1], fx[key + "base_f"][:21])
    if int(fx[key + "base_neval"]) == 21:
        assert_bit_exact([sums[0, 0]], [fx[key + "base_I"]])
    sums, nodes = quad_rule("X_Y", nm, 0.0, 1.0)
    assert sums.shape == (1, 4) and nodes.shape == (1, 30, 2)
    assert_bit_exact(nodes[0, ORDER30, 0], fx[key + "xy_x"][:30])
    assert_bit_exact(nodes[0, ORDER30, 1], fx[key + "xy_f"][:30])
    if int(fx[key + "xy_last"]) == 1:
        assert_bit_exact([sums[0, 0]], [fx[key + "xy_I"]])


@pytest.mark.parametrize("k", QUAD_CASES)
def test_integrals_vs_reference(gpu, fx, k):
    """Both integrals through the batch entry, P = 1: I (the reference's own mutual_information_base_scheme /
    mutual_information_X_Y) and abserr bit-equal, neval equal, (ier != 0) == warned, rounds == last."""
    from qamr.mutual_information import P_xhat, mutual_information_quad_batch, quad_batch_stats

    pa, nm = make_nm(fx, k)
    limit = int(fx[f"w{k}_limit"])
    for name, kind, pXs in (("base", "base", [P_xhat(nm)]), ("xy", "X_Y", None)):
        I, abserr, neval, ier = mutual_information_quad_batch(kind, [nm], pXs, limit=limit)
        eI, eabs, eneval, ewarned = quad_expected(fx, f"w{k}_", name)
        assert_bit_exact([I[0], abserr[0]], [eI, eabs])
        assert int(neval[0]) == eneval and (int(ier[0]) != 0) == ewarned, (name, neval, ier)
        st = quad_batch_stats()
        assert st["rounds"] == st["launches"] == int(fx[f"w{k}_{name}_last"]) and st["work_items"] == st["rounds"]


@pytest.mark.parametrize("bps", [3, 5, 6])
def test_batch_of_one_bps_equals_the_single_integrals(gpu, fx, bps):
    """Five problems in one call: the mappers of every case of one bps (repeated in turn), problems of different
    length side by side in the work list."""
    from qamr.mutual_information import P_xhat, mutual_information_quad_batch, quad_batch_stats

    cases = [k for k in QUAD_CASES if int(fx[f"w{k}_bps"]) == bps]
    assert cases and all(int(fx[f"w{k}_limit"]) == 50 for k in cases)
    pick = [cases[q % len(cases)] for q in range(5)]
    nms = [make_nm(fx, k)[1] for k in pick]
    for name, kind, pXs in (("base", "base", [P_xhat(nm) for nm in nms]), ("xy", "X_Y", None)):
        I, abserr, neval, ier = mutual_information_quad_batch(kind, nms, pXs)
        exp = [quad_expected(fx, f"w{k}_", name) for k in pick]
        assert_bit_exact(I, [e[0] for e in exp])
        assert_bit_exact(abserr, [e[1] for e in exp])
        assert neval.tolist() == [e[2] for e in exp]
        assert [bool(v) for v in ier] == [e[3] for e in exp]
        st = quad_batch_stats()
        assert st["rounds"] == max(int(fx[f"w{k}_{name}_last"]) for k in pick)
        assert st["work_items"] == sum(int(fx[f"w{k}_{name}_last"]) for k in pick)


def test_sign_configs_override_at_64pam(gpu, fx):
    """A uniform 64-PAM 28 dB mapper built with the alternating configuration, overridden per problem with case 2's
    random configuration (mask bits on both sides of index 32), gives case 2's stored integral; without the
    override it does not."""
    from qamr.mutual_information import P_xhat, mutual_information_quad_batch

    k = 2
    cfg = fx[f"w{k}_cfg"]
    assert cfg[:32].any() and cfg[32:].any() and not cfg[:32].all() and not cfg[32:].all()
    alt_cfg = (np.arange(64) & 1).astype(np.uint8)
    pa, alt = make_nm(fx, k, alt_cfg)
    pX = P_xhat(alt)
    assert_bit_exact(pX, fx[f"w{k}_p_Xhat"])   # p_Xhat does not depend on the configuration
    I, abserr, neval, ier = mutual_information_quad_batch("base", [alt, alt], [pX, pX], np.stack([cfg, alt_cfg]))
    eI, eabs, eneval, ewarned = quad_expected(fx, "w2_", "base")
    assert_bit_exact([I[0], abserr[0]], [eI, eabs])
    assert int(neval[0]) == eneval and (int(ier[0]) != 0) == ewarned
    assert I[1] != I[0]   # the configuration matters
    Io, ao, no, io = mutual_information_quad_batch("base", [alt], [pX])
    assert_bit_exact([I[1], abserr[1]], [Io[0], ao[0]])
    # a configuration that differs from case 2's in bit 63 alone gives another integral
    other = cfg.copy()
    other[63] ^= 1
    I2, _, _, _ = mutual_information_quad_batch("base", [alt], [pX], other[None, :])
    assert I2[0] != I[0]


def test_base_integral_64pam_with_reference_search(gpu, fx):
    """Case 2's base integral with the reference's own index search (interp_fast = 0)."""
    from qamr.mutual_information import P_xhat, mutual_information_quad_batch

    pa, nm = make_nm(fx, 2)
    with knobs(interp_fast=0):
        I, abserr, neval, ier = mutual_information_quad_batch("base", [nm], [P_xhat(nm)])
    eI, eabs, eneval, ewarned = quad_expected(fx, "w2_", "base")
    assert_bit_exact([I[0], abserr[0]], [eI, eabs])
    assert int(neval[0]) == eneval and (int(ier[0]) != 0) == ewarned


# ----------------------------------------------------------------- debug build
# The grids above 65 536 points (coarse segments of 32 and 64 entries), the shaped 32-PAM alphabet and the
# under- / overflow case: the index checks depend on the shape, not on the values.
DEBUG_CASES = (2, 3, 4, 7)
PARITY = ([f"test_grid_and_tables_match_reference[{k}]" for k in DEBUG_CASES] +
          [f"test_g_inv_and_formulation1_vs_reference[{k}-{f}]" for k in DEBUG_CASES for f in (1, 0)] +
          [f"test_device_block_vs_reference[{k}]" for k in DEBUG_CASES] +
          [f"test_montecarlo_blocks_vs_reference[{k}]" for k in DEBUG_CASES] +
          [f"test_integrands_and_rule_nodes_vs_reference[{k}]" for k in (2, 3, 4)] +
          [f"test_integrals_vs_reference[{k}]" for k in (2, 3, 4)])


def test_debug_build_wide_index_checks(gpu):
    """This file's parity tests for cases 2, 3, 4 and 7 in a child process on libqamr_debug.so: the grid, coarse
    table, symbol, decision, node, LDS-slot and problem-id index checks (grid_interp.hpp, mi.hip QR_DCHECK) never fail --
    conftest's autouse fixture fails any test after which one did."""
    rerun_on_debug_build([f"tests/test_gpu_wide_interp_mi.py::{t}" for t in PARITY], len(PARITY), timeout=600)
