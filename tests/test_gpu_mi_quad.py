"""The quad-integrated mutual-information evaluators on the GPU against tests/golden/mi_quad.npz (written by
tests/golden/make_golden_mi_quad.py: scipy.integrate.quad over the restated integrands of
mutual_information.pyx:43-119 and :175-199, every NoiseMapper value from the compiled reference).  Every
comparison is bit for bit (conftest.assert_bit_exact: infinities compare as bits, NaN matches NaN)."""
import warnings

import numpy as np
import pytest

from conftest import assert_bit_exact, golden

from debug_rerun import rerun_on_debug_build
from mapper_fixture import ORDER21, ORDER30, mapper, quad_expected

pytestmark = pytest.mark.gpu

CASES = list(range(1, 11))


@pytest.fixture(scope="module")
def fx():
    g = golden("mi_quad.npz")
    assert int(g["n_cases"]) == 10
    return g


_NM = {}


def make_nm(g, c):
    """One NoiseMapper per case for the whole module (its grid is built once)."""
    return mapper(g, f"c{c}_", cache=_NM)[1]


def check_integrands(g, cases):
    from qamr.mutual_information import (P_xhat, mutual_information_base_scheme_arg, mutual_information_base_scheme_arg_array,
                                         mutual_information_X_Y_int_arg, mutual_information_X_Y_int_arg_array)

    for c in cases:
        k = f"c{c}_"
        nm = make_nm(g, c)
        pX = P_xhat(nm)
        assert_bit_exact(pX, g[k + "p_Xhat"])
        assert_bit_exact(mutual_information_base_scheme_arg_array(g[k + "base_x"], nm, pX), g[k + "base_f"])
        assert_bit_exact(mutual_information_X_Y_int_arg_array(g[k + "xy_x"], nm), g[k + "xy_f"])
        # the scalar forms, and an array that is no multiple of the wave
        assert_bit_exact([mutual_information_base_scheme_arg(float(g[k + "base_x"][3]), nm, pX)], [g[k + "base_f"][3]])
        assert_bit_exact([mutual_information_X_Y_int_arg(float(g[k + "xy_x"][-1]), nm)], [g[k + "xy_f"][-1]])
        assert mutual_information_X_Y_int_arg_array(np.empty(0), nm).size == 0


@pytest.mark.parametrize("c", CASES)
def test_integrands_vs_reference(gpu, fx, c):
    """Both integrands at every stored abscissa (the first 64 quad visited, the range ends, +-1e3 sigma), NaN
    and +-inf included."""
    check_integrands(fx, [c])
    k = f"c{c}_"
    if c in (5, 8):   # an overflowed mixture (an infinite integrand value) is among these cases' stored points
        assert np.isinf(fx[k + "xy_f"]).sum() == 2


def test_rule_nodes_are_the_abscissae_quad_visited(gpu, fx):
    """One work item of k_mi_quad with its debug pointer: the lanes' abscissae and values, put in QUADPACK's
    evaluation order, are the abscissae quad visited and the integrand there -- round 1 on the whole range, and a
    pair of halves as in round 2; where quad stopped after the first rule the rule's result is the integral."""
    from qamr.mutual_information import P_xhat, quad_rule

    assert sorted(ORDER21) == list(range(21)) and sorted(ORDER30) == list(range(30))
    for c in (1, 3, 5, 7):
        k = f"c{c}_"
        nm = make_nm(fx, c)
        pX = P_xhat(nm)
        sums, nodes = quad_rule("base", nm, 0.0, 1.0, pX)
        assert sums.shape == (1, 4) and nodes.shape == (1, 21, 2)
        assert_bit_exact(nodes[0, ORDER21, 0], fx[k + "base_x"][:21])
        assert_bit_exact(nodes[0, ORDER21, 1], fx[k + "base_f"][:21])
        if int(fx[k + "base_neval"]) == 21:
            assert_bit_exact([sums[0, 0]], [fx[k + "base_I"]])
        sums, nodes = quad_rule("X_Y", nm, 0.0, 1.0)
        assert sums.shape == (1, 4) and nodes.shape == (1, 30, 2)
        assert_bit_exact(nodes[0, ORDER30, 0], fx[k + "xy_x"][:30])
        assert_bit_exact(nodes[0, ORDER30, 1], fx[k + "xy_f"][:30])
        if int(fx[k + "xy_last"]) == 1:
            assert_bit_exact([sums[0, 0]], [fx[k + "xy_I"]])
    assert int(fx["c5_base_neval"]) == 21   # the branch above is taken
    # round 2 bisects [0, 1]: both halves in one work item
    nm = make_nm(fx, 1)
    sums, nodes = quad_rule("base", nm, [0.0, 0.5], [0.5, 1.0], P_xhat(nm))
    assert sums.shape == (2, 4) and nodes.shape == (2, 21, 2)
    assert_bit_exact(nodes[0, ORDER21, 0], fx["c1_base_x"][21:42])
    assert_bit_exact(nodes[1, ORDER21, 0], fx["c1_base_x"][42:63])
    assert_bit_exact(nodes[0, ORDER21, 1], fx["c1_base_f"][21:42])
    assert_bit_exact(nodes[1, ORDER21, 1], fx["c1_base_f"][42:63])
    sums, nodes = quad_rule("X_Y", nm, [0.0, 0.5], [0.5, 1.0])
    assert_bit_exact(nodes[0, ORDER30, 0], fx["c1_xy_x"][30:60])
    assert_bit_exact(nodes[0, ORDER30, 1], fx["c1_xy_f"][30:60])
    assert_bit_exact(nodes[1, ORDER30[:4], 0], fx["c1_xy_x"][60:64])


@pytest.mark.parametrize("c", CASES)
def test_integrals_vs_reference(gpu, fx, c):
    """Both integrals of every case through the batch entry, P = 1: I and abserr bit-equal, neval equal,
    (ier != 0) == warned; the limit=5 case ends with ier == 1."""
    from qamr.mutual_information import P_xhat, mutual_information_quad_batch, quad_batch_stats

    nm = make_nm(fx, c)
    limit = int(fx[f"c{c}_limit"])
    for name, kind, pXs in (("base", "base", [P_xhat(nm)]), ("xy", "X_Y", None)):
        I, abserr, neval, ier = mutual_information_quad_batch(kind, [nm], pXs, limit=limit)
        eI, eabs, eneval, ewarned = quad_expected(fx, f"c{c}_", name)
        assert_bit_exact([I[0], abserr[0]], [eI, eabs])
        assert int(neval[0]) == eneval and (int(ier[0]) != 0) == ewarned, (name, neval, ier)
        st = quad_batch_stats()
        assert st["rounds"] == st["launches"] == int(fx[f"c{c}_{name}_last"]) and st["work_items"] == st["rounds"]
        if c == 10:
            assert int(ier[0]) == 1
    if c == 1:
        I, abserr, neval, ier = mutual_information_quad_batch("base", [nm], [P_xhat(nm)])
        assert int(ier[0]) == 2 and int(neval[0]) == 1071


@pytest.mark.parametrize("bps", [1, 2, 4])
def test_batch_equals_single_calls(gpu, fx, bps):
    """One call over all cases of one bps returns what the single calls return, at P = 1, 3 and 70 (cases
    repeated): 70 work items are more than one workgroup holds, and problems that end after the first rule sit
    beside problems that run 26 rounds, so the work list is compacted again and again."""
    from qamr.mutual_information import P_xhat, mutual_information_quad_batch, quad_batch_stats

    cases = [c for c in CASES if int(fx[f"c{c}_bps"]) == bps and int(fx[f"c{c}_limit"]) == 50]
    assert len(cases) >= 2
    for P in (1, 3, 70):
        pick = [cases[q % len(cases)] for q in range(P)]
        nms = [make_nm(fx, c) for c in pick]
        for name, kind, pXs in (("base", "base", [P_xhat(nm) for nm in nms]), ("xy", "X_Y", None)):
            I, abserr, neval, ier = mutual_information_quad_batch(kind, nms, pXs)
            exp = [quad_expected(fx, f"c{c}_", name) for c in pick]
            assert_bit_exact(I, [e[0] for e in exp])
            assert_bit_exact(abserr, [e[1] for e in exp])
            assert neval.tolist() == [e[2] for e in exp]
            assert [bool(v) for v in ier] == [e[3] for e in exp]
            st = quad_batch_stats()
            assert st["rounds"] == max(int(fx[f"c{c}_{name}_last"]) for c in pick)
            assert st["work_items"] == sum(int(fx[f"c{c}_{name}_last"]) for c in pick)


def test_sign_configs_override_equals_a_mapper_of_that_configuration(gpu, fx):
    """A uniform 4-PAM 4 dB mapper built with the alternating configuration, overridden per problem: the all-zero
    override gives case 9's integral (that case's own configuration), the others what a mapper constructed with
    that configuration gives."""
    import qamr
    from qamr.mutual_information import P_xhat, mutual_information_quad_batch

    pa = qamr.PAMAlphabet(2, 2.0)
    nv = float(fx["c9_noise_var"])
    alt = qamr.NoiseMapper(pa, nv, np.array([0, 1, 0, 1], np.uint8))
    pX = P_xhat(alt)
    assert_bit_exact(pX, fx["c9_p_Xhat"])   # p_Xhat does not depend on the configuration
    cfgs = np.array([[0, 0, 0, 0], [0, 1, 0, 1], [1, 1, 0, 0]], np.uint8)
    I, abserr, neval, ier = mutual_information_quad_batch("base", [alt] * 3, [pX] * 3, cfgs)
    assert_bit_exact([I[0], abserr[0]], [fx["c9_base_I"], fx["c9_base_abserr"]])
    assert int(neval[0]) == int(fx["c9_base_neval"])
    for q in (1, 2):
        own = qamr.NoiseMapper(pa, nv, cfgs[q])
        Io, ao, no, io = mutual_information_quad_batch("base", [own], [pX])
        assert_bit_exact([I[q], abserr[q]], [Io[0], ao[0]])
        assert int(neval[q]) == int(no[0]) and int(ier[q]) == int(io[0])
    assert I[0] != I[1] and I[1] != I[2]   # the configuration matters
    # the X;Y integrand does not read it
    Ix, ax, nx, ix = mutual_information_quad_batch("X_Y", [alt] * 2, sign_configs=cfgs[:2])
    assert_bit_exact(Ix, [fx["c9_xy_I"]] * 2)


def test_scalar_facade_warns_where_the_fixture_says(gpu, fx):
    from qamr.mutual_information import P_xhat, mutual_information_base_scheme, mutual_information_X_Y

    try:
        from scipy.integrate import IntegrationWarning as category
    except Exception:
        category = UserWarning
    for c in (1, 2, 4, 5, 10):
        nm = make_nm(fx, c)
        limit = int(fx[f"c{c}_limit"])
        for name, call in (("base", lambda: mutual_information_base_scheme(nm, P_xhat(nm), limit=limit)),
                           ("xy", lambda: mutual_information_X_Y(nm, limit=limit))):
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                I = call()
            assert isinstance(I, float)
            assert_bit_exact([I], [fx[f"c{c}_{name}_I"]])
            got = [x for x in w if issubclass(x.category, category)]
            assert bool(got) == bool(fx[f"c{c}_{name}_warned"]), (c, name, [str(x.message) for x in w])


def test_compare_signs_and_base_scheme_sweeps(gpu, fx, tmp_path):
    """compare_signs at bps 2, one SNR point: column 0 equals mutual_information_base_scheme of configuration 0,
    every column a single call with that configuration; base_scheme's CSV row equals the single calls."""
    import qamr
    from qamr import sim_mutual_information_base_scheme as sb
    from qamr import sim_mutual_information_compare_signs as sc
    from qamr.mutual_information import (P_xhat, mutual_information_base_scheme, mutual_information_X_Xhat,
                                         mutual_information_X_Y)

    out = str(tmp_path / "signs.csv")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rows = sc.main(["--snr", "4", "4", "--nsnr", "1", "--bps", "2", "--out", out])
        assert len(rows) == 1 and len(rows[0]) == 11 and rows[0][0] == 4.0
        pa = qamr.PAMAlphabet(2, 2)
        N0 = pa.variance * (10 ** (-4.0 / 10)) / 2
        cfgs = sc.config_list(2)
        nm0 = qamr.NoiseMapper(pa, N0, cfgs[0])
        pX = P_xhat(nm0)
        assert_bit_exact([rows[0][1]], [mutual_information_base_scheme(nm0, pX)])
        assert_bit_exact([rows[0][1]], [fx["c9_base_I"]])   # case 9: 4-PAM 4 dB, all-zero configuration
        for q in (1, 9):
            assert_bit_exact([rows[0][1 + q]], [mutual_information_base_scheme(qamr.NoiseMapper(pa, N0, cfgs[q]), pX)])
        lines = open(out).read().splitlines()
        assert lines[0] == "," + ",".join(sc.column_list(2)) and len(lines) == 2 and lines[1].startswith("0,4.0,")
        assert [float(v) for v in lines[1].split(",")[1:]] == list(rows[0])
        # the montecarlo branch: seeded, every column within the estimator's spread of the integral
        mc = sc.main(["--snr", "4", "4", "--nsnr", "1", "--bps", "2", "--montecarlo", "--nmontecarlo", "256", "--nloops",
                      "8", "--seed", "5", "--out", str(tmp_path / "mc.csv")])
        assert len(mc[0]) == 11 and all(abs(m - r) < 0.15 for m, r in zip(mc[0][1:], rows[0][1:]))
        out = str(tmp_path / "base.csv")
        rows = sb.main(["--snr", "4", "15", "--nsnr", "2", "--bps", "2", "--out", out])
        for r, e in zip(rows, (4.0, 15.0)):
            nm = qamr.NoiseMapper(pa, pa.variance * (10 ** (-e / 10)) / 2)
            pX = P_xhat(nm)
            I = (mutual_information_base_scheme(nm, pX), mutual_information_X_Xhat(nm, pX), mutual_information_X_Y(nm))
            assert_bit_exact([r[2], r[4], r[6]], I)
            assert_bit_exact([r[1], r[3], r[5]], [e - 10 * np.log10(v) for v in I])
    lines = open(out).read().splitlines()
    assert lines[0] == "," + ",".join(sb.COLUMNS) and len(lines) == 3


# ----------------------------------------------------------------- debug build
PARITY = ([f"test_integrands_vs_reference[{c}]" for c in CASES] + [f"test_integrals_vs_reference[{c}]" for c in (1, 3, 5, 7, 10)] +
          ["test_batch_equals_single_calls[2]", "test_sign_configs_override_equals_a_mapper_of_that_configuration",
           "test_rule_nodes_are_the_abscissae_quad_visited"])


def test_debug_build_quad_index_checks(gpu):
    """This file's parity tests in a child process on libqamr_debug.so: the node, LDS-slot, problem-id and grid
    index checks of k_mi_quad / k_mi_integrand (mi.hip, grid_interp.hpp QR_DCHECK) never fail -- conftest's autouse
    fixture fails any test after which one did."""
    rerun_on_debug_build([f"tests/test_gpu_mi_quad.py::{t}" for t in PARITY], len(PARITY), timeout=600)
