"""The host round trips of the C ABI (upload, launch, download through the handle's scratch): every
host entry, through the facade, with n = 0, 1, 1000 and then 3 on one handle -- the scratch grows and
is then reused while larger than needed -- equals the same call on a fresh handle bit for bit; and
through ctypes a null array or a negative size is a ValueError, never a dereference.  One 4-PAM
NoiseMapper and one Decoder of the Hamming (7,4) graph."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, assert_bit_exact

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 1000, 3)
V, NC, E = 7, 3, 12


def mapper():
    import qamr

    return qamr.NoiseMapper(qamr.PAMAlphabet(2, 2.0), 0.5, np.array([0, 1, 0, 1], np.uint8))


def decoder():
    import qamr
    from qamr import codes

    return qamr.Decoder(*codes.load_edge_csv(os.path.join(GOLDEN, "hamming_7-4.csv")))


def inputs(n):
    rng = np.random.default_rng(n)
    return rng.uniform(0.01, 0.99, n), rng.integers(0, 4, n).astype(np.int64), rng.normal(0.0, 3.0, n)


def mapper_calls():
    from qamr import mutual_information as mi

    pX = np.full(4, 0.25)
    return {
        "F_Y": lambda nm, u, j, y: nm.F_Y(y),
        "demap_noise_search": lambda nm, u, j, y: nm.demap_noise_search(u, j),
        "demap_lappr_array": lambda nm, u, j, y: nm.demap_lappr_array(u, j),
        "demap_noise": lambda nm, u, j, y: nm.demap_noise(u, j),
        "demap_lappr_simplified_array": lambda nm, u, j, y: nm.demap_lappr_simplified_array(u, j),
        "base_scheme_arg_array": lambda nm, u, j, y: mi.mutual_information_base_scheme_arg_array(u, nm, pX),
        "X_Y_int_arg_array": lambda nm, u, j, y: mi.mutual_information_X_Y_int_arg_array(y, nm),
    }


@pytest.mark.parametrize("name", list(mapper_calls()))
def test_mapper_entry_on_a_grown_scratch(gpu, name):
    call, nm = mapper_calls()[name], mapper()
    for n in SIZES:
        got = call(nm, *inputs(n))
        assert got.size == (n * 2 if "lappr" in name else n)
        if n:
            assert_bit_exact(got, call(mapper(), *inputs(n)))


def test_montecarlo_block_on_a_grown_scratch(gpu):
    """qr_mi_montecarlo_host refuses an empty block (the reference divides by N): 1, 1000, 3."""
    import qamr
    from qamr import mutual_information as mi

    pa, pX = qamr.PAMAlphabet(2, 2.0), np.full(4, 0.25)

    def block(nm, n):
        np.random.seed(n)
        terms = np.empty(3 * n)
        return np.array(mi.montecarlo_information(pa, nm, pX, n, _terms=terms)), terms

    nm = mapper()
    with pytest.raises(ValueError, match="N must be positive"):
        mi.montecarlo_information(pa, nm, pX, 0)
    for n in SIZES[1:]:
        for got, ref in zip(block(nm, n), block(mapper(), n)):
            assert_bit_exact(got, ref)


def node_calls(dec, rng):
    """Every host entry of the decoder's node surface on one random state: their outputs, in order."""
    lappr, synd = rng.normal(0, 4, V), rng.integers(0, 2, NC).astype(np.uint8)
    word = rng.integers(0, 2, V).astype(np.uint8)
    c2v, v2c, upd = rng.normal(0, 2, E), rng.normal(0, 2, E), np.zeros(V)
    out = [np.array([dec.check_lappr(lappr, synd), dec.check_word(word, synd)]),
           np.array([dec.check_synd_node(k, word, synd) for k in range(NC)])]
    for v in range(V):
        dec.process_var_node(v, lappr, c2v, v2c, upd)
    for k in range(NC):
        dec.process_check_node(k, synd, c2v, v2c)
    return out + [v2c, upd, c2v]


def test_decoder_entries_on_a_grown_scratch(gpu):
    """The node entries share the code's scratch with decode_batch: B = 0 is refused, B = 1, 1000 and
    3 frames grow it, and the node entries run before, between and after."""
    dec = decoder()
    with pytest.raises(ValueError, match="B must be positive"):
        dec.decode_batch(np.zeros((0, V)), np.zeros((0, NC), np.uint8), 5)
    for B in SIZES[1:]:
        for got, ref in zip(node_calls(dec, np.random.default_rng(B)), node_calls(decoder(), np.random.default_rng(B))):
            assert_bit_exact(got, ref)
        rng = np.random.default_rng(100 + B)
        lappr, synd = rng.normal(0, 4, (B, V)), rng.integers(0, 2, (B, NC)).astype(np.uint8)
        for got, ref in zip(dec.decode_batch(lappr, synd, 5), decoder().decode_batch(lappr, synd, 5)):
            assert_bit_exact(got.astype(np.float64), ref.astype(np.float64))


def host_entries(nm, dec):
    """(entry, arguments around the size, index of the size or None, indices of the arrays)."""
    h, d, one = nm.handle, dec.handle, C.c_double(0.0)
    buf = C.cast(C.pointer(one), C.c_void_p)
    return [
        ("qr_demap_host", [h, 1, buf, buf, buf], 1, (2, 3, 4)),
        ("qr_g_inv_search_host", [h, 1, buf, buf, 1e-9, buf], 1, (2, 3, 5)),
        ("qr_F_Y_host", [h, 1, buf, buf], 1, (2, 3)),
        ("qr_g_inv_host", [h, 1, buf, buf, buf], 1, (2, 3, 4)),
        ("qr_demap_simplified_host", [h, 1, buf, buf, buf], 1, (2, 3, 4)),
        ("qr_mi_integrand_host", [h, 1, 1, buf, buf], 2, (3, 4)),
        ("qr_mi_montecarlo_host", [h, 1, buf, buf, None, buf, None], 1, (2, 3, 5)),
        ("qr_check_lappr_host", [d, buf, buf, None, None], None, (1, 2)),
        ("qr_check_word_host", [d, buf, buf, None, None], None, (1, 2)),
        ("qr_process_var_nodes_host", [d, buf, 1, buf, buf, buf, buf], 2, (1, 3, 4, 5, 6)),
        ("qr_process_check_nodes_host", [d, buf, 1, buf, buf, buf], 2, (1, 3, 4, 5)),
    ]


def test_null_array_and_negative_size_are_value_errors(gpu):
    from qamr import _lib

    nm, dec = mapper(), decoder()
    nm.grid_info()                                             # the interpolated entries need the grid
    from qamr import mutual_information as mi
    mi._prepare(nm, np.full(4, 0.25))                          # and the estimators their tables
    L = _lib.load()
    for name, args, size_at, arrays in host_entries(nm, dec):
        for k in arrays:                                       # n = 1, one array null: never read
            bad = list(args)
            bad[k] = None
            with pytest.raises(ValueError, match="null pointer argument"):
                _lib.check(getattr(L, name)(*bad), name)
        if size_at is not None:
            bad = list(args)
            bad[size_at] = -1
            with pytest.raises(ValueError, match="negative size|N must be positive"):
                _lib.check(getattr(L, name)(*bad), name)
