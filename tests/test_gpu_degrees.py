"""Any check degree, as the reference allows (decoder.pyx:131-141 sizes its F/B buffer
per check): degrees above the templated range (2..16) run the runtime-degree kernel
with the forward values parked in an HBM scratch (decoder.hip k_check_generic).  Bit
for bit against the oracle for degrees 17, 33, 65, 100 (and 255 on a small code), in
every schedule, plus the node-level surface process_check_node on such checks.

What runs here: single checks of degree 17, 33, 65, 100 among low-degree ones (V = 300, B = 70, ld = 128)
with knob split 1 and 3; a code of runtime-degree classes only, one check of degree 255 (B = ld = 64);
process_check_node on finite messages; the workspace's closed form (no kernel).  The matrix of the
runtime-degree kernel -- whole classes of degrees 17 .. 255 at ld = 512, every knob that shapes its
launch, max_iterations 0 .. 30, special values, ragged batches, few frames, graph capture, the node
surface on special values, and the comparison with the compiled reference's own records -- is
tests/test_gpu_high_degrees.py."""
import numpy as np
import pytest

from conftest import assert_bit_exact

import oracle as O
from decode_fixture import himix_code, knobs, scattered_code
from workspace_fixture import decode_ws_map, graph_counts, map_bytes

pytestmark = pytest.mark.gpu


def _code(rng, degrees, V):
    """One check per listed degree (+ degree-3 filler checks), every variable used."""
    degrees = list(degrees)
    E0 = int(sum(degrees))
    extra = max(0, V - E0)
    degrees += [3] * ((extra + 2) // 3)
    return scattered_code(rng, degrees, V)


def _frames(rng, orc, B, V, sig=(0.5, 0.9)):
    word = rng.integers(0, 2, (B, V)).astype(np.uint8)
    synd = np.stack([orc.eval_syndrome(w) for w in word])
    s = rng.uniform(*sig, B)[:, None]
    llr = 2 / s ** 2 * ((1 - 2.0 * word) + s * rng.standard_normal((B, V)))
    return llr, synd


def _high_degree_code(rng, V=300):
    return _code(rng, [17, 33, 65, 100, 17, 5, 7], V)


@pytest.mark.parametrize("split", [1, 3])
def test_high_degree_checks_vs_oracle(gpu, split):
    import qamr
    rng = np.random.default_rng(17)
    V = 300
    vid, cid = _high_degree_code(rng, V)
    dec = qamr.Decoder(vid, cid)
    orc = O.OracleCode(vid, cid)
    llr, synd = _frames(rng, orc, 70, V)
    with knobs(split=split):
        s1, i1, f1 = dec.decode_batch(llr, synd, 30)
    s2, i2, f2 = orc.decode_batch(llr, synd, 30)
    assert np.array_equal(s1, s2) and np.array_equal(i1, i2)
    assert_bit_exact(f1, f2)


def _workspace_closed_form(vid, cid, ld, max_it, repack):
    """The decode workspace's size: the sum of the layout restated array by array in
    tests/workspace_fixture.py decode_ws_map (decoder.hip ws_layout), which the workspace-contract
    tests fill by; tests/test_workspace_cpu.py holds that sum to the closed form in the code's
    counts.  -> (bytes, F-scratch rows, second message buffer present)."""
    m = decode_ws_map(vid, cid, ld, max_it, repack)
    names = [e[0] for e in m]
    return map_bytes(m), graph_counts(vid, cid)[3], "c2v2" in names


def test_workspace_bytes_closed_form(gpu):
    """Decoder.workspace_bytes equals the closed form: base part (+ second message buffer for a
    one-launch-per-iteration code, + F scratch of the runtime-degree classes) and, with knob
    repack on and ld % 512 == 0, the repack work set.  No kernel runs."""
    import qamr
    from qamr import codes

    high = _high_degree_code(np.random.default_rng(17))
    mixed = himix_code()   # classes of degrees 7, 12, 17, 30, 64: 65 * 15 + 13 * 28 + 62 F rows
    cases = [(codes.regular_code(1008), 64), (codes.regular_code(1008), 512), (high, 128), (mixed, 512), (mixed, 64)]
    for repack in (1, 0):
        with knobs(repack=repack):
            for (vid, cid), ld in cases:
                dec = qamr.Decoder(vid, cid)
                for max_it in (0, 30):
                    want, fb_rows, iter_code = _workspace_closed_form(vid, cid, ld, max_it, repack)
                    runtime = vid is high[0] or vid is mixed[0]
                    assert (fb_rows > 0) == runtime and iter_code == (not runtime)
                    assert fb_rows == 65 * 15 + 13 * 28 + 62 or vid is not mixed[0]
                    assert dec.workspace_bytes(ld, max_it) == want, (vid.size, ld, max_it, repack)


def test_degree_255_and_all_large(gpu):
    """A code made only of large checks (no templated class at all) and one of degree 255."""
    import qamr
    rng = np.random.default_rng(5)
    V = 400
    vid, cid = _code(rng, [255, 40, 40, 40, 24], V)
    keep = cid < 5  # drop the degree-3 filler: only runtime-degree classes
    vid, cid = vid[keep], cid[keep]
    used = np.unique(vid)
    remap = np.full(V, -1, np.int64)
    remap[used] = np.arange(used.size)
    vid = remap[vid]
    dec = qamr.Decoder(vid, cid)
    orc = O.OracleCode(vid, cid)
    llr, synd = _frames(rng, orc, 64, int(vid.max()) + 1, sig=(0.3, 0.6))
    s1, i1, f1 = dec.decode_batch(llr, synd, 12)
    s2, i2, f2 = orc.decode_batch(llr, synd, 12)
    assert np.array_equal(s1, s2) and np.array_equal(i1, i2)
    assert_bit_exact(f1, f2)


def test_process_check_node_high_degree(gpu):
    import qamr
    rng = np.random.default_rng(3)
    V = 250
    vid, cid = _code(rng, [100, 65, 33, 17], V)
    dec = qamr.Decoder(vid, cid)
    orc = O.OracleCode(vid, cid)
    E = vid.size
    C = int(cid.max()) + 1
    synd = rng.integers(0, 2, C).astype(np.uint8)
    for c in range(4):
        v2c = rng.standard_normal(E) * rng.choice([0.5, 3.0, 20.0], E)
        c1 = rng.standard_normal(E)
        c2 = c1.copy()
        dec.process_check_node(c, synd, c1, v2c)
        orc.process_check_node(c, synd, c2, v2c)
        assert_bit_exact(c1, c2)
