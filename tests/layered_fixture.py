"""The layered decode schedule restated in Python from its definition (include/qamr.h), the Python
first-fit of its layers, and the cases of tests/test_layered_cpu.py and tests/test_gpu_layered.py;
every case is computed once, shared and never modified.

* ``first_fit``: layer_of[c] = the smallest l >= 0 such that no check c' < c of layer l shares a
  variable with c.  ``graph_of``: per check its edges in ascending edge id and their variables, the
  schedule order (layer_of[c], c), and which checks repeat a variable.
* ``layered_decode``: one frame, from the oracle's node rule (``OracleCode.process_check_node``,
  ``check_lappr``) alone; with ``snaps`` it also returns what a decode capped at each of those
  iteration counts returns (one pass serves every max_iterations of a test).
* ``layered_of(case, mi)``: (success, iterations, final) of a case's frames at max_iterations = mi.
* ``main_case`` (N = 1008, 64 frames), ``special_case`` (16 frames: exact codewords, inf, -inf,
  -0.0, 0.0, NaN), ``degree_case(D)`` (8 frames), ``mixed_case`` / ``mix12_case`` (16 frames).

Seen here for the main case at 30 iterations (default_rng(2024), sigma ~ U(0.7, 0.95)): 42 frames
succeed, 22 fail, the successful ones stop at iterations {2, 3, 4, 5, 6, 7, 8, 10, 11, 13, 15};
the oracle's flooding decode succeeds on the same 42 (tests/test_layered_cpu.py asserts all of it).
"""
import functools

import numpy as np

import decode_fixture as DF
import few_fixture as FF
import oracle as O

MI = 30
MIS = (0, 1, 2, MI)
MAIN_SIGMA = (0.7, 0.95)
MAIN_SEED = 2024
MAIN_STOPS = (2, 3, 4, 5, 6, 7, 8, 10, 11, 13, 15)
DVBS2_LAYER_SIZES = [3313, 3226, 3106, 2995, 2864, 2711, 2602, 2407, 2237, 1985, 1700, 1390, 1002, 594, 230, 36, 2]
REG1008_LAYER_SIZES = [91, 88, 87, 79, 66, 52, 31, 9, 1]
DEGREE_MIS = (1, 5)


def check_lists(vid, cid):
    """Per check: (edges in ascending edge id, their variables)."""
    vid, cid = np.asarray(vid, np.int64), np.asarray(cid, np.int64)
    order = np.argsort(cid, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(cid))])
    return [(order[ptr[c]:ptr[c + 1]], vid[order[ptr[c]:ptr[c + 1]]]) for c in range(ptr.size - 1)]


def first_fit(vid, cid):
    """(layer_of int32 [C], n_layers), first-fit in ascending check id."""
    V = int(np.max(vid)) + 1
    used = []
    lists = check_lists(vid, cid)
    layer_of = np.empty(len(lists), np.int32)
    for c, (_, vs) in enumerate(lists):
        l = 0
        while True:
            if l == len(used):
                used.append(np.zeros(V, bool))
            if not used[l][vs].any():
                break
            l += 1
        used[l][vs] = True
        layer_of[c] = l
    return layer_of, len(used)


@functools.lru_cache(maxsize=None)
def _graph_cached(vid_bytes, cid_bytes):
    vid, cid = np.frombuffer(vid_bytes, np.int64), np.frombuffer(cid_bytes, np.int64)
    lists = check_lists(vid, cid)
    layer_of, n_layers = first_fit(vid, cid)
    order = np.lexsort((np.arange(layer_of.size), layer_of))   # by (layer_of[c], c)
    repeat = np.array([np.unique(vs).size < vs.size for _, vs in lists])
    has_edge = np.zeros(int(vid.max()) + 1, bool)
    has_edge[vid] = True
    return dict(lists=lists, layer_of=layer_of, n_layers=n_layers, order=order, repeat=repeat, has_edge=has_edge,
                E=vid.size)


def graph_of(vid, cid):
    return _graph_cached(np.ascontiguousarray(vid, np.int64).tobytes(), np.ascontiguousarray(cid, np.int64).tobytes())


def layered_decode(orc, G, lappr, synd, max_iterations, snaps=()):
    """The definition, one frame.  Returns (success, iterations, final) and, per entry k of
    ``snaps`` (k <= max_iterations), the triple of a decode with max_iterations = k."""
    lappr = np.ascontiguousarray(lappr, np.float64)
    synd = np.ascontiguousarray(synd, np.uint8)
    if orc.check_lappr(lappr, synd):
        res = (1, 0, lappr.copy())
        return res, {k: res for k in snaps}
    post = lappr.copy()
    he = G["has_edge"][:post.size]
    post[:he.size][he] = post[:he.size][he] + 0.0
    c2v, v2c = np.zeros(G["E"]), np.zeros(G["E"])
    at = {0: (0, 0, post.copy())} if 0 in snaps else {}
    res = None
    for it in range(max_iterations):
        for c in G["order"]:
            es, vs = G["lists"][c]
            old = c2v[es]
            v2c[es] = post[vs] - old                     # m_i, all i, before any write
            orc.process_check_node(int(c), synd, c2v, v2c)   # c2v[es] = new
            if not G["repeat"][c]:
                post[vs] = (post[vs] - old) + c2v[es]
            else:
                for i in range(es.size):                 # ascending edge id, post read again
                    post[vs[i]] = (post[vs[i]] - old[i]) + c2v[es[i]]
        if orc.check_lappr(post, synd):
            res = (1, it + 1, post)
            break
        if it + 1 in snaps:
            at[it + 1] = (0, it + 1, post.copy())
    if res is None:
        res = (0, max_iterations, post)
    for k in snaps:   # a frame that stopped by iteration k returns the same whatever the cap >= k
        at.setdefault(k, res)
    return res, at


def layered_batch(case, mis):
    """mi -> (success uint8 [n], iterations int32 [n], final [n, V]) for every mi of ``mis``, from one
    pass at max(mis)."""
    G = graph_of(case["vid"], case["cid"])
    n = case["llr"].shape[0]
    out = {mi: (np.empty(n, np.uint8), np.empty(n, np.int32), np.empty_like(case["llr"])) for mi in mis}
    for f in range(n):
        _, at = layered_decode(case["orc"], G, case["llr"][f], case["synd"][f], max(mis), snaps=tuple(mis))
        for mi in mis:
            s, i, p = at[mi]
            if s and i > mi:   # stopped later than this cap
                raise AssertionError("snapshot missing")
            out[mi][0][f], out[mi][1][f], out[mi][2][f] = s, i, p
    for mi in mis:
        for a in out[mi]:
            a.setflags(write=False)
    return out


def layered_of(case, mi):
    """The restatement's (success, iterations, final) of the case at max_iterations = mi (the case
    was made with its ``mis``: one pass computes them all)."""
    if "lay" not in case:
        case["lay"] = layered_batch(case, case["mis"])
    return case["lay"][mi]


def _with(case, mis):
    case["mis"] = tuple(mis)
    return case


@functools.lru_cache(maxsize=None)
def main_case():
    from qamr import codes

    return _with(DF.make_case(*codes.regular_code(1008, 3, 6, 0), 64, MAIN_SIGMA, MAIN_SEED), MIS)


def assert_main_conditions(case):
    """From the restatement and the oracle alone, before any GPU output."""
    s, it, _ = layered_of(case, MI)
    assert int((s != 0).sum()) == 42 and int((s == 0).sum()) == 22, (int(s.sum()),)
    stops = tuple(sorted(set(it[s != 0].tolist())))
    assert stops == MAIN_STOPS, stops
    so, _, _ = DF.oracle_of(case, MI)
    assert np.array_equal(so != 0, s != 0)                    # flooding succeeds on the same 42
    assert len(stops) >= 5 and 0 < (s != 0).sum() < s.size    # the conditions to keep


SPECIAL_CODEWORDS = (0, 1, 2, 3)
SPECIAL_FRAMES = (8, 12)


@functools.lru_cache(maxsize=None)
def special_case():
    """16 frames of the N = 1008 code: frames 0..3 exact codewords ((1, 0), a plain copy), frames 8
    and 12 carry inf, -inf, -0.0, 0.0, NaN on their first five variables."""
    from qamr import codes

    def plant(orc, llr, word, sig):
        cw = np.array(SPECIAL_CODEWORDS)
        llr[cw] = 2 / sig[cw] ** 2 * (1 - 2.0 * word[cw])
        for f in SPECIAL_FRAMES:
            llr[f, :5] = DF.SPECIAL5

    return _with(DF.make_case(*codes.regular_code(1008, 3, 6, 0), 16, MAIN_SIGMA, MAIN_SEED + 1, plant=plant), MIS)


def assert_special_conditions(case):
    s, it, fin = layered_of(case, MI)
    cw = np.array(SPECIAL_CODEWORDS)
    assert (s[cw] == 1).all() and (it[cw] == 0).all()
    assert np.array_equal(fin[cw].view(np.int64), case["llr"][cw].view(np.int64))
    for f in SPECIAL_FRAMES:
        assert np.isnan(case["llr"][f]).any() and np.isinf(case["llr"][f]).any()


@functools.lru_cache(maxsize=None)
def degree_case(D):
    """8 frames of the regular (3, D) code of tests/test_gpu_degree_matrix.py."""
    from qamr import codes

    V = DF.v_of(D)
    case = DF.make_case(*codes.regular_code(V, 3, D, seed=100 + D), 8, DF.sigma_of(D), 3000 + D)
    assert set(np.bincount(case["cid"]).tolist()) == {D}
    return _with(case, DEGREE_MIS)


@functools.lru_cache(maxsize=None)
def mixed_case():
    """16 frames of few_fixture.mixed_code(): seven classes, one of a single check, a hub of degree
    70 (so dozens of tiny layers), isolated variables, parallel edges."""
    vid, cid = FF.mixed_code()
    return _with(DF.make_case(vid, cid, 16, FF.MIXED_SIGMA, 4100), (MI,))


@functools.lru_cache(maxsize=None)
def mix12_case():
    """16 frames of decode_fixture.small_code("mix12_16_5"): packed (5) and unpacked (12, 16) classes."""
    return _with(DF.make_case(*DF.small_code("mix12_16_5"), 16, (0.35, 0.6), 4200), (MI,))


def assert_mixed_conditions(case, min_layers):
    """Some frames succeed after at least one iteration; the graph has at least min_layers layers."""
    s, it, _ = layered_of(case, MI)
    assert ((s != 0) & (it >= 1)).any(), (s, it)
    assert graph_of(case["vid"], case["cid"])["n_layers"] >= min_layers


def layer_sizes(layer_of, n_layers):
    return np.bincount(layer_of, minlength=n_layers).tolist()
