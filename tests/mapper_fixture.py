"""What the demapper, interpolation-grid and mutual-information tests share: a fixture case's alphabet and
NoiseMapper, the readers of the fixtures' expected values, and the frame-innermost upload.  A case is
addressed by the loaded fixture and its key prefix ("c3_" in interp.npz, mi.npz, mi_quad.npz and
demap_wide.npz, "w5_" in wide_interp_mi.npz).

* ``alphabet`` / ``mapper`` / ``host_mapper``: the case's PAMAlphabet, with its NoiseMapper, or with what the
  host-only evaluators read of one.  ``mapper`` builds a fresh NoiseMapper unless the caller passes a cache.
* ``sha`` / ``block_expected`` / ``expected_terms`` / ``quad_expected`` / ``ORDER21`` / ``ORDER30``: the digest
  of the fixtures, and their expected values in the layout the device writes.
* ``to_dev`` / ``mc_inputs`` / ``run_device``: host [S][B] -> device [S][ld], the same for the block-major
  Monte-Carlo inputs, and one Monte-Carlo launch into NaN-filled outputs.
"""
import hashlib
import types

import numpy as np

FIXTURE = "fixture"   # mapper(cfg=FIXTURE): the case's own sign configuration

# QUADPACK's evaluation sequence in the kernel's node numbering: dqk21 takes the centre, then the pairs
# (below, above) of the even and of the odd nodes; dqk15i the centre's +T, -T, then per node f(T1), f(T2),
# f(-T1), f(-T2)
ORDER21 = [0] + [k for tw in (2, 4, 6, 8, 10) for k in (tw, 10 + tw)] + [k for tw in (1, 3, 5, 7, 9) for k in (tw, 10 + tw)]
ORDER30 = [0, 1] + [s for j in range(1, 8) for s in (2 * j, 2 * (7 + j), 2 * j + 1, 2 * (7 + j) + 1)]


def alphabet(g, prefix):
    import qamr

    probs = g[prefix + "probs"]
    return qamr.PAMAlphabet(int(g[prefix + "bps"]), 2.0, None if np.all(probs == probs[0]) else probs)


def mapper(g, prefix, cfg=FIXTURE, cache=None):
    """-> (PAMAlphabet, NoiseMapper) of the case, with its trunkation threshold and intervals per step where the
    fixture holds them; `cfg` replaces the case's sign configuration (None: NoiseMapper's default).  Every call
    builds a new NoiseMapper -- knob interp_seg is read when its grid is built -- unless `cache`, a dictionary of
    the caller's, is given: then one per (case, configuration) is built and kept there."""
    import qamr

    at = (prefix, cfg if cfg is None or cfg is FIXTURE else bytes(cfg))
    if cache is not None and at in cache:
        return cache[at]
    pa = alphabet(g, prefix)
    grid = (float(g[prefix + "trunc"]), int(g[prefix + "nips"])) if prefix + "trunc" in g.files else ()
    made = (pa, qamr.NoiseMapper(pa, float(g[prefix + "noise_var"]), g[prefix + "cfg"] if cfg is FIXTURE else cfg, *grid))
    if cache is not None:
        cache[at] = made
    return made


def host_mapper(g, prefix):
    """-> (PAMAlphabet, what P_xhat / mutual_information_X_Xhat read of a NoiseMapper), from the pure host_tables."""
    from qamr.noisemapper import host_tables

    pa = alphabet(g, prefix)
    sigma = float(np.sqrt(float(g[prefix + "noise_var"])))
    fw = host_tables(pa.constellation, pa.thresholds, pa.probabilities, sigma, pa.bit_per_symbol)[0]
    return pa, types.SimpleNamespace(order=pa.order, probabilities=pa.probabilities, fwrd_transition_probability=fw)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()


def block_expected(la, S, B, bps):
    """[S * B * bps] symbol-major LAPPRs -> the decoder's layout [S * bps][B] (v = s * bps + k)."""
    return np.ascontiguousarray(la.reshape(S, B, bps).transpose(0, 2, 1).reshape(S * bps, B))


def expected_terms(g, prefix, nblk=None):
    """The Monte-Carlo terms of the first nblk blocks (all of them by default), [3][S][nblk]."""
    return np.ascontiguousarray(g[prefix + "terms"][:, :nblk, :].transpose(0, 2, 1))


def quad_expected(g, prefix, name):
    """-> (I, abserr, neval, warned) of the case's integral `name` ("base" or "xy")."""
    k = f"{prefix}{name}_"
    return float(g[k + "I"]), float(g[k + "abserr"]), int(g[k + "neval"]), bool(g[k + "warned"])


def to_dev(a, ld, dtype):
    """Host [S][B] -> device [S][ld], padding columns zero."""
    import torch

    S, B = a.shape
    t = torch.zeros((S, ld), dtype=dtype, device="cuda")
    t[:, :B] = torch.from_numpy(np.ascontiguousarray(a)).to("cuda").to(dtype)
    return t


def mc_inputs(g, prefix, ld, nblk=None):
    """The symbols and channel outputs of the case's first nblk Monte-Carlo blocks (all by default), stored [B][S]
    block-major -> device (x int64, y fp64), each [S][ld] frame-innermost."""
    import torch

    return (to_dev(g[prefix + "x"][:nblk].astype(np.int64).T, ld, torch.int64),
            to_dev(g[prefix + "y"][:nblk].T, ld, torch.float64))


def run_device(nm, pX, x, y, nblk, ld, which=(1, 1, 1)):
    """montecarlo_information_device -> (info [3][ld], terms [3][S][ld]) as numpy, both pre-filled with NaN."""
    import torch
    from qamr.mutual_information import montecarlo_information_device

    Sq = x.shape[0]
    info = torch.full((3, ld), float("nan"), dtype=torch.float64, device="cuda")
    terms = torch.full((3, Sq, ld), float("nan"), dtype=torch.float64, device="cuda")
    ret, t = montecarlo_information_device(nm, pX, x, y, nblk, which=np.array(which, np.uint8), terms=terms, out=info)
    torch.cuda.synchronize()
    assert t.data_ptr() == terms.data_ptr() and ret.data_ptr() == info.data_ptr() and tuple(ret.shape) == (3, nblk)
    return info.cpu().numpy(), terms.cpu().numpy()
