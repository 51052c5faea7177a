"""Generate tests/golden/demap_wide.npz from the REFERENCE itself: the search demapper
(demap_lappr_array, noisemapper.pyx:450-559), its root search (g_inv_search / demap_noise_search,
:310-345, :407-419), the F_Y tables (:149-162) and the Bob side (hard_decide_index / map_noise,
:349-388) outside the box the other fixtures cover: shaped probabilities, 32..256-PAM, -12 dB
and 80..85 dB.

Run where the reference build is available, as tests/golden/make_golden.py:

    make -C oracle ref
    PYTHONPATH=oracle/_ref python3 tests/golden/make_golden_demap_wide.py

Every array stored is data: seeded inputs and what the reference's NoiseMapper returned for
them.  No reference source is stored.  Layout of demap_wide.npz, per case c (prefix "c<c>_"):

    bps, noise_var, cfg [M], probs [M]      the NoiseMapper's arguments (alternating configuration)
    Fthr [M+1], dF [M]                      F_Y_thresholds, delta_F_Y
    n [S][B], j [S][B] (int16)              the transformed noise and tx symbols, as a block for the
                                            device layout (symbol index s * B + b)
    la [S*B*bps]                            demap_lappr_array(n.ravel(), j.ravel())
    dns_i [K] (int16), dns [K]              demap_noise_search(n.ravel()[:K], dns_i), K = min(64, S*B)
    y_edge, xhat_edge (int16), nhat_edge    hard_decide_index(y_edge), map_noise(y_edge, xhat_edge)
  and, for the cases rerun with the all-zero configuration (HAS_BASE):
    base_la, base_dns, base_nhat_edge

The reference's search loops are unbounded.  Two conditions keep them finite and are asserted
before the reference is called: every n lies in [0, 1] (a target outside [0, 1] never ends the
bracket loop), and the in-order double sum of a non-uniform probability vector is exactly 1.0
(F_Y(+inf) is that sum; below 1.0, a target of 1.0 in the last region never ends the loop).
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "qam-reconciliation_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref"))

from qamreconciliation.alphabet import PAMAlphabet  # noqa: E402  (the reference build)
from qamreconciliation.noisemapper import NoiseMapper  # noqa: E402

from make_golden import alternating, noise_var  # noqa: E402
from make_golden_cases import DEMAP_WIDE_CASES, demap_wide_probs, inorder_sum  # noqa: E402

B_BLOCK = 70
N_LEAD = (1e-300, 1 - 2.0 ** -53, 2.0 ** -53, 0.5)


def edge_samples(pa):
    """Bob-side edge block: every threshold (the outer ones are +-100 a_max) with its two nextafter
    neighbours, +-0.0, every constellation point, +-1e300 and +-inf."""
    th = np.asarray(pa.thresholds, np.float64)
    return np.concatenate([th, np.nextafter(th, -np.inf), np.nextafter(th, np.inf), [0.0, -0.0],
                           np.asarray(pa.constellation, np.float64), [1e300, -1e300, np.inf, -np.inf]])


def gen(out):
    for c, (bps, snr, shape, symbols, has_base) in enumerate(DEMAP_WIDE_CASES):
        t0 = time.time()
        M = 1 << bps
        probs = demap_wide_probs(bps, shape)
        if probs is not None:
            assert inorder_sum(probs) == 1.0, (c, inorder_sum(probs))
            assert (probs > 0).all()
        pa = PAMAlphabet(bps, 2.0) if probs is None else PAMAlphabet(bps, 2.0, probs.copy())
        nv = float(noise_var(pa, snr))
        cfg = alternating(M)
        B = min(B_BLOCK, symbols)
        S = symbols // B
        assert S * B == symbols
        rng = np.random.default_rng(5200 + c)
        n = rng.uniform(0, 1, symbols)
        n[:len(N_LEAD)] = N_LEAD
        j = rng.integers(0, M, symbols).astype(np.int64)
        K = min(64, symbols)
        di = rng.integers(0, M, K).astype(np.int64)
        assert ((n >= 0.0) & (n <= 1.0)).all()
        y_edge = edge_samples(pa)
        k = f"c{c}_"
        for name, nm in (("", NoiseMapper(pa, nv, cfg)),) + ((("base_", NoiseMapper(pa, nv)),) if has_base else ()):
            la = np.asarray(nm.demap_lappr_array(n.copy(), j.copy())).copy()
            dns = np.asarray(nm.demap_noise_search(n[:K].copy(), di.copy())).copy()
            xh = np.asarray(nm.hard_decide_index(y_edge.copy()), np.int64).copy()
            nh = np.asarray(nm.map_noise(y_edge.copy(), xh.copy())).copy()
            out.update({k + name + "la": la, k + name + "dns": dns, k + name + "nhat_edge": nh})
            if not name:
                out.update({k + "bps": bps, k + "noise_var": nv, k + "cfg": cfg,
                            k + "probs": np.asarray(pa.probabilities, np.float64).copy(),
                            k + "Fthr": np.asarray(nm.F_Y_thresholds).copy(), k + "dF": np.asarray(nm.delta_F_Y).copy(),
                            k + "n": n.reshape(S, B), k + "j": j.reshape(S, B).astype(np.int16),
                            k + "dns_i": di.astype(np.int16), k + "y_edge": y_edge, k + "xhat_edge": xh.astype(np.int16)})
            print(f"  case {c}{' (all-zero cfg)' if name else ''}: {M}-PAM {snr} dB {shape} nv={nv:.4g} symbols={symbols} "
                  f"lappr inf={int(np.isinf(la).sum())} nan={int(np.isnan(la).sum())} of {la.size}; "
                  f"dns nan={int(np.isnan(dns).sum())}; nhat_edge nan={int(np.isnan(nh).sum())} "
                  f"inf={int(np.isinf(nh).sum())} of {nh.size}; {time.time() - t0:.1f} s", flush=True)
    out["n_cases"] = len(DEMAP_WIDE_CASES)


if __name__ == "__main__":
    out = {}
    gen(out)
    path = os.path.join(HERE, "demap_wide.npz")
    np.savez_compressed(path, **out)
    print(f"[golden] demap_wide.npz: {os.path.getsize(path)} bytes", flush=True)
