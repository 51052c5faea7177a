"""Generate tests/golden/llr_sources_wide.npz from the REFERENCE itself: the direct-reconciliation LAPPRs
(sims/reconciliation.pyx:25-72 through the cpdef y_to_lappr_grey_array) and the hard-reverse ones
(NoiseMapper.bare_llr / bare_llr_table, noisemapper.pyx:197-220, :423-432) where llr_sources.npz does not
reach: 3, 5, 6 and 8 bits per symbol, a shaped alphabet (its variance changes twoVariance), a low and a
high SNR each, and channel samples that drive exp and log into their tails -- subnormal and zero sums,
+-inf and NaN LAPPRs (tests/math_fixture.py lappr_samples).

Run where the reference build is available, as tests/golden/make_golden.py:

    make -C oracle ref
    PYTHONPATH=oracle/_ref python3 tests/golden/make_golden_llr_wide.py

Every array stored is data: seeded inputs and what the reference returned for them.  No reference source
is stored.  Layout of llr_sources_wide.npz, per case c of math_fixture.LAPPR_WIDE_CASES (prefix "c<c>_"):

    bps, probs [M], two_var                 the alphabet's arguments and twoVariance = Es 10^(-snr/10)
    y [S]                                   the channel samples
    direct [S * bps]                        y_to_lappr_grey_array(y, pa, two_var)
    x [S] (int16), bare [M][bps]            symbols and NoiseMapper(pa, two_var / 2).bare_llr_table
    bare_llr_x [S * bps]                    bare_llr(x)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref"))

from qamreconciliation.alphabet import PAMAlphabet  # noqa: E402  (the reference build)
from qamreconciliation.noisemapper import NoiseMapper  # noqa: E402
from sims.reconciliation import y_to_lappr_grey_array  # noqa: E402

from make_golden_cases import demap_wide_probs, inorder_sum  # noqa: E402
from math_fixture import LAPPR_WIDE_CASES, lappr_samples  # noqa: E402


def gen(out):
    for c, (bps, shape, snr) in enumerate(LAPPR_WIDE_CASES):
        probs = demap_wide_probs(bps, shape)
        if probs is not None:
            assert inorder_sum(probs) == 1.0 and (probs > 0).all()
        pa = PAMAlphabet(bps, 2.0) if probs is None else PAMAlphabet(bps, 2.0, probs.copy())
        two_var = float(pa.variance * (10 ** (-snr / 10)))   # sims/reconciliation.pyx:109-110
        y = lappr_samples(pa.constellation, pa.thresholds, two_var, 6100 + c)
        S = y.size
        direct = np.asarray(y_to_lappr_grey_array(y.copy(), pa, two_var)).copy()
        nm = NoiseMapper(pa, two_var / 2)
        x = np.random.default_rng(6200 + c).integers(0, pa.order, S).astype(np.int64)
        k = f"c{c}_"
        out.update({k + "bps": bps, k + "probs": np.asarray(pa.probabilities, np.float64).copy(), k + "two_var": two_var,
                    k + "y": y, k + "direct": direct, k + "x": x.astype(np.int16),
                    k + "bare": np.asarray(nm.bare_llr_table).copy(), k + "bare_llr_x": np.asarray(nm.bare_llr(x)).copy()})
        sub = int(((direct != 0) & (np.abs(direct) < 1e-300)).sum())
        print(f"  case {c}: {pa.order}-PAM {snr} dB shape={shape} two_var={two_var:.4g} S={S} "
              f"direct inf={int(np.isinf(direct).sum())} nan={int(np.isnan(direct).sum())} of {direct.size} (tiny {sub})",
              flush=True)
        assert np.isinf(direct).any() and np.isnan(direct).any(), c
    out["n_cases"] = len(LAPPR_WIDE_CASES)


if __name__ == "__main__":
    out = {}
    gen(out)
    path = os.path.join(HERE, "llr_sources_wide.npz")
    np.savez_compressed(path, **out)
    print(f"[golden] llr_sources_wide.npz: {os.path.getsize(path)} bytes", flush=True)
