"""Generate tests/golden/decoder_degrees.npz: what the REFERENCE's compiled Decoder.decode returns
for the frames the decoder's GPU tests decode, at every check degree they cover.

Run where the reference build is available, as the other make_golden*.py:

    make -C oracle all ref
    python3 tests/golden/make_golden_degrees.py

Two things to know:

* oracle/_ref must precede qam-reconciliation_amd on sys.path: the drop-in facade package there is
  also named ``qamreconciliation``.  This script puts it first itself and asserts where the
  Decoder it imported comes from.
* The reference's ``decode`` takes writable buffers only, and the fixtures' frames are read-only:
  every frame is passed as a copy.

The cases are ``decode_fixture.golden_cases()``, and the frames are taken from the cases themselves,
so what is recorded is exactly what the tests decode:

* ``case_of(D, variant)`` for D = 2..16 and HIGH_DEGREES, clean and special (512 frames each);
* ``small_case(name, "special")`` for the seven codes of CODES;
* ``few_fixture.mixed_case()`` (5 frames);
* ``himix_case(variant)``, clean and special.

The file holds digests of inputs and recorded results only (``decode_fixture.frame_digests`` /
``input_digest``: 8-byte BLAKE2b of the doubles' little-endian int64 view with every NaN replaced by
0x7ff8000000000000).  Arrays, cases concatenated in the order of ``names``:

  names [n], n_frames [n], vnum [n], input_digest [n][8]
  per mi in 1, 2, 3, 30:  mi<mi>_off [n + 1] and, per recorded frame (``golden_frames``: all at 30;
    at 1, 2, 3 the first 64 and every planted frame), mi<mi>_success u8, mi<mi>_iters i32,
    mi<mi>_digest [.][8] u8
  full_off [n + 1] (in doubles), full: the final LAPPRs at 30 iterations of ``golden_full_frames``
    (frames 8 and 300, which carry the special values, and frame 12), for diagnosis.

The members are written with a fixed timestamp, so the file regenerates byte for byte.  The
generator asserts that the file stays below 1 MB.
"""
from __future__ import annotations

import io
import multiprocessing
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import decode_fixture as DF  # noqa: E402  (its conftest import puts qam-reconciliation_amd on sys.path)

REF = os.path.join(ROOT, "oracle", "_ref")
sys.path.insert(0, REF)

from qamreconciliation.decoder import Decoder  # noqa: E402  (the reference build)

import qamreconciliation.decoder as _refmod  # noqa: E402

assert os.path.abspath(_refmod.__file__).startswith(REF + os.sep), _refmod.__file__

OUT = os.path.join(HERE, "decoder_degrees.npz")


def record(name):
    """One case: the reference's (success, iterations, final) per recorded frame and mi."""
    case = DF.golden_cases()[name]()
    llr, synd = case["llr"], case["synd"]
    n = llr.shape[0]
    dec = Decoder(np.array(case["vid"], dtype=np.int64), np.array(case["cid"], dtype=np.int64))
    rec = dict(name=name, n=n, vnum=llr.shape[1], input_digest=DF.input_digest(llr, synd))
    for mi in DF.GOLDEN_MIS:
        frames = DF.golden_frames(n, mi)
        succ = np.empty(frames.size, np.uint8)
        its = np.empty(frames.size, np.int32)
        fin = np.empty((frames.size, llr.shape[1]))
        for k, f in enumerate(frames):
            ok, it, out = dec.decode(llr[f].copy(), synd[f].copy(), mi)
            succ[k], its[k], fin[k] = ok, it, np.asarray(out)
        rec[mi] = (succ, its, DF.frame_digests(fin))
        if mi == DF.MI:
            rec["full"] = fin[DF.golden_full_frames(n)].copy()
            rec["stats"] = (int(succ.sum()), int(np.isnan(fin).any(axis=1).sum()))
    return rec


def save_npz(path, arrays):
    """np.savez_compressed with a fixed member timestamp (numpy stamps the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


if __name__ == "__main__":
    names = list(DF.golden_cases())
    with multiprocessing.get_context("fork").Pool(min(8, os.cpu_count() or 1)) as pool:
        recs = pool.map(record, names, chunksize=1)
    out = dict(names=np.array(names), n_frames=np.array([r["n"] for r in recs], np.int32),
               vnum=np.array([r["vnum"] for r in recs], np.int32),
               input_digest=np.stack([r["input_digest"] for r in recs]))
    for mi in DF.GOLDEN_MIS:
        out[f"mi{mi}_off"] = np.concatenate([[0], np.cumsum([r[mi][0].size for r in recs])]).astype(np.int64)
        out[f"mi{mi}_success"] = np.concatenate([r[mi][0] for r in recs])
        out[f"mi{mi}_iters"] = np.concatenate([r[mi][1] for r in recs])
        out[f"mi{mi}_digest"] = np.concatenate([r[mi][2] for r in recs])
    out["full_off"] = np.concatenate([[0], np.cumsum([r["full"].size for r in recs])]).astype(np.int64)
    out["full"] = np.concatenate([r["full"].ravel() for r in recs])
    for r in recs:
        print(f"  {r['name']}: {r['n']} frames, V = {r['vnum']}, at {DF.MI} iterations {r['stats'][0]} successes, "
              f"{r['stats'][1]} frames with NaN", flush=True)
    save_npz(OUT, out)
    size = os.path.getsize(OUT)
    print(f"[golden] decoder_degrees.npz: {size} bytes", flush=True)
    assert size < 1_000_000, size
