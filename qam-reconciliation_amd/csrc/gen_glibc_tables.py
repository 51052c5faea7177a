#!/usr/bin/env python3
"""Generate glibc_tables.inc: the data of the host libm's exp(), log() and log2().

The reference's box-plus (decoder.pyx:41-45) calls glibc's exp and log; on x86-64
with FMA, glibc 2.35 dispatches them (ifunc) to __exp_fma / __log_fma, compiled from
sysdeps/ieee754/dbl-64/e_exp.c and e_log.c (the ARM optimized-routines algorithms:
a 128-entry 2^(i/128) table with a degree-5 polynomial, and a 128-entry {1/c, log c}
table with a degree-6 polynomial plus a degree-12 polynomial near 1).  The strict
arithmetic of glibc_math.hpp restates those algorithms operation by operation; this
script pulls their constant data (struct exp_data / struct log_data of
sysdeps/ieee754/dbl-64/math_config.h) out of the libm binary the reference runs
against, located by the leading constants of each struct, so that the restatement
is pinned to the exact tables of the pinned library (tests/test_glibc_math.py
compares it against libm itself bit for bit).

    python gen_glibc_tables.py OUT.inc [LIBM]
"""
import struct
import sys

LIBM = "/lib/x86_64-linux-gnu/libm.so.6"


def _find_unique(data, pat, what):
    hits = []
    i = data.find(pat)
    while i >= 0:
        hits.append(i)
        i = data.find(pat, i + 1)
    if len(hits) != 1:
        raise SystemExit(f"gen_glibc_tables: {what}: expected one match in libm, found {len(hits)}")
    return hits[0]


def hexd(x):
    return float.hex(x)


def log2_lines(data):
    """struct log2_data {invln2hi, invln2lo, poly[6], poly1[10], tab[64] {invc, logc}, tab2[64] {chi, clo}}
    of sysdeps/ieee754/dbl-64/e_log2_data.c: the build without __FP_FAST_FMA (invln2hi has its low
    32 bits clear and tab2 is present), which is what libm's log2 symbol is on x86-64 (no ifunc
    variant; glibc_math.hpp g_log2_full).  New names only: everything above stays as it was."""
    o = _find_unique(data, struct.pack("<dd", float.fromhex("0x1.7154765200000p+0"),
                                       float.fromhex("0x1.705fc2eefa200p-33")), "log2_data")
    head = struct.unpack_from("<18d", data, o)
    tab = struct.unpack_from("<128d", data, o + 18 * 8)
    tab2 = struct.unpack_from("<128d", data, o + (18 + 128) * 8)
    # sanity: invc in (0.5, 2), chi = the centre c ~ 1 / invc and |clo| far below it, the first polynomials'
    # leading coefficients -1/(2 ln 2)
    ok = all(0.5 < tab[2 * i] < 2.0 and abs(tab2[2 * i] * tab[2 * i] - 1.0) < 1e-3 and abs(tab2[2 * i + 1]) < 1e-15
             for i in range(64))
    if not ok or abs(head[2] + 0.7213475204444817) > 1e-9 or abs(head[8] + 0.7213475204444817) > 1e-9:
        raise SystemExit("gen_glibc_tables: unexpected log2 table contents (not glibc 2.28+ non-FMA log2_data)")
    L = ["// glibc log2_data (e_log2_data.c, the build without __FP_FAST_FMA), see glibc_math.hpp g_log2_full.",
         f"constexpr double kGl2InvLn2hi = {hexd(head[0])};", f"constexpr double kGl2InvLn2lo = {hexd(head[1])};"]
    for i in range(6):
        L.append(f"constexpr double kGl2A{i} = {hexd(head[2 + i])};")
    for i in range(10):
        L.append(f"constexpr double kGl2B{i} = {hexd(head[8 + i])};")
    L.append("// log2: {invc, logc, chi, clo} for i = 0..63 (tab and tab2 of log2_data); the initializer of qr::GlibcLog2")
    L.append("#define QR_GLIBC_LOG2_INIT { { \\")
    for i in range(64):
        L.append("        {" + ", ".join(hexd(v) for v in (tab[2 * i], tab[2 * i + 1], tab2[2 * i], tab2[2 * i + 1])) +
                 "}, \\")
    L.append("    } }")
    return L


def main():
    out = sys.argv[1]
    data = open(sys.argv[2] if len(sys.argv) > 2 else LIBM, "rb").read()
    # struct exp_data {invln2N, shift, negln2hiN, negln2loN, poly[4], exp2_shift, exp2_poly[5], tab[256]}
    eo = _find_unique(data, struct.pack("<dd", float.fromhex("0x1.71547652b82fep7"), float.fromhex("0x1.8p52")),
                      "exp_data")
    ehead = struct.unpack_from("<14d", data, eo)
    etab = struct.unpack_from("<256Q", data, eo + 14 * 8)
    # struct log_data {ln2hi, ln2lo, poly[5], poly1[11], tab[128] {invc, logc}}; the first of the two
    # structs that start with ln2hi, ln2lo and continue with poly[0] = -0x1.0000000000001p-1
    lpat = struct.pack("<ddd", float.fromhex("0x1.62e42fefa3800p-1"), float.fromhex("0x1.ef35793c76730p-45"),
                       float.fromhex("-0x1.0000000000001p-1"))
    lo = _find_unique(data, lpat, "log_data")
    lhead = struct.unpack_from("<18d", data, lo)
    ltab = struct.unpack_from("<256d", data, lo + 18 * 8)
    # sanity: poly1[0] == -0.5 (B[0] of e_log.c), exp tab[1] = asuint64(1.0), log tab entries positive invc
    exd = [struct.unpack("<d", struct.pack("<Q", v))[0] for v in etab]
    if any(x != 0.0 and not (2.2250738585072014e-308 <= abs(x) < float("inf")) for x in exd):
        raise SystemExit("gen_glibc_tables: exp table entry is not a normal double")
    if lhead[7] != -0.5 or etab[1] != 0x3FF0000000000000 or not all(0.5 < ltab[2 * i] < 2.0 for i in range(128)):
        raise SystemExit("gen_glibc_tables: unexpected table contents (not glibc 2.28+ exp/log data)")
    L = ["// Generated by gen_glibc_tables.py from %s -- do not edit." % (sys.argv[2] if len(sys.argv) > 2 else LIBM),
         "// glibc exp_data / log_data (sysdeps/ieee754/dbl-64/math_config.h), see glibc_math.hpp.",
         "#pragma once", ""]
    names = ["kGxInvLn2N", "kGxShift", "kGxNegLn2hiN", "kGxNegLn2loN", "kGxC2", "kGxC3", "kGxC4", "kGxC5"]
    for n, v in zip(names, ehead[:8]):
        L.append(f"constexpr double {n} = {hexd(v)};")
    L.append(f"constexpr double kGlLn2hi = {hexd(lhead[0])};")
    L.append(f"constexpr double kGlLn2lo = {hexd(lhead[1])};")
    for i in range(5):
        L.append(f"constexpr double kGlA{i} = {hexd(lhead[2 + i])};")
    for i in range(11):
        L.append(f"constexpr double kGlB{i} = {hexd(lhead[7 + i])};")
    L.append("// exp: {tail, sbits} for i = 0..127 (tab[2i], tab[2i+1] of exp_data), bit patterns")
    L.append("static const uint64_t kGxTab[256] = {")
    for i in range(0, 256, 4):
        L.append("    " + ", ".join(f"0x{v:016x}ull" for v in etab[i:i + 4]) + ",")
    L.append("};")
    L.append("// log: {invc, logc} for i = 0..127 (tab of log_data)")
    L.append("static const double kGlTab[256] = {")
    for i in range(0, 256, 4):
        L.append("    " + ", ".join(hexd(v) for v in ltab[i:i + 4]) + ",")
    L.append("};")
    # the same data as an initializer of qr::GlibcTables {double2 ex[256]; GlibcLogK lk[128]; double2 lg[128];}
    # (every entry is a normal double or zero, so hex floats are exact)
    # ex[i] = {tail_i, tab[2i+1]}: the device adds ki << 45 as glibc does (glibc_math.hpp g_add_ki)
    ex = []
    for i in list(range(128)) * 2:  # stored twice (glibc_math.hpp GlibcTables)
        ex.append(struct.unpack("<d", struct.pack("<Q", etab[2 * i]))[0])
        ex.append(struct.unpack("<d", struct.pack("<Q", etab[2 * i + 1]))[0])
    L.append("#define QR_GLIBC_TABLES_INIT { \\")
    L.append("    { \\")
    for i in range(0, 256, 2):
        L.append("        " + " ".join(f"{{{hexd(ex[2 * k])}, {hexd(ex[2 * k + 1])}}}," for k in (i, i + 1)) + " \\")
    # member order of qr::GlibcTables: ex[256], lk[128], lg[128] (ex + lk = GlibcTablesBP, the
    # box-plus prefix the check sweep stages)
    # lk[(i + 48) & 127] = {invc 2^-k, fma(k, Ln2hi, logc), k ? Ln2lo : 0, 0}, k = (i <= 80)
    # (glibc_math.hpp GlibcTables / GlibcLogK; plain float ops are exact here: k in {0, 1})
    lk = [None] * 128
    for i in range(128):
        kk = 1 if i <= 80 else 0
        lk[(i + 48) & 127] = (ltab[2 * i] * 0.5 if kk else ltab[2 * i],
                              lhead[0] + ltab[2 * i + 1] if kk else ltab[2 * i + 1],
                              lhead[1] if kk else 0.0, 0.0)
    L.append("    }, { \\")
    for j in range(128):
        L.append("        {" + ", ".join(hexd(v) for v in lk[j]) + "}, \\")
    L.append("    }, { \\")
    for i in range(0, 128, 2):
        L.append("        " + " ".join(f"{{{hexd(ltab[2 * k])}, {hexd(ltab[2 * k + 1])}}}," for k in (i, i + 1)) + " \\")
    L.append("    } }")
    L += log2_lines(data)
    open(out, "w").write("\n".join(L) + "\n")


if __name__ == "__main__":
    main()
