"""The error behaviour of the qamr facade, pinned: one table of (public method and error path, bad
call, exact message), every one a plain ValueError, over NoiseMapper, Decoder, Matrix, the public functions of mutual_information,
Simulator, BinaryChannelSimulator and SofteningPipeline.  Every message is the facade's own text,
compared whole.  The code is the Hamming (7,4) graph, the alphabets 2-PAM and 4-PAM, S <= 8,
ld = 64 (63 for the ld % 64 rows)."""
import os
import types

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

V, C, E = 7, 3, 12      # the Hamming (7,4) graph
S, LD = 4, 64           # symbols per frame and leading dimension of the demapper rows

DT = "Buffer dtype mismatch, expected '{}' but got '{}'"
SIZES = "Sizes do not match"
SIZES_TX = "Sizes of transformed noise vector and tx symbols do not match"
CONTIG = "{}: must be contiguous (the kernels assume dense rows)"
GPU = "{}: must be a GPU tensor"
BATCH = "{}: need ld % 64 == 0 and 0 < B <= ld (B={}, ld={})"
MI_BATCH = "montecarlo_information_device: need ld % 64 == 0, 0 < B <= ld, S >= 1 (B={}, ld={}, S={})"
KIND = "kind must be 'base' or 'X_Y' (0 or 1), got 'x'"
LIMIT = "limit must be at least 1, got 0"
DEMAPPER = "demapper must be one of ('search', 'simplified'), got 'x'"
F64, I64 = np.float64, np.int64


@pytest.fixture(scope="module")
def c(gpu):
    """Everything the bad calls start from; nothing here is changed by a row."""
    import torch

    import qamr
    from qamr import codes, mutual_information as mi
    from qamr.pipeline import SofteningPipeline
    from qamr.sim import Simulator
    from qamr.sim_binary import BinaryChannelSimulator

    vid, cid = codes.load_edge_csv(os.path.join(GOLDEN, "hamming_7-4.csv"))
    dev = torch.device("cuda", 0)

    def t(shape, dtype=torch.float64, device=dev):
        return torch.zeros(shape, dtype=dtype, device=device)

    pa2, pa4 = qamr.PAMAlphabet(1, 2.0), qamr.PAMAlphabet(2, 2.0)
    dec = qamr.Decoder(vid, cid)
    return types.SimpleNamespace(
        torch=torch, qamr=qamr, mi=mi, t=t, vid=vid, cid=cid, dec=dec, pa2=pa2, pa4=pa4,
        nm2=qamr.NoiseMapper(pa2, 0.5), nm4=qamr.NoiseMapper(pa4, 0.5), mat=qamr.Matrix(vid, cid),
        Simulator=Simulator, Binary=BinaryChannelSimulator, Pipeline=SofteningPipeline,
        pipe=SofteningPipeline(dec, 1, 3.0, 2),
        y=t((S, LD)), j=t((S, LD), torch.int64), y63=t((S, 63)), j63=t((S, 63), torch.int64),
        y32=t((S, LD), torch.float32), ycpu=t((S, LD), device="cpu"), ystrided=t((S, 2 * LD))[:, ::2],
        lap=t((V, LD)), syn=t((C, LD), torch.uint8), lap63=t((V, 63)), syn63=t((C, 63), torch.uint8),
        fl=t((2, V)), fs=t((2, C), torch.uint8), word=t((V, LD), torch.uint8),
        pX4=np.full(4, 0.25), u8=torch.uint8, i32=torch.int32, i64=torch.int64)


def z(n, dtype=F64):
    return np.zeros(n, dtype)


def pair_rows(method, size_msg):
    """The (n, j) array methods of NoiseMapper: dtype of either array, then the sizes."""
    return [
        (f"{method}-n-dtype", lambda c: getattr(c.nm4, method)(z(3, np.float32), z(3, I64)), DT.format("double", "float32")),
        (f"{method}-j-dtype", lambda c: getattr(c.nm4, method)(z(3), z(3, np.int32)), DT.format("long", "int32")),
        (f"{method}-size", lambda c: getattr(c.nm4, method)(z(3), z(2, I64)), size_msg),
    ]


def demap_rows(method):
    """demap_device and demap_simplified_device: n_fi, j_fi, B, out."""
    f = lambda c: getattr(c.nm4, method)  # noqa: E731
    return [
        (f"{method}-1d", lambda c: f(c)(c.y[0], c.j, 1), f"{method}: n_fi must be a 2-D tensor [S, ld]"),
        (f"{method}-numpy", lambda c: f(c)(z((S, LD)), c.j, 1), f"{method}: n_fi must be a 2-D tensor [S, ld]"),
        (f"{method}-ld63", lambda c: f(c)(c.y63, c.j63, 1), BATCH.format(method, 1, 63)),
        (f"{method}-B0", lambda c: f(c)(c.y, c.j, 0), BATCH.format(method, 0, LD)),
        (f"{method}-B65", lambda c: f(c)(c.y, c.j, 65), BATCH.format(method, 65, LD)),
        (f"{method}-dtype", lambda c: f(c)(c.y32, c.j, 1), "n_fi: dtype torch.float32, expected torch.float64"),
        (f"{method}-j-dtype", lambda c: f(c)(c.y, c.j.to(c.i32), 1), "j_fi: dtype torch.int32, expected torch.int64"),
        (f"{method}-j-shape", lambda c: f(c)(c.y, c.j[:3], 1), f"j_fi: shape (3, {LD}), expected ({S}, {LD})"),
        (f"{method}-strided", lambda c: f(c)(c.ystrided, c.j, 1), CONTIG.format("n_fi")),
        (f"{method}-cpu", lambda c: f(c)(c.ycpu, c.j, 1), GPU.format("n_fi")),
        (f"{method}-j-cpu", lambda c: f(c)(c.y, c.j.cpu(), 1), GPU.format("j_fi")),
        (f"{method}-out-shape", lambda c: f(c)(c.y, c.j, 1, out=c.y), f"out: shape ({S}, {LD}), expected ({2 * S}, {LD})"),
        (f"{method}-out-type", lambda c: f(c)(c.y, c.j, 1, out=z((2 * S, LD))), "out: expected a torch tensor, got ndarray"),
    ]


def y_rows(method, call):
    """bob_map_device and map_noise_device: the checks on y_fi and B."""
    return [
        (f"{method}-1d", lambda c: call(c, c.y[0], 1), f"{method}: y_fi must be a 2-D tensor [S, ld]"),
        (f"{method}-ld63", lambda c: call(c, c.y63, 1), BATCH.format(method, 1, 63)),
        (f"{method}-B0", lambda c: call(c, c.y, 0), BATCH.format(method, 0, LD)),
        (f"{method}-B65", lambda c: call(c, c.y, 65), BATCH.format(method, 65, LD)),
        (f"{method}-dtype", lambda c: call(c, c.y32, 1), "y_fi: dtype torch.float32, expected torch.float64"),
        (f"{method}-strided", lambda c: call(c, c.ystrided, 1), CONTIG.format("y_fi")),
        (f"{method}-cpu", lambda c: call(c, c.ycpu, 1), GPU.format("y_fi")),
    ]


NOISEMAPPER = [
    ("init-variance", lambda c: c.qamr.NoiseMapper(c.pa4, 0.0), "noise variance must be strictly positive, got 0.0"),
    ("init-cfg-dtype", lambda c: c.qamr.NoiseMapper(c.pa4, 0.5, z(4)), DT.format("unsigned char", "float64")),
    ("init-cfg-short", lambda c: c.qamr.NoiseMapper(c.pa4, 0.5, z(3, np.uint8)),
     "Not enough data for a monotonicity sign configuration"),
    ("F_Y-dtype", lambda c: c.nm4.F_Y(z(3, np.float32)), DT.format("double", "float32")),
    ("F_Y-int", lambda c: c.nm4.F_Y([1, 2]), DT.format("double", "int64")),
    *pair_rows("demap_noise_search", SIZES),
    *pair_rows("demap_noise", SIZES),
    *pair_rows("demap_lappr_array", SIZES_TX),
    *pair_rows("demap_lappr_simplified_array", SIZES_TX),
    ("map_noise-size", lambda c: c.nm4.map_noise(z(3), z(2, I64)), "Input vectors sizes do not match"),
    *y_rows("bob_map_device", lambda c, y, B: c.nm4.bob_map_device(y, B)),
    *y_rows("map_noise_device", lambda c, y, B: c.nm4.map_noise_device(y, c.j63 if y.shape[-1] == 63 else c.j, B)),
    ("map_noise_device-index-dtype", lambda c: c.nm4.map_noise_device(c.y, c.j.to(c.i32), 1),
     "index_fi: dtype torch.int32, expected torch.int64"),
    ("map_noise_device-index-shape", lambda c: c.nm4.map_noise_device(c.y, c.j[:3], 1),
     f"index_fi: shape (3, {LD}), expected ({S}, {LD})"),
    ("map_noise_device-index-cpu", lambda c: c.nm4.map_noise_device(c.y, c.j.cpu(), 1), GPU.format("index_fi")),
    *demap_rows("demap_device"),
    *demap_rows("demap_simplified_device"),
]

BUF = "Buffer has wrong number of dimensions (expected 1, got 2) ({})"
SHORT_V = "message/LAPPR arrays are shorter than the graph"
SHORT_C = "message/syndrome arrays are shorter than the graph"
DEC_B = "decode_device: success/iters must hold at least B=2 entries"
FR_B = "decode_frames_device: success/iters must hold at least B=2 entries"
u8 = lambda n: z(n, np.uint8)  # noqa: E731

DECODER = [
    ("init-dtype", lambda c: c.qamr.Decoder(c.vid.astype(np.int32), c.cid), DT.format("long", "int32") + " (e_to_v)"),
    ("init-c-dtype", lambda c: c.qamr.Decoder(c.vid, c.cid.astype(F64)), DT.format("long", "float64") + " (e_to_c)"),
    ("init-2d", lambda c: c.qamr.Decoder(c.vid.reshape(2, 6), c.cid), BUF.format("e_to_v")),
    ("check_word-dtype", lambda c: c.dec.check_word(z(V), u8(C)), DT.format("unsigned char", "float64") + " (word)"),
    ("check_word-synd-dtype", lambda c: c.dec.check_word(u8(V), z(C, np.int8)),
     DT.format("unsigned char", "int8") + " (synd)"),
    ("check_word-2d", lambda c: c.dec.check_word(u8((1, V)), u8(C)), BUF.format("word")),
    ("check_word-size", lambda c: c.dec.check_word(u8(V - 1), u8(C)), "Size of word does not match number of vnodes"),
    ("check_word-synd-size", lambda c: c.dec.check_word(u8(V), u8(C + 1)), "Size of synd does not match number of cnodes"),
    ("check_synd_node-dtype", lambda c: c.dec.check_synd_node(0, z(V), u8(C)),
     DT.format("unsigned char", "float64") + " (word)"),
    ("check_synd_node-size", lambda c: c.dec.check_synd_node(0, u8(V + 1), u8(C)),
     "Size of word does not match number of vnodes"),
    ("check_synd_node-synd-size", lambda c: c.dec.check_synd_node(0, u8(V), u8(C - 1)),
     "Size of synd does not match number of cnodes"),
    ("check_lappr-dtype", lambda c: c.dec.check_lappr(z(V, np.float32), u8(C)), DT.format("double", "float32") + " (lappr)"),
    ("check_lappr-synd-dtype", lambda c: c.dec.check_lappr(z(V), z(C)), DT.format("unsigned char", "float64") + " (synd)"),
    ("check_lappr-2d", lambda c: c.dec.check_lappr(z(V), u8((C, 1))), BUF.format("synd")),
    ("check_lappr-size", lambda c: c.dec.check_lappr(z(V - 1), u8(C)), "Size of lappr does not match number of vnodes"),
    ("check_lappr-synd-size", lambda c: c.dec.check_lappr(z(V), u8(C - 1)), "Size of synd does not match number of cnodes"),
    ("var_node-dtype", lambda c: c.dec.process_var_node(0, z(V, np.float32), z(E), z(E), z(V)),
     DT.format("double", "float32") + " (lappr_data)"),
    ("var_node-inout-list", lambda c: c.dec.process_var_node(0, z(V), z(E), [0.0] * E, z(V)),
     "var_to_check must be a numpy array (written in place)"),
    ("var_node-inout-dtype", lambda c: c.dec.process_var_node(0, z(V), z(E), z(E), z(V, np.float32)),
     DT.format("double", "float32") + " (updated_lappr)"),
    ("var_node-inout-strided", lambda c: c.dec.process_var_node(0, z(V), z(E), z(2 * E)[::2], z(V)),
     "var_to_check must be a writeable 1-D C-contiguous array"),
    ("var_node-short", lambda c: c.dec.process_var_node(0, z(V), z(E - 1), z(E), z(V)), SHORT_V),
    ("var_node-short-lappr", lambda c: c.dec.process_var_node(0, z(V - 1), z(E), z(E), z(V)), SHORT_V),
    ("check_node-dtype", lambda c: c.dec.process_check_node(0, z(C), z(E), z(E)),
     DT.format("unsigned char", "float64") + " (synd)"),
    ("check_node-inout-list", lambda c: c.dec.process_check_node(0, u8(C), [0.0] * E, z(E)),
     "check_to_var must be a numpy array (written in place)"),
    ("check_node-inout-2d", lambda c: c.dec.process_check_node(0, u8(C), z((1, E)), z(E)),
     "check_to_var must be a writeable 1-D C-contiguous array"),
    ("check_node-short", lambda c: c.dec.process_check_node(0, u8(C), z(E), z(E - 1)), SHORT_C),
    ("check_node-short-synd", lambda c: c.dec.process_check_node(0, u8(C - 1), z(E), z(E)), SHORT_C),
    ("decode-dtype", lambda c: c.dec.decode(z(V, np.float32), u8(C), 5), DT.format("double", "float32") + " (lappr_data)"),
    ("decode-synd-dtype", lambda c: c.dec.decode(z(V), z(C, np.int32), 5), DT.format("unsigned char", "int32") + " (synd)"),
    ("decode-size", lambda c: c.dec.decode(z(V - 1), u8(C), 5), "lappr has 6 entries, the code has 7 variable nodes"),
    ("decode-synd-size", lambda c: c.dec.decode(z(V), u8(C - 1), 5), "synd has 2 entries, the code has 3 check nodes"),
    ("decode_batch-dtype", lambda c: c.dec.decode_batch(z((2, V), np.float32), u8((2, C)), 5),
     "decode_batch expects float64 LAPPRs and uint8 syndromes"),
    ("decode_batch-synd-dtype", lambda c: c.dec.decode_batch(z((2, V)), z((2, C)), 5),
     "decode_batch expects float64 LAPPRs and uint8 syndromes"),
    ("decode_batch-1d", lambda c: c.dec.decode_batch(z(V), u8(C), 5), "decode_batch expects lappr [B, V] and synd [B, C]"),
    ("decode_batch-B", lambda c: c.dec.decode_batch(z((2, V)), u8((3, C)), 5),
     "decode_batch expects lappr [B, V] and synd [B, C]"),
    ("decode_batch-shape", lambda c: c.dec.decode_batch(z((2, V - 1)), u8((2, C)), 5),
     "decode_batch: shape does not match the code"),
    ("decode_device-1d", lambda c: c.dec.decode_device(c.lap[0], c.syn, 2, 5),
     "decode_device: lappr_fi must be a 2-D tensor [V, ld]"),
    ("decode_device-V", lambda c: c.dec.decode_device(c.lap[:6], c.syn, 2, 5),
     "decode_device: tensor shapes do not match the code"),
    ("decode_device-ld63", lambda c: c.dec.decode_device(c.lap63, c.syn63, 2, 5), BATCH.format("decode_device", 2, 63)),
    ("decode_device-B0", lambda c: c.dec.decode_device(c.lap, c.syn, 0, 5), BATCH.format("decode_device", 0, LD)),
    ("decode_device-B65", lambda c: c.dec.decode_device(c.lap, c.syn, 65, 5), BATCH.format("decode_device", 65, LD)),
    ("decode_device-dtype", lambda c: c.dec.decode_device(c.lap.float(), c.syn, 2, 5),
     "lappr_fi: dtype torch.float32, expected torch.float64"),
    ("decode_device-synd-shape", lambda c: c.dec.decode_device(c.lap, c.syn[:2], 2, 5),
     f"synd_fi: shape (2, {LD}), expected ({C}, {LD})"),
    ("decode_device-synd-dtype", lambda c: c.dec.decode_device(c.lap, c.syn.to(c.i32), 2, 5),
     "synd_fi: dtype torch.int32, expected torch.uint8"),
    ("decode_device-cpu", lambda c: c.dec.decode_device(c.lap.cpu(), c.syn, 2, 5), GPU.format("lappr_fi")),
    ("decode_device-synd-cpu", lambda c: c.dec.decode_device(c.lap, c.syn.cpu(), 2, 5), GPU.format("synd_fi")),
    ("decode_device-strided", lambda c: c.dec.decode_device(c.t((V, 2 * LD))[:, ::2], c.syn, 2, 5), CONTIG.format("lappr_fi")),
    ("decode_device-final-shape", lambda c: c.dec.decode_device(c.lap, c.syn, 2, 5, final_fi=c.lap[:6]),
     f"final_fi: shape (6, {LD}), expected ({V}, {LD})"),
    ("decode_device-success-short", lambda c: c.dec.decode_device(c.lap, c.syn, 2, 5, success=c.t(1, c.u8)), DEC_B),
    ("decode_device-iters-short", lambda c: c.dec.decode_device(c.lap, c.syn, 2, 5, iters=c.t(1, c.i32)), DEC_B),
    ("decode_device-success-dtype", lambda c: c.dec.decode_device(c.lap, c.syn, 2, 5, success=c.t(2, c.i32)),
     "success: dtype torch.int32, expected torch.uint8"),
    ("decode_device-iters-dtype", lambda c: c.dec.decode_device(c.lap, c.syn, 2, 5, iters=c.t(2, c.i64)),
     "iters: dtype torch.int64, expected torch.int32"),
    ("decode_device-iters-cpu", lambda c: c.dec.decode_device(c.lap, c.syn, 2, 5, iters=c.t(2, c.i32, "cpu")),
     GPU.format("iters")),
    ("frames-1d", lambda c: c.dec.decode_frames_device(c.fl[0], c.fs, 5),
     "decode_frames_device: lappr must be a 2-D tensor [B, V] with B >= 1"),
    ("frames-B0", lambda c: c.dec.decode_frames_device(c.fl[:0], c.fs[:0], 5),
     "decode_frames_device: lappr must be a 2-D tensor [B, V] with B >= 1"),
    ("frames-shape", lambda c: c.dec.decode_frames_device(c.t((2, V - 1)), c.fs, 5), f"lappr: shape (2, 6), expected (2, {V})"),
    ("frames-dtype", lambda c: c.dec.decode_frames_device(c.fl.float(), c.fs, 5),
     "lappr: dtype torch.float32, expected torch.float64"),
    ("frames-synd-shape", lambda c: c.dec.decode_frames_device(c.fl, c.fs[:1], 5), f"synd: shape (1, {C}), expected (2, {C})"),
    ("frames-cpu", lambda c: c.dec.decode_frames_device(c.fl.cpu(), c.fs, 5), GPU.format("lappr")),
    ("frames-strided", lambda c: c.dec.decode_frames_device(c.t((2, 2 * V))[:, ::2][:, :V], c.fs, 5), CONTIG.format("lappr")),
    ("frames-final-short", lambda c: c.dec.decode_frames_device(c.fl, c.fs, 5, final=c.fl[:1]),
     "decode_frames_device: final must hold at least B=2 rows of V"),
    ("frames-final-1d", lambda c: c.dec.decode_frames_device(c.fl, c.fs, 5, final=c.t(2 * V)),
     "decode_frames_device: final must hold at least B=2 rows of V"),
    ("frames-final-shape", lambda c: c.dec.decode_frames_device(c.fl, c.fs, 5, final=c.t((2, V + 1))),
     f"final: shape (2, {V + 1}), expected (2, {V})"),
    ("frames-success-short", lambda c: c.dec.decode_frames_device(c.fl, c.fs, 5, success=c.t(1, c.u8)), FR_B),
    ("frames-iters-short", lambda c: c.dec.decode_frames_device(c.fl, c.fs, 5, iters=c.t(1, c.i32)), FR_B),
    ("frames-success-dtype", lambda c: c.dec.decode_frames_device(c.fl, c.fs, 5, success=c.t(2, c.i32)),
     "success: dtype torch.int32, expected torch.uint8"),
    ("repack_stats-none", lambda c: c.qamr.Decoder(c.vid, c.cid).repack_stats(LD, 5),
     "repack_stats: no decode_device has run on this stream"),
]

MATRIX = [
    ("matrix-init-dtype", lambda c: c.qamr.Matrix(c.vid.astype(np.int32), c.cid), DT.format("long", "int32") + " (vnode_array)"),
    ("matrix-init-sizes", lambda c: c.qamr.Matrix(c.vid, c.cid[:-1]), "Incompatible sizes for input vectors"),
    ("eval_syndrome-dtype", lambda c: c.mat.eval_syndrome(z(V)), DT.format("unsigned char", "float64") + " (word)"),
    ("eval_syndrome-size", lambda c: c.mat.eval_syndrome(u8(V - 1)), "Size of word does not match number of vnodes"),
    ("eval_syndrome_device-1d", lambda c: c.mat.eval_syndrome_device(c.word[0], 1),
     "eval_syndrome_device: word_fi must be a 2-D tensor [V, ld]"),
    ("eval_syndrome_device-ld63", lambda c: c.mat.eval_syndrome_device(c.word[:, :63], 1),
     BATCH.format("eval_syndrome_device", 1, 63)),
    ("eval_syndrome_device-B0", lambda c: c.mat.eval_syndrome_device(c.word, 0), BATCH.format("eval_syndrome_device", 0, LD)),
    ("eval_syndrome_device-B65", lambda c: c.mat.eval_syndrome_device(c.word, 65), BATCH.format("eval_syndrome_device", 65, LD)),
    ("eval_syndrome_device-dtype", lambda c: c.mat.eval_syndrome_device(c.lap, 1),
     "word_fi: dtype torch.float64, expected torch.uint8"),
    ("eval_syndrome_device-shape", lambda c: c.mat.eval_syndrome_device(c.word[:6], 1),
     f"word_fi: shape (6, {LD}), expected ({V}, {LD})"),
    ("eval_syndrome_device-cpu", lambda c: c.mat.eval_syndrome_device(c.word.cpu(), 1), GPU.format("word_fi")),
]

THREE = "which must hold three flags"
PX = "p_Xhat has 3 entries, the alphabet 4"
mcd = lambda c, **k: c.mi.montecarlo_information_device(  # noqa: E731
    k.pop("nm", c.nm4), k.pop("pX", c.pX4), k.pop("x", c.j), k.pop("y", c.y), k.pop("B", 1), **k)

MUTUAL_INFORMATION = [
    ("which_mask-two", lambda c: c.mi.which_mask([1, 1]), THREE),
    ("montecarlo-which-two", lambda c: c.mi.montecarlo_information(c.pa4, c.nm4, c.pX4, 4, which=[1, 0]), THREE),
    ("montecarlo-pX", lambda c: c.mi.montecarlo_information(c.pa4, c.nm4, z(3), 4), PX),
    ("montecarlo_device-1d", lambda c: mcd(c, y=c.y[0]), "montecarlo_information_device: y_fi must be a 2-D tensor [S, ld]"),
    ("montecarlo_device-ld63", lambda c: mcd(c, x=c.j63, y=c.y63), MI_BATCH.format(1, 63, S)),
    ("montecarlo_device-B0", lambda c: mcd(c, B=0), MI_BATCH.format(0, LD, S)),
    ("montecarlo_device-B65", lambda c: mcd(c, B=65), MI_BATCH.format(65, LD, S)),
    ("montecarlo_device-S0", lambda c: mcd(c, x=c.j[:0], y=c.y[:0]), MI_BATCH.format(1, LD, 0)),
    ("montecarlo_device-dtype", lambda c: mcd(c, y=c.y32), "y_fi: dtype torch.float32, expected torch.float64"),
    ("montecarlo_device-x-dtype", lambda c: mcd(c, x=c.j.to(c.i32)), "x_fi: dtype torch.int32, expected torch.int64"),
    ("montecarlo_device-x-shape", lambda c: mcd(c, x=c.j[:3]), f"x_fi: shape (3, {LD}), expected ({S}, {LD})"),
    ("montecarlo_device-strided", lambda c: mcd(c, y=c.ystrided), CONTIG.format("y_fi")),
    ("montecarlo_device-cpu", lambda c: mcd(c, y=c.ycpu), GPU.format("y_fi")),
    ("montecarlo_device-which-two", lambda c: mcd(c, which=[1, 1]), THREE),
    ("montecarlo_device-pX", lambda c: mcd(c, pX=z(3)), PX),
    ("montecarlo_device-out-shape", lambda c: mcd(c, out=c.t((2, LD))), f"out: shape (2, {LD}), expected (3, {LD})"),
    ("montecarlo_device-terms-shape", lambda c: mcd(c, terms=c.t((3, S, 2 * LD))),
     f"terms: shape (3, {S}, {2 * LD}), expected (3, {S}, {LD})"),
    ("base_arg_array-pX", lambda c: c.mi.mutual_information_base_scheme_arg_array(z(3), c.nm4, z(3)), PX),
    ("base_arg-pX", lambda c: c.mi.mutual_information_base_scheme_arg(0.5, c.nm4, z(5)),
     "p_Xhat has 5 entries, the alphabet 4"),
    ("quad_batch-kind", lambda c: c.mi.mutual_information_quad_batch("x", [c.nm4]), KIND),
    ("quad_batch-kind-bool", lambda c: c.mi.mutual_information_quad_batch(True, [c.nm4]),
     "kind must be 'base' or 'X_Y' (0 or 1), got True"),
    ("quad_batch-limit", lambda c: c.mi.mutual_information_quad_batch("X_Y", [c.nm4], limit=0), LIMIT),
    ("quad_batch-mixed-bps", lambda c: c.mi.mutual_information_quad_batch("X_Y", [c.nm4, c.nm2]),
     "the mappers of one batch must share bit_per_symbol (mapper 1 has 1, mapper 0 2)"),
    ("quad_batch-no-pX", lambda c: c.mi.mutual_information_quad_batch("base", [c.nm4]),
     "the base-scheme integrals need p_Xhats"),
    ("quad_batch-pX-rows", lambda c: c.mi.mutual_information_quad_batch("base", [c.nm4, c.nm4], [c.pX4]),
     "p_Xhats has 1 rows for 2 mappers"),
    ("quad_batch-pX-length", lambda c: c.mi.mutual_information_quad_batch("base", [c.nm4], [z(3)]),
     "p_Xhats[0] has 3 entries, the alphabet 4"),
    ("quad_batch-cfg-dtype", lambda c: c.mi.mutual_information_quad_batch("X_Y", [c.nm4], sign_configs=z((1, 4))),
     "sign_configs must be uint8 of shape (1, 4), got float64 (1, 4)"),
    ("quad_batch-cfg-shape", lambda c: c.mi.mutual_information_quad_batch("X_Y", [c.nm4], sign_configs=u8((1, 3))),
     "sign_configs must be uint8 of shape (1, 4), got uint8 (1, 3)"),
    ("quad_batch-cfg-bool-shape", lambda c: c.mi.mutual_information_quad_batch("X_Y", [c.nm4], sign_configs=z(4, bool)),
     "sign_configs must be uint8 of shape (1, 4), got uint8 (4,)"),
    ("quad_rule-kind", lambda c: c.mi.quad_rule("x", c.nm4, 0.0, 1.0), KIND),
    ("quad_rule-intervals", lambda c: c.mi.quad_rule("X_Y", c.nm4, z(3), z(3)),
     "a and b must hold the ends of one or two intervals"),
    ("quad_rule-pX", lambda c: c.mi.quad_rule("base", c.nm4, 0.0, 1.0, z(3)), PX),
    ("quad_rule-cfg", lambda c: c.mi.quad_rule("X_Y", c.nm4, 0.0, 1.0, sign_config=u8(3)),
     "sign_config has 3 entries, the alphabet 4"),
    ("base_scheme-limit", lambda c: c.mi.mutual_information_base_scheme(c.nm4, c.pX4, limit=0), LIMIT),
    ("base_scheme-pX", lambda c: c.mi.mutual_information_base_scheme(c.nm4, z(3)), PX),
    ("X_Y-limit", lambda c: c.mi.mutual_information_X_Y(c.nm4, limit=0), LIMIT),
    ("quad_host-kind", lambda c: c.mi.quad_host(abs, "x", 0.0, 1.0), KIND),
    ("quad_host-limit", lambda c: c.mi.quad_host(abs, "base", 0.0, 1.0, limit=0), LIMIT),
]

SIMULATIONS = [
    ("Simulator-mode", lambda c: c.Simulator(c.dec, 1, "x"), "mode must be one of ('softening', 'direct', 'hard')"),
    ("Simulator-demapper", lambda c: c.Simulator(c.dec, 1, demapper="x"), DEMAPPER),
    ("Simulator-bps", lambda c: c.Simulator(c.dec, 2), "V=7 is not a multiple of bit_per_symbol=2"),
    ("Binary-channel", lambda c: c.Binary(c.dec, "x"), "channel must be one of ('biawgn', 'biawgn_hard', 'bsc'), got 'x'"),
    ("Pipeline-demapper", lambda c: c.Pipeline(c.dec, 1, 3.0, 2, demapper="x"), DEMAPPER),
    ("Pipeline-bps", lambda c: c.Pipeline(c.dec, 2, 3.0, 2), "V=7 is not a multiple of bit_per_symbol=2"),
    ("Pipeline-decode-success-short",
     lambda c: c.pipe.decode(c.lap, c.pipe.generate(), success=c.t(1, c.u8)), DEC_B),
    ("Pipeline-decode-final-shape", lambda c: c.pipe.decode(c.lap, c.pipe.generate(), final=c.lap[:6]),
     f"final_fi: shape (6, {LD}), expected ({V}, {LD})"),
    ("Pipeline-demap-out-shape", lambda c: c.pipe.demap(c.pipe.generate(), out=c.t((V - 1, LD))),
     f"out: shape ({V - 1}, {LD}), expected ({V}, {LD})"),
]

TABLE = NOISEMAPPER + DECODER + MATRIX + MUTUAL_INFORMATION + SIMULATIONS


@pytest.mark.parametrize("call,message", [pytest.param(f, m, id=i) for i, f, m in TABLE])
def test_bad_call_raises(c, call, message):
    with pytest.raises(ValueError) as e:
        call(c)
    assert type(e.value) is ValueError and str(e.value) == message
