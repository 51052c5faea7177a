"""The marshalling helpers of qamr._lib and the argument checks of qamr.mutual_information that need no
device: their messages, letter for letter (tests/test_gpu_facade_errors.py pins the same texts through
the public methods)."""
import numpy as np
import pytest
import torch

from qamr import _lib
from qamr import mutual_information as mi


def raises(message, call, *args, **kw):
    with pytest.raises(ValueError) as e:
        call(*args, **kw)
    assert str(e.value) == message


@pytest.mark.parametrize("dtype,c_name", [(np.float64, "double"), (np.int64, "long"), (np.uint8, "unsigned char")])
def test_as_buffer_dtype_message(dtype, c_name):
    bad = np.zeros(3, np.float32)
    raises(f"Buffer dtype mismatch, expected '{c_name}' but got 'float32'", _lib.as_buffer, bad, dtype)
    raises(f"Buffer dtype mismatch, expected '{c_name}' but got 'float32' (word)", _lib.as_buffer, bad, dtype, name="word")
    raises(f"Buffer dtype mismatch, expected '{c_name}' but got 'float32'", _lib.as_buffer, bad, dtype, flat=True)
    good = _lib.as_buffer([dtype(1), dtype(0)], dtype)
    assert good.dtype == dtype and good.tolist() == [1, 0]


def test_as_buffer_views_bool_as_unsigned_char_only():
    flags = np.array([True, False, True])
    got = _lib.as_buffer(flags, np.uint8, name="synd")
    assert got.dtype == np.uint8 and got.tolist() == [1, 0, 1] and np.shares_memory(got, flags)
    raises("Buffer dtype mismatch, expected 'double' but got 'bool'", _lib.as_buffer, flags, np.float64)
    raises("Buffer dtype mismatch, expected 'long' but got 'bool' (e_to_v)", _lib.as_buffer, flags, np.int64, name="e_to_v")


def test_as_buffer_one_dimension_or_ravel():
    a = np.arange(12.0).reshape(3, 4)
    raises("Buffer has wrong number of dimensions (expected 1, got 2) (lappr)", _lib.as_buffer, a, np.float64, name="lappr")
    raises("Buffer has wrong number of dimensions (expected 1, got 0)", _lib.as_buffer, np.float64(1.0), np.float64)
    flat = _lib.as_buffer(a.T, np.float64, flat=True)
    assert flat.shape == (12,) and flat.flags.c_contiguous and flat.tolist() == a.T.ravel().tolist()
    strided = _lib.as_buffer(np.arange(10.0)[::2], np.float64)
    assert strided.flags.c_contiguous and strided.tolist() == [0.0, 2.0, 4.0, 6.0, 8.0]


@pytest.mark.parametrize("B,ld", [(0, 64), (65, 64), (-1, 64), (1, 63), (1, 0 + 32), (200, 192)])
def test_check_batch_message(B, ld):
    for what in ("decode_device", "bob_map_device", "eval_syndrome_device"):
        raises(f"{what}: need ld % 64 == 0 and 0 < B <= ld (B={B}, ld={ld})", _lib.check_batch, B, ld, what)


def test_check_batch_accepts_the_whole_range():
    for B, ld in ((1, 64), (64, 64), (65, 128), (4096, 4096)):
        _lib.check_batch(B, ld, "x")


def test_check_2d_message():
    raises("demap_device: n_fi must be a 2-D tensor [S, ld]", _lib.check_2d, torch.zeros(4), "demap_device", "n_fi", "[S, ld]")
    raises("decode_device: lappr_fi must be a 2-D tensor [V, ld]", _lib.check_2d, np.zeros((2, 2)), "decode_device",
           "lappr_fi", "[V, ld]")
    assert tuple(_lib.check_2d(torch.zeros((3, 64)), "x", "y", "[S, ld]")) == (3, 64)


def test_check_tensor_refuses_cpu_and_strided_tensors():
    t = torch.zeros((4, 64), dtype=torch.float64)
    raises("y_fi: must be a GPU tensor", _lib.check_tensor, t, "y_fi", (4, 64), torch.float64, 0)
    raises("y_fi: must be a GPU tensor", _lib.check_tensor, t[:, ::2], "y_fi")
    raises("y_fi: dtype torch.float64, expected torch.int64", _lib.check_tensor, t, "y_fi", (4, 64), torch.int64)
    raises("y_fi: shape (4, 64), expected (4, 128)", _lib.check_tensor, t, "y_fi", (4, 128), torch.float64)
    raises("y_fi: expected a torch tensor, got ndarray", _lib.check_tensor, np.zeros(3), "y_fi")
    # a strided tensor in host memory is refused for where it lives; the stride message itself needs a
    # GPU tensor (the "-strided" rows of tests/test_gpu_facade_errors.py)
    raises("y_fi: must be a GPU tensor", _lib.check_tensor, t[:, ::2], "y_fi", (4, 32), torch.float64)


def test_dptr_and_stream_arg_pass_none_through():
    assert _lib.dptr(None) is None
    t = torch.zeros(4)
    assert _lib.dptr(t).value == t.data_ptr()


def test_which_mask():
    assert [mi.which_mask(w) for w in ([1, 0, 0], [0, 1, 0], [0, 0, 1], np.ones(3, np.uint8), [[1, 1], [0, 9]])] == \
        [1, 2, 4, 7, 3]
    raises("which must hold three flags", mi.which_mask, [1, 1])
    raises("which must hold three flags", mi.which_mask, [])


def test_kind_and_limit():
    assert [mi._kind(k) for k in ("base", "X_Y", 0, 1)] == [0, 1, 0, 1]
    for bad in ("x", 2, True, None):
        raises(f"kind must be 'base' or 'X_Y' (0 or 1), got {bad!r}", mi._kind, bad)
    assert mi._check_limit(1) == 1 and mi._check_limit(50.0) == 50
    raises("limit must be at least 1, got 0", mi._check_limit, 0)
    raises("limit must be at least 1, got -3", mi._check_limit, -3)


def test_check_pX_message():
    assert mi._check_pX([[0.25, 0.25], [0.25, 0.25]], 4).tolist() == [0.25] * 4
    raises("p_Xhat has 3 entries, the alphabet 4", mi._check_pX, np.zeros(3), 4)
    raises("p_Xhats[2] has 5 entries, the alphabet 4", mi._check_pX, np.zeros(5), 4, "p_Xhats[2]")
