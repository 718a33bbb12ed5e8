"""omega_gpu._marshal: the layout, dtype, state and allocation rules every facade shares, pinned on CPU
torch tensors and numpy arrays. Nothing here calls the library or opens a device (utility_engine does, and
the facades' GPU tests construct through it).

The device rule: a [F, n] tensor is read in place exactly when stride(1) == 1 and (F <= 1 or stride(0) >= 1);
the reported row stride is stride(0) for F > 1 and n otherwise. Host input comes back C-contiguous with row
stride n.
"""
import numpy as np
import pytest
import torch

from omega_gpu import _marshal as M

MSG = "the facade's own message"
STATE_LEN = 7


def dev_rows(x, audio=True):
    """(array, row stride, f64 flag) of a device-side operand; the pointer is checked against the array."""
    x, ptr, stride, f64 = M.rows(x, True, MSG, audio=audio)
    assert ptr == x.data_ptr()
    return x, stride, f64


def host_rows(x, audio=True):
    x, ptr, stride, f64 = M.rows(x, False, MSG, audio=audio)
    assert ptr == x.ctypes.data
    return x, stride, f64


def test_unfold_view_is_read_in_place():
    stream = torch.arange(192, dtype=torch.float32)
    view = stream.unfold(0, 64, 16)
    assert tuple(view.shape) == (9, 64)
    x, stride, f64 = dev_rows(view)
    assert x.data_ptr() == stream.data_ptr() and tuple(x.stride()) == (16, 1)
    assert (stride, f64) == (16, 0)


def test_column_slice_of_wider_rows_is_read_in_place():
    wide = torch.rand(5, 40)
    x, stride, _ = dev_rows(wide[:, :33], audio=False)
    assert x.data_ptr() == wide.data_ptr() and tuple(x.shape) == (5, 33)
    assert stride == 40


def test_transposed_rows_are_copied():
    t = torch.rand(8, 8).t()
    assert t.stride(1) != 1
    x, stride, _ = dev_rows(t)
    assert x.is_contiguous() and x.data_ptr() != t.data_ptr() and torch.equal(x, t)
    assert stride == 8


def test_broadcast_rows_are_copied_but_one_row_is_not():
    row = torch.rand(1, 32)
    four = row.expand(4, 32)
    assert four.stride(0) == 0
    x, stride, _ = dev_rows(four)
    assert x.is_contiguous() and x.data_ptr() != row.data_ptr() and torch.equal(x, four)
    assert stride == 32
    one = row.expand(1, 32)
    x, stride, _ = dev_rows(one)
    assert x.data_ptr() == row.data_ptr()
    assert stride == 32
    # (a single row reports n whatever stride the tensor carries)
    x, stride, _ = dev_rows(torch.rand(3, 64)[1:2, :32])
    assert stride == 32


@pytest.mark.parametrize("empty", [torch.empty(0, 48), np.empty((0, 48), np.float32)], ids=["torch", "numpy"])
def test_no_rows_report_stride_n(empty):
    x, stride, f64 = (dev_rows if M._is_torch(empty) else host_rows)(empty)
    assert tuple(x.shape) == (0, 48) and (stride, f64) == (48, 0)


@pytest.mark.parametrize("given, kept, f64", [("float32", "float32", 0), ("float64", "float64", 1),
                                              ("int16", "float64", 1), ("float16", "float64", 1)])
def test_audio_dtypes(given, kept, f64):
    values = np.arange(-6, 6).reshape(3, 4)
    x, stride, flag = dev_rows(torch.as_tensor(values).to(getattr(torch, given)))
    assert x.dtype == getattr(torch, kept) and flag == f64 and stride == 4
    assert np.array_equal(x.numpy(), values)
    # host: the same dtypes, C-contiguous with row stride n (here from a Fortran-ordered array)
    x, stride, flag = host_rows(np.asfortranarray(values.astype(given)))
    assert x.dtype == np.dtype(kept) and flag == f64 and stride == 4 and x.flags.c_contiguous
    assert np.array_equal(x, values)


def test_spectra_become_float32():
    values = np.arange(12, dtype=np.float64).reshape(3, 4)
    x, stride, flag = dev_rows(torch.as_tensor(values), audio=False)
    assert x.dtype == torch.float32 and (stride, flag) == (4, 0)
    x, stride, flag = host_rows(values[:, ::-1], audio=False)
    assert x.dtype == np.float32 and (stride, flag) == (4, 0) and x.flags.c_contiguous
    assert np.array_equal(x, values[:, ::-1])
    x, _, _ = host_rows([[1, 2], [3, 4]], audio=False)  # (anything numpy converts)
    assert x.dtype == np.float32 and x.shape == (2, 2)


@pytest.mark.parametrize("shape", [(8,), (2, 3, 4)])
def test_operands_that_are_not_2d_raise_the_facades_message(shape):
    for x, dev in ((torch.zeros(shape), True), (np.zeros(shape, np.float32), False)):
        for audio in (True, False):
            with pytest.raises(ValueError, match=MSG):
                M.rows(x, dev, MSG, audio=audio)


def test_two_operands_of_one_call_are_judged_by_the_first():
    """dev comes from the facade's first operand: a CPU tensor beside host spectra is host input."""
    spec, frames = np.zeros((3, 20), np.float32), torch.rand(3, 64, dtype=torch.float64)
    x, _, stride, f64 = M.rows(frames, M._is_torch(spec), M.SPECTRA_FRAMES, audio=True)
    assert isinstance(x, np.ndarray) and (stride, f64) == (64, 1) and np.array_equal(x, frames.numpy())
    with pytest.raises(ValueError, match=r"spectra must be \[F, K\] and frames \[F, m\]"):
        M.rows(frames[0], False, M.SPECTRA_FRAMES, audio=True)


def test_state_blob():
    values = [float(i) for i in range(STATE_LEN)]
    host_like, dev_like = np.zeros(1, np.float32), torch.zeros(1)
    assert M.state_blob(None, host_like, STATE_LEN) is None and M.state_blob(None, dev_like, STATE_LEN) is None
    for given in (values, np.array(values, np.float32), torch.tensor(values, dtype=torch.float32),
                  torch.tensor([v for v in values for _ in range(2)], dtype=torch.float64)[::2]):  # (strided)
        h = M.state_blob(given, host_like, STATE_LEN)
        assert isinstance(h, np.ndarray) and h.dtype == np.float64 and h.flags.c_contiguous
        assert h.tolist() == values
        d = M.state_blob(given, dev_like, STATE_LEN)
        assert M._is_torch(d) and d.dtype == torch.float64 and d.is_contiguous() and d.device == dev_like.device
        assert d.tolist() == values
    for like in (host_like, dev_like):
        with pytest.raises(ValueError, match=f"state must hold {STATE_LEN} values"):
            M.state_blob(values[:-1], like, STATE_LEN)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32])
def test_alloc_follows_the_operand(dtype):
    h = M.alloc(np.zeros(3, np.float64), (4, 5), dtype)
    assert isinstance(h, np.ndarray) and h.shape == (4, 5) and h.dtype == np.dtype(dtype)
    like = torch.zeros(3, dtype=torch.float64)
    d = M.alloc(like, (4, 5), dtype)
    assert M._is_torch(d) and tuple(d.shape) == (4, 5) and d.dtype == getattr(torch, dtype.__name__)
    assert d.device == like.device and d.is_contiguous()
    assert tuple(M.alloc(like, (0, 5), dtype).shape) == (0, 5)


def test_ptr():
    a, t = np.zeros(4, np.float32), torch.zeros(4)
    assert M._ptr(None) is None and M._ptr(a) == a.ctypes.data and M._ptr(t) == t.data_ptr()
    assert M._is_torch(t) and not M._is_torch(a) and not M._is_torch([1.0])
