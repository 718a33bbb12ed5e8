"""What every facade does between its caller's arrays and a libomega.so entry point, once: which memory
an operand lives in, how a [F, n] batch reaches the library without a copy, where outputs are allocated,
and the call itself. Host operands are numpy (or anything numpy converts); device operands are torch
tensors, used only as carriers of device memory. DESIGN.md ("Facade marshalling") states the rules.

Nothing here decides what a facade does with an empty batch, in which order it checks and configures, or
how two operands of one call pair up: those differ per family and stay in the facades. Genre and hip-hop,
whose per-frame host cost these helpers raised measurably, keep their hand-written calls.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _lib as L


def _is_torch(a) -> bool:
    return hasattr(a, "data_ptr") and hasattr(a, "is_cuda")


def _ptr(a) -> Optional[int]:
    if a is None:
        return None
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def rows(x, dev: bool, message: str, audio: bool = False):
    """A [F, n] batch as the library takes it: (the array to pass, its pointer, its row stride in elements,
    the f64 flag). The pointer is taken here, where the side is known; the array keeps the memory alive.

    dev says which side the call runs on -- the facade takes it from its first operand, so that every
    operand of one call is judged alike. audio: float32 and float64 are kept and anything else becomes
    float64; without it everything becomes float32 (spectra).

    Host: C-contiguous, row stride n. Device: the tensor is read in place when its elements are adjacent
    within a row and, for more than one row, the row stride is positive -- overlapping rows (an ``unfold``
    view) and rows of a wider table stay where they are; anything else is copied. The stride of a single
    row is reported as n, whatever the tensor says. A batch that is not 2-D raises ValueError(message)."""
    if dev:
        import torch
        if x.dim() != 2:
            raise ValueError(message)
        if audio:
            if x.dtype not in (torch.float32, torch.float64):
                x = x.double()
        elif x.dtype != torch.float32:
            x = x.float()
        F, n = x.shape
        if x.stride(1) != 1 or (F > 1 and x.stride(0) < 1):
            x = x.contiguous()
        return x, x.data_ptr(), (x.stride(0) if F > 1 else n), int(audio and x.dtype == torch.float64)
    if audio:
        x = np.asarray(x)
        x = np.ascontiguousarray(x if x.dtype in (np.float32, np.float64) else x.astype(np.float64))
    else:
        x = np.ascontiguousarray(x, np.float32)
    if x.ndim != 2:
        raise ValueError(message)
    return x, x.ctypes.data, x.shape[1], int(audio and x.dtype == np.float64)


# the calls that take spectra [F, K] beside frames [F, m] share these two refusals
MIXED_SIDES = "spectra and frames must both be device tensors or both host arrays"
SPECTRA_FRAMES = "spectra must be [F, K] and frames [F, m]"


def alloc(like, shape, dtype):
    """An uninitialised output beside `like`, an operand as rows() returns it (a numpy array or a tensor): a
    numpy array, or a tensor on its device. dtype is np.float32, np.float64 or np.int32."""
    if isinstance(like, np.ndarray):
        return np.empty(shape, dtype)
    import torch
    return torch.empty(shape, dtype=getattr(torch, dtype.__name__), device=like.device)


def state_blob(state, like, length: int):
    """A stream's optional state beside the input `like`: None, or `length` contiguous float64 values (a
    tensor on the input's device, or numpy; a tensor handed to a host call is read back)."""
    if state is None:
        return None
    if _is_torch(like):
        import torch
        state = torch.as_tensor(state, dtype=torch.float64, device=like.device).contiguous()
        size = state.numel()
    else:
        if _is_torch(state):
            state = state.detach().cpu().numpy()
        state = np.ascontiguousarray(state, np.float64)
        size = state.size
    if size != length:
        raise ValueError(f"state must hold {length} values")
    return state


def call(eng, fn, like, *args, bind: bool = True) -> None:
    """fn(context, *args, mem), checked, with mem from where `like` lives (an operand as rows() returns it: a
    numpy array or a tensor). For a tensor the call is enqueued on torch's current stream of its device
    (bind=False: a call that reads no device memory)."""
    dev = not isinstance(like, np.ndarray)
    if dev and bind:
        eng._bind_stream(like)
    eng._check(fn(eng._ctx, *args, L.MEM_DEVICE if dev else L.MEM_HOST))
