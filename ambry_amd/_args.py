"""What every wrapper of device.py, messages.py and multi.py does to its arguments before the C call: one check
of a device tensor, one pointer, the stream and workspace handles, one coercion of a host buffer. Private.
Torch stays a deferred import: a CPU-only caller of the *_cpu entries never loads it."""
from __future__ import annotations

import ctypes

import numpy as np


def torch():
    import torch  # deferred: CPU-only tests import the wrappers' modules without a GPU

    return torch


def dev_tensor(name, t, dtype, numel=None, like=None, optional=False, unit=1):
    """`t` if it is a contiguous CUDA tensor of `dtype` (one dtype, a tuple of them, or None for any), of
    numel * unit elements (numel None: a multiple of unit), on the device of `like`; TypeError naming the
    argument otherwise. optional: None passes."""
    if t is None and optional:
        return None
    many = type(dtype) is tuple
    if not (t.is_cuda and (dtype is None or (t.dtype in dtype if many else t.dtype is dtype))
            and t.is_contiguous() and (t.numel() % unit == 0 if numel is None else t.numel() == numel * unit)
            and (like is None or t.device == like.device)):
        kinds = "" if dtype is None else "/".join(str(d)[6:] for d in (dtype if many else (dtype,))) + " "
        count = f" of {numel * unit} elements" if numel is not None else f" of {unit}-element records" * (unit > 1)
        raise TypeError(f"{name} must be a contiguous {kinds}CUDA tensor{count}"
                        + (f" on {like.device}" if like is not None else ""))
    return t


def message_batch(region, msg_off, names=("region", "msg_off")):
    """m after checking a batch of messages (or, by other names, of payloads): a contiguous uint8 CUDA tensor and
    the int64 starts in it, on its device."""
    dev_tensor(names[0], region, torch().uint8)
    return dev_tensor(names[1], msg_off, torch().int64, like=region).numel()


def ptr(t, empty_null=False):
    """The tensor's address for the C ABI; None (and, for the entries that always did so, an empty tensor) is
    NULL."""
    return None if t is None or (empty_null and t.numel() == 0) else ctypes.c_void_p(t.data_ptr())


def stream_handle(stream=None):
    s = stream if stream is not None else torch().cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def workspace(ws, like):
    """(pointer, byte size) of a caller workspace (any dtype: its byte size is what counts)."""
    if ws is None:
        return None, 0
    dev_tensor("workspace", ws, None, like=like)
    return ptr(ws), ws.numel() * ws.element_size()


def host_buffer(name, buf, writable=False):
    """(object to keep alive, address -- 0 when empty --, byte count) of a host buffer: anything with the buffer
    protocol (bytes, bytearray, memoryview, mmap), a uint8 numpy array (copied when it is not contiguous) or a
    contiguous uint8 CPU tensor. writable: the callee writes in place, so a read-only buffer or one that would
    need a copy is refused. TypeError naming the argument."""
    if hasattr(buf, "data_ptr"):
        if buf.is_cuda or buf.element_size() != 1 or not buf.is_contiguous():
            raise TypeError(f"{name} must be a contiguous uint8 CPU tensor")
        return buf, buf.data_ptr() if buf.numel() else 0, buf.numel()
    try:
        arr = buf if isinstance(buf, np.ndarray) else np.frombuffer(buf, dtype=np.uint8)
    except (TypeError, ValueError, AttributeError):
        arr = None
    if arr is None or arr.dtype != np.uint8 or (writable and not (arr.flags.writeable and arr.flags.c_contiguous)):
        raise TypeError(f"{name} must be a {'writable contiguous ' * writable}bytes-like object or uint8 array")
    if not arr.flags.c_contiguous:
        arr = np.ascontiguousarray(arr)
    return arr, arr.ctypes.data if arr.nbytes else 0, arr.nbytes
