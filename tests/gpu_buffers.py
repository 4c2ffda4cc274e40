"""Device buffers for the GPU tests: a tensor between two 64-byte guards of 0xA5 at a chosen shift from a 64-B
boundary, the checks that the guards (and an input) survived a call, and the host <-> device converters the
tests share. torch is imported inside the functions, so a CPU run collects the modules that import this one."""
import numpy as np

GUARD = 64
FILL = 0xA5


def _u8(data) -> np.ndarray:
    """bytes or any numpy array as a flat uint8 array of its bytes."""
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(data, dtype=np.uint8)
    return np.ascontiguousarray(data).reshape(-1).view(np.uint8)


def guarded(data_or_size, shift: int = 0, size=None):
    """(the whole tensor, the view of `size` bytes in it): 64 guard bytes of 0xA5, `shift` more, the view, 64
    guard bytes. The allocation is 64-aligned (asserted), so the view starts `shift` bytes past a 64-B boundary.
    The view holds the bytes of data_or_size (bytes or a numpy array; an int: that many bytes and no data) and
    0xA5 from there to `size` (default: the data's length)."""
    import torch

    a = np.zeros(0, dtype=np.uint8) if isinstance(data_or_size, (int, np.integer)) else _u8(data_or_size)
    if size is None:
        size = int(data_or_size) if isinstance(data_or_size, (int, np.integer)) else len(a)
    assert len(a) <= size, "%d bytes of data for a view of %d" % (len(a), size)
    whole = torch.full((GUARD + shift + size + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 64 == 0, "the allocation starts at %#x: not 64-B aligned" % whole.data_ptr()
    view = whole[GUARD + shift:GUARD + shift + size]
    if len(a):
        view[:len(a)].copy_(torch.from_numpy(np.array(a, copy=True)))
    return whole, view


def guarded_workspace(nbytes: int):
    """(the whole tensor, the view) of a caller workspace of exactly nbytes between two guards, the workspace
    itself 0xA5 as the guards are: a call must neither rely on what it holds nor write past it."""
    return guarded(int(nbytes))


def assert_guards(whole, view_or_size, shift: int = 0):
    """Both guards of guarded()'s tensor still hold 0xA5 (checked on the device)."""
    n = view_or_size if isinstance(view_or_size, (int, np.integer)) else view_or_size.numel()
    assert bool((whole[:GUARD + shift] == FILL).all()), "guard bytes below the view overwritten"
    assert bool((whole[GUARD + shift + n:] == FILL).all()), "guard bytes past the view overwritten"


def guards_intact(whole, shift: int, size: int) -> np.ndarray:
    """The view's bytes on the host, after checking the guards."""
    h = whole.cpu().numpy()
    for name, g in (("below", h[:GUARD + shift]), ("past", h[GUARD + shift + size:])):
        bad = np.nonzero(g != FILL)[0]
        assert not len(bad), "guard bytes %s the view overwritten: %d of them, the first at guard byte %d" % (
            name, len(bad), bad[0])
    return h[GUARD + shift:GUARD + shift + size]


def assert_untouched(whole, view, data, shift: int = 0):
    """The guards hold and the view still holds `data`: the call changed neither."""
    import torch

    assert_guards(whole, view, shift)
    assert torch.equal(view.cpu(), torch.from_numpy(np.array(_u8(data), copy=True))), "the call changed its input"


def dev(data):
    """bytes or any numpy array -> a uint8 CUDA tensor of its bytes (with a device address even when it has none)."""
    import torch

    a = _u8(data)
    return torch.from_numpy(a.copy()).cuda() if len(a) else torch.zeros(1, dtype=torch.uint8, device="cuda")[:0]


def u64_dev(values):
    """Unsigned 64-bit values (UINT64_MAX included) -> the int64 CUDA tensor the bindings take."""
    import torch

    return torch.from_numpy(np.asarray(values, dtype=np.uint64).reshape(-1).view(np.int64).copy()).cuda()


def host(t, dtype):
    """A device tensor's bytes as a flat numpy array of dtype."""
    return t.cpu().numpy().reshape(-1).view(dtype)
