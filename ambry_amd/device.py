"""Device-resident batch API over torch-allocated HBM (thin layer on the C ABI).

Torch is only plumbing here: it allocates HBM and provides the stream; every
CRC is computed by libambrycrc's gfx950 kernels via ``ambrycrc_batch_dev`` /
``ambrycrc_verify_dev``. Offsets/lengths are int64 device tensors (uint64 in
the ABI), CRCs are int32 device tensors holding the uint32 bit patterns
(``.view(torch.uint32)`` / numpy ``.view(np.uint32)`` to read them).
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._args import dev_tensor, host_buffer, message_batch, ptr, stream_handle, workspace as _workspace
from ._args import torch as _torch
from ._lib import check, lib
from .abi import (HARD_DELETE_INFO, MESSAGE_INFO, MSG_BAD_INFO, NO_MESSAGE, RECOVER_RESULT,  # noqa: F401
                  UNIQUE_ID_BYTES, Shard)


def init(device: int = 0) -> None:
    check(lib().ambrycrc_init(device), f"ambrycrc_init({device})")


def _check_batch(base, off, length, crc=()):
    """n after checking a CRC batch: base uint8, off and len int64[n], the (name, tensor) pairs of crc int32 or
    uint32[n] or None, all contiguous CUDA tensors on base's device."""
    torch = _torch()
    dev_tensor("base", base, torch.uint8)
    n = dev_tensor("off", off, torch.int64, like=base).numel()
    dev_tensor("len", length, torch.int64, n, base)
    for name, t in crc:
        dev_tensor(name, t, (torch.int32, torch.uint32), n, base, optional=True)
    return n


def crc32_batch(base, off, length, crc_in=None, out=None, workspace=None, stream=None):
    """out[i] = crc32(crc_in[i] or 0, base[off[i]:off[i]+len[i]]) for every chunk i (on the GPU).
    out may be crc_in itself (an in-place continuation)."""
    n = _check_batch(base, off, length, (("crc_in", crc_in), ("out", out)))
    if out is None:
        out = _torch().empty(n, dtype=_torch().int32, device=base.device)
    ws, ws_bytes = _workspace(workspace, base)
    check(lib().ambrycrc_batch_dev(ptr(base), ptr(off), ptr(length), ptr(crc_in), ptr(out), n, ws, ws_bytes,
                                   stream_handle(stream)), "ambrycrc_batch_dev")
    return out


def crc32_verify(base, off, length, expected, crc_in=None, out=None, stream=None, mismatch=None,
                 count=True):
    """Returns (crc int32[n], mismatch uint8[n], mismatch_count int32[1] or None) computed on the GPU.
    mismatch: optional preallocated uint8[n]; count=False skips the counter (and its zeroing)."""
    torch = _torch()
    n = _check_batch(base, off, length, (("crc_in", crc_in), ("out", out), ("expected", expected)))
    if expected is None:
        raise TypeError("expected is required")
    dev_tensor("mismatch", mismatch, torch.uint8, n, base, optional=True)
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=base.device)
    if mismatch is None:
        mismatch = torch.empty(n, dtype=torch.uint8, device=base.device)
    count = torch.zeros(1, dtype=torch.int32, device=base.device) if count else None
    check(lib().ambrycrc_verify_dev(ptr(base), ptr(off), ptr(length), ptr(crc_in), ptr(expected), ptr(out),
                                    ptr(mismatch), ptr(count), n, None, 0, stream_handle(stream)),
          "ambrycrc_verify_dev")
    return out, mismatch, count


def fill_random(buf, seed: int, stream_off: int = 0, stream=None) -> None:
    """Deterministic splitmix64 bytes (same stream as oracle_fill_splitmix)."""
    dev_tensor("buf", buf, _torch().uint8)
    check(lib().ambrycrc_fill_random_dev(ptr(buf), buf.numel(), seed & (2**64 - 1), stream_off,
                                         stream_handle(stream)), "ambrycrc_fill_random_dev")


def _host_chunks(chunks, crc_in):
    n = len(chunks)
    ptrs = (ctypes.c_void_p * n)()
    lens = (ctypes.c_uint64 * n)()
    for i, c in enumerate(chunks):
        if isinstance(c, tuple):
            ptrs[i], lens[i] = c
        else:
            ptrs[i], lens[i] = c.data_ptr(), c.numel()
    cin = None
    if crc_in is not None:
        cin = (ctypes.c_uint32 * n)(*[int(x) & 0xFFFFFFFF for x in crc_in])
    return n, ptrs, lens, cin


def crc32_batch_host(chunks, device: int = 0, pinned: bool = False, crc_in=None):
    """CRC of host buffers through pinned staging + hipMemcpyAsync (PCIe-inclusive path).

    ``chunks``: sequence of objects exposing ``data_ptr()``/``numel()`` (uint8
    CPU tensors) or (address, length) tuples.
    """
    n, ptrs, lens, cin = _host_chunks(chunks, crc_in)
    out = (ctypes.c_uint32 * n)()
    check(lib().ambrycrc_batch_host(ptrs, lens, cin, out, n, device, 1 if pinned else 0), "ambrycrc_batch_host")
    return list(out)


def crc32_batch_multi(chunks, devices, pinned: bool = False, crc_in=None):
    """ambrycrc_batch_multi: host chunks split by bytes over ``devices`` (one host thread each)."""
    n, ptrs, lens, cin = _host_chunks(chunks, crc_in)
    out = (ctypes.c_uint32 * n)()
    devs = (ctypes.c_int * len(devices))(*devices)
    check(lib().ambrycrc_batch_multi(ptrs, lens, cin, out, n, devs, len(devices), 1 if pinned else 0),
          "ambrycrc_batch_multi")
    return list(out)


def set_variant(device: int, variant: int) -> None:
    check(lib().ambrycrc_set_variant(device, variant), "ambrycrc_set_variant")


def get_variant(device: int = 0) -> int:
    return check(lib().ambrycrc_get_variant(device), "ambrycrc_get_variant")


def set_region_mode(device: int, mode) -> None:
    """Message verify form (ambrycrc_set_region_mode): 2 = region mode in two passes (the
    default), 1 / True = region mode in one pass, 0 / False = CRC jobs through the batch engine.
    The transform's one-pass fast path runs whenever region mode is on (1 or 2)."""
    m = int(mode) if not isinstance(mode, bool) else (1 if mode else 0)
    check(lib().ambrycrc_set_region_mode(device, m), "ambrycrc_set_region_mode")


def get_region_mode(device: int = 0) -> int:
    return check(lib().ambrycrc_get_region_mode(device), "ambrycrc_get_region_mode")


def last_message_mode(device: int = 0) -> int:
    """The form the device's last message verify took: 0 jobs, 1 region one-pass, 2 region two-pass
    (-1: none yet); ambrycrc_last_message_mode."""
    return lib().ambrycrc_last_message_mode(device)


def last_transform_path(device: int = 0) -> int:
    """The path the device's last transform took: 1 the one-pass fast path, 0 the general path
    (-1: none yet); ambrycrc_last_transform_path."""
    return lib().ambrycrc_last_transform_path(device)


def set_transform_verdict(device: int, host: bool) -> int:
    """How the transform learns whether its fast path took the batch (ambrycrc_set_transform_verdict):
    False = on the device, the call stays asynchronous (the default); True = read back by the
    calling thread (one stream synchronization, no gated dispatches). Returns the previous value."""
    return check(lib().ambrycrc_set_transform_verdict(device, 1 if host else 0), "ambrycrc_set_transform_verdict")


def set_put_stream_max(device: int, nbytes: int) -> int:
    """Serialize copy mode streams messages of at most nbytes (ambrycrc_set_put_stream_max; 6144 the default,
    0 = every message through the job path). Returns the previous value."""
    return check(lib().ambrycrc_set_put_stream_max(device, int(nbytes)), "ambrycrc_set_put_stream_max")


HOST_AUTO, HOST_GPU, HOST_CPU = 0, 1, 2


def set_host_policy(device: int, policy: int) -> int:
    """Host-resident dispatch of the *_host entries (ambrycrc_set_host_policy): HOST_AUTO (the
    default: the CPU leg for pageable bytes when the CPU threads beat the GPU host path), HOST_GPU,
    HOST_CPU. Returns the previous policy."""
    return check(lib().ambrycrc_set_host_policy(device, int(policy)), "ambrycrc_set_host_policy")


def host_rates(device: int = 0) -> dict:
    """The rates the auto policy compares (ambrycrc_host_rates) and the leg it takes for pageable bytes."""
    c, g, t = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    leg = check(lib().ambrycrc_host_rates(device, ctypes.byref(c), ctypes.byref(g), ctypes.byref(t)),
                "ambrycrc_host_rates")
    return {"cpu_gibps": c.value, "gpu_gibps": g.value, "cpu_threads": t.value, "auto_leg": "gpu" if leg else "cpu"}


def set_host_cpu_threads(device: int, threads: int) -> int:
    """The CPU leg's thread budget on `device` (-1: the process's; 0: the default, half this process's CPU
    share) -- ambrycrc_set_host_cpu_threads. Returns the previous setting (0 = default)."""
    return check(lib().ambrycrc_set_host_cpu_threads(device, int(threads)), "ambrycrc_set_host_cpu_threads")


def host_calibrate(device: int = -1) -> float:
    """Calibrates the CPU leg at `device`'s budget now (ambrycrc_host_calibrate); returns its GiB/s."""
    r = ctypes.c_double()
    check(lib().ambrycrc_host_calibrate(device, ctypes.byref(r)), "ambrycrc_host_calibrate")
    return r.value


def host_msg_rates(device: int = 0, op: str = "verify") -> dict:
    """The rates auto compares for the host message entries (op "verify" / "transform";
    ambrycrc_host_msg_rates) and the leg it takes for pageable bytes."""
    c, g = ctypes.c_double(), ctypes.c_double()
    leg = check(lib().ambrycrc_host_msg_rates(device, {"verify": 0, "transform": 1}[op], ctypes.byref(c),
                                              ctypes.byref(g)), "ambrycrc_host_msg_rates")
    return {"cpu_gibps": c.value, "gpu_gibps": g.value, "auto_leg": "gpu" if leg else "cpu"}


def last_host_path(device: int = 0) -> int:
    """The leg the device's last host call took: 0 CPU, 1 GPU (-1: none yet)."""
    return lib().ambrycrc_last_host_path(device)


def last_host_slabs(device: int = 0) -> dict:
    """The host path's staging geometry and what the device's last GPU-leg host call staged
    (ambrycrc_last_host_slabs): slab_bytes, slab_chunks, slab_msgs, xform_out_bytes, and the call's
    slabs (committed) and oversize (messages through the oversize path) counts."""
    info = (ctypes.c_uint64 * 6)()
    check(lib().ambrycrc_last_host_slabs(device, info), "ambrycrc_last_host_slabs")
    return dict(zip(("slab_bytes", "slab_chunks", "slab_msgs", "xform_out_bytes", "slabs", "oversize"),
                    [int(x) for x in info]))


def set_grid(device: int, workgroups: int) -> None:
    check(lib().ambrycrc_set_grid(device, workgroups), "ambrycrc_set_grid")


def set_window(device: int, nbytes: int) -> None:
    """Sweep rounds of at most nbytes (0 = one round); see ambrycrc_set_window."""
    check(lib().ambrycrc_set_window(device, nbytes), "ambrycrc_set_window")


def grid_size(device: int = 0) -> int:
    return lib().ambrycrc_grid_size(device)


def timing_enable(device: int, enable: bool = True) -> None:
    check(lib().ambrycrc_timing_enable(device, 1 if enable else 0), "ambrycrc_timing_enable")


def timing_collect(device: int = 0):
    """(sum of sweep-kernel ms, launches) since the last collect (HIP events on the launch stream)."""
    ms = ctypes.c_double()
    cnt = ctypes.c_int()
    check(lib().ambrycrc_timing_collect(device, ctypes.byref(ms), ctypes.byref(cnt)), "ambrycrc_timing_collect")
    return ms.value, cnt.value


def timing_collect_each(device: int = 0, cap: int = 4096):
    """Per-launch sweep-kernel durations (ms, launch order) since the last collect."""
    buf = (ctypes.c_float * cap)()
    cnt = ctypes.c_int()
    check(lib().ambrycrc_timing_collect_each(device, buf, cap, ctypes.byref(cnt)), "ambrycrc_timing_collect_each")
    return [buf[i] for i in range(min(cap, cnt.value))]


def workspace_bytes(n: int) -> int:
    """Bytes of caller workspace ambrycrc_batch_dev needs for n chunks."""
    return lib().ambrycrc_workspace_bytes(n)


def messages_workspace_bytes(m: int) -> int:
    return lib().ambrycrc_messages_workspace_bytes(m)


def verify_messages(region, msg_off, stream=None, want_end: bool = True):
    """GPU verify of every CRC of the messages starting at msg_off (int64 CUDA tensor) in `region`.

    Returns (status int32[m] of AMBRYCRC_MSG_* bits, msg_end int64[m] or None).
    """
    torch = _torch()
    m = message_batch(region, msg_off)
    status = torch.empty(m, dtype=torch.int32, device=region.device)
    end = torch.empty(m, dtype=torch.int64, device=region.device) if want_end else None
    check(lib().ambrycrc_verify_messages_dev(ptr(region), region.numel(), ptr(msg_off), m, ptr(status),
                                             ptr(end), None, 0, stream_handle(stream)),
          "ambrycrc_verify_messages_dev")
    return status, end


def hard_delete_workspace_bytes(m: int) -> int:
    """Bytes of caller workspace ambrycrc_hard_delete_messages_dev needs for m messages."""
    return lib().ambrycrc_hard_delete_workspace_bytes(m)


def hard_delete_messages(region, msg_off, recovery=None, plan_only: bool = False, stream=None, workspace=None):
    """GPU hard delete, in place, of the PUT messages starting at msg_off (int64 CUDA tensor) in `region`
    (ambrycrc_hard_delete_messages_dev): each clean PUT's user-metadata and blob records get zero bodies and
    fresh CRCs. recovery: the `info` of an earlier plan_only call (uint8[m, 32] CUDA tensor; rows whose
    header_version is 0 mean "no recovery info") -- the record CRCs are then not read. plan_only: every
    check, no write.

    Returns (status int32[m] of AMBRYCRC_MSG_* bits, 0 = hard-deleted; info uint8[m, 32] CUDA tensor:
    rows of HARD_DELETE_INFO, zero for a refused message)."""
    torch = _torch()
    m = message_batch(region, msg_off)
    dev_tensor("recovery", recovery, torch.uint8, m, region, optional=True, unit=32)
    status = torch.empty(m, dtype=torch.int32, device=region.device)
    info = torch.empty((m, 32), dtype=torch.uint8, device=region.device)
    ws, ws_bytes = _workspace(workspace, region)
    check(lib().ambrycrc_hard_delete_messages_dev(ptr(region), region.numel(), ptr(msg_off), m, ptr(recovery),
                                                  1 if plan_only else 0, ptr(status), ptr(info), ws, ws_bytes,
                                                  stream_handle(stream)),
          "ambrycrc_hard_delete_messages_dev")
    return status, info


def hard_delete_message_cpu(region, off: int, recovery=None, plan_only: bool = False):
    """ambrycrc_hard_delete_message_cpu: the same for the one message at `off` of a region in host memory,
    in place (a writable numpy uint8 array or bytearray). recovery: a HARD_DELETE_INFO record (or None).
    Returns (status, info: a HARD_DELETE_INFO record, zero when refused)."""
    _keep, base, nbytes = host_buffer("region", region, writable=True)
    rec = None
    if recovery is not None:
        rec = np.zeros(1, dtype=HARD_DELETE_INFO)
        rec[0] = recovery
    info = np.zeros(1, dtype=HARD_DELETE_INFO)
    status = ctypes.c_uint32()
    check(lib().ambrycrc_hard_delete_message_cpu(base, nbytes, off, None if rec is None else rec.ctypes.data,
                                                 1 if plan_only else 0, ctypes.byref(status), info.ctypes.data),
          "ambrycrc_hard_delete_message_cpu")
    return status.value, info[0]


def verify_trailed(base, off, length, stream=None):
    """CRC-trailered items on the GPU: item i = base[off[i]:off[i]+len[i]] ends in the big-endian
    8-B CRC of the bytes before it. Returns (mismatch uint8[n], count int32[1])."""
    torch = _torch()
    n = _check_batch(base, off, length)
    mismatch = torch.empty(n, dtype=torch.uint8, device=base.device)
    count = torch.zeros(1, dtype=torch.int32, device=base.device)
    check(lib().ambrycrc_verify_trailed_dev(ptr(base), ptr(off), ptr(length), ptr(mismatch), ptr(count), n,
                                            None, 0, stream_handle(stream)),
          "ambrycrc_verify_trailed_dev")
    return mismatch, count


def verify_trailed_host(buffers, device: int = 0, pinned: bool = False):
    """The same over host buffers (bytes-likes, e.g. whole files): returns a list of bools, True =
    the trailer does not match (IndexSegment.checkDataIntegrityInByteBufferWithCRC is False)."""
    bufs = [host_buffer("buffers[%d]" % i, b) for i, b in enumerate(buffers)]
    n = len(bufs)
    ptrs = (ctypes.c_void_p * n)(*[b[1] or None for b in bufs])
    lens = (ctypes.c_uint64 * n)(*[b[2] for b in bufs])
    mism = (ctypes.c_uint8 * n)()
    check(lib().ambrycrc_verify_trailed_host(ptrs, lens, mism, n, device, 1 if pinned else 0),
          "ambrycrc_verify_trailed_host")
    return [bool(x) for x in mism]


def verify_messages_host(region, msg_off, device: int = 0, pinned: bool = False):
    """verify_messages for a region in host memory (bytes, numpy uint8, or a CPU uint8 tensor;
    pinned=True for a hipHostMalloc'd / pin_memory() buffer). Returns (status uint32[m],
    msg_end uint64[m]) as numpy arrays."""
    _keep, base, nbytes = host_buffer("region", region)
    offs = np.ascontiguousarray(np.asarray(msg_off, dtype=np.uint64))
    m = len(offs)
    status = np.zeros(m, dtype=np.uint32)
    end = np.zeros(m, dtype=np.uint64)
    check(lib().ambrycrc_verify_messages_host(
        base, nbytes, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), m,
        status.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), end.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
        device, 1 if pinned else 0), "ambrycrc_verify_messages_host")
    return status, end


def chain_messages_host(region: bytes, start: int = 0, max_messages: int = 1 << 20):
    """Offsets of consecutive messages from `start` in a host buffer (BlobStoreRecovery's hop)."""
    _keep, base, nbytes = host_buffer("region", region)  # no copy for bytes, mmaps and uint8 arrays
    offs = np.zeros(max_messages, dtype=np.uint64)
    n = lib().ambrycrc_chain_messages_host(base, nbytes, start, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                           max_messages)
    return [int(x) for x in offs[:n]]


# ------------------------------------------------ log-region recovery on the device

def chain_workspace_bytes(region_len: int, max_messages: int) -> int:
    """Bytes of caller workspace ambrycrc_chain_messages_dev needs."""
    return lib().ambrycrc_chain_workspace_bytes(region_len, max_messages)


def recover_workspace_bytes(region_len: int, max_messages: int) -> int:
    """Bytes of caller workspace ambrycrc_recover_messages_dev needs."""
    return lib().ambrycrc_recover_workspace_bytes(region_len, max_messages)


def chain_messages(region, start: int = 0, max_messages: int = 1 << 20, stream=None, workspace=None, out=None):
    """The message chain of a log region in HBM, found on the GPU (ambrycrc_chain_messages_dev): no host
    synchronisation. out: (msg_off, result) of an earlier call, to write into (a captured graph's outputs).

    Returns (msg_off int64[max_messages] CUDA tensor: the starts in log order, then -1 (UINT64_MAX);
    result uint8[32] CUDA tensor: one RECOVER_RESULT record -- recover_result(result) reads it)."""
    torch = _torch()
    dev_tensor("region", region, torch.uint8)
    msg_off, result = out if out is not None else (
        torch.empty(max_messages, dtype=torch.int64, device=region.device),
        torch.empty(32, dtype=torch.uint8, device=region.device))
    ws, ws_bytes = _workspace(workspace, region)
    check(lib().ambrycrc_chain_messages_dev(ptr(region), region.numel(), start, max_messages, ptr(msg_off),
                                            ptr(result), ws, ws_bytes, stream_handle(stream)),
          "ambrycrc_chain_messages_dev")
    return msg_off, result


def recover_messages(region, start: int = 0, max_messages: int = 1 << 20, stream=None, workspace=None, out=None):
    """BlobStoreRecovery.recover over region[start:] on the GPU (ambrycrc_recover_messages_dev): the chain, the
    verify of every chained message, the MessageInfo fields. No host synchronisation. out: the four tensors of
    an earlier call, to write into.

    Returns (msg_off int64[max_messages], info uint8[max_messages, 48]: rows of MESSAGE_INFO, zero unless the
    status is 0; status int32[max_messages]; result uint8[32]: one RECOVER_RESULT record), CUDA tensors."""
    torch = _torch()
    dev_tensor("region", region, torch.uint8)
    msg_off, info, status, result = out if out is not None else (
        torch.empty(max_messages, dtype=torch.int64, device=region.device),
        torch.empty((max_messages, 48), dtype=torch.uint8, device=region.device),
        torch.empty(max_messages, dtype=torch.int32, device=region.device),
        torch.empty(32, dtype=torch.uint8, device=region.device))
    ws, ws_bytes = _workspace(workspace, region)
    check(lib().ambrycrc_recover_messages_dev(ptr(region), region.numel(), start, max_messages, ptr(msg_off),
                                              ptr(info), ptr(status), ptr(result), ws, ws_bytes,
                                              stream_handle(stream)),
          "ambrycrc_recover_messages_dev")
    return msg_off, info, status, result


def recover_result(result):
    """The RECOVER_RESULT record of a result tensor (copies it to the host: synchronises)."""
    return np.frombuffer(result.cpu().numpy().tobytes(), dtype=RECOVER_RESULT)[0]


def recover_messages_cpu(region, start: int = 0, max_messages: int = 1 << 20):
    """ambrycrc_recover_messages_cpu: the same over a region in host memory (bytes-like or numpy uint8).
    Returns (msg_off uint64[max_messages], info MESSAGE_INFO[max_messages], status uint32[max_messages],
    result: a RECOVER_RESULT record), numpy."""
    _keep, base, nbytes = host_buffer("region", region)
    n = int(max_messages) if 0 < max_messages < (1 << 31) else 0  # (the entry refuses the others)
    msg_off = np.zeros(n, dtype=np.uint64)
    info = np.zeros(n, dtype=MESSAGE_INFO)
    status = np.zeros(n, dtype=np.uint32)
    res = np.zeros(1, dtype=RECOVER_RESULT)
    check(lib().ambrycrc_recover_messages_cpu(base, nbytes, start, max_messages, msg_off.ctypes.data, info.ctypes.data,
                                              status.ctypes.data, res.ctypes.data),
          "ambrycrc_recover_messages_cpu")
    return msg_off, info, status, res[0]


# ------------------------------------------------ multi-GPU batch + RCCL all-gather (§8e)

def shard_by_bytes(lengths, nshards: int):
    """ambrycrc_shard_by_bytes: contiguous chunk ranges [lo, hi) of about equal bytes per shard."""
    lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.uint64))
    cuts = (ctypes.c_size_t * (nshards + 1))()
    check(lib().ambrycrc_shard_by_bytes(lens.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(lens), nshards,
                                        cuts), "ambrycrc_shard_by_bytes")
    return [(int(cuts[g]), int(cuts[g + 1])) for g in range(nshards)]


def crc32_batch_cpu(chunks, crc_in=None, threads: int = 0):
    """ambrycrc_batch_cpu: per-chunk CRCs of host buffers on `threads` CPU threads (0 = all allowed)."""
    n, ptrs, lens, cin = _host_chunks(chunks, crc_in)
    out = (ctypes.c_uint32 * n)()
    check(lib().ambrycrc_batch_cpu(ptrs, lens, cin, out, n, threads), "ambrycrc_batch_cpu")
    return list(out)


def unique_id() -> bytes:
    """ambrycrc_unique_id: the 128-byte RCCL id rank 0 sends to every rank."""
    buf = (ctypes.c_uint8 * UNIQUE_ID_BYTES)()
    check(lib().ambrycrc_unique_id(buf), "ambrycrc_unique_id")
    return bytes(buf)


class Comm:
    """An ambrycrc_comm (RCCL communicator): Comm.all_devices([0, 1, ...]) for one process driving
    several GPUs, Comm.rank(uid, nranks, rank, device) for one process per GPU."""

    def __init__(self, handle: int, devices):
        self.handle = ctypes.c_void_p(handle)
        self.devices = list(devices)

    @classmethod
    def all_devices(cls, devices):
        devs = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        check(lib().ambrycrc_comm_init_all(devs, len(devices), ctypes.byref(h)), "ambrycrc_comm_init_all")
        return cls(h.value, devices)

    @classmethod
    def rank(cls, uid: bytes, nranks: int, rank: int, device: int):
        if len(uid) != UNIQUE_ID_BYTES:
            raise ValueError(f"unique id must be {UNIQUE_ID_BYTES} bytes")
        buf = (ctypes.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(uid)
        h = ctypes.c_void_p()
        check(lib().ambrycrc_comm_init_rank(buf, nranks, rank, device, ctypes.byref(h)), "ambrycrc_comm_init_rank")
        c = cls(h.value, [device])
        c.rank_id = rank
        return c

    def size(self) -> int:
        return check(lib().ambrycrc_comm_size(self.handle), "ambrycrc_comm_size")

    def destroy(self) -> None:
        if self.handle.value:
            check(lib().ambrycrc_comm_destroy(self.handle), "ambrycrc_comm_destroy")
            self.handle = ctypes.c_void_p()


def _shard(base, off, length, gathered, crc_in=None, stream=None):
    torch = _torch()
    n = _check_batch(base, off, length, (("crc_in", crc_in),))
    dev_tensor("gathered", gathered, (torch.int32, torch.uint32), like=base)
    s = stream if stream is not None else torch.cuda.current_stream(base.device)
    return Shard(base.device.index, base.data_ptr(), off.data_ptr(), length.data_ptr(),
                 None if crc_in is None else crc_in.data_ptr(), n, gathered.data_ptr(), s.cuda_stream)


def crc32_batch_multi_dev(comm: Comm, shards):
    """ambrycrc_batch_dev_multi. shards: one dict per device of comm, in comm order, with keys
    base, off, len, gathered (int32[total chunks] on that device), optional crc_in and stream.
    Every device's `gathered` receives all CRCs (shard order). Asynchronous."""
    arr = (Shard * len(shards))(*[_shard(s["base"], s["off"], s["len"], s["gathered"], s.get("crc_in"),
                                         s.get("stream")) for s in shards])
    total = sum(int(s["off"].numel()) for s in shards)
    for s in shards:
        if s["gathered"].numel() != total:
            raise TypeError(f"gathered must hold all {total} CRCs")
    check(lib().ambrycrc_batch_dev_multi(comm.handle, arr, len(shards)), "ambrycrc_batch_dev_multi")


def crc32_batch_gather(comm: Comm, base, off, length, gathered, counts, crc_in=None, stream=None):
    """ambrycrc_batch_dev_gather: this rank's shard, then the all-gather into `gathered`
    (int32[sum(counts)]). counts: chunks per rank, the same on every rank. Asynchronous."""
    if gathered.numel() != sum(int(c) for c in counts):
        raise TypeError("gathered must hold sum(counts) CRCs")
    sh = _shard(base, off, length, gathered, crc_in, stream)
    cnt = (ctypes.c_uint64 * len(counts))(*[int(c) for c in counts])
    check(lib().ambrycrc_batch_dev_gather(comm.handle, ctypes.byref(sh), cnt), "ambrycrc_batch_dev_gather")
