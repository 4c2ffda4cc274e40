"""PUT message serialization (the write side of Ambry's message path).

Mirrors PutMessageFormatInputStream (PutMessageFormatInputStream.java:60-124): a message is
described by its store key, optional encryption key, BlobPropertiesSerDe bytes, user metadata
and blob content, plus header version / life version / blob type / compression flag. The bytes
and every CRC trailer are produced by libambrycrc -- on the CPU for one message
(ambrycrc_serialize_put_host), on the GPU for a batch (ambrycrc_serialize_puts_dev).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from ._lib import PutDesc, check, lib

# numpy mirror of struct ambrycrc_put_desc (80 bytes), for descriptor arrays copied to HBM
PUT_DESC_DTYPE = np.dtype([
    ("out_off", "<u8"), ("key_src", "<u8"), ("enckey_src", "<u8"), ("props_src", "<u8"), ("usermeta_src", "<u8"),
    ("blob_src", "<u8"), ("blob_len", "<u8"), ("key_len", "<u4"), ("enckey_len", "<i4"), ("props_len", "<u4"),
    ("usermeta_len", "<u4"), ("life_version", "<i2"), ("blob_type", "<i2"), ("compressed", "u1"),
    ("header_version", "u1"), ("reserved", "u1", (2,))])
assert PUT_DESC_DTYPE.itemsize == ctypes.sizeof(PutDesc) == 80

FIELDS = ("key", "enckey", "props", "usermeta", "blob")


@dataclass
class PutMessage:
    """One PUT: the arguments of PutMessageFormatInputStream's constructor, as bytes."""
    key: bytes                # StoreKey.toBytes()
    props: bytes              # BlobPropertiesSerDe bytes
    usermeta: bytes
    blob: bytes
    enckey: bytes | None = None
    header_version: int = 3   # MessageFormatRecord.headerVersionToUse
    life_version: int = 0
    blob_type: int = 0        # BlobType ordinal (0 = DataBlob)
    compressed: bool = False

    def desc(self, out_off: int = 0, src: dict | None = None) -> PutDesc:
        src = src or {}
        d = PutDesc()
        d.out_off = out_off
        d.key_src, d.enckey_src, d.props_src = src.get("key", 0), src.get("enckey", 0), src.get("props", 0)
        d.usermeta_src, d.blob_src = src.get("usermeta", 0), src.get("blob", 0)
        d.blob_len = len(self.blob)
        d.key_len, d.props_len, d.usermeta_len = len(self.key), len(self.props), len(self.usermeta)
        d.enckey_len = -1 if self.enckey is None else len(self.enckey)
        d.life_version, d.blob_type = self.life_version, self.blob_type
        d.compressed, d.header_version = 1 if self.compressed else 0, self.header_version
        return d


def layout(msg: PutMessage):
    """(message length, {field: offset from the message start}) -- ambrycrc_put_layout."""
    offs = (ctypes.c_uint64 * 5)()
    n = lib().ambrycrc_put_layout(ctypes.byref(msg.desc()), offs)
    if n == 0:
        raise ValueError("invalid PUT descriptor")
    return n, dict(zip(FIELDS, list(offs)))


def serialize_host(msg: PutMessage):
    """(message bytes, [header, enckey, props, usermeta, blob record CRCs]) on the CPU."""
    fields = b"".join([msg.key, msg.enckey or b"", msg.props, msg.usermeta])
    src = {"key": 0, "enckey": len(msg.key), "props": len(msg.key) + len(msg.enckey or b""),
           "usermeta": len(msg.key) + len(msg.enckey or b"") + len(msg.props), "blob": 0}
    n, _ = layout(msg)
    out = ctypes.create_string_buffer(max(n, 1))
    fb = ctypes.create_string_buffer(fields, max(len(fields), 1))
    bb = ctypes.create_string_buffer(msg.blob, max(len(msg.blob), 1))
    crcs = (ctypes.c_uint32 * 5)()
    check(lib().ambrycrc_serialize_put_host(ctypes.byref(msg.desc(0, src)), fb, bb, out, n, crcs),
          "ambrycrc_serialize_put_host")
    return out.raw[:n], list(crcs)


def pack_batch(msgs, out_align: int = 1, field_align: int = 1, gap: int = 0):
    """Host-side packing for ambrycrc_serialize_puts_dev: (descriptor array, fields bytes, blobs
    bytes, message offsets, total output bytes). Fields go back to back (each at field_align),
    blobs likewise, messages at out_align with `gap` spare bytes between them."""
    descs = np.zeros(len(msgs), dtype=PUT_DESC_DTYPE)
    fields, blobs = bytearray(), bytearray()
    offs, pos = [], 0
    for i, m in enumerate(msgs):
        src = {}
        for name in FIELDS[:4]:
            b = getattr(m, name) or b""
            fields += bytes((-len(fields)) % field_align)
            src[name] = len(fields)
            fields += b
        blobs += bytes((-len(blobs)) % field_align)
        src["blob"] = len(blobs)
        blobs += m.blob
        pos += (-pos) % out_align
        offs.append(pos)
        d = m.desc(pos, src)
        descs[i] = np.frombuffer(bytes(d), dtype=PUT_DESC_DTYPE)[0]
        pos += layout(m)[0] + gap
    return descs, bytes(fields), bytes(blobs), offs, pos


def serialize_dev(descs, out, fields=None, blobs=None, msg_len=None, stream=None):
    """ambrycrc_serialize_puts_dev: descs is a uint8 CUDA tensor holding the PUT_DESC_DTYPE array;
    fields / blobs uint8 CUDA tensors or None (bytes already in place in `out`)."""
    import torch

    from .device import _stream_handle

    if descs.dtype != torch.uint8 or not descs.is_cuda or descs.numel() % PUT_DESC_DTYPE.itemsize:
        raise TypeError("descs must be a uint8 CUDA tensor of 80-byte descriptors")
    m = descs.numel() // PUT_DESC_DTYPE.itemsize
    for name, t in (("out", out), ("fields", fields), ("blobs", blobs)):
        if t is not None and (t.dtype != torch.uint8 or not t.is_cuda or t.device != descs.device):
            raise TypeError(f"{name} must be a uint8 CUDA tensor on {descs.device}")
    if msg_len is not None and (msg_len.dtype != torch.int64 or msg_len.numel() != m or not msg_len.is_cuda):
        raise TypeError("msg_len must be an int64 CUDA tensor of m elements")
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    check(lib().ambrycrc_serialize_puts_dev(ptr(descs), m, ptr(fields), ptr(blobs), ptr(out), ptr(msg_len), None, 0,
                                            ctypes.c_void_p(_stream_handle(stream))), "ambrycrc_serialize_puts_dev")


def verify_message_cpu(region, off: int):
    """ambrycrc_verify_message_cpu: (AMBRYCRC_MSG_* status bits, message end or 0) for the message
    at `off` in a host buffer (bytes / bytearray / uint8 numpy array)."""
    buf = np.frombuffer(region, dtype=np.uint8) if not isinstance(region, np.ndarray) else region
    st, end = ctypes.c_uint32(0), ctypes.c_uint64(0)
    check(lib().ambrycrc_verify_message_cpu(buf.ctypes.data_as(ctypes.c_void_p), buf.size, off, ctypes.byref(st),
                                            ctypes.byref(end)), "ambrycrc_verify_message_cpu")
    return st.value, end.value


def transform_message_cpu(region, off: int, header_version: int = 3, life=None, out_cap=None):
    """ambrycrc_transform_message_cpu: (status bits, the re-serialized message or None)."""
    buf = np.frombuffer(region, dtype=np.uint8) if not isinstance(region, np.ndarray) else region
    # default: the ABI's bound (the stored bytes after off + TRANSFORM_GROWTH_MAX), never NO_ROOM
    cap = out_cap if out_cap is not None else out_bound(buf.size - min(off, buf.size), 1)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    st, n = ctypes.c_uint32(0), ctypes.c_uint64(0)
    check(lib().ambrycrc_transform_message_cpu(buf.ctypes.data_as(ctypes.c_void_p), buf.size, off,
                                               -1 if life is None else int(life), header_version,
                                               out.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(n),
                                               ctypes.byref(st)), "ambrycrc_transform_message_cpu")
    return st.value, (out[:n.value].tobytes() if st.value == 0 else None)


# status bits added by the transform (include/ambrycrc.h)
MSG_NOT_PUT = 1 << 10
MSG_BAD_RECORD = 1 << 11
MSG_NO_ROOM = 1 << 12
MSG_NOT_ENCODABLE = 1 << 13

# A transformed message is at most this many bytes longer than the stored one: header V1 -> V3 (+6),
# BlobProperties SerDe V1 -> V5 (+17), Blob_Format_V1 -> V3 head (+3) (AMBRYCRC_TRANSFORM_GROWTH_MAX).
TRANSFORM_GROWTH_MAX = 26


def out_bound(region_len: int, m: int) -> int:
    """ambrycrc_transform_out_bound: an output capacity that never yields MSG_NO_ROOM for m
    messages that share no bytes of a region_len-byte region."""
    return int(lib().ambrycrc_transform_out_bound(region_len, m))


def transform_dev(region, msg_off, header_version: int = 3, life_version=None, out=None, stream=None):
    """ambrycrc_transform_messages_dev -- ValidatingTransformer.transform for a batch of stored
    messages in HBM: every clean PUT re-serialized at `header_version` (and life version
    life_version[i], an int16 CUDA tensor, or the stored one), packed in order into `out` (a uint8
    CUDA tensor; default: out_bound(region bytes, m), enough for every message of a region whose
    messages do not overlap -- TRANSFORM_GROWTH_MAX = 26 B of growth per message).
    Returns (out, out_off int64[m], out_len int64[m], status int32[m])."""
    import torch

    from .device import _stream_handle

    if region.dtype != torch.uint8 or not region.is_cuda:
        raise TypeError("region must be a uint8 CUDA tensor")
    if msg_off.dtype != torch.int64 or not msg_off.is_cuda or not msg_off.is_contiguous() or \
            msg_off.device != region.device:
        raise TypeError("msg_off must be a contiguous int64 CUDA tensor on the region's device")
    m = msg_off.numel()
    if life_version is not None and (life_version.dtype != torch.int16 or life_version.numel() != m
                                     or not life_version.is_cuda or not life_version.is_contiguous()):
        raise TypeError("life_version must be a contiguous int16 CUDA tensor of m elements")
    if out is None:
        out = torch.empty(out_bound(region.numel(), m), dtype=torch.uint8, device=region.device)
    elif out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.device != region.device:
        raise TypeError("out must be a contiguous uint8 CUDA tensor on the region's device")
    out_off = torch.empty(m, dtype=torch.int64, device=region.device)
    out_len = torch.empty(m, dtype=torch.int64, device=region.device)
    status = torch.empty(m, dtype=torch.int32, device=region.device)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    check(lib().ambrycrc_transform_messages_dev(ptr(region), region.numel(), ptr(msg_off), m, ptr(life_version),
                                                header_version, ptr(out), out.numel(), ptr(out_off), ptr(out_len),
                                                ptr(status), None, 0, ctypes.c_void_p(_stream_handle(stream))),
          "ambrycrc_transform_messages_dev")
    return out, out_off, out_len, status


def transform_host(region, msg_off, header_version: int = 3, life_version=None, out_cap=None, device: int = 0,
                   pinned: bool = False):
    """ambrycrc_transform_messages_host: the batched transform of a region in host memory (bytes,
    bytearray, uint8 numpy array or uint8 CPU tensor; pinned=True for a pin_memory() tensor), staged
    through the pinned slabs. Returns (out bytes packed in message order, out_off int64[m] (-1: not
    transformed), out_len int64[m], status uint32[m])."""
    if hasattr(region, "data_ptr"):
        base, n = region.data_ptr(), region.numel()
        keep = region
    else:
        keep = np.frombuffer(region, dtype=np.uint8) if not isinstance(region, np.ndarray) else region
        base, n = keep.ctypes.data, keep.size
    offs = np.ascontiguousarray(np.asarray(msg_off, dtype=np.uint64))
    m = offs.size
    cap = out_bound(n, m) if out_cap is None else int(out_cap)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    life = None if life_version is None else np.ascontiguousarray(np.asarray(life_version, dtype=np.int16))
    oo = np.zeros(m, dtype=np.uint64)
    ol = np.zeros(m, dtype=np.uint64)
    st = np.zeros(m, dtype=np.uint32)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    check(lib().ambrycrc_transform_messages_host(
        ctypes.c_void_p(base), n, offs.ctypes.data_as(u64p), m, None if life is None else life.ctypes.data,
        header_version, out.ctypes.data, cap, oo.ctypes.data_as(u64p), ol.ctypes.data_as(u64p),
        st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), device, 1 if pinned else 0),
        "ambrycrc_transform_messages_host")
    del keep
    used = int((oo[st == 0] + ol[st == 0]).max()) if (st == 0).any() else 0
    return out[:used].tobytes(), oo.view(np.int64), ol.view(np.int64), st


# ------------------------------------------------------------------ re-keying (BlobIdTransformer)
# status bits added by the re-key (include/ambrycrc.h)
MSG_NEEDS_CONTENT = 1 << 14
MSG_BAD_DESC = 1 << 15

REKEY_KEEP = 0xFFFFFFFFFFFFFFFF  # ambrycrc_rekey_desc.content_src: keep the stored blob content

# numpy mirror of struct ambrycrc_rekey_desc (40 bytes): what the caller's StoreKeyConverter decided for
# one message. key_src / content_src are offsets into one auxiliary buffer; key_len 0 skips the message.
REKEY_DESC_DTYPE = np.dtype([
    ("key_src", "<u8"), ("content_src", "<u8"), ("content_len", "<u8"), ("props_blob_size", "<i8"),
    ("key_len", "<u4"), ("account_id", "<i2"), ("container_id", "<i2")])
assert REKEY_DESC_DTYPE.itemsize == 40


def rekey_out_bound(region_len: int, m: int, aux_len: int) -> int:
    """ambrycrc_rekey_out_bound: an output capacity that never yields MSG_NO_ROOM for m messages that share
    no region bytes, when every aux byte is used by at most one descriptor."""
    return int(lib().ambrycrc_rekey_out_bound(region_len, m, aux_len))


def rekey_workspace_bytes(m: int) -> int:
    return int(lib().ambrycrc_rekey_workspace_bytes(m))


def rekey_message_cpu(region, off: int, desc, aux, header_version: int = 3, life=None, out_cap=None):
    """ambrycrc_rekey_message_cpu: BlobIdTransformer.transform of the message at `off` of a host buffer.
    desc: one REKEY_DESC_DTYPE record; aux: the bytes its offsets refer to.
    Returns (status bits, the re-keyed message; None when refused, b"" when skipped)."""
    buf = np.frombuffer(region, dtype=np.uint8) if not isinstance(region, np.ndarray) else region
    ax = np.frombuffer(aux, dtype=np.uint8) if not isinstance(aux, np.ndarray) else aux
    d = np.zeros(1, dtype=REKEY_DESC_DTYPE)
    d[0] = desc
    cap = out_cap if out_cap is not None else rekey_out_bound(buf.size - min(off, buf.size), 1, ax.size)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    st, n = ctypes.c_uint32(0), ctypes.c_uint64(0)
    check(lib().ambrycrc_rekey_message_cpu(ctypes.c_void_p(buf.ctypes.data if buf.size else 0), buf.size, off,
                                           ctypes.c_void_p(d.ctypes.data),
                                           ctypes.c_void_p(ax.ctypes.data if ax.size else 0), ax.size,
                                           -1 if life is None else int(life), header_version,
                                           ctypes.c_void_p(out.ctypes.data), cap, ctypes.byref(n), ctypes.byref(st)),
          "ambrycrc_rekey_message_cpu")
    return st.value, (out[:n.value].tobytes() if st.value == 0 else None)


def rekey_dev(region, msg_off, descs, aux, header_version: int = 3, life_version=None, out=None, stream=None,
              workspace=None):
    """ambrycrc_rekey_messages_dev -- BlobIdTransformer.transform for a batch of stored messages in HBM:
    every clean PUT re-serialized at `header_version` under the new store key of descs[i] (a uint8 CUDA
    tensor holding the REKEY_DESC_DTYPE array; the keys and replacement contents in `aux`, a uint8 CUDA
    tensor), packed in order into `out` (default: rekey_out_bound bytes). life_version: an int16 CUDA
    tensor, or None for the stored ones. workspace: a CUDA tensor of rekey_workspace_bytes(m) bytes
    (needed to capture the call into a graph), or None for the stream's default one.
    Returns (out, out_off int64[m] (-1: not written), out_len int64[m], status int32[m])."""
    import torch

    from .device import _stream_handle, _workspace

    if region.dtype != torch.uint8 or not region.is_cuda:
        raise TypeError("region must be a uint8 CUDA tensor")
    dev = region.device
    if msg_off.dtype != torch.int64 or not msg_off.is_cuda or not msg_off.is_contiguous() or msg_off.device != dev:
        raise TypeError("msg_off must be a contiguous int64 CUDA tensor on the region's device")
    m = msg_off.numel()
    if descs.dtype != torch.uint8 or not descs.is_cuda or not descs.is_contiguous() or descs.device != dev or \
            descs.numel() != m * REKEY_DESC_DTYPE.itemsize:
        raise TypeError("descs must be a contiguous uint8 CUDA tensor of m 40-byte descriptors")
    if aux.dtype != torch.uint8 or not aux.is_cuda or not aux.is_contiguous() or aux.device != dev:
        raise TypeError("aux must be a contiguous uint8 CUDA tensor on the region's device")
    if life_version is not None and (life_version.dtype != torch.int16 or life_version.numel() != m
                                     or not life_version.is_cuda or not life_version.is_contiguous()):
        raise TypeError("life_version must be a contiguous int16 CUDA tensor of m elements")
    if out is None:
        out = torch.empty(rekey_out_bound(region.numel(), m, aux.numel()), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.device != dev:
        raise TypeError("out must be a contiguous uint8 CUDA tensor on the region's device")
    out_off = torch.empty(m, dtype=torch.int64, device=dev)
    out_len = torch.empty(m, dtype=torch.int64, device=dev)
    status = torch.empty(m, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace(workspace, dev)
    ptr = lambda t: None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    check(lib().ambrycrc_rekey_messages_dev(ptr(region), region.numel(), ptr(msg_off), m, ptr(descs), ptr(aux),
                                            aux.numel(), ptr(life_version), header_version, ptr(out), out.numel(),
                                            ptr(out_off), ptr(out_len), ptr(status), ws, ws_bytes,
                                            ctypes.c_void_p(_stream_handle(stream))),
          "ambrycrc_rekey_messages_dev")
    return out, out_off, out_len, status


# ------------------------------------------------------------------ PutRequest ingest (AmbryRequests.handlePutRequest)
# numpy mirror of struct ambrycrc_put_request_ref (16 bytes): one frame of a wire buffer.
PUT_REQUEST_REF_DTYPE = np.dtype([("off", "<u8"), ("key_len", "<u4"), ("reserved", "<u4")])
assert PUT_REQUEST_REF_DTYPE.itemsize == 16

MSG_WIRE_CRC = 1 << 17   # AMBRYCRC_MSG_WIRE_CRC: "CRC mismatch, data in PutRequest is unreliable"
INGEST_GROWTH_MAX = 72   # AMBRYCRC_INGEST_GROWTH_MAX


def ingest_out_bound(wire_len: int, m: int) -> int:
    """ambrycrc_ingest_out_bound: an output capacity that never yields MSG_NO_ROOM for m frames that share no
    wire bytes."""
    return int(lib().ambrycrc_ingest_out_bound(wire_len, m))


def ingest_workspace_size(m: int) -> int:
    return int(lib().ambrycrc_ingest_puts_workspace_size(m))


def ingest_put_request_cpu(wire, off: int, key_len: int, header_version: int = 3, out_cap=None, reserved: int = 0):
    """ambrycrc_ingest_put_request_cpu: PutRequest.readFrom and getMessageFormatWriteSet for the frame at `off`
    of a host buffer whose serialized blob id is key_len bytes long.
    Returns (status bits, the stored message or None when refused, the computed wire CRC, its MESSAGE_INFO
    record)."""
    from .device import _recover_dtypes

    buf = np.frombuffer(wire, dtype=np.uint8) if not isinstance(wire, np.ndarray) else wire
    ref = np.zeros(1, dtype=PUT_REQUEST_REF_DTYPE)
    ref[0] = (off, key_len, reserved)
    cap = out_cap if out_cap is not None else ingest_out_bound(buf.size, 1)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    info = np.zeros(1, dtype=_recover_dtypes()[0])
    st, crc, n = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
    check(lib().ambrycrc_ingest_put_request_cpu(ctypes.c_void_p(buf.ctypes.data if buf.size else 0), buf.size,
                                                ctypes.c_void_p(ref.ctypes.data), header_version,
                                                ctypes.c_void_p(out.ctypes.data), cap, ctypes.byref(n),
                                                ctypes.c_void_p(info.ctypes.data), ctypes.byref(crc),
                                                ctypes.byref(st)),
          "ambrycrc_ingest_put_request_cpu")
    return st.value, (out[:n.value].tobytes() if st.value == 0 else None), crc.value, info[0]


def ingest_put_requests_dev(wire, refs, header_version: int = 3, out=None, stream=None, workspace=None):
    """ambrycrc_ingest_put_requests_dev -- AmbryRequests.handlePutRequest for a batch of PutRequest frames in
    HBM: every frame parsed, its wire CRC checked, and the clean ones written as stored PUT messages at
    `header_version`, packed in request order into `out` (default: ingest_out_bound bytes). wire: a uint8
    CUDA tensor; refs: a uint8 CUDA tensor holding the PUT_REQUEST_REF_DTYPE array. workspace: a CUDA tensor
    of ingest_workspace_size(m) bytes (needed to capture the call into a graph), or None for the stream's
    default one.
    Returns (out, out_off int64[m] (-1: not written), out_len int64[m], info uint8[m, 48] (rows of
    MESSAGE_INFO, zero unless the status is 0), wire_crc int32[m], total int64[1], status int32[m])."""
    import torch

    from .device import _stream_handle, _workspace

    if wire.dtype != torch.uint8 or not wire.is_cuda or not wire.is_contiguous():
        raise TypeError("wire must be a contiguous uint8 CUDA tensor")
    dev = wire.device
    if refs.dtype != torch.uint8 or not refs.is_cuda or not refs.is_contiguous() or refs.device != dev or \
            refs.numel() % PUT_REQUEST_REF_DTYPE.itemsize:
        raise TypeError("refs must be a contiguous uint8 CUDA tensor of 16-byte request references")
    m = refs.numel() // PUT_REQUEST_REF_DTYPE.itemsize
    if out is None:
        out = torch.empty(ingest_out_bound(wire.numel(), m), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.device != dev:
        raise TypeError("out must be a contiguous uint8 CUDA tensor on the wire buffer's device")
    out_off = torch.empty(m, dtype=torch.int64, device=dev)
    out_len = torch.empty(m, dtype=torch.int64, device=dev)
    info = torch.empty((m, 48), dtype=torch.uint8, device=dev)
    wire_crc = torch.empty(m, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    status = torch.empty(m, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace(workspace, dev)
    ptr = lambda t: None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    check(lib().ambrycrc_ingest_put_requests_dev(ptr(wire), wire.numel(), ptr(refs), m, header_version, ptr(out),
                                                 out.numel(), ptr(out_off), ptr(out_len), ptr(info), ptr(wire_crc),
                                                 ptr(total), ptr(status), ws, ws_bytes,
                                                 ctypes.c_void_p(_stream_handle(stream))),
          "ambrycrc_ingest_put_requests_dev")
    return out, out_off, out_len, info, wire_crc, total, status


# ------------------------------------------------------------------ serving a GET (MessageFormatSend)
# MessageFormatFlags ordinals (AMBRYCRC_SEND_*)
SEND_BLOB_PROPERTIES = 0
SEND_BLOB_USER_METADATA = 1
SEND_BLOB = 2
SEND_ALL = 3
SEND_BLOB_INFO = 4

SEND_NOWHERE = 0xFFFFFFFFFFFFFFFF  # ambrycrc_send_info.out_off of a message not sent

# numpy mirror of struct ambrycrc_send_info (32 bytes): SendInfo, the encryption key's place for
# MessageMetadata, and the findings the reference only counts.
SEND_INFO_DTYPE = np.dtype([("out_off", "<u8"), ("send_len", "<u8"), ("rel_off", "<u4"), ("enckey_rel", "<u4"),
                            ("enckey_len", "<u4"), ("check", "<u4")])
assert SEND_INFO_DTYPE.itemsize == 32


def send_workspace_bytes(m: int) -> int:
    return int(lib().ambrycrc_send_workspace_bytes(m))


def send_message_cpu(region, off: int, flag: int, size=None, out_cap=None):
    """ambrycrc_send_message_cpu: MessageFormatSend.fetchDataFromReadSet for the message at `off` of a host
    buffer under `flag`. size: readSet.sizeInBytes, or None for the header's own message length.
    Returns (status bits, one SEND_INFO_DTYPE record, the sent bytes; None when nothing was sent)."""
    buf = np.frombuffer(region, dtype=np.uint8) if not isinstance(region, np.ndarray) else region
    cap = out_cap if out_cap is not None else buf.size
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    info = np.zeros(1, dtype=SEND_INFO_DTYPE)
    st = ctypes.c_uint32(0)
    check(lib().ambrycrc_send_message_cpu(ctypes.c_void_p(buf.ctypes.data if buf.size else 0), buf.size, off,
                                          0 if size is None else int(size), flag, ctypes.c_void_p(out.ctypes.data),
                                          cap, ctypes.c_void_p(info.ctypes.data), ctypes.byref(st)),
          "ambrycrc_send_message_cpu")
    sent = out[:int(info[0]["send_len"])].tobytes() if st.value == 0 else None
    return st.value, info[0].copy(), sent


def send_messages_dev(region, msg_off, flag: int, msg_size=None, out=None, stream=None, workspace=None):
    """ambrycrc_send_messages_dev -- MessageFormatSend.fetchDataFromReadSet for a batch of stored messages in
    HBM under one flag: the selected spans, stored bytes verbatim, packed in message order into `out` (a
    uint8 CUDA tensor; default: the sum of the sizes, or the region's size without sizes). msg_size: an
    int64 CUDA tensor of readSet.sizeInBytes values, or None for each header's own length. workspace: a
    CUDA tensor of send_workspace_bytes(m) bytes (needed to capture the call into a graph), or None.
    Returns (out, info: a uint8 CUDA tensor holding the SEND_INFO_DTYPE array, status int32[m])."""
    import torch

    from .device import _stream_handle, _workspace

    if region.dtype != torch.uint8 or not region.is_cuda:
        raise TypeError("region must be a uint8 CUDA tensor")
    dev = region.device
    if msg_off.dtype != torch.int64 or not msg_off.is_cuda or not msg_off.is_contiguous() or msg_off.device != dev:
        raise TypeError("msg_off must be a contiguous int64 CUDA tensor on the region's device")
    m = msg_off.numel()
    if msg_size is not None and (msg_size.dtype != torch.int64 or not msg_size.is_cuda or msg_size.device != dev
                                 or not msg_size.is_contiguous() or msg_size.numel() != m):
        raise TypeError("msg_size must be a contiguous int64 CUDA tensor of m elements on the region's device")
    if out is None:
        out = torch.empty(max(region.numel(), 1), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.device != dev:
        raise TypeError("out must be a contiguous uint8 CUDA tensor on the region's device")
    info = torch.empty(m * SEND_INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    status = torch.empty(m, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace(workspace, dev)
    ptr = lambda t: None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    check(lib().ambrycrc_send_messages_dev(ptr(region), region.numel(), ptr(msg_off), ptr(msg_size), m, flag,
                                           ptr(out), out.numel(), ptr(info), ptr(status), ws, ws_bytes,
                                           ctypes.c_void_p(_stream_handle(stream))),
          "ambrycrc_send_messages_dev")
    return out, info, status


# ------------------------------------------------------------------ receiving a GET (GetBlobOperation.handleBody)
MSG_BAD_RANGE = 1 << 18  # AMBRYCRC_MSG_BAD_RANGE: the requested range does not lie inside the blob content

RECV_NOWHERE = 0xFFFFFFFFFFFFFFFF  # ambrycrc_recv_info.out_off of a payload that delivers nothing
RECV_TO_END = 0xFFFFFFFFFFFFFFFF   # a range's hi: to the content's end

# numpy mirror of struct ambrycrc_recv_info (56 bytes): where the content went, BlobData's fields, and under
# ALL the places of the encryption key, the BlobPropertiesSerDe bytes and the user metadata in the payload.
RECV_INFO_DTYPE = np.dtype([("out_off", "<u8"), ("out_len", "<u8"), ("blob_size", "<u8"), ("content_rel", "<u4"),
                            ("enckey_rel", "<u4"), ("enckey_len", "<u4"), ("props_rel", "<u4"), ("props_len", "<u4"),
                            ("usermeta_rel", "<u4"), ("usermeta_len", "<u4"), ("blob_type", "u1"),
                            ("compressed", "u1"), ("blob_version", "u1"), ("header_version", "u1")])
assert RECV_INFO_DTYPE.itemsize == 56


def receive_workspace_bytes(m: int) -> int:
    return int(lib().ambrycrc_receive_workspace_size(m))


def receive_blob_cpu(payload, flag: int, lo: int = 0, hi=None, out_cap=None):
    """ambrycrc_receive_blob_cpu: deserializeBlob (SEND_BLOB: a bare blob record) or deserializeBlobAll
    (SEND_ALL: a whole stored message) over one payload in host memory, the content sliced to [lo, hi)
    (hi None: to the content's end). Returns (status bits, one RECV_INFO_DTYPE record, the delivered bytes;
    None when refused)."""
    buf = np.frombuffer(payload, dtype=np.uint8) if not isinstance(payload, np.ndarray) else payload
    cap = out_cap if out_cap is not None else buf.size
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    info = np.zeros(1, dtype=RECV_INFO_DTYPE)
    st = ctypes.c_uint32(0)
    check(lib().ambrycrc_receive_blob_cpu(ctypes.c_void_p(buf.ctypes.data if buf.size else 0), buf.size, flag, int(lo),
                                          RECV_TO_END if hi is None else int(hi), ctypes.c_void_p(out.ctypes.data),
                                          cap, ctypes.c_void_p(info.ctypes.data), ctypes.byref(st)),
          "ambrycrc_receive_blob_cpu")
    got = None if int(info[0]["out_off"]) == RECV_NOWHERE else out[:int(info[0]["out_len"])].tobytes()
    return st.value, info[0].copy(), got


def receive_blobs_dev(body, pay_off, flag: int, pay_size=None, ranges=None, dst_off=None, out=None, stream=None,
                      workspace=None):
    """ambrycrc_receive_blobs_dev -- the router's GET receive for a batch of payloads of a GetResponse body in
    HBM under SEND_BLOB or SEND_ALL: each blob record verified, its content sliced to the payload's range and
    written to `out` (a uint8 CUDA tensor; default: the body's size). pay_off / pay_size: int64 CUDA tensors,
    the out_off / send_len columns of the sending side (pay_size None: each payload runs to the body's end).
    ranges: an int64 CUDA tensor of 2m elements (lo, hi per payload; hi -1: to the content's end) or None.
    dst_off: an int64 CUDA tensor of m destinations in `out`, or None to pack in payload order. workspace: a
    CUDA tensor of receive_workspace_bytes(m) bytes (needed to capture the call into a graph), or None.
    Returns (out, info: a uint8 CUDA tensor holding the RECV_INFO_DTYPE array, status int32[m])."""
    import torch

    from .device import _stream_handle, _workspace

    if body.dtype != torch.uint8 or not body.is_cuda:
        raise TypeError("body must be a uint8 CUDA tensor")
    dev = body.device
    if pay_off.dtype != torch.int64 or not pay_off.is_cuda or not pay_off.is_contiguous() or pay_off.device != dev:
        raise TypeError("pay_off must be a contiguous int64 CUDA tensor on the body's device")
    m = pay_off.numel()
    for name, t, n in (("pay_size", pay_size, m), ("ranges", ranges, 2 * m), ("dst_off", dst_off, m)):
        if t is not None and (t.dtype != torch.int64 or not t.is_cuda or t.device != dev or not t.is_contiguous()
                              or t.numel() != n):
            raise TypeError(f"{name} must be a contiguous int64 CUDA tensor of {n} elements on the body's device")
    if out is None:
        out = torch.empty(max(body.numel(), 1), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.device != dev:
        raise TypeError("out must be a contiguous uint8 CUDA tensor on the body's device")
    info = torch.empty(m * RECV_INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    status = torch.empty(m, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace(workspace, dev)
    ptr = lambda t: None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    check(lib().ambrycrc_receive_blobs_dev(ptr(body), body.numel(), ptr(pay_off), ptr(pay_size), m, flag, ptr(ranges),
                                           ptr(dst_off), ptr(out), out.numel(), ptr(info), ptr(status), ws, ws_bytes,
                                           ctypes.c_void_p(_stream_handle(stream))),
          "ambrycrc_receive_blobs_dev")
    return out, info, status
