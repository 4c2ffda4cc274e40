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

from ._args import dev_tensor, host_buffer, message_batch, ptr, stream_handle, torch as _torch, workspace as _workspace
from ._lib import check, lib
from .abi import (INGEST_GROWTH_MAX, MESSAGE_INFO, MSG_BAD_DESC, MSG_BAD_RANGE, MSG_BAD_RECORD,  # noqa: F401
                  MSG_NEEDS_CONTENT, MSG_NO_ROOM, MSG_NOT_ENCODABLE, MSG_NOT_PUT, MSG_WIRE_CRC, PUT_DESC_DTYPE,
                  PUT_REQUEST_REF_DTYPE, RECV_INFO_DTYPE, RECV_NOWHERE, RECV_TO_END, REKEY_DESC_DTYPE, REKEY_KEEP,
                  SEND_ALL, SEND_BLOB, SEND_BLOB_INFO, SEND_BLOB_PROPERTIES, SEND_BLOB_USER_METADATA, SEND_INFO_DTYPE,
                  SEND_NOWHERE, TRANSFORM_GROWTH_MAX, PutDesc)

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
    torch = _torch()
    m = dev_tensor("descs", descs, torch.uint8, unit=80).numel() // 80
    dev_tensor("out", out, torch.uint8, like=descs)
    dev_tensor("fields", fields, torch.uint8, like=descs, optional=True)
    dev_tensor("blobs", blobs, torch.uint8, like=descs, optional=True)
    dev_tensor("msg_len", msg_len, torch.int64, m, descs, optional=True)
    check(lib().ambrycrc_serialize_puts_dev(ptr(descs), m, ptr(fields), ptr(blobs), ptr(out), ptr(msg_len), None, 0,
                                            stream_handle(stream)), "ambrycrc_serialize_puts_dev")


def _cpu_out(cap):
    """(output array of cap bytes -- at least 1 --, status, length) for a one-message CPU entry."""
    return np.zeros(max(cap, 1), dtype=np.uint8), ctypes.c_uint32(0), ctypes.c_uint64(0)


def verify_message_cpu(region, off: int):
    """ambrycrc_verify_message_cpu: (AMBRYCRC_MSG_* status bits, message end or 0) for the message
    at `off` in a host buffer (bytes / bytearray / uint8 numpy array)."""
    _keep, base, n = host_buffer("region", region)
    st, end = ctypes.c_uint32(0), ctypes.c_uint64(0)
    check(lib().ambrycrc_verify_message_cpu(base, n, off, ctypes.byref(st), ctypes.byref(end)),
          "ambrycrc_verify_message_cpu")
    return st.value, end.value


def transform_message_cpu(region, off: int, header_version: int = 3, life=None, out_cap=None):
    """ambrycrc_transform_message_cpu: (status bits, the re-serialized message or None)."""
    _keep, base, size = host_buffer("region", region)
    # default: the ABI's bound (the stored bytes after off + TRANSFORM_GROWTH_MAX), never NO_ROOM
    cap = out_cap if out_cap is not None else out_bound(size - min(off, size), 1)
    out, st, n = _cpu_out(cap)
    check(lib().ambrycrc_transform_message_cpu(base, size, off, -1 if life is None else int(life), header_version,
                                               out.ctypes.data, cap, ctypes.byref(n), ctypes.byref(st)),
          "ambrycrc_transform_message_cpu")
    return st.value, (out[:n.value].tobytes() if st.value == 0 else None)


def out_bound(region_len: int, m: int) -> int:
    """ambrycrc_transform_out_bound: an output capacity that never yields MSG_NO_ROOM for m
    messages that share no bytes of a region_len-byte region."""
    return int(lib().ambrycrc_transform_out_bound(region_len, m))


def _packed_out(region, m, out, default_cap, life_version=None):
    """(out, out_off int64[m], out_len int64[m], status int32[m]) of an entry that packs messages into `out`: the
    caller's checked `out`, or a new one of default_cap() bytes; life_version checked on the way."""
    torch = _torch()
    dev_tensor("life_version", life_version, torch.int16, m, region, optional=True)
    if out is None:
        out = torch.empty(default_cap(), dtype=torch.uint8, device=region.device)
    dev_tensor("out", out, torch.uint8, like=region)
    return (out, torch.empty(m, dtype=torch.int64, device=region.device),
            torch.empty(m, dtype=torch.int64, device=region.device),
            torch.empty(m, dtype=torch.int32, device=region.device))


def transform_dev(region, msg_off, header_version: int = 3, life_version=None, out=None, stream=None):
    """ambrycrc_transform_messages_dev -- ValidatingTransformer.transform for a batch of stored
    messages in HBM: every clean PUT re-serialized at `header_version` (and life version
    life_version[i], an int16 CUDA tensor, or the stored one), packed in order into `out` (a uint8
    CUDA tensor; default: out_bound(region bytes, m), enough for every message of a region whose
    messages do not overlap -- TRANSFORM_GROWTH_MAX = 26 B of growth per message).
    Returns (out, out_off int64[m], out_len int64[m], status int32[m])."""
    m = message_batch(region, msg_off)
    out, out_off, out_len, status = _packed_out(region, m, out, lambda: out_bound(region.numel(), m), life_version)
    check(lib().ambrycrc_transform_messages_dev(ptr(region), region.numel(), ptr(msg_off), m, ptr(life_version),
                                                header_version, ptr(out), out.numel(), ptr(out_off), ptr(out_len),
                                                ptr(status), None, 0, stream_handle(stream)),
          "ambrycrc_transform_messages_dev")
    return out, out_off, out_len, status


def transform_host(region, msg_off, header_version: int = 3, life_version=None, out_cap=None, device: int = 0,
                   pinned: bool = False):
    """ambrycrc_transform_messages_host: the batched transform of a region in host memory (bytes,
    bytearray, uint8 numpy array or uint8 CPU tensor; pinned=True for a pin_memory() tensor), staged
    through the pinned slabs. Returns (out bytes packed in message order, out_off int64[m] (-1: not
    transformed), out_len int64[m], status uint32[m])."""
    _keep, base, n = host_buffer("region", region)
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
        base, n, offs.ctypes.data_as(u64p), m, None if life is None else life.ctypes.data,
        header_version, out.ctypes.data, cap, oo.ctypes.data_as(u64p), ol.ctypes.data_as(u64p),
        st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), device, 1 if pinned else 0),
        "ambrycrc_transform_messages_host")
    used = int((oo[st == 0] + ol[st == 0]).max()) if (st == 0).any() else 0
    return out[:used].tobytes(), oo.view(np.int64), ol.view(np.int64), st


# ------------------------------------------------------------------ re-keying (BlobIdTransformer)
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
    _keep, base, size = host_buffer("region", region)
    _keep_aux, aux_base, aux_size = host_buffer("aux", aux)
    d = np.zeros(1, dtype=REKEY_DESC_DTYPE)
    d[0] = desc
    cap = out_cap if out_cap is not None else rekey_out_bound(size - min(off, size), 1, aux_size)
    out, st, n = _cpu_out(cap)
    check(lib().ambrycrc_rekey_message_cpu(base, size, off, d.ctypes.data, aux_base, aux_size,
                                           -1 if life is None else int(life), header_version, out.ctypes.data, cap,
                                           ctypes.byref(n), ctypes.byref(st)),
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
    m = message_batch(region, msg_off)
    dev_tensor("descs", descs, _torch().uint8, m, region, unit=40)
    dev_tensor("aux", aux, _torch().uint8, like=region)
    out, out_off, out_len, status = _packed_out(region, m, out,
                                                lambda: rekey_out_bound(region.numel(), m, aux.numel()), life_version)
    ws, ws_bytes = _workspace(workspace, region)
    check(lib().ambrycrc_rekey_messages_dev(ptr(region, True), region.numel(), ptr(msg_off, True), m, ptr(descs, True),
                                            ptr(aux, True), aux.numel(), ptr(life_version, True), header_version,
                                            ptr(out, True), out.numel(), ptr(out_off, True), ptr(out_len, True),
                                            ptr(status, True), ws, ws_bytes, stream_handle(stream)),
          "ambrycrc_rekey_messages_dev")
    return out, out_off, out_len, status


# ------------------------------------------------------------------ PutRequest ingest (AmbryRequests.handlePutRequest)
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
    _keep, base, size = host_buffer("wire", wire)
    ref = np.zeros(1, dtype=PUT_REQUEST_REF_DTYPE)
    ref[0] = (off, key_len, reserved)
    cap = out_cap if out_cap is not None else ingest_out_bound(size, 1)
    out, st, n = _cpu_out(cap)
    info = np.zeros(1, dtype=MESSAGE_INFO)
    crc = ctypes.c_uint32(0)
    check(lib().ambrycrc_ingest_put_request_cpu(base, size, ref.ctypes.data, header_version, out.ctypes.data, cap,
                                                ctypes.byref(n), info.ctypes.data, ctypes.byref(crc),
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
    torch = _torch()
    dev_tensor("wire", wire, torch.uint8)
    m = dev_tensor("refs", refs, torch.uint8, like=wire, unit=16).numel() // 16
    out, out_off, out_len, status = _packed_out(wire, m, out, lambda: ingest_out_bound(wire.numel(), m))
    info = torch.empty((m, 48), dtype=torch.uint8, device=wire.device)
    wire_crc = torch.empty(m, dtype=torch.int32, device=wire.device)
    total = torch.empty(1, dtype=torch.int64, device=wire.device)
    ws, ws_bytes = _workspace(workspace, wire)
    check(lib().ambrycrc_ingest_put_requests_dev(ptr(wire, True), wire.numel(), ptr(refs, True), m, header_version,
                                                 ptr(out, True), out.numel(), ptr(out_off, True), ptr(out_len, True),
                                                 ptr(info, True), ptr(wire_crc, True), ptr(total), ptr(status, True),
                                                 ws, ws_bytes, stream_handle(stream)),
          "ambrycrc_ingest_put_requests_dev")
    return out, out_off, out_len, info, wire_crc, total, status


# ------------------------------------------------------------------ serving a GET (MessageFormatSend)
def send_workspace_bytes(m: int) -> int:
    return int(lib().ambrycrc_send_workspace_bytes(m))


def send_message_cpu(region, off: int, flag: int, size=None, out_cap=None):
    """ambrycrc_send_message_cpu: MessageFormatSend.fetchDataFromReadSet for the message at `off` of a host
    buffer under `flag`. size: readSet.sizeInBytes, or None for the header's own message length.
    Returns (status bits, one SEND_INFO_DTYPE record, the sent bytes; None when nothing was sent)."""
    _keep, base, n = host_buffer("region", region)
    cap = out_cap if out_cap is not None else n
    out, st, _ = _cpu_out(cap)
    info = np.zeros(1, dtype=SEND_INFO_DTYPE)
    check(lib().ambrycrc_send_message_cpu(base, n, off, 0 if size is None else int(size), flag, out.ctypes.data, cap,
                                          info.ctypes.data, ctypes.byref(st)),
          "ambrycrc_send_message_cpu")
    sent = out[:int(info[0]["send_len"])].tobytes() if st.value == 0 else None
    return st.value, info[0].copy(), sent


def _info_out(region, m, out, itemsize):
    """(out, info uint8[m * itemsize], status int32[m]) of send and receive: the caller's checked `out`, or one
    of the input's size."""
    torch = _torch()
    if out is None:
        out = torch.empty(max(region.numel(), 1), dtype=torch.uint8, device=region.device)
    dev_tensor("out", out, torch.uint8, like=region)
    return (out, torch.empty(m * itemsize, dtype=torch.uint8, device=region.device),
            torch.empty(m, dtype=torch.int32, device=region.device))


def send_messages_dev(region, msg_off, flag: int, msg_size=None, out=None, stream=None, workspace=None):
    """ambrycrc_send_messages_dev -- MessageFormatSend.fetchDataFromReadSet for a batch of stored messages in
    HBM under one flag: the selected spans, stored bytes verbatim, packed in message order into `out` (a
    uint8 CUDA tensor; default: the sum of the sizes, or the region's size without sizes). msg_size: an
    int64 CUDA tensor of readSet.sizeInBytes values, or None for each header's own length. workspace: a
    CUDA tensor of send_workspace_bytes(m) bytes (needed to capture the call into a graph), or None.
    Returns (out, info: a uint8 CUDA tensor holding the SEND_INFO_DTYPE array, status int32[m])."""
    m = message_batch(region, msg_off)
    dev_tensor("msg_size", msg_size, _torch().int64, m, region, optional=True)
    out, info, status = _info_out(region, m, out, SEND_INFO_DTYPE.itemsize)
    ws, ws_bytes = _workspace(workspace, region)
    check(lib().ambrycrc_send_messages_dev(ptr(region, True), region.numel(), ptr(msg_off, True), ptr(msg_size, True),
                                           m, flag, ptr(out, True), out.numel(), ptr(info, True), ptr(status, True),
                                           ws, ws_bytes, stream_handle(stream)),
          "ambrycrc_send_messages_dev")
    return out, info, status


# ------------------------------------------------------------------ receiving a GET (GetBlobOperation.handleBody)
def receive_workspace_bytes(m: int) -> int:
    return int(lib().ambrycrc_receive_workspace_size(m))


def receive_blob_cpu(payload, flag: int, lo: int = 0, hi=None, out_cap=None):
    """ambrycrc_receive_blob_cpu: deserializeBlob (SEND_BLOB: a bare blob record) or deserializeBlobAll
    (SEND_ALL: a whole stored message) over one payload in host memory, the content sliced to [lo, hi)
    (hi None: to the content's end). Returns (status bits, one RECV_INFO_DTYPE record, the delivered bytes;
    None when refused)."""
    _keep, base, n = host_buffer("payload", payload)
    cap = out_cap if out_cap is not None else n
    out, st, _ = _cpu_out(cap)
    info = np.zeros(1, dtype=RECV_INFO_DTYPE)
    check(lib().ambrycrc_receive_blob_cpu(base, n, flag, int(lo), RECV_TO_END if hi is None else int(hi),
                                          out.ctypes.data, cap, info.ctypes.data, ctypes.byref(st)),
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
    m = message_batch(body, pay_off, ("body", "pay_off"))
    for name, t, n in (("pay_size", pay_size, m), ("ranges", ranges, 2 * m), ("dst_off", dst_off, m)):
        dev_tensor(name, t, _torch().int64, n, body, optional=True)
    out, info, status = _info_out(body, m, out, RECV_INFO_DTYPE.itemsize)
    ws, ws_bytes = _workspace(workspace, body)
    check(lib().ambrycrc_receive_blobs_dev(ptr(body, True), body.numel(), ptr(pay_off, True), ptr(pay_size, True), m,
                                           flag, ptr(ranges, True), ptr(dst_off, True), ptr(out, True), out.numel(),
                                           ptr(info, True), ptr(status, True), ws, ws_bytes, stream_handle(stream)),
          "ambrycrc_receive_blobs_dev")
    return out, info, status
