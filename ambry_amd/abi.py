"""The constants and structs of include/ambrycrc.h, each mirrored once (tests/test_abi_mirror.py compares every
value, field offset and size with the header through a compiled C program). A macro AMBRYCRC_X is X here, except
the error codes, which keep the names the package always exported. _lib, device and messages re-export from here.
"""
from __future__ import annotations

import ctypes

import numpy as np

AMBRYCRC_OK = 0
AMBRYCRC_EINVAL = -1
AMBRYCRC_EHIP = -2
AMBRYCRC_ENOMEM = -3
AMBRYCRC_ENOINIT = -4
AMBRYCRC_ENODEV = -5
AMBRYCRC_ECOMM = -6
AMBRYCRC_EPROBE = -7

# per-message status bits (d_status of every message entry; ambrycrc_send_info.check)
MSG_HEADER_CRC = 1 << 0
MSG_ENCKEY_CRC = 1 << 1
MSG_PROPS_CRC = 1 << 2
MSG_UPDATE_CRC = 1 << 3
MSG_USERMETA_CRC = 1 << 4
MSG_BLOB_CRC = 1 << 5
MSG_BAD_VERSION = 1 << 8
MSG_BAD_LAYOUT = 1 << 9
MSG_NOT_PUT = 1 << 10         # the transform's: an update record
MSG_BAD_RECORD = 1 << 11
MSG_NO_ROOM = 1 << 12
MSG_NOT_ENCODABLE = 1 << 13
MSG_NEEDS_CONTENT = 1 << 14   # the re-key's
MSG_BAD_DESC = 1 << 15
MSG_BAD_INFO = 1 << 16        # recovery: an operation time below -1 (MessageInfo's constructor throws)
MSG_WIRE_CRC = 1 << 17        # ingest: "CRC mismatch, data in PutRequest is unreliable"
MSG_BAD_RANGE = 1 << 18       # receive: the requested range does not lie inside the blob content

# MessageFormatFlags ordinals
SEND_BLOB_PROPERTIES = 0
SEND_BLOB_USER_METADATA = 1
SEND_BLOB = 2
SEND_ALL = 3
SEND_BLOB_INFO = 4

# A transformed message is at most this many bytes longer than the stored one: header V1 -> V3 (+6),
# BlobProperties SerDe V1 -> V5 (+17), Blob_Format_V1 -> V3 head (+3).
TRANSFORM_GROWTH_MAX = 26
INGEST_GROWTH_MAX = 72   # a stored message over the PutRequest frame it comes from
UNIQUE_ID_BYTES = 128

# sentinels, all UINT64_MAX (the header names them in its comments, not as macros)
REKEY_KEEP = 0xFFFFFFFFFFFFFFFF    # ambrycrc_rekey_desc.content_src: keep the stored blob content
SEND_NOWHERE = 0xFFFFFFFFFFFFFFFF  # ambrycrc_send_info.out_off of a message not sent
RECV_NOWHERE = 0xFFFFFFFFFFFFFFFF  # ambrycrc_recv_info.out_off of a payload that delivers nothing
RECV_TO_END = 0xFFFFFFFFFFFFFFFF   # a range's hi: to the content's end
NO_MESSAGE = 0xFFFFFFFFFFFFFFFF    # d_msg_off of a slot past the chain (-1 in the int64 tensor)


class Shard(ctypes.Structure):
    """struct ambrycrc_shard: one GPU's part of a multi-GPU batch."""
    _fields_ = [("device", ctypes.c_int), ("d_base", ctypes.c_void_p), ("d_off", ctypes.c_void_p),
                ("d_len", ctypes.c_void_p), ("d_crc_in", ctypes.c_void_p), ("n", ctypes.c_size_t),
                ("d_gathered", ctypes.c_void_p), ("stream", ctypes.c_void_p)]


class PutDesc(ctypes.Structure):
    """struct ambrycrc_put_desc: one PUT message to serialize (80 bytes)."""
    _fields_ = [("out_off", ctypes.c_uint64), ("key_src", ctypes.c_uint64), ("enckey_src", ctypes.c_uint64),
                ("props_src", ctypes.c_uint64), ("usermeta_src", ctypes.c_uint64), ("blob_src", ctypes.c_uint64),
                ("blob_len", ctypes.c_uint64), ("key_len", ctypes.c_uint32), ("enckey_len", ctypes.c_int32),
                ("props_len", ctypes.c_uint32), ("usermeta_len", ctypes.c_uint32), ("life_version", ctypes.c_int16),
                ("blob_type", ctypes.c_int16), ("compressed", ctypes.c_uint8), ("header_version", ctypes.c_uint8),
                ("reserved", ctypes.c_uint8 * 2)]


# the same struct for descriptor arrays copied to HBM
PUT_DESC_DTYPE = np.dtype(PutDesc)
# ambrycrc_rekey_desc: what the caller's StoreKeyConverter decided for one message. key_src / content_src are
# offsets into one auxiliary buffer; key_len 0 skips the message.
REKEY_DESC_DTYPE = np.dtype([
    ("key_src", "<u8"), ("content_src", "<u8"), ("content_len", "<u8"), ("props_blob_size", "<i8"),
    ("key_len", "<u4"), ("account_id", "<i2"), ("container_id", "<i2")])
HARD_DELETE_INFO = np.dtype([
    ("blob_size", "<u8"), ("size", "<u8"), ("start", "<u4"), ("usermeta_size", "<u4"), ("header_version", "<i2"),
    ("usermeta_version", "<i2"), ("blob_version", "<i2"), ("blob_type", "<i2")])
# ambrycrc_send_info: SendInfo, the encryption key's place for MessageMetadata, and the findings the reference
# only counts.
SEND_INFO_DTYPE = np.dtype([("out_off", "<u8"), ("send_len", "<u8"), ("rel_off", "<u4"), ("enckey_rel", "<u4"),
                            ("enckey_len", "<u4"), ("check", "<u4")])
# ambrycrc_recv_info: where the content went, BlobData's fields, and under ALL the places of the encryption key,
# the BlobPropertiesSerDe bytes and the user metadata in the payload.
RECV_INFO_DTYPE = np.dtype([
    ("out_off", "<u8"), ("out_len", "<u8"), ("blob_size", "<u8"), ("content_rel", "<u4"), ("enckey_rel", "<u4"),
    ("enckey_len", "<u4"), ("props_rel", "<u4"), ("props_len", "<u4"), ("usermeta_rel", "<u4"),
    ("usermeta_len", "<u4"), ("blob_type", "u1"), ("compressed", "u1"), ("blob_version", "u1"),
    ("header_version", "u1")])
MESSAGE_INFO = np.dtype([
    ("msg_off", "<u8"), ("size", "<u8"), ("expires_at_ms", "<i8"), ("operation_time_ms", "<i8"), ("key_rel", "<u4"),
    ("key_len", "<u4"), ("account_id", "<i2"), ("container_id", "<i2"), ("life_version", "<i2"), ("flags", "u1"),
    ("header_version", "u1")])
RECOVER_RESULT = np.dtype([("chained", "<u8"), ("recovered", "<u8"), ("end_off", "<u8"), ("end_status", "<u4"),
                           ("more", "<u4")])
# ambrycrc_put_request_ref: one frame of a wire buffer
PUT_REQUEST_REF_DTYPE = np.dtype([("off", "<u8"), ("key_len", "<u4"), ("reserved", "<u4")])

# every struct of the header by its C name (less the ambrycrc_ prefix)
STRUCTS = {"put_desc": PutDesc, "rekey_desc": REKEY_DESC_DTYPE, "hard_delete_info": HARD_DELETE_INFO,
           "send_info": SEND_INFO_DTYPE, "recv_info": RECV_INFO_DTYPE, "message_info": MESSAGE_INFO,
           "recover_result": RECOVER_RESULT, "put_request_ref": PUT_REQUEST_REF_DTYPE, "shard": Shard}
