"""Expected results of a hard delete (BlobStoreHardDelete.getHardDeleteInfo, BlobStoreHardDelete.java:97-179;
HardDeleteMessageFormatInputStream.java:58-124), from oracle/message_format.py and zlib alone -- independent
of the library's GF(2) shift. Shared by test_hard_delete_cpu.py and test_gpu_hard_delete.py, with the helpers
both use: the CPU entry over a region, the damage a crash mid-write leaves, and recovery structs that must be
refused."""
import struct

import numpy as np

from msgfmt import MF
from oracle_common import BLOB_HEAD, crc_bad

INFO = np.dtype([("blob_size", "<u8"), ("size", "<u8"), ("start", "<u4"), ("usermeta_size", "<u4"),
                 ("header_version", "<i2"), ("usermeta_version", "<i2"), ("blob_version", "<i2"), ("blob_type", "<i2")])


def _crc_bit(rec: bytes, bit: int) -> int:
    return bit if crc_bad(rec, 0, len(rec)) else 0


def replacement(um_size: int, blob_version: int, blob_type: int, blob_size: int) -> bytes:
    um = MF.usermeta_record(bytes(um_size))
    if blob_version == 1:
        return um + MF.blob_record_v1(bytes(blob_size))
    return um + MF.blob_record(bytes(blob_size), version=blob_version, blob_type=blob_type, compressed=False)


def one(region: bytes, off: int, recovery=None):
    """(status, info record or None, (start, replacement bytes) or None) for the message at off."""
    if off + 2 > len(region):
        return MF.BAD_LAYOUT, None, None
    vst, end = MF.verify_message(region, off)
    if end == 0:
        return vst, None, None  # the header verdict: nothing else was read
    v, _, rel = MF.parse_header(region, off)
    _, _, upd, um, blob = rel
    if upd != MF.INVALID:
        return MF.NOT_PUT, None, None
    um_rec, bl_rec = region[off + um:off + blob], region[off + blob:end]
    if recovery is not None and int(recovery["header_version"]) != 0:
        r = recovery
        ok = int(r["usermeta_version"]) == 1 and 1 <= int(r["blob_version"]) <= 3 and 0 <= int(r["blob_type"]) < 2
        ok = ok and int(r["usermeta_size"]) + 14 == len(um_rec)
        ok = ok and BLOB_HEAD[int(r["blob_version"])] + int(r["blob_size"]) + 8 == len(bl_rec)
        if not ok:
            return MF.BAD_RECORD, None, None
        n, bv, bt, size = int(r["usermeta_size"]), int(r["blob_version"]), int(r["blob_type"]), int(r["blob_size"])
    else:
        st = MF._record_check(3, um_rec) | _crc_bit(um_rec, MF.USERMETA_CRC)
        st |= MF._record_check(4, bl_rec) | _crc_bit(bl_rec, MF.BLOB_CRC)
        if st:
            return st, None, None
        n = struct.unpack_from(">i", um_rec, 2)[0]
        bv = struct.unpack_from(">h", bl_rec, 0)[0]
        bt = 0 if bv == 1 else struct.unpack_from(">h", bl_rec, 2)[0]
        size = struct.unpack_from(">q", bl_rec, {1: 2, 2: 4, 3: 5}[bv])[0]
    info = np.zeros((), dtype=INFO)
    info["blob_size"], info["size"], info["start"], info["usermeta_size"] = size, len(um_rec) + len(bl_rec), um, n
    info["header_version"], info["usermeta_version"], info["blob_version"], info["blob_type"] = v, 1, bv, bt
    rep = replacement(n, bv, bt, size)
    assert len(rep) == len(um_rec) + len(bl_rec)
    return 0, info, (off + um, rep)


def hard_delete(region: bytes, offs, recovery=None):
    """(status list, info array, the region after the delete) for messages at offs; every message is
    judged on the region as given (messages do not overlap)."""
    out = bytearray(region)
    status, info = [], np.zeros(len(offs), dtype=INFO)
    for i, off in enumerate(offs):
        st, inf, rep = one(region, off, None if recovery is None else recovery[i])
        status.append(st)
        if st == 0:
            info[i] = inf
            out[rep[0]:rep[0] + len(rep[1])] = rep[1]
    return status, info, bytes(out)


def counts(region: bytes, offs, status):
    """(deleted, refused for a header or record fault, NOT_PUT, deleted although another record is corrupt)."""
    deleted = sum(1 for s in status if s == 0)
    not_put = sum(1 for s in status if s == MF.NOT_PUT)
    other = sum(1 for o, s in zip(offs, status) if s == 0 and MF.verify_message(region, o)[0] != 0)
    return deleted, len(status) - deleted - not_put, not_put, other


def run_cpu(device, region: bytes, offs, recovery=None, plan_only=False):
    """(status list, info array, region after) through the CPU entry, message by message, in place."""
    buf = np.frombuffer(region, dtype=np.uint8).copy()
    status, info = [], np.zeros(len(offs), dtype=INFO)
    for i, off in enumerate(offs):
        st, inf = device.hard_delete_message_cpu(buf, off, None if recovery is None else recovery[i], plan_only)
        status.append(st)
        info[i] = inf
    return status, info, buf.tobytes()


def flip_blob_bodies(region: bytes, offs, info):
    """One byte flipped in the blob body of every third PUT with a non-empty blob (a crash mid-write)."""
    buf, n, flipped = bytearray(region), 0, 0
    for off, r in zip(offs, info):
        if int(r["header_version"]) == 0:
            continue
        n += 1
        if n % 3 == 0 and int(r["blob_size"]) > 0:
            body = off + int(r["start"]) + int(r["usermeta_size"]) + 14 + BLOB_HEAD[int(r["blob_version"])]
            buf[body + int(r["blob_size"]) // 2] ^= 0x40
            flipped += 1
    return bytes(buf), flipped


def bad_recoveries(good):
    """Recovery structs the entry must refuse (AMBRYCRC_MSG_BAD_RECORD), from a valid one."""
    out = []
    for field, value in (("usermeta_size", int(good["usermeta_size"]) + 1), ("usermeta_size", int(good["usermeta_size"]) - 1),
                         ("blob_size", int(good["blob_size"]) + 1), ("blob_size", int(good["blob_size"]) - 1),
                         ("blob_type", 2), ("blob_version", 0), ("blob_version", 4)):
        r = good.copy()
        r[field] = value
        out.append(r)
    return out
