"""Expected results of a PutRequest ingest (PutRequest.readFrom, ambry-protocol/.../PutRequest.java:191-204,
:440-521, then AmbryRequests.getMessageFormatWriteSet, AmbryRequests.java:1957-1970), from
oracle/message_format.py and zlib alone: independent of the library's wire parse, of its combination of the
wire CRC from segment CRCs and of its V5 re-encoding. Shared by test_ingest.py and test_gpu_ingest.py, with
the frame and wire builders both use.

The skeleton is the reference's: read the frame field by field (a read that throws or passes the frame's end
refuses it), compare zlib's CRC of the bytes between the client id and the CRC with the stored long, parse the
properties, serialize them again at VERSION_5 and write the message through MF.put_message."""
import struct
import zlib

import numpy as np

from datagen import stream_bytes
from msgfmt import MF
from oracle_common import (BAD_DESC, BAD_INFO, INT_MAX, MESSAGE_INFO as INFO, NO_ROOM, NOWHERE, WIRE_CRC,
                           add_seconds_to_epoch, place_packed)

BAD_VERSION = MF.BAD_VERSION
NOT_PUT = MF.NOT_PUT
BAD_RECORD = MF.BAD_RECORD
NOT_ENCODABLE = MF.NOT_ENCODABLE
# every refusal a small wire buffer can hold (NO_ROOM comes from out_cap; the Java-int refusal needs a 2 GiB frame,
# which test_gpu_big_blob.py builds on the device and big_message.frame_with_usermeta describes)
WIRE_STATUSES = (BAD_DESC, NOT_PUT, BAD_VERSION, BAD_RECORD, WIRE_CRC, NOT_ENCODABLE, BAD_INFO)
FIXED = 20      # size, type, version, correlationId, clientIdLen
MIN_FRAME = 81  # FIXED + SerDe V1 with empty strings (39) + umSize + blobType + blobSize + CRC
GROWTH_MAX = 72  # AMBRYCRC_INGEST_GROWTH_MAX

REF = np.dtype([("off", "<u8"), ("key_len", "<u4"), ("reserved", "<u4")])


# ---------------------------------------------------------------- frames
def frame(version, blob_id, props, um, blob, blob_type=0, enc_key=b"", compressed=0, client_id=b"", correlation=7,
          slack=0, type_=0, um_size=None, enc_len=None, blob_size=None, client_len=None, size=None, crc=None,
          wire_version=None):
    """A PutRequest frame at `version` 3..5 (RequestOrResponse.writeHeader + PutRequest.prepareBuffer). The
    keyword overrides write a size field or the CRC other than the true one; compressed is the raw byte."""
    body = blob_id + props + struct.pack(">i", len(um) if um_size is None else um_size) + um
    body += struct.pack(">h", blob_type)
    if version >= 4:
        body += struct.pack(">h", len(enc_key) if enc_len is None else enc_len) + enc_key
    if version >= 5:
        body += struct.pack(">B", compressed)
    body += struct.pack(">q", len(blob) if blob_size is None else blob_size) + blob
    tail = struct.pack(">Q", zlib.crc32(body) if crc is None else crc)
    head = struct.pack(">hhii", type_, version if wire_version is None else wire_version, correlation,
                       len(client_id) if client_len is None else client_len) + client_id
    n = 8 + len(head) + len(body) + 8 + slack
    return struct.pack(">q", n if size is None else size) + head + body + tail + bytes([0x5A]) * slack


def ingest_request(wire: bytes, off: int, key_len: int, header_version: int = 3, reserved: int = 0):
    """(status, message bytes or None, wire CRC (0 where the parse refused), info tuple or None) for the
    frame at `off`; info as the INFO record with msg_off 0."""
    n = len(wire)
    if reserved != 0 or off > n or n - off < FIXED:
        return BAD_DESC, None, 0, None
    size, type_, version, _corr, client = struct.unpack_from(">qhhii", wire, off)
    if size < MIN_FRAME or off + size > n:
        return BAD_DESC, None, 0, None
    if type_ != 0:
        return NOT_PUT, None, 0, None
    if version not in (3, 4, 5):
        return BAD_VERSION, None, 0, None
    end = off + size
    pos = off + FIXED

    class Eof(Exception):
        pass

    def take(k):
        nonlocal pos
        if k < 0 or pos + k > end:
            raise Eof()
        s = wire[pos:pos + k]
        pos += k
        return s

    try:
        take(client)
        start = pos
        blob_id = take(key_len)
        try:
            f, pos = MF.parse_blob_properties(wire, pos, end)
        except MF.PropsParseError:
            raise Eof()
        um = take(struct.unpack(">i", take(4))[0])
        blob_type = struct.unpack(">h", take(2))[0]
        if blob_type not in (0, 1):
            raise Eof()
        enc_key = take(struct.unpack(">h", take(2))[0]) if version >= 4 else b""
        compressed = take(1)[0] == 1 if version >= 5 else False
        blob_size = struct.unpack(">q", take(8))[0]
        if blob_size > INT_MAX:
            raise Eof()
        blob = take(blob_size)
        computed = zlib.crc32(wire[start:pos])
        stored = struct.unpack(">Q", take(8))[0]
    except Eof:
        return BAD_RECORD, None, 0, None
    if computed != stored:
        return WIRE_CRC, None, computed, None
    try:
        props = MF.serialize_blob_properties_v5(f)
    except MF.NotEncodable:
        return NOT_ENCODABLE, None, computed, None
    if f["creation"] < -1:
        return BAD_INFO, None, computed, None
    msg = MF.put_message(blob_id, props, um, blob, version=header_version,
                         enc_key=enc_key if len(enc_key) else None, life=0, compressed=compressed,
                         blob_type=blob_type)
    info = (0, len(msg), add_seconds_to_epoch(f["creation"], f["ttl"]), f["creation"], MF.HEADER_SIZE[header_version],
            len(blob_id), f["account"], f["container"], 0, 0, header_version)
    return 0, msg, computed, info


def expected(wire: bytes, refs, header_version: int = 3, out_cap=None):
    """The batch: (status uint32[m], out bytes, out_off uint64[m], out_len uint64[m], wire_crc uint32[m],
    info INFO[m], total). Packed in request order; a message past out_cap is NO_ROOM and still advances."""
    m = len(refs)
    status = np.zeros(m, dtype=np.uint32)
    out_off = np.full(m, NOWHERE, dtype=np.uint64)
    out_len = np.zeros(m, dtype=np.uint64)
    crc = np.zeros(m, dtype=np.uint32)
    info = np.zeros(m, dtype=INFO)
    res = [ingest_request(wire, int(r["off"]), int(r["key_len"]), header_version, int(r["reserved"])) for r in refs]
    place = place_packed([len(msg) if st == 0 else None for st, msg, _, _ in res], out_cap)
    packed = bytearray()
    for i, ((st, msg, c, inf), at) in enumerate(zip(res, place)):
        crc[i] = c
        if at is not None:
            packed += bytes(at - len(packed)) + msg
            out_off[i], out_len[i] = at, len(msg)
            info[i] = (at,) + inf[1:]
        elif st == 0:
            st = NO_ROOM
        status[i] = st
    return status, bytes(packed), out_off, out_len, crc, info, len(packed)


# ---------------------------------------------------------------- wire buffers
def nonzero_bytes(stream, lane, n):
    """n content bytes, none zero."""
    b = stream_bytes(stream, lane, n).copy()
    b[b == 0] = 0xA7
    return b.tobytes()


def props_for(rng, blob_size, serde, non_ascii=False, creation=None):
    owner = "owéner".encode() if non_ascii else "owner%d" % int(rng.integers(0, 1000))
    return MF.blob_properties_bytes(
        blob_size, owner_id=owner, ttl=int(rng.choice([-1, 0, 3600, 1 << 40])),
        private=int(rng.choice([0, 1, 2, -1])), encrypted=int(rng.choice([0, 1, 3])),
        creation_ms=int(rng.choice([-1, 0, 1_700_000_000_000])) if creation is None else creation,
        account=int(rng.integers(-1, 3000)), container=int(rng.integers(-1, 3000)),
        content_encoding=None if rng.integers(0, 2) else "gzip", filename=None if rng.integers(0, 2) else "f.bin",
        reserved=None if rng.integers(0, 2) else "rsv", serde_version=serde)


REFUSALS = ("reserved", "off_past", "size_small", "size_big", "type", "version_low", "version_high", "client_neg",
            "key_over", "serde", "um_neg", "blob_type", "enc_neg", "blob_neg", "blob_huge", "no_crc", "flip_key",
            "flip_props", "flip_um", "flip_enc", "flip_blob", "crc_high", "non_ascii", "creation")


# pairs of REFUSALS that write the same field of a frame, so one frame cannot hold both
INCOMPATIBLE = {frozenset(p): why for p, why in (
    (("version_low", "version_high"), "both set the request version"),
    (("size_small", "size_big"), "both set the frame size"),
    (("size_small", "no_crc"), "both set the frame size"),
    (("size_big", "no_crc"), "both set the frame size"),
    (("blob_neg", "blob_huge"), "both set the blob size"))}


def one_frame(rng, i, seed, refusal=None, blob_len=None):
    """(frame bytes, key_len, reserved, off_delta) of request i. refusal: None, one of REFUSALS, or a tuple of
    them that can coexist in one frame (INCOMPATIBLE lists the pairs that cannot)."""
    rs = () if refusal is None else (refusal,) if isinstance(refusal, str) else tuple(refusal)
    assert all(r in REFUSALS for r in rs) and not any(frozenset((a, b)) in INCOMPATIBLE for a in rs for b in rs)
    version = 3 + i % 3
    serde = 1 + (i // 3) % 5
    key_len = int(rng.choice([0, 24, 40, 57]))
    um_len = int(rng.choice([0, 1, 100, 777]))
    enc_len = int(rng.choice([0, 0, 32, 100])) if version >= 4 else 0
    if "flip_enc" in rs:
        version, enc_len = 4 + i % 2, 32
    if "enc_neg" in rs:
        version = 4 + i % 2
    if "flip_key" in rs or "key_over" in rs:
        key_len = 24
    if "flip_um" in rs:
        um_len = 100
    if blob_len is None:
        blob_len = int(rng.choice([0, 1, 63, 300, 4096, 5000, 20000, 70001]))
    if "flip_blob" in rs:
        blob_len = max(blob_len, 1)
    client = b"" if i % 4 == 0 else b"client-%d" % i
    kw = dict(blob_type=i % 2, enc_key=nonzero_bytes(seed, 4 * i + 1, enc_len), compressed=int(rng.choice([0, 1, 2])),
              client_id=client, correlation=i, slack=int(rng.choice([0, 0, 0, 5])))
    props = props_for(rng, blob_len, serde, non_ascii="non_ascii" in rs,
                      creation=-5 if "creation" in rs else None)
    reserved, ref_key = 0, key_len
    if "reserved" in rs:
        reserved = 1
    if "size_small" in rs:
        kw["size"] = MIN_FRAME - 1
    if "size_big" in rs:
        kw["size"] = 1 << 40
    if "type" in rs:
        kw["type_"] = 2
    if "version_low" in rs:
        kw["wire_version"] = 2
    if "version_high" in rs:
        kw["wire_version"] = 6
    if "client_neg" in rs:
        kw["client_len"] = -1
    if "serde" in rs:
        props = struct.pack(">h", 9) + props[2:]
    if "um_neg" in rs:
        kw["um_size"] = -2
    if "blob_type" in rs:
        kw["blob_type"] = 2
    if "enc_neg" in rs:
        kw["enc_len"] = -1
    if "blob_neg" in rs:
        kw["blob_size"] = -1
    if "blob_huge" in rs:
        kw["blob_size"] = INT_MAX + 1
    if "crc_high" in rs:
        kw["crc"] = None
    fr = frame(version, nonzero_bytes(seed, 4 * i, key_len), props, nonzero_bytes(seed, 4 * i + 2, um_len),
               nonzero_bytes(seed, 4 * i + 3, blob_len), **kw)
    if "key_over" in rs:
        ref_key = len(fr)
    if "no_crc" in rs:  # the frame ends 4 bytes into its CRC
        fr = struct.pack(">q", len(fr) - kw["slack"] - 4) + fr[8:]
    for r in rs:
        if not (r.startswith("flip_") or r == "crc_high"):
            continue
        body = FIXED + len(client)
        at = {"flip_key": body, "flip_props": body + key_len + 5, "flip_um": body + key_len + len(props) + 4 + 7,
              "flip_enc": body + key_len + len(props) + 4 + um_len + 4 + 5,
              "flip_blob": len(fr) - kw["slack"] - 8 - 1, "crc_high": len(fr) - kw["slack"] - 8 + 2}[r]
        fr = fr[:at] + bytes([fr[at] ^ 0x10]) + fr[at + 1:]
    return fr, ref_key, reserved, (1 << 50 if "off_past" in rs else 0)


def pair_wire(seed=5, clean_between=False):
    """(wire, refs, pairs, skipped): one frame for every pair of REFUSALS that one frame can hold, in REFUSALS
    order, small blobs, frames end to end; skipped: {pair: why} for the pairs left out (INCOMPATIBLE).
    clean_between: a clean frame before each of them (None in pairs), so refused requests lie among placed ones."""
    rng = np.random.default_rng(seed)
    parts, refs, pairs, skipped, pos = [], [], [], {}, 0
    for x, a in enumerate(REFUSALS):
        for b in REFUSALS[x + 1:]:
            if frozenset((a, b)) in INCOMPATIBLE:
                skipped[a, b] = INCOMPATIBLE[frozenset((a, b))]
                continue
            for kind in ((None, (a, b)) if clean_between else ((a, b),)):
                fr, key_len, reserved, delta = one_frame(rng, len(pairs), seed, kind, 40 + len(pairs) % 60)
                parts.append(fr)
                refs.append((pos + delta, key_len, reserved))
                pairs.append(kind)
                pos += len(fr)
    return b"".join(parts), np.array(refs, dtype=REF), pairs, skipped


def build_wire(n, seed, refused=0.1, gap=3, blobs=None):
    """(wire bytes, refs REF[n], kinds: the refusal each request was built with or None). Every request
    version, SerDe V1..V5 with non-canonical flag bytes, keys and encryption keys absent and present, both blob
    types, empty client ids; about `refused` of them refused, cycling through REFUSALS. blobs: the blob
    lengths to draw from (default: 0 to 70,001 bytes)."""
    rng = np.random.default_rng(seed)
    parts, refs, kinds, pos, nref = [], np.zeros(n, dtype=REF), [], 0, 0
    for i in range(n):
        kind = None
        if rng.random() < refused:
            kind = REFUSALS[(nref + seed) % len(REFUSALS)]
            nref += 1
        fr, key_len, reserved, delta = one_frame(rng, i, seed, kind,
                                                 None if blobs is None else int(rng.choice(blobs)))
        pad = bytes(int(rng.integers(0, gap + 1)))
        parts += [pad, fr]
        pos += len(pad)
        refs[i] = (pos + delta, key_len, reserved)
        pos += len(fr)
        kinds.append(kind)
    return b"".join(parts), refs, kinds


def assert_mix(wire, refs, status):
    """Every wire status and every request version occurs, and most requests are clean."""
    seen = set(int(s) for s in status)
    for s in WIRE_STATUSES:
        assert s in seen, hex(s)
    versions = set()
    for r, s in zip(refs, status):
        if s == 0:
            versions.add(struct.unpack_from(">h", wire, int(r["off"]) + 10)[0])
    assert versions == {3, 4, 5}
    assert (status == 0).sum() >= len(status) * 3 // 4


# ---------------------------------------------------------------- a tile, repeated
TILE = 1201
_TILE = []


def tile_case():
    """(wire, refs, expected) of one tile of TILE mixed small frames, laid end to end."""
    if not _TILE:
        wire, refs, _ = build_wire(TILE, 77, blobs=(0, 1, 63, 300), gap=0)
        _TILE.append((wire, refs, expected(wire, refs)))
    return _TILE[0]


def tiled(refs, exp, k, wire_len):
    """The references and expectations of k concatenated tiles, derived from one tile's: (refs, status, out_off,
    out_len, wire_crc, info). A reference that points past the tile keeps pointing past all of them."""
    est, _, eoff, eln, ecrc, einfo, etotal = exp
    step = np.arange(k, dtype=np.uint64)[:, None]
    r = np.tile(refs, k).reshape(k, -1).copy()
    inside = refs["off"] < wire_len
    r["off"] = np.where(inside[None, :], refs["off"][None, :] + step * np.uint64(wire_len), refs["off"][None, :])
    off = np.where((eln > 0)[None, :], eoff[None, :] + step * np.uint64(etotal), eoff[None, :])
    info = np.tile(einfo, k).reshape(k, -1).copy()
    info["msg_off"] = np.where((eln > 0)[None, :], einfo["msg_off"][None, :] + step * np.uint64(etotal), 0)
    return r.reshape(-1), np.tile(est, k), off.reshape(-1), np.tile(eln, k), np.tile(ecrc, k), info.reshape(-1)
