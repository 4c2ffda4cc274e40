"""Expected results of the router's GET receive (GetBlobOperation.handleBody: deserializeBlob / deserializeBlobAll,
the content sliced to the request's range) as ambrycrc_receive_blobs_dev / ambrycrc_receive_blob_cpu define them,
from oracle/message_format.py, struct and zlib alone: independent of the library's parser, of its piecewise CRC
and of its copy-through pass. Bodies come from send_oracle.expected -- the oracle's packed spans -- so the receive
is checked against an independent producer. Shared by test_recv_cpu.py and test_gpu_recv.py."""
import functools
import struct

import numpy as np

import send_oracle as SO
from msgfmt import MF
from oracle_common import BAD_RANGE, BLOB_HEAD as HEAD, INT_MAX, NO_ROOM, NOWHERE, crc_bad, flip as _flip, place_packed, same

BLOB, ALL = SO.BLOB, SO.ALL
TO_END = 0xFFFFFFFFFFFFFFFF
CRC_BITS = MF.ENCKEY_CRC | MF.PROPS_CRC | MF.USERMETA_CRC | MF.BLOB_CRC

INFO = np.dtype([("out_off", "<u8"), ("out_len", "<u8"), ("blob_size", "<u8"), ("content_rel", "<u4"),
                 ("enckey_rel", "<u4"), ("enckey_len", "<u4"), ("props_rel", "<u4"), ("props_len", "<u4"),
                 ("usermeta_rel", "<u4"), ("usermeta_len", "<u4"), ("blob_type", "u1"), ("compressed", "u1"),
                 ("blob_version", "u1"), ("header_version", "u1")])


def _zero_info():
    f = {n: 0 for n in INFO.names}
    f["out_off"] = NOWHERE
    return f


def _refused(status):
    return status, _zero_info(), None


def receive_payload(payload: bytes, flag: int, lo: int = 0, hi: int = TO_END):
    """(status, info fields, delivered bytes or None) for one payload -- exactly its available bytes. out_off is
    0 for a delivered payload (expected() places it); rule 5 (NO_ROOM) belongs to the placement."""
    if len(payload) == 0:
        return _refused(MF.BAD_LAYOUT)
    f = _zero_info()
    rec, crc_bits = 0, 0
    if flag == ALL:
        vst, vend = MF.verify_message(payload, 0)
        if vend == 0:
            return _refused(vst)
        hv, total, rel = MF.parse_header(payload, 0)
        if rel[2] != MF.INVALID:
            return _refused(MF.NOT_PUT)
        if vst & (MF.BAD_VERSION | MF.BAD_RECORD):
            return _refused(vst & (MF.BAD_VERSION | MF.BAD_RECORD))
        crc_bits = vst & (CRC_BITS & ~MF.BLOB_CRC)  # the blob record's own below, over the record as parsed here
        rec = rel[4]
        f["header_version"] = hv
        if rel[0] != MF.INVALID:
            f["enckey_rel"], f["enckey_len"] = rel[0] + 6, MF._be32(payload, rel[0] + 2)
        f["props_rel"], f["props_len"] = rel[1] + 2, rel[3] - 8 - (rel[1] + 2)
        f["usermeta_rel"], f["usermeta_len"] = rel[3] + 6, MF._be32(payload, rel[3] + 2)
        span = vend - rec
    else:
        span = len(payload)
    # Blob_Format_V1 / V2 / V3 (MessageFormatRecord.java:1681-1833), read as a stream would
    if span < 2:
        return _refused(MF.BAD_RECORD)
    bv = struct.unpack_from(">H", payload, rec)[0]
    if bv not in HEAD:
        return _refused(MF.BAD_VERSION)
    head = HEAD[bv]
    if span < head + 8:
        return _refused(MF.BAD_RECORD)
    btype = 0 if bv == 1 else struct.unpack_from(">H", payload, rec + 2)[0]
    comp = 1 if bv == 3 and payload[rec + 4] == 1 else 0
    size = struct.unpack_from(">Q", payload, rec + head - 8)[0]
    if btype >= 2 or size > INT_MAX:
        return _refused(MF.BAD_RECORD)
    if head + size + 8 > span:
        return _refused(MF.BAD_LAYOUT)  # the stream runs dry
    end = size if hi == TO_END else hi
    if end > size or lo > end:
        return _refused(BAD_RANGE)
    content = rec + head
    if crc_bad(payload, rec, content + size + 8):
        crc_bits |= MF.BLOB_CRC
    f.update(out_off=0, out_len=end - lo, blob_size=size, content_rel=content, blob_type=btype, compressed=comp,
             blob_version=bv)
    return crc_bits, f, payload[content + lo:content + end]


def payload_of(body: bytes, off: int, size):
    """Rule 1: the payload's bytes, b"" where the offset or the size leaves the body (or the size is 0)."""
    if off >= len(body) or (size is not None and (size == 0 or off + size > len(body))):
        return b""
    return body[off:] if size is None else body[off:off + size]


def expected(body: bytes, offs, sizes, flag: int, ranges=None, dst_off=None, out_cap=None):
    """(status list, INFO array, out: uint8 array of out_cap bytes -- 0xA5 where nothing is delivered --, loose: a
    bool mask of the bytes inside the spans of payloads that failed only on a CRC, which are unspecified).
    Packed (dst_off None): slices in payload order, one past out_cap refused with NO_ROOM while the running offset
    still advances. out_cap None: exactly what the packed slices need."""
    m = len(offs)
    res = [receive_payload(payload_of(body, int(offs[i]), None if sizes is None else int(sizes[i])), flag,
                           *((0, TO_END) if ranges is None else (int(ranges[i][0]), int(ranges[i][1]))))
           for i in range(m)]
    if out_cap is None:
        assert dst_off is None
        out_cap = sum(f["out_len"] for st, f, b in res if b is not None)
    out = np.full(out_cap, 0xA5, dtype=np.uint8)
    loose = np.zeros(out_cap, dtype=bool)
    status, info = [], np.zeros(m, dtype=INFO)
    lengths = [None if b is None else len(b) for _, _, b in res]
    if dst_off is None:
        place = place_packed(lengths, out_cap)
    else:  # placed by the caller: each span alone against out_cap
        place = [None if n is None or int(d) + n > out_cap else int(d) for n, d in zip(lengths, dst_off)]
    for i, (st, f, b) in enumerate(res):
        if b is not None:
            at = place[i]
            if at is not None:
                f = dict(f, out_off=at)
                if st:
                    loose[at:at + len(b)] = True
                else:
                    out[at:at + len(b)] = np.frombuffer(b, dtype=np.uint8)
            else:
                st, f = NO_ROOM, _zero_info()
        status.append(st)
        info[i] = tuple(f[n] for n in INFO.names)
    return status, info, out, loose


def assert_outputs(got, exp):
    """Status, every info field, every delivered byte, and 0xA5 everywhere outside the delivered spans; only the
    bytes inside a CRC-failed payload's own span are exempt."""
    st, info, out = got
    est, einfo, eout, loose = exp
    same(list(st), list(est), "status")
    same(info, einfo, "info")
    out = np.asarray(out)
    assert len(out) == len(eout)
    bad = np.nonzero((out != eout) & ~loose)[0]
    assert len(bad) == 0, "output byte %d is %#x, expected %#x (%d bytes differ)" % (bad[0], out[bad[0]], eout[bad[0]], len(bad))


def mix(status):
    """How many payloads were clean, failed only on CRCs, and were refused."""
    clean = sum(1 for s in status if s == 0)
    crc = sum(1 for s in status if s and not s & ~CRC_BITS)
    return clean, crc, len(status) - clean - crc


def run_cpu(messages, body: bytes, offs, sizes, flag, ranges=None, out_cap=None):
    """A packed batch through the CPU entry, payload by payload, placed as expected() places it."""
    calls = []
    for i in range(len(offs)):
        p = payload_of(body, int(offs[i]), None if sizes is None else int(sizes[i]))
        lo, hi = (0, TO_END) if ranges is None else (int(ranges[i][0]), int(ranges[i][1]))
        calls.append((np.frombuffer(p, dtype=np.uint8), flag, lo, None if hi == TO_END else hi))
    res = [messages.receive_blob_cpu(*c) for c in calls]
    if out_cap is None:
        out_cap = sum(len(b) for _, _, b in res if b is not None)
    out = np.full(out_cap, 0xA5, dtype=np.uint8)
    status, info, pos = [], np.zeros(len(offs), dtype=INFO), 0
    place = place_packed([None if b is None else len(b) for _, _, b in res], out_cap)
    for i, (st, f, b) in enumerate(res):
        f = f.copy()
        if b is not None:
            at = place[i]
            if at is not None:
                f["out_off"] = at
                out[at:at + len(b)] = np.frombuffer(b, dtype=np.uint8)
            else:  # the call again with the room that is left: the entry's own NO_ROOM
                st, f, b2 = messages.receive_blob_cpu(*calls[i], out_cap=max(out_cap - pos, 0))
                assert b2 is None, "payload %d: delivered into %d bytes of room" % (i, max(out_cap - pos, 0))
            pos += len(b)
        status.append(st)
        info[i] = f
    return status, info, out


# ---------------------------------------------------------------- bodies from the sending side
@functools.lru_cache(maxsize=None)
def sent_region(flag: int, n=300, seed=1):
    """(body, pay_off, pay_size): rekey_oracle.build_region(n) sent under `flag` by the send oracle -- every message
    of the region, so a message the send refused arrives as (UINT64_MAX, 0), which rule 1 refuses here too."""
    import rekey_oracle as RK

    region, offs, _ = RK.build_region(n=n, seed=seed)
    _, sinfo, body = SO.expected(region, offs, None, flag)
    return body, [int(x) for x in sinfo["out_off"]], [int(x) for x in sinfo["send_len"]]


def some_ranges(body, offs, sizes, flag, seed=5):
    """A range for every payload: most inside the content (from the oracle's own blob size), every eighth to the
    content's end, every thirteenth past it (BAD_RANGE), every seventeenth empty."""
    rng = np.random.default_rng(seed)
    out = []
    for i, (o, s) in enumerate(zip(offs, sizes)):
        st, f, b = receive_payload(payload_of(body, o, s), flag)
        n = int(f["blob_size"])
        lo = int(rng.integers(0, n + 1))
        hi = int(rng.integers(lo, n + 1))
        if i % 8 == 0:
            hi = TO_END
        if i % 13 == 0:
            hi = n + 1 + i
        if i % 17 == 0:
            hi = lo
        out.append((lo, hi))
    return out


# ---------------------------------------------------------------- each rule once
def _blob(content: bytes, bv=3, btype=0, comp=False) -> bytes:
    return MF.blob_record_v1(content) if bv == 1 else MF.blob_record(content, version=bv, blob_type=btype, compressed=comp)


@functools.lru_cache(maxsize=None)
def rule_cases():
    """[(name, payload, flag, lo, hi, out_cap or None, the status the rules give)]: every refusal once, for each
    adjacent pair of rules one payload where both apply, and the clean shapes. The wanted status is written out
    here, not computed: the test holds both the library and receive_payload() to it."""
    from datagen import stream_bytes

    import rekey_oracle as RK

    content = stream_bytes(11, 0, 1000).tobytes()
    cases = []

    def add(name, payload, flag, want, lo=0, hi=TO_END, cap=None):
        cases.append((name, payload, flag, lo, hi, cap, want))

    b3 = _blob(content)
    for bv in (1, 2, 3):
        add("blob-v%d-clean" % bv, _blob(content, bv), BLOB, 0)
    add("blob-metadata-type", _blob(content, 2, btype=1), BLOB, 0)
    add("blob-compressed", _blob(content, 3, comp=True), BLOB, 0)
    add("blob-compressed-byte-2", b3[:4] + b"\x02" + b3[5:], BLOB, MF.BLOB_CRC)  # not 1: false, and the CRC sees it
    add("blob-size-0", _blob(b""), BLOB, 0)
    add("blob-size-0-v1", _blob(b"", 1), BLOB, 0)
    add("blob-trailing-bytes", b3 + b"\xEE" * 37, BLOB, 0)
    add("blob-range", b3, BLOB, 0, lo=100, hi=900)
    add("blob-range-empty", b3, BLOB, 0, lo=1000, hi=1000)
    add("blob-range-to-end", b3, BLOB, 0, lo=999)
    # rule 1
    add("r1-no-bytes", b"", BLOB, MF.BAD_LAYOUT)
    add("r1-no-bytes-all", b"", ALL, MF.BAD_LAYOUT)
    # rule 2
    add("r2-one-byte", b"\x00", BLOB, MF.BAD_RECORD)
    add("r2-version-0", b"\x00\x00" + b3[2:], BLOB, MF.BAD_VERSION)
    add("r2-version-4", b"\x00\x04" + b3[2:], BLOB, MF.BAD_VERSION)
    add("r2-version-and-short", b"\x00\x09\x00", BLOB, MF.BAD_VERSION)
    add("r2-short", b3[:20], BLOB, MF.BAD_RECORD)
    add("r2-short-v1", _blob(content, 1)[:17], BLOB, MF.BAD_RECORD)
    add("r2-type-2", b3[:2] + b"\x00\x02" + b3[4:], BLOB, MF.BAD_RECORD)
    add("r2-type-negative", b3[:2] + b"\xff\xff" + b3[4:], BLOB, MF.BAD_RECORD)
    add("r2-size-above-max-int", b3[:5] + struct.pack(">Q", 1 << 31) + b3[13:], BLOB, MF.BAD_RECORD)
    add("r2-size-negative", b3[:5] + struct.pack(">q", -1) + b3[13:], BLOB, MF.BAD_RECORD)
    add("r2-record-and-layout", b3[:2] + b"\x00\x02" + b3[4:40], BLOB, MF.BAD_RECORD)  # a bad type in a cut record
    add("r2-cut-by-one", b3[:-1], BLOB, MF.BAD_LAYOUT)
    add("r2-cut-in-content", b3[:500], BLOB, MF.BAD_LAYOUT)
    # rule 3
    put = RK.stored_put(MF.store_key("rule"), MF.blob_properties_bytes(1000), stream_bytes(3, 1, 50).tobytes(), content,
                        hv=3, enc_key=b"k" * 32, bv=2)
    _, _, rel = MF.parse_header(put, 0)
    add("all-clean", put, ALL, 0)
    add("all-clean-v1", RK.stored_put(MF.store_key("rule1"), MF.blob_properties_bytes(1000, serde_version=2), b"", content,
                                      hv=1, bv=1), ALL, 0)
    add("all-trailing-bytes", put + b"\xEE" * 21, ALL, 0)
    add("all-range", put, ALL, 0, lo=1, hi=999)
    add("r3-header-version", b"\x00\x07" + put[2:], ALL, MF.BAD_VERSION)
    add("r3-header-crc", _flip(put, 5), ALL, MF.HEADER_CRC)
    add("r3-header-cut", put[:30], ALL, MF.BAD_LAYOUT)
    add("r3-message-cut", put[:-1], ALL, MF.BAD_LAYOUT)
    upd = MF.update_message(MF.store_key("rule-u"), version=3, kind="ttl")
    add("r3-update", upd, ALL, MF.NOT_PUT)
    add("r3-update-bad-record", _flip(upd, MF.parse_header(upd, 0)[2][2] + 1), ALL, MF.NOT_PUT)  # NOT_PUT comes first
    add("r3-enckey-version", SO._refit(put, rel[0], rel[1], lambda r: r.__setitem__(1, 2)), ALL, MF.BAD_VERSION)
    add("r3-enckey-size", SO._refit(put, rel[0], rel[1], lambda r: r.__setitem__(5, r[5] + 1)), ALL, MF.BAD_RECORD)
    add("r3-blob-type", SO._refit(put, rel[4], len(put), lambda r: r.__setitem__(3, 2)), ALL, MF.BAD_RECORD)
    two = SO._refit(SO._refit(put, rel[0], rel[1], lambda r: r.__setitem__(1, 2)), rel[3], rel[4],
                    lambda r: r.__setitem__(5, r[5] + 1))
    add("r3-two-records", two, ALL, MF.BAD_VERSION | MF.BAD_RECORD)  # every record-check bit
    # rule 4
    add("r4-lo-above-hi", b3, BLOB, BAD_RANGE, lo=10, hi=9)
    add("r4-hi-above-size", b3, BLOB, BAD_RANGE, lo=0, hi=1001)
    add("r4-lo-above-size-to-end", b3, BLOB, BAD_RANGE, lo=1001)
    add("r4-all", put, ALL, BAD_RANGE, lo=0, hi=1001)
    # rule 5
    add("r5-exact", b3, BLOB, 0, cap=1000)
    add("r5-one-less", b3, BLOB, NO_ROOM, cap=999)
    add("r5-range-exact", b3, BLOB, 0, lo=10, hi=20, cap=10)
    add("r5-range-one-less", put, ALL, NO_ROOM, lo=10, hi=20, cap=9)
    add("r5-empty-in-no-room", b3, BLOB, 0, lo=7, hi=7, cap=0)
    # rule 6
    add("r6-head", _flip(b3, 4, 0x02), BLOB, MF.BLOB_CRC)  # the compressed byte becomes 2: still a valid head
    add("r6-content", _flip(b3, 13 + 500), BLOB, MF.BLOB_CRC)
    add("r6-content-outside-the-range", _flip(b3, 13 + 5), BLOB, MF.BLOB_CRC, lo=100, hi=200)
    add("r6-trailer-low", _flip(b3, len(b3) - 1), BLOB, MF.BLOB_CRC)
    add("r6-trailer-high", _flip(b3, len(b3) - 6), BLOB, MF.BLOB_CRC)
    add("r6-all-enckey", _flip(put, rel[0] + 10), ALL, MF.ENCKEY_CRC)
    add("r6-all-props", _flip(put, rel[1] + 12), ALL, MF.PROPS_CRC)
    add("r6-all-usermeta", _flip(put, rel[3] + 9), ALL, MF.USERMETA_CRC)
    add("r6-all-blob", _flip(put, rel[4] + 500), ALL, MF.BLOB_CRC)
    add("r6-all-three", _flip(_flip(_flip(put, rel[0] + 10), rel[3] + 9), len(put) - 7), ALL,
        MF.ENCKEY_CRC | MF.USERMETA_CRC | MF.BLOB_CRC)
    add("r6-all-key-is-not-hashed", _flip(put, 40 + 3), ALL, 0)  # the store key: the caller's comparison
    # adjacent pairs: the earlier rule wins
    add("p24-version-and-range", b"\x00\x04" + b3[2:], BLOB, MF.BAD_VERSION, lo=10, hi=9)
    add("p24-layout-and-range", b3[:-1], BLOB, MF.BAD_LAYOUT, lo=0, hi=5000)
    add("p34-update-and-range", upd, ALL, MF.NOT_PUT, lo=10, hi=9)
    add("p34-record-and-range", SO._refit(put, rel[0], rel[1], lambda r: r.__setitem__(1, 2)), ALL, MF.BAD_VERSION, lo=0, hi=5000)
    add("p45-range-and-no-room", b3, BLOB, BAD_RANGE, lo=0, hi=1001, cap=0)
    add("p56-no-room-and-crc", _flip(b3, 13 + 500), BLOB, NO_ROOM, cap=999)
    add("p56-no-room-and-crc-all", _flip(put, rel[1] + 12), ALL, NO_ROOM, cap=3)
    return cases
