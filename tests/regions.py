"""Region and message builders of the suite: stored messages and log regions for the verify, hard delete and
transform tests, PutMessage batches for the write side and PutRequest fields for the protocol tests. Every byte comes from oracle/message_format.py (MF), struct, zlib and datagen's streams; a
builder's output for given arguments is fixed (tools/test_data_digests.py prints a digest per case)."""
import struct
import zlib

import numpy as np

from datagen import stream_bytes
from msgfmt import MF


def join(msgs):
    """(region, starts) of messages laid end to end."""
    offs, pos = [], 0
    for m in msgs:
        offs.append(pos)
        pos += len(m)
    return b"".join(msgs), offs


# ---------------------------------------------------------------- regions for the message verify
def verify_region(n=300, seed=7, corrupt_frac=0.1, big_every=17):
    """A log region of PUT (V1/V2/V3, +/- encryption key) and update messages, some corrupted.
    Returns (region bytes, message offsets, expected status list from the oracle)."""
    rng = np.random.default_rng(seed)
    out = bytearray()
    offs = []
    for i in range(n):
        key = MF.store_key(f"blob-{i:06d}-{seed}")
        kind = rng.integers(0, 10)
        if kind == 0:
            msg = MF.update_message(key, version=3, kind=["ttl", "delete", "undelete"][i % 3])
        else:
            ver = [1, 2, 3, 3][int(rng.integers(0, 4))]
            size = int(rng.integers(0, 5000)) if i % big_every else int(rng.integers(60000, 300000))
            content = stream_bytes(seed * 100003 + i, 0, size).tobytes()
            um = stream_bytes(seed + i, 7, int(rng.integers(0, 1200))).tobytes()
            enc = stream_bytes(i, 3, 100).tobytes() if (ver >= 2 and i % 2) else None
            msg = MF.put_message(key, MF.blob_properties_bytes(size), um, content, version=ver, enc_key=enc,
                                 life=int(i % 3), compressed=bool(i % 5 == 0))
        offs.append(len(out))
        out += msg
    region = bytearray(out)
    for i in rng.choice(n, size=int(n * corrupt_frac), replace=False):
        start = offs[i]
        end = offs[i + 1] if i + 1 < n else len(region)
        pos = int(rng.integers(start, end))
        region[pos] ^= 1 << int(rng.integers(0, 8))
    region = bytes(region)
    expect = [MF.verify_message(region, o) for o in offs]
    return region, offs, expect


# ---------------------------------------------------------------- CRC-valid messages with bad record fields
def _seal(body: bytes) -> bytes:
    return body + struct.pack(">q", zlib.crc32(body))


def _assemble(version, key, enc, pr, um, bl, upd=None):
    """A message from already-sealed records (header offsets from their lengths, header CRC valid)."""
    h = MF.HEADER_SIZE[version]
    if upd is not None:
        return MF.header(version, len(upd), MF.INVALID, MF.INVALID, h + len(key), MF.INVALID, MF.INVALID) + key + upd
    enc = enc or b""
    bp = h + len(key) + len(enc)
    total = len(enc) + len(pr) + len(um) + len(bl)
    return MF.header(version, total, h + len(key) if enc else MF.INVALID, bp, MF.INVALID, bp + len(pr),
                     bp + len(pr) + len(um)) + key + enc + pr + um + bl


def record_level_cases():
    """(message, expected status) pairs whose every CRC is valid but whose record fields are not
    what the reference's deserializers accept (MessageFormatRecord.java:147-239, 1588-1833):
    unknown record versions -> BAD_VERSION; size fields that disagree with the header's record
    span, blob type ordinals >= 2, blob sizes > Integer.MAX_VALUE -> BAD_RECORD."""
    key = MF.store_key("rec-level")
    props = MF.blob_properties_bytes(300)
    content = bytes(range(200)) + bytes(100)
    ek = b"e" * 32
    pr, um = MF.props_record(props), MF.usermeta_record(b"meta" * 5)
    bl, enc = MF.blob_record(content), MF.enckey_record(ek)
    cases = [
        (_assemble(3, key, enc, pr, um, bl), 0),
        (_assemble(2, key, None, pr, um, MF.blob_record_v1(content)), 0),
        (_assemble(3, key, None, pr, um, MF.blob_record(content, version=2, blob_type=1)), 0),
        (_assemble(3, key, _seal(struct.pack(">hi", 2, len(ek)) + ek), pr, um, bl), MF.BAD_VERSION),
        (_assemble(3, key, _seal(struct.pack(">hi", 1, len(ek) + 1) + ek), pr, um, bl), MF.BAD_RECORD),
        (_assemble(3, key, None, _seal(struct.pack(">h", 2) + props), um, bl), MF.BAD_VERSION),
        (_assemble(3, key, None, pr, _seal(struct.pack(">hi", 0, 20) + b"meta" * 5), bl), MF.BAD_VERSION),
        (_assemble(3, key, None, pr, _seal(struct.pack(">hi", 1, 19) + b"meta" * 5), bl), MF.BAD_RECORD),
        (_assemble(3, key, None, pr, _seal(struct.pack(">hi", 1, -4) + b"meta" * 5), bl), MF.BAD_RECORD),
        (_assemble(3, key, None, pr, um, _seal(struct.pack(">hhbq", 3, 2, 0, len(content)) + content)),
         MF.BAD_RECORD),
        (_assemble(3, key, None, pr, um, _seal(struct.pack(">hhbq", 4, 0, 0, len(content)) + content)),
         MF.BAD_VERSION),
        (_assemble(3, key, None, pr, um, _seal(struct.pack(">hhbq", 3, 0, 0, len(content) - 1) + content)),
         MF.BAD_RECORD),
        (_assemble(3, key, None, pr, um, _seal(struct.pack(">hhbq", 3, 0, 0, len(content) + (1 << 32)) + content)),
         MF.BAD_RECORD),
        (_assemble(1, key, None, pr, um, _seal(struct.pack(">hq", 1, len(content) + 3) + content)), MF.BAD_RECORD),
        (_assemble(3, key, None, pr, um, _seal(struct.pack(">hhq", 2, 7, len(content)) + content)), MF.BAD_RECORD),
    ]
    upd = bytearray(MF.update_record_v3())
    upd[0:2] = struct.pack(">h", 4)
    cases.append((_assemble(3, key, None, None, None, None, upd=_seal(bytes(upd[:-8]))), MF.BAD_VERSION))
    cases.append((_assemble(3, key, None, None, None, None, upd=MF.update_record_v3(kind="delete")), 0))
    cases += props_level_cases(key, um, bl) + update_level_cases(key)
    return cases


def _props_msg(key, um, bl, serde: bytes, version=3):
    return _assemble(version, key, None, _seal(struct.pack(">h", 1) + serde), um, bl)


def props_level_cases(key, um, bl):
    """CRC-valid BlobProperties records through BlobPropertiesSerDe.getBlobPropertiesFromStream
    (BlobPropertiesSerDe.java:56-77) under deserializeBlobPropertiesRecord's catch-all
    (MessageFormatRecord.java:1179-1195: any exception -> DataCorrupt = BAD_RECORD)."""
    cases = []
    for v in (1, 2, 3, 4, 5):  # every stored version reads clean
        cases.append((_props_msg(key, um, bl, MF.blob_properties_bytes(
            300, serde_version=v, content_encoding="gzip", filename="f", reserved="r")), 0))
    good = MF.blob_properties_bytes(300, content_encoding="gzip", filename="name.bin")
    for bad_v in (0, 6, 9, -1):  # "stream has unknown blob property version"
        cases.append((_props_msg(key, um, bl, struct.pack(">h", bad_v) + good[2:]), MF.BAD_RECORD))
    # contentType's int size: past the span / negative / one short (the fields end early)
    ct = 27
    for n, want in ((1 << 20, MF.BAD_RECORD), (-2, MF.BAD_RECORD), (0x7FFFFFFF, MF.BAD_RECORD)):
        b = bytearray(good)
        b[ct:ct + 4] = struct.pack(">i", n)
        cases.append((_props_msg(key, um, bl, bytes(b)), want))
    cases.append((_props_msg(key, um, bl, good + b"\0"), MF.BAD_RECORD))  # trailing byte: CRC read early
    cases.append((_props_msg(key, um, bl, good[:-1]), MF.BAD_RECORD))      # last string cut: EOF
    cases.append((_props_msg(key, um, bl, good[:20]), MF.BAD_RECORD))      # inside the fixed fields
    v4 = MF.blob_properties_bytes(300, serde_version=4, filename="abc")
    cases.append((_props_msg(key, um, bl, v4[:-7] + struct.pack(">i", -1) + b"abc"), MF.BAD_RECORD))
    # non-canonical private / encrypted bytes and non-ASCII strings still verify (decoding never throws)
    cases.append((_props_msg(key, um, bl, MF.blob_properties_bytes(300, private=7, encrypted=2)), 0))
    cases.append((_props_msg(key, um, bl, MF.blob_properties_bytes(300, owner_id=b"\xc3\xa9t\xff")), 0))
    return cases


def update_level_cases(key):
    """CRC-valid update records through deserializeUpdateRecord (MessageFormatRecord.java:158-172,
    1217-1228, 1253-1266, 1388-1464)."""
    def upd_msg(body):
        return _assemble(3, key, None, None, None, None, upd=_seal(body))

    base = struct.pack(">hhhq", 3, 101, 5, 1_700_000_000_123)
    return [
        (upd_msg(struct.pack(">hb", 1, 1)), 0),                                  # V1: a delete flag
        (upd_msg(struct.pack(">hb", 1, 1) + b"x"), MF.BAD_RECORD),
        (upd_msg(struct.pack(">hhhq", 2, 101, 5, 7)), 0),                          # V2
        (upd_msg(struct.pack(">hhhq", 2, 101, 5, 7)[:-1]), MF.BAD_RECORD),
        (upd_msg(base + struct.pack(">hhq", 1, 1, 99)), 0),                        # V3 TTL_UPDATE
        (upd_msg(base + struct.pack(">hh", 2, 1)), 0),                             # V3 UNDELETE
        (upd_msg(base + struct.pack(">hh", 3, 1)), MF.BAD_RECORD),                 # Type.values()[3]
        (upd_msg(base + struct.pack(">hh", -1, 1)), MF.BAD_RECORD),
        (upd_msg(base + struct.pack(">hh", 0, 2)), MF.BAD_VERSION),                # delete sub-record v2
        (upd_msg(base + struct.pack(">hhq", 1, 0, 99)), MF.BAD_VERSION),           # ttl sub-record v0
        (upd_msg(base + struct.pack(">hh", 0, 1) + bytes(8)), MF.BAD_RECORD),      # delete + 8 stray bytes
        (upd_msg(base + struct.pack(">hh", 1, 1)), MF.BAD_RECORD),                 # TTL without its expiry
        (upd_msg(base), MF.BAD_RECORD),                                          # no type
        (upd_msg(struct.pack(">hhhq", 0, 1, 1, 1) + bytes(2)), MF.BAD_VERSION),
    ]


# ---------------------------------------------------------------- regions as replication reads them
def blob_v1_message(key, props, um, content, version):
    """A PUT whose blob record is Blob_Format_V1 (stored by old servers)."""
    h = MF.HEADER_SIZE[version]
    pr, ur, bl = MF.props_record(props), MF.usermeta_record(um), MF.blob_record_v1(content)
    bp = h + len(key)
    return MF.header(version, len(pr) + len(ur) + len(bl), MF.INVALID, bp, MF.INVALID, bp + len(pr),
                     bp + len(pr) + len(ur), 0) + key + pr + ur + bl


def stored_props(rng, blen, i):
    """BlobPropertiesSerDe bytes as servers of every version stored them (V1..V5), some with
    non-canonical private / encrypted bytes (read as `== 1`), a few with a non-ASCII string
    (the transform cannot re-encode those: NOT_ENCODABLE)."""
    v = int(rng.choice([1, 2, 3, 4, 5], p=[0.15, 0.15, 0.15, 0.15, 0.4]))
    odd = rng.random() < 0.15
    s = rng.random()
    owner = b"own\xc3\xa9r" if s < 0.03 else ("o%d" % (i % 5) if s < 0.8 else None)
    return MF.blob_properties_bytes(
        blen, service_id="s%d" % (i % 7), owner_id=owner, content_type=None if i % 9 == 0 else "application/x",
        ttl=int(rng.integers(-1, 10**6)), private=int(rng.choice([0, 1, 2])) if odd else bool(i % 2),
        encrypted=int(rng.choice([0, 1, 5])) if odd else bool(i % 3 == 0),
        content_encoding="gzip" if i % 4 == 0 else None, filename="file-%d.bin" % i if i % 5 else None,
        reserved="res%d" % i if i % 6 == 0 else None, account=int(rng.integers(-5, 30000)), container=i % 300,
        serde_version=v)


def replica_region(n, seed, corrupt=True):
    """(region, offsets) as replication reads them: stored messages of every header version, SerDe V1..V5
    properties, blob records V1 / V2 / V3, update messages and bad blob types, about 7 % with a flipped bit
    (corrupt), 0-4 bytes of gap before each message."""
    rng = np.random.default_rng(seed)
    msgs = []
    for i in range(n):
        kind = rng.random()
        v = int(rng.choice([1, 2, 3]))
        key = MF.store_key("rep-%d" % i)
        blen = int(rng.choice([0, 1, 100, 4096, 4109, 70000]))
        content = stream_bytes(seed + i, 0, blen).tobytes()
        um = stream_bytes(seed + i, 1 << 20, int(rng.choice([0, 7, 1000]))).tobytes()
        props = stored_props(rng, blen, i)
        if kind < 0.08:
            m = MF.update_message(key, version=3)
        elif kind < 0.14:
            m = blob_v1_message(key, props, um, content, 1 if v == 1 else 2)
        else:
            enc = stream_bytes(seed, 9, 32).tobytes() if (v >= 2 and rng.random() < 0.4) else None
            bt = int(rng.choice([0, 1, 2], p=[0.6, 0.35, 0.05]))
            m = MF.put_message(key, props, um, content, version=v, enc_key=enc, life=int(rng.integers(0, 4)) if v == 3
                               else 0, blob_version=int(rng.choice([2, 3])), compressed=bool(rng.random() < 0.3),
                               blob_type=bt)
        m = bytearray(m)
        if rng.random() < 0.07 and corrupt:  # corrupt a byte somewhere
            m[int(rng.integers(0, len(m)))] ^= 0x40
        msgs.append(bytes(m))
    region, offs = bytearray(), []
    for m in msgs:
        region += bytes(int(rng.integers(0, 5)))  # gaps and odd alignment between messages
        offs.append(len(region))
        region += m
    return bytes(region), offs


def dense_old_region(n, seed):
    """A dense, gap-free region of clean messages as old servers stored them -- header V1 (some
    V2), BlobProperties at SerDe V1 (some V2 / V3), Blob_Format_V1 -- so a transform to header V3
    grows nearly every message by the full 26 B (+6 header, +17 props, +3 blob head): an old
    replica being re-replicated (PutMessageFormatInputStream.java:88-90,122)."""
    rng = np.random.default_rng(seed)
    msgs = []
    for i in range(n):
        blen = int(rng.choice([0, 1, 100, 4096]))
        content = stream_bytes(seed + i, 0, blen).tobytes()
        um = stream_bytes(seed + i, 1 << 20, int(rng.choice([0, 5, 300]))).tobytes()
        sv = int(rng.choice([1, 2, 3], p=[0.7, 0.15, 0.15]))
        props = MF.blob_properties_bytes(blen, service_id="s%d" % (i % 7), owner_id="o%d" % (i % 3),
                                         private=bool(i % 2), serde_version=sv)
        hv = 1 if rng.random() < 0.8 else 2
        msgs.append(blob_v1_message(MF.store_key("old-%d" % i), props, um, content, hv))
    return join(msgs)


def dense_v3_region(n, seed, lead=0, trail=0):
    """Clean PUTs as a current server stores them -- header V3, BlobProperties at VERSION_5, a
    Blob_Format_V3 record, some with an encryption key -- back to back after `lead` junk bytes and
    before `trail` more: replication's common case, which the transform's one-pass fast path takes
    (the output is the messages' own bytes with each header's life version rewritten)."""
    rng = np.random.default_rng(seed)
    msgs = []
    for i in range(n):
        blen = int(rng.choice([0, 1, 100, 1000, 4096, 4109]))
        content = stream_bytes(seed + i, 0, blen).tobytes()
        um = stream_bytes(seed + i, 1 << 20, int(rng.choice([0, 7, 300]))).tobytes()
        props = MF.blob_properties_bytes(blen, service_id="s%d" % (i % 7), private=bool(i % 2),
                                         encrypted=bool(i % 3 == 0), filename="f%d" % i if i % 4 else None)
        enc = stream_bytes(seed, 9, 32).tobytes() if i % 5 == 0 else None
        msgs.append(MF.put_message(MF.store_key("v3-%d" % i), props, um, content, version=3, enc_key=enc,
                                   life=int(rng.integers(0, 3)), compressed=bool(i % 6 == 0),
                                   blob_type=int(i % 7 == 0)))
    junk = stream_bytes(seed, 1 << 30, lead + trail).tobytes()
    region = junk[:lead] + b"".join(msgs) + junk[lead:]
    offs = (lead + np.cumsum([0] + [len(x) for x in msgs[:-1]])).tolist()
    return region, offs


# ---------------------------------------------------------------- messages a delete or a re-key refuses
def refused_messages(n, tag):
    """n messages a hard delete refuses, by turns: an update message (NOT_PUT), a PUT whose blob record CRC is
    wrong (refused by the record check), a PUT whose header CRC is wrong (refused before any record is read)."""
    out = []
    for i in range(n):
        key = MF.store_key("%s-%d" % (tag, i))
        if i % 3 == 0:
            out.append(MF.update_message(key, version=3, kind=["ttl", "delete", "undelete"][i // 3 % 3]))
            continue
        size = (i * 37) % 500
        m = bytearray(MF.put_message(key, MF.blob_properties_bytes(size), b"u" * (i % 11),
                                     stream_bytes(3000 + i, 0, size).tobytes(), version=1 + i % 3))
        m[-1 if i % 3 == 1 else 9] ^= 0x04
        out.append(bytes(m))
    return out


# ---------------------------------------------------------------- the write side
def random_messages(n, seed, max_blob=70000):
    from ambry_amd.messages import PutMessage

    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        v = int(rng.choice([1, 2, 3], p=[0.15, 0.15, 0.7]))
        enc = None
        if v >= 2 and rng.random() < 0.4:
            enc = stream_bytes(seed + i, 5, int(rng.choice([0, 1, 16, 32, 300]))).tobytes()
        blen = int(rng.choice([0, 1, 3, 13, 100, 1000, 4096, 4109, int(rng.integers(0, max_blob))]))
        um = stream_bytes(seed + i, 7 << 20, int(rng.choice([0, 1, 5, 1000, int(rng.integers(0, 3000))]))).tobytes()
        key = MF.store_key("blob-%d-%s" % (i, "x" * int(rng.integers(0, 40))))
        props = MF.blob_properties_bytes(blen, service_id="svc%d" % i, ttl=int(rng.integers(-1, 10**6)))
        out.append(PutMessage(key=key, props=props, usermeta=um, blob=stream_bytes(seed ^ i, 0, blen).tobytes(),
                              enckey=enc, header_version=v, life_version=int(rng.integers(0, 5)) if v == 3 else 0,
                              blob_type=int(rng.integers(0, 3)), compressed=bool(rng.random() < 0.3)))
    return out


def put_expected(m):
    """oracle/message_format.py lays out blob type 0; other types differ only in the blob record's
    type field (and so in its CRC): patch and re-CRC that record."""
    b = bytearray(MF.put_message(m.key, m.props, m.usermeta, m.blob, version=m.header_version, enc_key=m.enckey,
                                 life=m.life_version, compressed=m.compressed))
    v, total, rel = MF.parse_header(bytes(b), 0)
    blob_rel = rel[4]
    struct.pack_into(">h", b, blob_rel + 2, m.blob_type)
    end = len(b) - 8
    struct.pack_into(">q", b, end, zlib.crc32(bytes(b[blob_rel:end])))
    return bytes(b)


# ---------------------------------------------------------------- PutRequest fields
def put_request_fields(blob_id: bytes, props: bytes, um: bytes, blob_type: int, key: bytes, compressed: bool,
                       blob_size: int) -> bytes:
    return (blob_id + props + struct.pack(">i", len(um)) + um + struct.pack(">hh", blob_type, len(key)) + key +
            struct.pack(">bq", 1 if compressed else 0, blob_size))


def make_requests(n=20, seed=3):
    rng = np.random.default_rng(seed)
    reqs = []
    for i in range(n):
        size = int(rng.integers(0, 300000))
        blob = stream_bytes(seed * 7919 + i, 0, size).tobytes()
        key = stream_bytes(i, 1, 32 if i % 2 else 0).tobytes()
        fields = put_request_fields(stream_bytes(i, 2, 40).tobytes(), MF.blob_properties_bytes(size),
                                    stream_bytes(i, 3, int(rng.integers(0, 2000))).tobytes(), i % 3, key,
                                    bool(i % 4 == 0), size)
        reqs.append((fields, blob, bool(i % 4 == 0), i % 3))
    return reqs
