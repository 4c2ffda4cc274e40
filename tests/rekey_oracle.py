"""Expected results of a re-key (BlobIdTransformer.transform / newMessage, ambry-replication/.../
BlobIdTransformer.java:72-87,159-281), from oracle/message_format.py and zlib alone: independent of the
library's parser, its V5 re-encoding in place and its GF(2) shifts. Shared by test_rekey_cpu.py and
test_gpu_rekey.py, with the region and descriptor builders both use.

The skeleton is MF.transform_message's (verify, refuse update records, deserialize, re-serialize through
put_message) with the store key, the properties' account / container / blob size and a metadata blob's
content substituted, and the re-key's own refusals."""
import struct

import numpy as np

from datagen import stream_bytes
from msgfmt import MF
from oracle_common import BAD_DESC, INT_MAX, NEEDS_CONTENT, NO_ROOM, NOWHERE, place_packed

KEEP = 0xFFFFFFFFFFFFFFFF

DESC = np.dtype([("key_src", "<u8"), ("content_src", "<u8"), ("content_len", "<u8"), ("props_blob_size", "<i8"),
                 ("key_len", "<u4"), ("account_id", "<i2"), ("container_id", "<i2")])
VERIFY_BITS = (MF.HEADER_CRC | MF.ENCKEY_CRC | MF.PROPS_CRC | MF.UPDATE_CRC | MF.USERMETA_CRC | MF.BLOB_CRC |
               MF.BAD_VERSION | MF.BAD_LAYOUT)


# ---------------------------------------------------------------- the oracle
def desc_ok(d, aux_len: int) -> bool:
    ks, kl = int(d["key_src"]), int(d["key_len"])
    if ks + kl > aux_len:
        return False
    if int(d["content_src"]) == KEEP:
        return True
    cs, cl = int(d["content_src"]), int(d["content_len"])
    return cl <= INT_MAX and cs + cl <= aux_len


def rekey_message(region: bytes, off: int, d, aux: bytes, life=None, version: int = 3):
    """(status, bytes): b"" for a skipped message, None for a refused one."""
    if int(d["key_len"]) == 0:
        return 0, b""  # the converter returned no key: TransformationOutput(null), nothing read
    if not desc_ok(d, len(aux)):
        return BAD_DESC, None
    status, _ = MF.verify_message(region, off)
    if status:
        return status, None
    v, total, rel = MF.parse_header(region, off)
    enc, bp, upd, um, blob = rel
    if upd != MF.INVALID or bp == MF.INVALID or um == MF.INVALID or blob == MF.INVALID:
        return MF.NOT_PUT, None
    h = MF.HEADER_SIZE[v]
    first = enc if enc != MF.INVALID else bp
    enc_key = None
    if enc != MF.INVALID:
        n = MF._be32(region, off + enc + 2)
        if n < 0 or enc + 6 + n + 8 != bp:
            return MF.BAD_RECORD, None
        enc_key = region[off + enc + 6:off + enc + 6 + n]
    if um - 8 < bp + 2:
        return MF.BAD_RECORD, None
    fields, _ = MF.parse_blob_properties(region, off + bp + 2, off + um - 8)
    fields = dict(fields)
    fields["account"], fields["container"] = int(d["account_id"]), int(d["container_id"])  # :249-254
    if int(d["props_blob_size"]) >= 0:
        fields["size"] = int(d["props_blob_size"])  # compositeBlobInfo.getTotalSize(), :242
    try:
        props = MF.serialize_blob_properties_v5(fields)
    except MF.NotEncodable:
        return MF.NOT_ENCODABLE, None
    n = MF._be32(region, off + um + 2)
    if n < 0 or um + 6 + n + 8 != blob:
        return MF.BAD_RECORD, None
    usermeta = region[off + um + 6:off + um + 6 + n]
    bv = MF._be16(region, off + blob)
    btype, comp = 0, False
    if bv == 1:
        size, head = MF._be64(region, off + blob + 2), 10
    elif bv == 2:
        btype, size, head = MF._be16(region, off + blob + 2), MF._be64(region, off + blob + 4), 12
    elif bv == 3:
        btype = MF._be16(region, off + blob + 2)
        comp = region[off + blob + 4] == 1
        size, head = MF._be64(region, off + blob + 5), 13
    else:
        return MF.BAD_RECORD, None
    if not (0 <= btype < 2) or not (0 <= size <= INT_MAX) or blob + head + size + 8 != first + total:
        return MF.BAD_RECORD, None
    repl = int(d["content_src"]) != KEEP
    if repl and btype == 0:
        return BAD_DESC, None  # content is rewritten for a MetadataBlob only (:183)
    if not repl and btype == 1:
        return NEEDS_CONTENT, None  # ... and always for one (:185-247)
    if repl:
        content = aux[int(d["content_src"]):int(d["content_src"]) + int(d["content_len"])]
    else:
        content = region[off + blob + head:off + blob + head + size]
    key = aux[int(d["key_src"]):int(d["key_src"]) + int(d["key_len"])]
    stored_life = MF._be16(region, off + 2) if v == 3 else 0
    out = MF.put_message(key, props, usermeta, content, version=version,
                         enc_key=enc_key if version >= 2 else None, life=stored_life if life is None else life,
                         compressed=comp, blob_type=btype)
    return 0, out


def expected(region: bytes, offs, descs, aux: bytes, life=None, version: int = 3, out_cap=None):
    """(status, out_off, out_len lists, the packed output) of a batch: outputs in message order, a message
    past out_cap refused with NO_ROOM while still advancing the running offset."""
    res = [rekey_message(region, off, descs[i], aux, None if life is None else int(life[i]), version)
           for i, off in enumerate(offs)]
    place = place_packed([len(b) if st == 0 and b else None for st, b in res], out_cap)
    status, out_off, out_len, packed = [], [], [], bytearray()
    for (st, b), at in zip(res, place):
        if at is not None:
            packed += bytes(at - len(packed)) + b
        elif st == 0 and b:
            st = NO_ROOM
        status.append(st)
        out_off.append(NOWHERE if at is None else at)
        out_len.append(0 if at is None else len(b))
    return status, out_off, out_len, bytes(packed)


def counts(descs, status):
    """The mix of a batch, from the oracle's statuses: transformed, refused by the verify, NOT_PUT,
    NEEDS_CONTENT, skipped, BAD_DESC."""
    skipped = sum(1 for d, s in zip(descs, status) if s == 0 and int(d["key_len"]) == 0)
    return {"transformed": sum(1 for s in status if s == 0) - skipped,
            "verify": sum(1 for s in status if s & VERIFY_BITS or s == MF.BAD_RECORD),
            "not_put": sum(1 for s in status if s == MF.NOT_PUT),
            "needs_content": sum(1 for s in status if s == NEEDS_CONTENT),
            "skipped": skipped,
            "bad_desc": sum(1 for s in status if s == BAD_DESC)}


def assert_mix(descs, status):
    c = counts(descs, status)
    assert c["transformed"] >= 180 and c["verify"] >= 20 and c["not_put"] >= 15 and c["needs_content"] >= 5 and \
        c["skipped"] >= 5 and c["bad_desc"] >= 5, c


# ---------------------------------------------------------------- stored messages
def stored_put(key, props, um, content, hv=3, enc_key=None, life=0, bv=3, btype=0, comp=False) -> bytes:
    """A stored PUT with header version hv and blob record version bv (MF.put_message writes V3 records)."""
    h = MF.HEADER_SIZE[hv]
    enc = MF.enckey_record(enc_key) if (enc_key is not None and hv >= 2) else b""
    pr, umr = MF.props_record(props), MF.usermeta_record(um)
    bl = MF.blob_record_v1(content) if bv == 1 else MF.blob_record(content, version=bv, blob_type=btype,
                                                                   compressed=comp)
    bp_off = h + len(key) + len(enc)
    um_off = bp_off + len(pr)
    return MF.header(hv, len(enc) + len(pr) + len(umr) + len(bl), h + len(key) if enc else MF.INVALID, bp_off,
                     MF.INVALID, um_off, um_off + len(umr), life) + key + enc + pr + umr + bl


def build_region(n=300, seed=1, corrupt_frac=0.1, big_every=17, max_blob=5000, max_usermeta=1200):
    """(region, offsets, is_metadata flags): headers V1/V2/V3 with and without an encryption key, properties at
    SerDe V1..V5 (a few with a non-canonical `private` byte, about 1 % with a non-ASCII string), blob records
    V1/V2/V3, about one MetadataBlob in eight, one update message in ten, corrupt_frac of the messages with one
    flipped bit, a blob of 60-300 KB every big_every-th message and under max_blob bytes otherwise, user
    metadata under max_usermeta bytes."""
    rng = np.random.default_rng(seed * 7919 + 11)
    out, offs, meta = bytearray(), [], []
    for i in range(n):
        key = MF.store_key(f"blob-{i:06d}-{seed}")
        is_meta = False
        if rng.integers(0, 10) == 0:
            msg = MF.update_message(key, version=3, kind=["ttl", "delete", "undelete"][i % 3])
        else:
            hv = [1, 2, 3, 3][int(rng.integers(0, 4))]
            is_meta = rng.integers(0, 8) == 0
            bv = int(rng.integers(2, 4)) if is_meta else int(rng.integers(1, 4))
            if is_meta:
                size = 2 + 8 + 4 + 24 * int(rng.integers(1, 40))  # a list of chunk ids
            elif (i + 1) % big_every == 0:
                size = int(rng.integers(60000, 300000))
            else:
                size = int(rng.integers(0, max_blob))
            content = stream_bytes(seed * 100003 + i, 0, size).tobytes()
            um = stream_bytes(seed + i, 7, int(rng.integers(0, max_usermeta))).tobytes()
            enc = stream_bytes(i, 3, int(rng.integers(1, 120))).tobytes() if (hv >= 2 and rng.integers(0, 2)) else None
            sv = int(rng.integers(1, 6))
            ctype = "application/octet" if rng.integers(0, 100) else b"caf\xc3\xa9"
            props = MF.blob_properties_bytes(size, serde_version=sv, content_type=ctype,
                                             private=[False, True, 2][int(rng.integers(0, 3))],
                                             encrypted=bool(rng.integers(0, 2)), account=int(rng.integers(0, 3000)),
                                             container=int(rng.integers(0, 300)), owner_id="o" * int(rng.integers(0, 40)),
                                             filename="f.bin" if rng.integers(0, 2) else None)
            msg = stored_put(key, props, um, content, hv=hv, enc_key=enc, life=int(i % 3), bv=bv,
                             btype=1 if is_meta else 0, comp=bool(bv == 3 and i % 5 == 0))
        offs.append(len(out))
        meta.append(bool(is_meta))
        out += msg
    region = bytearray(out)
    for i in rng.choice(n, size=int(n * corrupt_frac), replace=False):
        start = offs[i]
        end = offs[i + 1] if i + 1 < n else len(region)
        region[int(rng.integers(start, end))] ^= 1 << int(rng.integers(0, 8))
    return bytes(region), offs, meta


def build_descs(offs, meta, seed=1, skip_frac=0.05, bad_frac=0.04, same_key_len=None):
    """(descriptor array, aux bytes) for the messages of build_region: new keys of 1..80 B (same_key_len: that
    length for all), about skip_frac of the descriptors with key_len 0, a metadata blob's replacement content
    for about two in three of them, about bad_frac unusable descriptors of every kind. The first span starts
    at aux offset 0 and the last ends at its end; no aux byte is used by two descriptors."""
    rng = np.random.default_rng(seed * 104729 + 3)
    n = len(offs)
    descs = np.zeros(n, dtype=DESC)
    aux = bytearray()
    bad = {}
    for i in range(n):
        d = descs[i]
        d["content_src"], d["props_blob_size"] = KEEP, -1
        d["account_id"], d["container_id"] = int(rng.integers(-2, 32767)), int(rng.integers(-2, 32767))
        if rng.random() < skip_frac:
            continue  # key_len 0
        klen = same_key_len or int(rng.integers(1, 81))
        d["key_src"], d["key_len"] = len(aux), klen
        aux += stream_bytes(seed * 31 + i, 5, klen).tobytes()
        if meta[i] and rng.integers(0, 3):
            clen = 2 + 8 + 4 + 24 * int(rng.integers(0, 50))
            d["content_src"], d["content_len"] = len(aux), clen
            aux += stream_bytes(seed * 77 + i, 9, clen).tobytes()
            d["props_blob_size"] = int(rng.integers(0, 1 << 40))
        elif rng.integers(0, 6) == 0:
            d["props_blob_size"] = int(rng.integers(0, 1 << 33))
        if rng.random() < bad_frac:
            bad[i] = int(rng.integers(0, 4))
    for i, kind in bad.items():  # once aux has its final length
        d = descs[i]
        if kind == 0:
            d["key_src"] = len(aux) - int(d["key_len"]) + 1  # one byte past the end
        elif kind == 1:
            d["content_src"], d["content_len"] = len(aux) - 3, 4
        elif kind == 2:
            d["content_src"], d["content_len"] = 0, INT_MAX + 1
        elif not meta[i]:
            d["content_src"], d["content_len"] = 0, 16  # replacement content for a DataBlob
    return descs, bytes(aux)


def metadata_region(content_lens, seed=5):
    """Clean MetadataBlob messages (headers V1..V3, blob records V2 / V3) and descriptors whose replacement
    contents have the given lengths."""
    msgs, descs, aux = [], np.zeros(len(content_lens), dtype=DESC), bytearray()
    for i, clen in enumerate(content_lens):
        stored = stream_bytes(seed * 13 + i, 1, 38 + 24 * i).tobytes()
        msgs.append(stored_put(MF.store_key(f"meta-{i}"), MF.blob_properties_bytes(len(stored), serde_version=1 + i % 5),
                               b"um" * i, stored, hv=1 + i % 3, enc_key=b"e" * 32 if i % 2 else None, bv=2 + i % 2,
                               btype=1))
        d = descs[i]
        d["key_src"], d["key_len"] = len(aux), 7 + 5 * i
        aux += stream_bytes(seed * 17 + i, 2, 7 + 5 * i).tobytes()
        d["content_src"], d["content_len"] = len(aux), clen
        aux += stream_bytes(seed * 19 + i, 3, clen).tobytes()
        d["props_blob_size"], d["account_id"], d["container_id"] = 1000 * clen + i, 100 + i, -1 - i
    offs = [int(x) for x in np.cumsum([0] + [len(x) for x in msgs[:-1]])]
    return b"".join(msgs), offs, descs, bytes(aux)


def run_cpu(messages, region: bytes, offs, descs, aux: bytes, life=None, version: int = 3):
    """(status list, list of outputs) through the CPU entry, message by message."""
    buf, ax = np.frombuffer(region, dtype=np.uint8), np.frombuffer(aux, dtype=np.uint8)
    status, outs = [], []
    for i, off in enumerate(offs):
        st, b = messages.rekey_message_cpu(buf, off, descs[i], ax, header_version=version,
                                           life=None if life is None else int(life[i]))
        status.append(st)
        outs.append(b)
    return status, outs


def identity_descs(region: bytes, offs):
    """Descriptors that change nothing: the stored key, the stored account / container, no content, for every
    message whose header and properties parse (others: a one-byte key)."""
    descs, aux = np.zeros(len(offs), dtype=DESC), bytearray(b"k")
    for i, off in enumerate(offs):
        d = descs[i]
        d["content_src"], d["props_blob_size"], d["key_src"], d["key_len"] = KEEP, -1, 0, 1
        if MF.verify_message(region, off)[0]:
            continue
        v, _, rel = MF.parse_header(region, off)
        if rel[1] == MF.INVALID:
            continue
        first = rel[0] if rel[0] != MF.INVALID else rel[1]
        key = region[off + MF.HEADER_SIZE[v]:off + first]
        f, _ = MF.parse_blob_properties(region, off + rel[1] + 2, off + rel[3] - 8)
        d["key_src"], d["key_len"] = len(aux), len(key)
        aux += key
        d["account_id"], d["container_id"] = f["account"], f["container"]
    return descs, bytes(aux)


def blob_type_of(region: bytes, off: int) -> int:
    """Blob type of a verified PUT's blob record."""
    _, _, rel = MF.parse_header(region, off)
    return 0 if MF._be16(region, off + rel[4]) == 1 else struct.unpack_from(">h", region, off + rel[4] + 2)[0]
