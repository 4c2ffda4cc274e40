"""The stored-message header rule, every branch placed on purpose (test_header_lattice.py on the CPU,
test_gpu_header_lattice.py on the device): version -> header size, the fields of each layout, the stored header
CRC, checkHeaderConstraints (MessageFormatRecord.java:985-1030), "a record ends where the next present one
starts", and the record reads that follow an intact header. Built from oracle/message_format.py alone.

packed()    (names, region, offsets): about 250 messages of about 150 B end to end, one mutation each, every
            mutated header re-sealed with a valid CRC unless the case is about the CRC.
truncated() [(name, region, offset)]: regions that end inside or right at a message, and offsets at and past the
            region's end.

Two faults in one message (test_pair_lattice.py, test_gpu_pair_lattice.py): every mutation is an operation
(operations(): a name, a site, a stage), and build() applies any set of them in a fixed order.
pairs()            (names, region, offsets): per base every unordered pair of operations of two different sites,
                   about 6,300 messages end to end.
truncated_pairs()  [(name, region, offset)]: each cut of truncated() with each header or record-CRC operation
                   that changes a byte before the cut."""
import functools
import struct
import zlib

import numpy as np

import rekey_oracle as RK
import send_oracle as SO
from msgfmt import MF

INV = MF.INVALID
SLOT = ("enckey", "props", "update", "usermeta", "blob")


class Msg:
    """A message held as its header fields and its bytes after the header."""

    def __init__(self, hv, total, rel, body, life=0):
        self.hv, self.total, self.rel, self.body, self.life = hv, total, list(rel), body, life

    @property
    def hs(self):
        return MF.HEADER_SIZE[self.hv]

    @property
    def end(self):
        return self.hs + len(self.body)

    def present(self):
        return [k for k in range(5) if self.rel[k] != INV]

    def span(self, k):
        """[start, end) of present record k as the clean base lays it out."""
        p = self.present()
        i = p.index(k)
        return self.rel[k], self.rel[p[i + 1]] if i + 1 < len(p) else self.end

    def with_(self, **kw):
        m = Msg(self.hv, self.total, self.rel, self.body, self.life)
        for k, v in kw.items():
            setattr(m, k, list(v) if k == "rel" else v)
        return m

    def with_rel(self, k, v):
        rel = list(self.rel)
        rel[k] = v
        return self.with_(rel=rel)

    def header(self):
        return MF.header(self.hv, self.total, *self.rel, life=self.life)

    def bytes(self):
        return self.header() + self.body


def bases():
    """{name: Msg}: headers V1 / V2 / V3 as a PUT (blob record V1 / V2 / V3 in turn), a PUT with an encryption
    key (V2 / V3) and an update."""
    out = {}
    for hv in (1, 2, 3):
        h = MF.HEADER_SIZE[hv]
        for enc in ((None, b"k" * 9) if hv >= 2 else (None,)):
            key = MF.store_key("put-%d%s" % (hv, "e" if enc else ""))
            content = bytes(range(17 + hv))
            recs = [MF.enckey_record(enc) if enc else b"", MF.props_record(MF.blob_properties_bytes(len(content),
                    serde_version=2 + hv)), MF.usermeta_record(b"um" * hv),
                    MF.blob_record_v1(content) if hv == 1 else MF.blob_record(content, version=hv, compressed=hv == 3)]
            at = h + len(key)
            rel = [at if enc else INV, at + len(recs[0]), INV, at + len(recs[0]) + len(recs[1]),
                   at + len(recs[0]) + len(recs[1]) + len(recs[2])]
            out["v%d-put%s" % (hv, "-enc" if enc else "")] = Msg(hv, sum(len(r) for r in recs), rel,
                                                                 key + b"".join(recs), life=hv - 1)
        key = MF.store_key("upd-%d" % hv)
        rec = MF.update_record_v3(kind=("delete", "ttl", "undelete")[hv - 1])
        out["v%d-update" % hv] = Msg(hv, len(rec), [INV, INV, h + len(key), INV, INV], key + rec, life=1)
    return out


def _reseal_header(raw: bytes, hs: int) -> bytes:
    return raw[:hs - 8] + struct.pack(">q", zlib.crc32(raw[:hs - 8])) + raw[hs:]


def _pack(fmt, at, value):
    def edit(rec):
        struct.pack_into(fmt, rec, at, value)
    return edit


class Op:
    """One fault: a name, the site it edits, the stage it is applied at and the edit itself. `single`: part of the
    single-fault lattice (mutations(), packed()). Stages, applied in this order by build():
      1  a record-field edit: fn(bytearray of record k as the clean base spans it), the record's CRC recomputed
      2  a header-field edit: fn(Msg) -> Msg (life, total, the slots); the header is sealed afterwards
      3  the version field: fn is the value; the rest of the header re-sealed as the base's layout
      4  a raw flip: fn(bytearray of the message), nothing re-sealed
    Sites: h.version, h.crc, h.life, h.total, h.rel0 .. h.rel4, r<k>.field and r<k>.crc of each record."""

    def __init__(self, name, site, stage, fn, single=True, k=None):
        self.name, self.site, self.stage, self.fn, self.single, self.k, self.order = name, site, stage, fn, single, k, 0


# the byte of each record whose flip faults the record's CRC and nothing else: key material, the creation time's
# low byte, the update time's low byte, user metadata; the blob's is its last content byte
_CONTENT_AT = {0: 6, 1: 20, 2: 13, 3: 6}
OWNER_AT = 2 + 27 + 4 + len("application/octet") + 4  # the owner's first byte in a properties record of bases()


def _xor(at, bit):
    def flip(raw):
        raw[at] ^= bit
    return flip


def _put(at, data):
    def put(raw):
        raw[at:at + len(data)] = data
    return put


def operations(m: Msg):
    """[Op] of one base in the fixed order build() applies them in within a stage: what mutations() has always
    held (single), total-1, three CRC faults per present record (a content bit, a bit of the trailer's low word,
    a bit of its high word), and for the properties and the update record the faults of their own parsers."""
    out = []
    raw, hs = m.bytes(), m.hs
    for v in (0, 4, -1):
        out.append(Op("version=%d" % v, "h.version", 3, v))
    out.append(Op("crc-low-bit", "h.crc", 4, _xor(hs - 1, 1)))
    out.append(Op("crc-upper-word", "h.crc", 4, _put(hs - 8, b"\x00\x00\x00\x01")))
    if m.hv == 3:
        out.append(Op("life=-1", "h.life", 2, lambda x: x.with_(life=-1)))
    out.append(Op("total=0", "h.total", 2, lambda x: x.with_(total=0)))
    out.append(Op("total=-1", "h.total", 2, lambda x: x.with_(total=-1)))
    out.append(Op("total+1", "h.total", 2, lambda x: x.with_(total=m.total + 1)))  # packed: one byte of the next
    out.append(Op("total-1", "h.total", 2, lambda x: x.with_(total=m.total - 1), single=False))
    p = m.present()
    for i, k in enumerate(p):
        s, site = SLOT[k], "h.rel%d" % k
        out.append(Op("%s=-1" % s, site, 2, lambda x, k=k: x.with_rel(k, INV)))
        out.append(Op("%s=hs-1" % s, site, 2, lambda x, k=k: x.with_rel(k, hs - 1)))
        if i:
            out.append(Op("%s=previous" % s, site, 2, lambda x, k=k, v=m.rel[p[i - 1]]: x.with_rel(k, v)))
        if i + 1 < len(p):
            nk = p[i + 1]
            out.append(Op("%s<->%s" % (s, SLOT[nk]), site, 2,
                          lambda x, k=k, nk=nk: x.with_rel(k, m.rel[nk]).with_rel(nk, m.rel[k])))
        if len(p) == 1:  # the only record: the message end follows it, so the total makes it short
            out.append(Op("%s=next-7" % s, "h.total", 2, lambda x: x.with_(total=7)))
        else:
            out.append(Op("%s=next-7" % s, site, 2, lambda x, k=k, v=m.span(k)[1] - 7: x.with_rel(k, v)))
    if m.rel[2] == INV:  # a PUT: the update slot set too; the records' own reads behind an intact header
        out.append(Op("update-slot-set", "h.rel2", 2, lambda x: x.with_rel(2, m.rel[1] + 1)))
        for k in (0, 3):
            if m.rel[k] == INV:
                continue
            n = struct.unpack_from(">i", raw, m.rel[k] + 2)[0]
            for d in (-1, 1):
                out.append(Op("%s-size%+d" % (SLOT[k], d), "r%d.field" % k, 1, _pack(">i", 2, n + d), k=k))
        for k in p[:-1]:
            out.append(Op("%s-version=2" % SLOT[k], "r%d.field" % k, 1, _pack(">h", 0, 2), k=k))
        bv = struct.unpack_from(">h", raw, m.rel[4])[0]
        at = {1: 2, 2: 4, 3: 5}[bv]
        size = struct.unpack_from(">q", raw, m.rel[4] + at)[0]
        for v in (0, 4):
            out.append(Op("blob-version=%d" % v, "r4.field", 1, _pack(">h", 0, v), k=4))
        if bv > 1:
            out.append(Op("blob-type=2", "r4.field", 1, _pack(">h", 2, 2), k=4))
        out.append(Op("blob-size=2^31", "r4.field", 1, _pack(">q", at, 1 << 31), k=4))
        for d in (-1, 1):
            out.append(Op("blob-size%+d" % d, "r4.field", 1, _pack(">q", at, size + d), k=4))
        assert raw[m.rel[1] + OWNER_AT - 4:m.rel[1] + OWNER_AT + 5] == b"\x00\x00\x00\x05owner"
        out.append(Op("props-serde=9", "r1.field", 1, _pack(">h", 2, 9), single=False, k=1))
        out.append(Op("props-string=-1", "r1.field", 1, _pack(">i", 2 + 27, -1), single=False, k=1))
        out.append(Op("props-owner-non-ascii", "r1.field", 1, _pack(">B", OWNER_AT, 0xE9), single=False, k=1))
    else:  # an update: one more slot set
        for k in (0, 1, 3, 4):
            if m.hv == 1 and k == 0:
                continue  # V1 has no such slot
            out.append(Op("%s-slot-set" % SLOT[k], "h.rel%d" % k, 2,
                          lambda x, k=k: x.with_rel(k, m.rel[2] + (k - 2) * 9)))
        out.append(Op("update-version=4", "r2.field", 1, _pack(">h", 0, 4), single=False, k=2))
        out.append(Op("update-type=3", "r2.field", 1, _pack(">h", 14, 3), single=False, k=2))
        out.append(Op("update-subrecord-version=2", "r2.field", 1, _pack(">h", 16, 2), single=False, k=2))
    for k in p:
        lo, hi = m.span(k)
        content = hi - 9 if k == 4 else lo + _CONTENT_AT[k]
        for what, at, bit in (("content", content, 0x04), ("crc-low", hi - 1, 0x01), ("crc-high", hi - 6, 0x10)):
            out.append(Op("%s-%s-flip" % (SLOT[k], what), "r%d.crc" % k, 4, _xor(at, bit), single=False, k=k))
    for i, op in enumerate(out):
        op.order = i
    return out


def build(m: Msg, ops) -> bytes:
    """m's bytes with every op of `ops` applied, stage by stage and in operations()'s order within a stage.
    Record edits land at the clean base's spans whatever the header ops do to the slots; no op changes the
    message's length."""
    ops = sorted(ops, key=lambda op: (op.stage, op.order))
    raw = bytearray(m.bytes())
    for op in (o for o in ops if o.stage == 1):
        lo, hi = m.span(op.k)
        rec = raw[lo:hi]
        op.fn(rec)
        rec[-8:] = struct.pack(">q", zlib.crc32(bytes(rec[:-8])))
        raw[lo:hi] = rec
    x = m.with_(body=bytes(raw[m.hs:]))
    for op in (o for o in ops if o.stage == 2):
        x = op.fn(x)
    raw = x.bytes()
    for op in (o for o in ops if o.stage == 3):
        raw = _reseal_header(struct.pack(">h", op.fn) + raw[2:], m.hs)
    raw = bytearray(raw)
    for op in (o for o in ops if o.stage == 4):
        op.fn(raw)
    assert len(raw) == m.end
    return bytes(raw)


def mutations(name: str, m: Msg):
    """[(case name, message bytes)] of one base: the clean message, then one single-fault operation each."""
    out = [("clean", m.bytes())] + [(op.name, build(m, [op])) for op in operations(m) if op.single]
    return [("%s/%s" % (name, n), b) for n, b in out]


@functools.lru_cache(maxsize=None)
def packed():
    """(names, region, offsets): every mutation of every base end to end, a clean PUT last."""
    names, offs, region = [], [], bytearray()
    for name, m in bases().items():
        for n, b in mutations(name, m):
            names.append(n)
            offs.append(len(region))
            region += b
    names.append("tail/clean")
    offs.append(len(region))
    region += bases()["v3-put-enc"].bytes()
    return names, bytes(region), offs


@functools.lru_cache(maxsize=None)
def truncated():
    """[(name, region, offset)]: behind one clean message, a message whose region ends 0 (the offset equals the
    region's length), 1, hs - 1, hs or first + total - 1 bytes after its start; the offset one past the region's
    end; and a total one byte more than the region holds."""
    lead = bases()["v3-put"].bytes()
    out = []
    for name in ("v1-put", "v2-put-enc", "v3-update"):
        m = bases()[name]
        raw = m.bytes()
        for cut in (0, 1, m.hs - 1, m.hs, len(raw) - 1):
            out.append(("%s/cut=%d" % (name, cut), lead + raw[:cut], len(lead)))
        out.append(("%s/offset-past-end" % name, lead + raw, len(lead) + len(raw) + 1))
        out.append(("%s/total+1-at-end" % name, lead + m.with_(total=m.total + 1).bytes(), len(lead)))
    return out


@functools.lru_cache(maxsize=None)
def pair_cases():
    """[(base, op a, op b, message bytes)]: for each base every unordered pair of operations from two different
    sites. r<k>.field and r<k>.crc are two sites, so a record's field fault also meets its own CRC faults: the
    record re-sealed over the edited field (stage 1), then flipped (stage 4)."""
    out = []
    for name, m in bases().items():
        ops = operations(m)
        for i, a in enumerate(ops):
            for b in ops[i + 1:]:
                if a.site != b.site:
                    out.append((name, a, b, build(m, [a, b])))
    return out


@functools.lru_cache(maxsize=None)
def pairs():
    """(names, region, offsets), shaped like packed(): every case of pair_cases() end to end, a clean PUT last."""
    names, offs, region = [], [], bytearray()
    for base, a, b, raw in pair_cases():
        names.append("%s/%s+%s" % (base, a.name, b.name))
        offs.append(len(region))
        region += raw
    names.append("tail/clean")
    offs.append(len(region))
    region += bases()["v3-put-enc"].bytes()
    return names, bytes(region), offs


@functools.lru_cache(maxsize=None)
def truncated_pairs():
    """[(name, region, offset)]: each (base, cut) of truncated() behind the same clean lead, the cut message
    built with one header-site operation or one record-CRC operation that changes a byte before the cut."""
    lead = bases()["v3-put"].bytes()
    out = []
    for name in ("v1-put", "v2-put-enc", "v3-update"):
        m = bases()[name]
        raw = m.bytes()
        for cut in (0, 1, m.hs - 1, m.hs, len(raw) - 1):
            for op in operations(m):
                if not (op.site.startswith("h.") or op.site.endswith(".crc")):
                    continue
                b = build(m, [op])
                if b[:cut] != raw[:cut]:
                    out.append(("%s/cut=%d+%s" % (name, cut, op.name), lead + b[:cut], len(lead)))
    return out


def cases():
    """[(name, region, offset)]: every case, the packed ones in the packed region."""
    names, region, offs = packed()
    return [(n, region, o) for n, o in zip(names, offs)] + truncated()


# ---------------------------------------------------------------- inputs of the entries run over the lattice
def sizes_of(region, offs):
    """readSet.sizeInBytes for each message: the header's length where it parses, else up to the next offset."""
    ends = list(offs[1:]) + [len(region)]
    return [SO.header_length(region, o) or max(e - o, 0) for o, e in zip(offs, ends)]


def rekey_desc():
    d = np.zeros(1, dtype=RK.DESC)[0]
    d["key_src"], d["key_len"], d["content_src"], d["props_blob_size"] = 1, 11, RK.KEEP, -1
    d["account_id"], d["container_id"] = 77, -3
    return d, b"." + b"new-key-xyz" + b"."


def pair_descs(n: int):
    """(descriptors, aux) for n messages, by i % 3: keep the content; replace it from aux (BAD_DESC for a data
    blob, after the message verified); a key span past aux's end (BAD_DESC before the message is read). So a bad
    descriptor meets a bad message in both orders."""
    d, aux = rekey_desc()
    descs = np.repeat(np.asarray([d], dtype=RK.DESC), n)
    descs["content_src"][1::3], descs["content_len"][1::3] = 2, 9
    descs["key_src"][2::3] = len(aux) - 10
    return descs, aux


@functools.lru_cache(maxsize=None)
def recover_starts():
    """Indices into pairs() at which the device chain and recover are started, under 700 of about 6,400 (a start
    is a call): each base's first case; of the cases with an operation at a header site (a chain ends at a header
    fault, so most of these stop at their first message) the first one of every such operation of every base and
    every 13th; every 16th of the other cases (the header intact: the chain goes on into the next two cases)."""
    cases = pair_cases()
    header = [i for i, (_, a, b, _) in enumerate(cases) if a.site[0] == "h" or b.site[0] == "h"]
    other = [i for i, (_, a, b, _) in enumerate(cases) if a.site[0] != "h" and b.site[0] != "h"]
    first = {}
    for i, (base, a, b, _) in enumerate(cases):
        first.setdefault(base, i)
        for op in (a, b):
            if op.site[0] == "h":
                first.setdefault((base, op.name), i)
    return sorted(set(first.values()) | set(header[::13]) | set(other[::16]))
