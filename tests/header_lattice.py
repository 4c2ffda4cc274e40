"""The stored-message header rule, every branch placed on purpose (test_header_lattice.py on the CPU,
test_gpu_header_lattice.py on the device): version -> header size, the fields of each layout, the stored header
CRC, checkHeaderConstraints (MessageFormatRecord.java:985-1030), "a record ends where the next present one
starts", and the record reads that follow an intact header. Built from oracle/message_format.py alone.

packed()    (names, region, offsets): about 250 messages of about 150 B end to end, one mutation each, every
            mutated header re-sealed with a valid CRC unless the case is about the CRC.
truncated() [(name, region, offset)]: regions that end inside or right at a message, and offsets at and past the
            region's end."""
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


def _edit_record(m: Msg, k: int, edit) -> bytes:
    """m's bytes with record k edited (edit(bytearray of the record)) and the record's CRC recomputed."""
    lo, hi = m.span(k)
    raw = bytearray(m.bytes())
    rec = raw[lo:hi]
    edit(rec)
    rec[-8:] = struct.pack(">q", zlib.crc32(bytes(rec[:-8])))
    raw[lo:hi] = rec
    return bytes(raw)


def _pack(fmt, at, value):
    def edit(rec):
        struct.pack_into(fmt, rec, at, value)
    return edit


def mutations(name: str, m: Msg):
    """[(case name, message bytes)] of one base: the clean message, then one mutation each."""
    out = [("clean", m.bytes())]
    raw, hs = m.bytes(), m.hs
    for v in (0, 4, -1):  # the version field, the rest of the header re-sealed as the base's layout
        out.append(("version=%d" % v, _reseal_header(struct.pack(">h", v) + raw[2:], hs)))
    out.append(("crc-low-bit", raw[:hs - 1] + bytes([raw[hs - 1] ^ 1]) + raw[hs:]))
    out.append(("crc-upper-word", raw[:hs - 8] + b"\x00\x00\x00\x01" + raw[hs - 4:]))
    if m.hv == 3:
        out.append(("life=-1", m.with_(life=-1).bytes()))
    out.append(("total=0", m.with_(total=0).bytes()))
    out.append(("total=-1", m.with_(total=-1).bytes()))
    out.append(("total+1", m.with_(total=m.total + 1).bytes()))  # packed: one byte of the next message
    p = m.present()
    for i, k in enumerate(p):
        s = SLOT[k]
        out.append(("%s=-1" % s, m.with_rel(k, INV).bytes()))
        out.append(("%s=hs-1" % s, m.with_rel(k, hs - 1).bytes()))
        if i:
            out.append(("%s=previous" % s, m.with_rel(k, m.rel[p[i - 1]]).bytes()))
        if i + 1 < len(p):
            rel = list(m.rel)
            rel[k], rel[p[i + 1]] = rel[p[i + 1]], rel[k]
            out.append(("%s<->%s" % (s, SLOT[p[i + 1]]), m.with_(rel=rel).bytes()))
        if len(p) == 1:  # the only record: the message end follows it, so the total makes it short
            out.append(("%s=next-7" % s, m.with_(total=7).bytes()))
        else:
            out.append(("%s=next-7" % s, m.with_rel(k, m.span(k)[1] - 7).bytes()))
    if m.rel[2] == INV:  # a PUT: the update slot set too; the records' own reads behind an intact header
        out.append(("update-slot-set", m.with_rel(2, m.rel[1] + 1).bytes()))
        for k in (0, 3):
            if m.rel[k] == INV:
                continue
            n = struct.unpack_from(">i", raw, m.rel[k] + 2)[0]
            for d in (-1, 1):
                out.append(("%s-size%+d" % (SLOT[k], d), _edit_record(m, k, _pack(">i", 2, n + d))))
        for k in p[:-1]:
            out.append(("%s-version=2" % SLOT[k], _edit_record(m, k, _pack(">h", 0, 2))))
        bv = struct.unpack_from(">h", raw, m.rel[4])[0]
        at = {1: 2, 2: 4, 3: 5}[bv]
        size = struct.unpack_from(">q", raw, m.rel[4] + at)[0]
        for v in (0, 4):
            out.append(("blob-version=%d" % v, _edit_record(m, 4, _pack(">h", 0, v))))
        if bv > 1:
            out.append(("blob-type=2", _edit_record(m, 4, _pack(">h", 2, 2))))
        out.append(("blob-size=2^31", _edit_record(m, 4, _pack(">q", at, 1 << 31))))
        for d in (-1, 1):
            out.append(("blob-size%+d" % d, _edit_record(m, 4, _pack(">q", at, size + d))))
    else:  # an update: one more slot set
        for k in (0, 1, 3, 4):
            if m.hv == 1 and k == 0:
                continue  # V1 has no such slot
            out.append(("%s-slot-set" % SLOT[k], m.with_rel(k, m.rel[2] + (k - 2) * 9).bytes()))
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
