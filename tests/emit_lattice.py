"""The writer of a stored PUT message, every branch placed on purpose (test_emit_lattice.py on the CPU,
test_gpu_emit_lattice.py on the device): the output header at each version, the encryption-key record kept,
dropped and empty, the BlobProperties payload re-encoded at VERSION_5 from every stored SerDe version with its
length and the stored length at every residue of the 8-byte words the device writes it in, the blob record's
head moved from Blob_Format_V1 / V2 / V3 (a non-canonical isCompressed byte included) to V3, empty and one-byte
bodies, and the re-key's overlays. Built from oracle/message_format.py alone.

A case is its attributes, and its name spells them ("hv=3/enc=set/sv=2/w=5/..."), so a test can say which
branches the lattice holds from the names alone:

  hv    stored header version 1..3            enc   encryption key: none, set, empty (a record of 0 bytes)
  sv    stored SerDe version 1..5             w     owner-id length 0..7: steps the payload length through a word
  priv  stored `private` byte                 encb  stored `encrypted` byte (sv >= 3)
  bv    stored blob record version 1..3       comp  stored isCompressed byte (bv 3)
  n     content bytes                         um    user-metadata bytes
  meta  1: a MetadataBlob (bv >= 2)           repl  the re-key's content: keep, or a replacement of 0 / 1 bytes
  bs    the re-key's props_blob_size: given or none        ids   the re-key's account / container ids: pos or neg

cases()        [Case] in region order.
region()       (region bytes, offsets): the stored messages end to end.
fast_region()  the same for the cases the transform's fast path takes (a dense run of them).
rekey_inputs(), wire(), put_messages(v): the same fields as re-key descriptors, PutRequest frames and
PutMessage descriptors for output header version v."""
import functools
import struct
import zlib

import ingest_oracle as IO
import rekey_oracle as RK
from msgfmt import MF

KEYS = ("hv", "enc", "sv", "w", "priv", "encb", "bv", "comp", "n", "um", "meta", "repl", "bs", "ids")
DEFAULTS = dict(hv=3, enc="none", sv=5, w=3, priv=0, encb=0, bv=3, comp=0, n=17, um=5, meta=0, repl="keep", bs="none",
                ids="pos")
APPENDIX = {1: 17, 2: 13, 3: 12, 4: 4, 5: 0}  # bytes VERSION_5 adds to a stored SerDe version's payload
BIG_BLOB = 7001  # the serialize batch's one message above the streamed form's 6,144 B


class Case:
    def __init__(self, index, **attrs):
        a = dict(DEFAULTS, **attrs)
        if a["hv"] == 1:
            a["enc"] = "none"  # a V1 header has no slot for the record
        if a["sv"] < 3:
            a["encb"] = 0
        if a["bv"] != 3:
            a["comp"] = 0
        if a["meta"]:
            a["bv"] = max(a["bv"], 2)  # Blob_Format_V1 has no type
            a["repl"] = a["repl"] if a["repl"] != "keep" else 1
        else:
            a["repl"] = "keep"
        self.index, self.attrs = index, a
        self.name = "/".join("%s=%s" % (k, a[k]) for k in KEYS)
        i = index
        self.key = MF.store_key("emit-%03d" % i)
        self.enckey = {"none": None, "empty": b"", "set": bytes(0x40 + (i + t) % 50 for t in range(1 + i % 9))}[a["enc"]]
        self.props = MF.blob_properties_bytes(
            a["n"], service_id="sv%d" % (i % 10), owner_id="o" * a["w"], content_type="t/%d" % (i % 7), ttl=3600 + i,
            private=a["priv"], creation_ms=1_700_000_000_000 + i, account=100 + i, container=7 + i % 9,
            encrypted=a["encb"], content_encoding="gz" if i % 2 else None, filename="f%d" % i if i % 3 else None,
            reserved="r" if i % 5 == 0 else None, serde_version=a["sv"])
        self.usermeta = bytes(0x61 + (i + t) % 26 for t in range(a["um"]))
        self.content = bytes(1 + (7 * i + t) % 255 for t in range(a["n"]))
        self.life = i % 4 if a["hv"] == 3 else 0

    def __getattr__(self, k):
        try:
            return self.__dict__["attrs"][k]
        except KeyError:
            raise AttributeError(k)

    @property
    def out_props_len(self):
        return len(self.props) + APPENDIX[self.sv]

    def stored(self) -> bytes:
        """The stored message: header hv, blob record bv with the raw isCompressed byte."""
        a = self.attrs
        h = MF.HEADER_SIZE[a["hv"]]
        enc = MF.enckey_record(self.enckey) if self.enckey is not None else b""
        pr, um = MF.props_record(self.props), MF.usermeta_record(self.usermeta)
        if a["bv"] == 1:
            body = struct.pack(">hq", 1, len(self.content))
        elif a["bv"] == 2:
            body = struct.pack(">hhq", 2, a["meta"], len(self.content))
        else:
            body = struct.pack(">hhBq", 3, a["meta"], a["comp"], len(self.content))
        body += self.content
        bl = body + struct.pack(">q", zlib.crc32(body))
        bp = h + len(self.key) + len(enc)
        return MF.header(a["hv"], len(enc) + len(pr) + len(um) + len(bl), h + len(self.key) if enc else MF.INVALID, bp,
                         MF.INVALID, bp + len(pr), bp + len(pr) + len(um), self.life) + self.key + enc + pr + um + bl

    def fast(self) -> bool:
        """The transform's fast path (header V3 out) takes it: its own bytes are the output's."""
        a = self.attrs
        return a["hv"] == 3 and a["bv"] == 3 and a["sv"] == 5 and a["priv"] in (0, 1) and a["encb"] in (0, 1) and \
            a["comp"] in (0, 1)


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(**kw):
        i = len(out)
        rot = dict(hv=1 + i % 3, enc=("none", "set", "empty")[(i // 3) % 3], bv=1 + (i // 2) % 3, bs=("none", "given")[i % 2],
                   ids=("pos", "neg")[(i // 4) % 2])
        out.append(Case(i, **dict(rot, **kw)))

    # the stored header, the encryption key and the blob record's version against each other
    for hv in (1, 2, 3):
        for enc in ("none", "set", "empty"):
            for bv in (1, 2, 3):
                add(hv=hv, enc=enc, bv=bv)
    # every stored SerDe version at eight consecutive payload lengths: the stored length and the output length
    # (stored + 17 / 13 / 12 / 4 / 0) each at every position of a word
    for sv in (1, 2, 3, 4, 5):
        for w in range(8):
            add(sv=sv, w=w)
            add(sv=sv, w=w, hv=3, enc="set", bv=3)
    # flag bytes other than 0 / 1, and 1 itself
    for sv, priv, encb in ((5, 2, 0), (5, 0, 2), (5, 1, 1), (5, -1, -1), (4, 0, 3), (3, 0, 3), (4, 1, 1), (3, 2, 1),
                           (2, 2, 0), (1, 2, 0), (1, 1, 0)):
        for hv in (2, 3):
            add(sv=sv, priv=priv, encb=encb, hv=hv, bv=3)
    # the blob record: every input version, isCompressed 0 / 1 / other, bodies of 0 and 1 bytes
    for bv, comp in ((1, 0), (2, 0), (3, 0), (3, 1), (3, 2)):
        for n in (0, 1, 17):
            for hv in (1, 3):
                add(bv=bv, comp=comp, n=n, hv=hv, sv=5 if hv == 3 else 2)
    for um in (0, 1):
        for hv in (1, 2, 3):
            add(um=um, hv=hv, sv=5, bv=3)
    # the re-key's overlays: metadata blobs with their content replaced (0 and 1 bytes), the blob size given and
    # not, ids of either sign; data blobs keep their content
    for bv in (2, 3):
        for repl in (0, 1):
            for bs in ("given", "none"):
                for ids in ("pos", "neg"):
                    add(meta=1, bv=bv, repl=repl, bs=bs, ids=ids, sv=1 + len(out) % 5)
    for sv in (1, 2, 3, 4, 5):
        for bs in ("given", "none"):
            for ids in ("pos", "neg"):
                add(sv=sv, bs=bs, ids=ids, bv=1 + sv % 3)
    # a dense run the fast path takes, flags 0 and 1, with and without the encryption key
    for t in range(24):
        add(hv=3, bv=3, sv=5, priv=t % 2, encb=(t // 2) % 2, comp=(t // 4) % 2, enc=("none", "set", "empty")[t % 3],
            w=t % 8, n=t % 3, um=t % 2)
    return out


@functools.lru_cache(maxsize=None)
def region(fast_only: bool = False):
    """(region, offsets, cases): the stored messages end to end."""
    cs = [c for c in cases() if c.fast()] if fast_only else cases()
    offs, buf = [], bytearray()
    for c in cs:
        offs.append(len(buf))
        buf += c.stored()
    return bytes(buf), offs, cs


def fast_region():
    return region(True)


@functools.lru_cache(maxsize=None)
def rekey_inputs():
    """(descs as rekey_oracle.DESC, aux): a new key of 3 + i % 14 bytes for every case, its other fields as the
    case says."""
    import numpy as np

    cs = cases()
    descs, aux = np.zeros(len(cs), dtype=RK.DESC), bytearray(b"#")
    for i, c in enumerate(cs):
        d = descs[i]
        klen = 3 + i % 14
        d["key_src"], d["key_len"] = len(aux), klen
        aux += bytes(0x30 + (i + t) % 40 for t in range(klen))
        d["content_src"], d["content_len"] = RK.KEEP, 0
        if c.repl != "keep":
            d["content_src"], d["content_len"] = len(aux), c.repl
            aux += bytes(0x80 + (i + t) % 100 for t in range(c.repl))
        d["props_blob_size"] = (1 << 33) + 1000 * i + 7 if c.bs == "given" else -1
        d["account_id"], d["container_id"] = (-2 - i % 300, -32768 + i) if c.ids == "neg" else (300 + i, 1 + i % 90)
    return descs, bytes(aux) + b"#"


@functools.lru_cache(maxsize=None)
def wire():
    """(wire bytes, refs as ingest_oracle.REF): each case's fields framed as a PutRequest. The request version is
    the lowest that carries the case's fields: 3, 4 with an encryption key (an empty one reads as none), 5 with
    an isCompressed byte."""
    import numpy as np

    cs = cases()
    refs, buf = np.zeros(len(cs), dtype=IO.REF), bytearray()
    for i, c in enumerate(cs):
        version = 5 if c.comp else 4 if c.enc != "none" else 3
        fr = IO.frame(version, c.key, c.props, c.usermeta, c.content, blob_type=c.meta, enc_key=c.enckey or b"",
                      compressed=c.comp, client_id=b"" if i % 4 == 0 else b"cl-%d" % i, correlation=i)
        buf += bytes(i % 3)
        refs[i] = (len(buf), len(c.key), 0)
        buf += fr
    return bytes(buf), refs


@functools.lru_cache(maxsize=None)
def put_messages(version: int, big_tail: bool = False):
    """(PutMessages, the oracle's bytes of each) at output header `version`: the stored payload written as it is
    (the serializer re-encodes nothing). big_tail: one more message above the streamed form's limit, so that a
    copy-mode batch also runs the job path."""
    from ambry_amd.messages import PutMessage

    msgs, exp = [], []
    for c in cases():
        enc = c.enckey if version >= 2 else None
        msgs.append(PutMessage(key=c.key, props=c.props, usermeta=c.usermeta, blob=c.content, enckey=enc,
                               header_version=version, life_version=c.index % 5 if version == 3 else 0,
                               blob_type=c.meta, compressed=c.comp == 1))
    if big_tail:
        blob = bytes(1 + t % 251 for t in range(BIG_BLOB))
        msgs.append(PutMessage(key=MF.store_key("emit-big"), props=MF.blob_properties_bytes(BIG_BLOB), usermeta=b"um",
                               blob=blob, enckey=b"k" * 16 if version >= 2 else None, header_version=version))
    for m in msgs:
        exp.append(MF.put_message(m.key, m.props, m.usermeta, m.blob, version=version, enc_key=m.enckey,
                                  life=m.life_version, compressed=m.compressed, blob_type=m.blob_type))
    return msgs, exp


# ---------------------------------------------------------------- what the oracles give over the lattice
OUT_VERSIONS = (1, 2, 3)


def life_of(i: int, version: int, use_life: bool):
    return (i % 5 if use_life else None)


@functools.lru_cache(maxsize=None)
def transform_expected(version: int, use_life: bool, fast_only: bool = False):
    """[(status, bytes)] of MF.transform_message over the lattice's region."""
    stored, offs, _ = region(fast_only)
    return [MF.transform_message(stored, o, life=life_of(i, version, use_life), version=version)
            for i, o in enumerate(offs)]


@functools.lru_cache(maxsize=None)
def rekey_expected(version: int, use_life: bool):
    stored, offs, _ = region()
    descs, aux = rekey_inputs()
    return [RK.rekey_message(stored, o, descs[i], aux, life=life_of(i, version, use_life), version=version)
            for i, o in enumerate(offs)]


@functools.lru_cache(maxsize=None)
def ingest_expected(version: int):
    frames, refs = wire()
    return IO.expected(frames, refs, version)


def assert_packed(out, oo, ol, st, exp, names):
    """A batch's outputs against [(status, bytes)]: packed in message order from 0."""
    pos = 0
    for i, (est, b) in enumerate(exp):
        assert int(st[i]) == est, "%s: status %#x, expected %#x" % (names[i], int(st[i]), est)
        assert int(oo[i]) == pos and int(ol[i]) == len(b), "%s: placed at %d + %d, expected %d + %d" % (
            names[i], int(oo[i]), int(ol[i]), pos, len(b))
        have = bytes(out[pos:pos + len(b)])
        assert have == b, "%s: output differs from byte %d of %d on" % (
            names[i], next((k for k, (x, y) in enumerate(zip(have, b)) if x != y), min(len(have), len(b))), len(b))
        pos += len(b)
