"""Expected results of MessageFormatSend.fetchDataFromReadSet (ambry-messageformat/.../MessageFormatSend.java
:112-242) as ambrycrc_send_messages_dev / ambrycrc_send_message_cpu define them, from oracle/message_format.py
and zlib alone: independent of the library's parser and of its copy-through pass. Shared by test_send_cpu.py
and test_gpu_send.py."""
import numpy as np

from msgfmt import MF
from oracle_common import NO_ROOM, NOWHERE, crc_bad as _crc_bad, flip as _flip, place_packed, refit as _refit

BLOB_PROPERTIES, BLOB_USER_METADATA, BLOB, ALL, BLOB_INFO = 0, 1, 2, 3, 4
FLAGS = (BLOB_PROPERTIES, BLOB_USER_METADATA, BLOB, ALL, BLOB_INFO)

INFO = np.dtype([("out_off", "<u8"), ("send_len", "<u8"), ("rel_off", "<u4"), ("enckey_rel", "<u4"),
                 ("enckey_len", "<u4"), ("check", "<u4")])
RECORD_BITS = (MF.ENCKEY_CRC, MF.PROPS_CRC, MF.UPDATE_CRC, MF.USERMETA_CRC, MF.BLOB_CRC)


def _refused(status):
    return status, dict(out_off=NOWHERE, send_len=0, rel_off=0, enckey_rel=0, enckey_len=0, check=0), None


def send_message(region: bytes, off: int, size, flag: int):
    """(status, info fields, sent bytes or None) for one message. size None: the header's own message length.
    out_off is 0 for a sent message (expected() places it)."""
    if off > len(region) or (size is not None and (size == 0 or off + size > len(region))):
        return _refused(MF.BAD_LAYOUT)
    vst, vend = MF.verify_message(region, off)
    hdr = vst if vend == 0 else 0  # verify_message ends at 0 exactly when the header does not parse
    if hdr:
        if flag == ALL and size is not None:  # :142: sent whole, the header never parsed; deserializeBlobAll counted
            return 0, dict(out_off=0, send_len=size, rel_off=0, enckey_rel=0, enckey_len=0, check=hdr), \
                region[off:off + size]
        return _refused(hdr)
    v, total, rel = MF.parse_header(region, off)
    present = [(k, r) for k, r in enumerate(rel) if r != MF.INVALID]
    length = present[0][1] + total
    ends = {k: (present[i + 1][1] if i + 1 < len(present) else length) for i, (k, _) in enumerate(present)}
    is_update = rel[2] != MF.INVALID
    if flag == ALL:
        sz = length if size is None else size
        check = vst | (MF.NOT_PUT if is_update else 0) | (MF.BAD_LAYOUT if sz < length else 0)
        return 0, dict(out_off=0, send_len=sz, rel_off=0, enckey_rel=0, enckey_len=0, check=check), \
            region[off:off + sz]
    if is_update:
        return _refused(MF.NOT_PUT)
    sz = length if size is None else size
    sent = {BLOB: (4,), BLOB_PROPERTIES: (1,), BLOB_USER_METADATA: (3,), BLOB_INFO: (1, 3)}[flag]
    lo, hi = rel[sent[0]], ends[sent[-1]]
    reads_enc = flag != BLOB_PROPERTIES and rel[0] != MF.INVALID
    if hi > sz or (reads_enc and ends[0] > sz):
        return _refused(MF.BAD_LAYOUT)
    enckey_rel = enckey_len = 0
    if reads_enc:  # deserializeBlobEncryptionKey throws
        bits = MF._record_check(0, region[off + rel[0]:off + ends[0]])
        if _crc_bad(region, off + rel[0], off + ends[0]):
            bits |= MF.ENCKEY_CRC
        if bits:
            return _refused(bits)
        enckey_rel, enckey_len = rel[0] + 6, MF._be32(region, off + rel[0] + 2)
    if flag == BLOB:
        check = vst
    else:
        check = 0
        for k in sent:
            check |= MF._record_check(k, region[off + rel[k]:off + ends[k]])
            if _crc_bad(region, off + rel[k], off + ends[k]):
                check |= RECORD_BITS[k]
    return 0, dict(out_off=0, send_len=hi - lo, rel_off=lo, enckey_rel=enckey_rel, enckey_len=enckey_len,
                   check=check), region[off + lo:off + hi]


def expected(region: bytes, offs, sizes, flag: int, out_cap=None):
    """(status list, INFO array, the packed output) of a batch: spans in message order over the sent messages,
    a span past out_cap refused with NO_ROOM (send_len 0, nowhere; rel_off, the key fields and check kept)
    while still advancing the running offset."""
    res = [send_message(region, int(off), None if sizes is None else int(sizes[i]), flag) for i, off in enumerate(offs)]
    at = place_packed([len(b) if st == 0 else None for st, _, b in res], out_cap)
    status, info, packed = [], np.zeros(len(offs), dtype=INFO), bytearray()
    for i, (st, f, b) in enumerate(res):
        if st == 0 and at[i] is None:
            st = NO_ROOM
            f["out_off"], f["send_len"] = NOWHERE, 0
        elif st == 0:
            f["out_off"] = at[i]
            packed += bytes(at[i] - len(packed)) + b
        status.append(st)
        info[i] = tuple(f[n] for n in INFO.names)
    return status, info, bytes(packed)


# ---------------------------------------------------------------- each rule once
def rule_cases():
    """(names, region, offsets, sizes): one message per rule of ambrycrc_send_messages_dev. sizes[i] is what a
    sized batch passes for message i (the header's own length where the rule is not about the size); a batch
    without sizes runs the same messages. Built once."""
    from datagen import stream_bytes

    def put(hv, enc):
        return MF.put_message(MF.store_key(f"rule-{hv}"), MF.blob_properties_bytes(1000), stream_bytes(3, 1, 50).tobytes(),
                              stream_bytes(4, 2, 1000).tobytes(), version=hv, enc_key=enc, life=1)

    cases = []  # (name, bytes, size: None = the header's length, or an int)
    for tag, msg in (("v3", put(3, b"k" * 32)), ("v1", put(1, None))):
        _, _, rel = MF.parse_header(msg, 0)
        h = MF.HEADER_SIZE[MF._be16(msg, 0)]
        cases.append((tag + "-clean", msg, None))
        cases.append((tag + "-header", _flip(msg, 5), None))
        cases.append((tag + "-key", _flip(msg, h + 3), None))
        if rel[0] != MF.INVALID:
            cases.append((tag + "-enckey", _flip(msg, rel[0] + 10), None))
            cases.append((tag + "-enckey-version", _refit(msg, rel[0], rel[1], lambda r: r.__setitem__(1, 2)), None))
            cases.append((tag + "-enckey-size", _refit(msg, rel[0], rel[1], lambda r: r.__setitem__(5, r[5] + 1)), None))
        cases.append((tag + "-props", _flip(msg, rel[1] + 12), None))
        cases.append((tag + "-usermeta", _flip(msg, rel[3] + 9), None))
        cases.append((tag + "-content", _flip(msg, rel[4] + 500), None))
        cases.append((tag + "-trailer", _flip(msg, len(msg) - 2), None))
        cases.append((tag + "-larger", msg, len(msg) + 7))
        cases.append((tag + "-smaller", msg, len(msg) - 5))
        cases.append((tag + "-much-smaller", msg, rel[3] + 3))
        cases.append((tag + "-equal", msg, len(msg)))
        cases.append((tag + "-bad-version-sized", b"\x00\x09" + msg[2:], len(msg)))
        cases.append((tag + "-size-0", msg, 0))
    cases.append(("update", MF.update_message(MF.store_key("rule-u"), version=3, kind="ttl"), None))
    upd = MF.update_message(MF.store_key("rule-d"), version=3, kind="delete")
    cases.append(("update-record", _flip(upd, MF.parse_header(upd, 0)[2][2] + 5), None))
    last = put(3, b"z" * 16)
    cases.append(("past-region", last, len(last) + 1))  # the region ends with this message
    names, offs, sizes, region = [], [], [], bytearray()
    for name, b, size in cases:
        names.append(name)
        offs.append(len(region))
        sizes.append(len(b) if size is None else size)
        region += b
    return names, bytes(region), offs, sizes


def header_length(region: bytes, off: int):
    """The header's own message length, or None when it does not parse."""
    end = MF.verify_message(region, off)[1]
    return end - off if end else None


def mix(status, info):
    """How many messages were sent clean, sent with findings, and refused."""
    clean = sum(1 for s, f in zip(status, info) if s == 0 and int(f["check"]) == 0)
    found = sum(1 for s, f in zip(status, info) if s == 0 and int(f["check"]) != 0)
    return clean, found, sum(1 for s in status if s != 0)


def run_cpu(messages, region: bytes, offs, sizes, flag: int, out_cap=None):
    """The batch through the CPU entry, message by message, packed as expected() packs it."""
    buf = np.frombuffer(region, dtype=np.uint8)
    status, info, packed, pos = [], np.zeros(len(offs), dtype=INFO), bytearray(), 0
    for i, off in enumerate(offs):
        left = None if out_cap is None else max(out_cap - pos, 0)
        st, f, b = messages.send_message_cpu(buf, int(off), flag, size=None if sizes is None else int(sizes[i]),
                                             out_cap=left)
        if st == 0:
            f["out_off"] = pos
            packed += bytes(pos - len(packed)) + b
            pos += len(b)
        elif st == NO_ROOM:  # its length, for the running offset: the call again with room
            _, g, _ = messages.send_message_cpu(buf, int(off), flag, size=None if sizes is None else int(sizes[i]))
            pos += int(g["send_len"])
        status.append(st)
        info[i] = f
    return status, info, bytes(packed)
