"""Expected results of a recovery scan (BlobStoreRecovery.recover, ambry-messageformat/.../BlobStoreRecovery.java
:43-139), from oracle/message_format.py (parse_header, verify_message, parse_blob_properties), zlib and plain
Python integers: independent of the library's header walk, its field reader and its 64-bit arithmetic. Shared by
test_recover_cpu.py and test_gpu_recover.py, with the message and region builders both use."""
import struct
import zlib

import numpy as np

from msgfmt import MF
from oracle_common import BAD_INFO, LONG_MAX, MESSAGE_INFO as INFO, add_seconds_to_epoch, same
from regions import join

NO_MESSAGE = 0xFFFFFFFFFFFFFFFF
RESULT = np.dtype([("chained", "<u8"), ("recovered", "<u8"), ("end_off", "<u8"), ("end_status", "<u4"),
                   ("more", "<u4")])
DELETED, TTL_UPDATED, UNDELETED = 1, 2, 4


# ---------------------------------------------------------------- the oracle
def accept_header(region: bytes, off: int):
    """(0, next start) when the walk hops over the header at off, else (why it stops, None): the version,
    the header inside the region, verifyHeader, then the sizes (BlobStoreRecovery.java:51-71 and what
    ambrycrc_chain_messages_host asks of the sizes)."""
    n = len(region)
    if off + 2 > n:
        return MF.BAD_LAYOUT, None  # IndexOutOfBounds, :51
    v = MF._be16(region, off)
    if v not in MF.HEADER_SIZE:
        return MF.BAD_VERSION, None
    h = MF.HEADER_SIZE[v]
    if off + h > n:
        return MF.BAD_LAYOUT, None  # IndexOutOfBounds, :64
    if zlib.crc32(region[off:off + h - 8]) != MF._be64(region, off + h - 8):
        return MF.HEADER_CRC, None
    _, total, rel = MF.parse_header(region, off)
    present = [r for r in rel if r != MF.INVALID]
    if total <= 0 or not present or present[0] < h or off + present[0] + total > n:
        return MF.BAD_LAYOUT, None
    return 0, off + present[0] + total


def message_info(region: bytes, off: int):
    """(status, info dict or None) of the message at off: the verify, then BlobStoreRecovery.java:75-116."""
    status, _ = MF.verify_message(region, off)
    if status:
        return status, None
    v, total, rel = MF.parse_header(region, off)
    enc, bp, upd, um, blob = rel
    h = MF.HEADER_SIZE[v]
    first = [r for r in rel if r != MF.INVALID][0]
    f = {"msg_off": off, "size": first + total, "key_rel": h, "key_len": first - h, "header_version": v,
         "life_version": MF._be16(region, off + 2) if v == 3 else 0}
    if bp != MF.INVALID:
        p, _ = MF.parse_blob_properties(region, off + bp + 2, off + um - 8)
        f.update(flags=0, account_id=p["account"], container_id=p["container"], operation_time_ms=p["creation"],
                 expires_at_ms=add_seconds_to_epoch(p["creation"], p["ttl"]))
    else:
        uv = MF._be16(region, off + upd)
        kind, account, container, when = 0, -1, -1, -1  # Update_Format_V1: MessageFormatRecord.java:1242
        if uv >= 2:
            account, container, when = struct.unpack_from(">hhq", region, off + upd + 2)
        if uv == 3:
            kind = MF._be16(region, off + upd + 14)
        f.update(flags=1 << kind, account_id=account, container_id=container, operation_time_ms=when,
                 expires_at_ms=-1)  # MessageInfo.java:104-108
    if f["operation_time_ms"] < -1:
        return BAD_INFO, None  # IllegalArgumentException, MessageInfo.java:172
    return 0, f


def recover(region: bytes, start: int = 0, max_m: int = 1 << 20, chain_only=False):
    """(offsets, statuses, infos, result dict) of one call: the hop over every accepted header, each
    message's status and info, the clean prefix and where recovery stops."""
    offs, sts, infos = [], [], []
    off, end_status = start, 0
    while off < len(region) and len(offs) < max_m:
        end_status, nxt = accept_header(region, off)
        if end_status:
            break
        st, f = (0, None) if chain_only else message_info(region, off)
        offs.append(off)
        sts.append(st)
        infos.append(f)
        off = nxt
    res = {"chained": len(offs), "recovered": len(offs), "end_off": off, "end_status": end_status,
           "more": int(end_status == 0 and off != len(region))}
    bad = [i for i, s in enumerate(sts) if s]
    if bad and not chain_only:
        res.update(recovered=bad[0], end_off=offs[bad[0]], end_status=sts[bad[0]], more=0)
    return offs, sts, infos, res


def chain_result(region: bytes, start: int = 0, max_m: int = 1 << 20):
    """(offsets, result dict) of the chain entry: recover's walk without the messages' verdicts."""
    offs, _, _, res = recover(region, start, max_m, chain_only=True)
    return offs, res


def info_array(infos, max_m=None):
    """The infos as an INFO array of max_m rows: zero rows for the refused messages and the unused slots."""
    a = np.zeros(len(infos) if max_m is None else max_m, dtype=INFO)
    for i, f in enumerate(infos):
        if f is not None:
            for k, v in f.items():
                a[i][k] = v
    return a


def assert_call(got, exp, max_m):
    """One recover call's outputs (numpy: msg_off, info, status, result) against recover()'s."""
    msg_off, info, status, res = got
    offs, sts, infos, eres = exp
    have = {k: int(res[k]) for k in RESULT.names}
    assert have == eres, "result struct %s, expected %s" % (have, eres)
    same(msg_off, np.array(offs + [NO_MESSAGE] * (max_m - len(offs)), dtype=np.uint64), "msg_off")
    same(status, np.array(sts + [MF.BAD_LAYOUT] * (len(status) - len(sts)), dtype=np.uint32), "status")
    same(info, info_array(infos, max_m), "info")


# ---------------------------------------------------------------- stored messages
def update_record(uv=3, kind="delete", account=101, container=5, when=1_700_000_000_123, expiry=-1) -> bytes:
    """Update_Format_V1 (a byte), V2 (account, container, time: a delete) or V3 (MF.update_record_v3)."""
    if uv == 3:
        return MF.update_record_v3(account=account, container=container, update_ms=when, kind=kind, expiry=expiry)
    body = struct.pack(">hb", 1, 1) if uv == 1 else struct.pack(">hhhq", 2, account, container, when)
    return body + MF._crc_long(body)


def update_message(key: bytes, hv=3, life=1, **kw) -> bytes:
    h = MF.HEADER_SIZE[hv]
    rec = update_record(**kw)
    return MF.header(hv, len(rec), MF.INVALID, MF.INVALID, h + len(key), MF.INVALID, MF.INVALID, life) + key + rec


def put_message(key: bytes, content: bytes, hv=3, um=b"", enc_key=None, life=0, **props) -> bytes:
    import rekey_oracle as RK

    return RK.stored_put(key, MF.blob_properties_bytes(len(content), **props), um, content, hv=hv, enc_key=enc_key,
                         life=life)


def scan_geometry(names=("kScanBlock", "kScanWave")):
    """(kScanBlock, kScanWave) of ambry_amd/csrc/recover.h: the candidate scan's block and wave-load bytes."""
    import os
    import re

    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ambry_amd", "csrc",
                           "recover.h")) as f:
        text = f.read()
    return tuple(int(re.search(r"constexpr uint32_t %s = (\d+);" % n, text).group(1)) for n in names)


def sized_put(key: bytes, size: int, hv=3, fill=b"\xa5", **props) -> bytes:
    """A clean PUT of exactly `size` bytes: the user metadata takes up the slack."""
    base = len(put_message(key, b"12345678", hv=hv, **props))
    assert size >= base, (size, base)
    m = put_message(key, b"12345678", hv=hv, um=fill * (size - base), **props)
    assert len(m) == size
    return m


def residue_region():
    """65 PUTs of 193 = 3 * 64 + 1 bytes: the starts take every residue mod 64."""
    return join([sized_put(MF.store_key("r%02d" % i), 193, hv=1 + i % 3) for i in range(65)])


def straddle_region(d: int):
    """Messages that start at W + d, B + d and 2B + d (W: the scan's wave-load bytes, B: its block), after one
    at 0 and before a short update: for d in -40 .. 1 a version pair and a header straddling each boundary."""
    block, wave = scan_geometry()
    starts = [0, wave + d, block + d, 2 * block + d]
    msgs = [sized_put(MF.store_key("s%d" % i), b - a, hv=1 + (i + d) % 3)
            for i, (a, b) in enumerate(zip(starts, starts[1:]))]
    msgs += [sized_put(MF.store_key("s3"), 300), update_message(MF.store_key("s4"), kind="undelete")]
    region, offs = join(msgs)
    assert offs[:4] == starts
    return region, offs


def embedded_header(nxt: int, hv=3) -> bytes:
    """A header with a good CRC whose walk would hop `nxt` bytes: accepted wherever the region holds nxt bytes
    from it on."""
    h = MF.HEADER_SIZE[hv]
    return MF.header(hv, nxt - h, MF.INVALID, h, MF.INVALID, h + 1, h + 2, 0)


def false_node_region():
    """(region, real starts, embedded positions: {name: [positions]}): real messages whose blobs hold valid
    headers -- a whole clean 50-message region, one header whose next is a later real message's start, one
    whose message would overrun the region."""
    import rekey_oracle as RK

    inner, inner_offs, _ = RK.build_region(n=50, seed=5, corrupt_frac=0.0, big_every=10**9, max_blob=600,
                                           max_usermeta=100)
    key = MF.store_key
    msgs = [put_message(key("f0"), b"first", hv=2), put_message(key("f1"), inner, hv=3)]
    pad = b"\x5a" * 100
    tail = [put_message(key("f3"), b"after", hv=1), update_message(key("f4"), kind="ttl"),
            put_message(key("f5"), b"last" * 50, hv=3)]
    # the header that points at f4's start, and the one that points one byte past the region's end
    probe = put_message(key("f2"), pad + embedded_header(40) + pad + embedded_header(40) + pad, hv=3)
    at = sum(len(m) for m in msgs)
    body = probe.index(embedded_header(40))
    p1 = at + body
    p2 = p1 + 40 + len(pad)
    f4 = at + len(probe) + len(tail[0])
    end = at + len(probe) + sum(len(m) for m in tail)
    msgs.append(put_message(key("f2"), pad + embedded_header(f4 - p1) + pad + embedded_header(end + 1 - p2) + pad,
                            hv=3))
    region, offs = join(msgs + tail)
    assert len(region) == end and offs[4] == f4
    inner_at = offs[1] + msgs[1].index(inner)
    return region, offs, {"region": [inner_at + o for o in inner_offs], "lands": [p1], "overruns": [p2]}


def dense_false_node_region():
    """(region, real starts, the embedded positions): a blob of 300 headers 48 bytes apart, each hopping onto
    the next -- more nodes in a scan block than the scan stages (kStageMax of recover.h)."""
    key = MF.store_key
    msgs = [put_message(key("g0"), b"first", hv=1), put_message(key("g1"), (embedded_header(48) + b"\xee" * 8) * 300, hv=3),
            update_message(key("g2"), kind="ttl"), put_message(key("g3"), b"last", hv=2)]
    region, offs = join(msgs)
    at = offs[1] + msgs[1].index(embedded_header(48))
    return region, offs, [at + 48 * i for i in range(300)]


def decoy_region():
    """(region, starts): two PUTs whose 64 KiB blobs repeat `00 01` and `00 00 03` (period 3: every residue),
    between small messages."""
    key = MF.store_key
    return join([update_message(key("d0")), put_message(key("d1"), b"\x00\x01" * 32768, hv=3),
                 put_message(key("d2"), (b"\x00\x00\x03" * 21846)[:65536], hv=2), update_message(key("d3"), kind="ttl")])


def candidates(region: bytes) -> int:
    """Byte positions holding a big-endian short in 1..3."""
    a = np.frombuffer(region, dtype=np.uint8)
    return int(np.count_nonzero((a[:-1] == 0) & (a[1:] >= 1) & (a[1:] <= 3)))


def update_chain(n: int):
    """(region, message length): n update messages end to end (the doubling rounds' chains)."""
    one = update_message(MF.store_key("update-chain-message-00"), hv=3, kind="delete")
    return one * n, len(one)


def mixed_region():
    """A clean region of every stored format, and the same with one message in ten corrupted."""
    import rekey_oracle as RK

    return RK.build_region(n=300, seed=2, corrupt_frac=0.0), RK.build_region(n=300, seed=2, corrupt_frac=0.1)


def stop_cases():
    """[(name, region)]: five clean messages (PUT with key, PUT, update, PUT, update) with one thing wrong."""
    key = MF.store_key
    msgs = [put_message(key("a"), b"A" * 300, hv=3, um=b"um" * 20, enc_key=b"k" * 32),
            put_message(key("b"), b"B" * 100, hv=2, um=b"x"), update_message(key("c"), kind="delete"),
            put_message(key("d"), b"D" * 500, hv=1, um=b"meta"), update_message(key("e"), kind="ttl")]
    region, offs = join(msgs)

    def flipped(pos, bit=1):
        b = bytearray(region)
        b[pos] ^= bit
        return bytes(b)

    def resized(i, total):  # message i's size field rewritten under a fresh header CRC
        v, _, rel = MF.parse_header(region, offs[i])
        return region[:offs[i]] + MF.header(v, total, *rel) + region[offs[i] + MF.HEADER_SIZE[v]:]

    _, _, rel0 = MF.parse_header(region, offs[0])
    _, _, rel2 = MF.parse_header(region, offs[2])
    cases = [("clean", region), ("version", flipped(offs[1] + 1, 0x10)), ("version-0", flipped(offs[3] + 1, 1)),
             ("header-crc", flipped(offs[2] + 39)), ("size-flip", flipped(offs[1] + 9)),
             ("size-zero", resized(3, 0)), ("size-over", resized(4, 10**6)), ("size-negative", resized(1, -5)),
             ("one-byte-short", region[:-1]), ("one-trailing", region + b"\x00"),
             ("trailing-header", region + b"\x00\x03" + b"\x11" * 31), ("trailing-version", region + b"\x00\x07")]
    for name, k, at in (("enckey", 0, 9), ("props", 1, 9), ("usermeta", 3, 9), ("blob", 4, 14)):
        cases.append(("record-" + name, flipped(offs[0] + rel0[k] + at, 4)))
    cases.append(("record-update", flipped(offs[2] + rel2[2] + 5, 2)))
    return cases


def recovery_test_region(hv: int, partial=False, ttl=9999, seed=3):
    """BlobStoreRecoveryTest.ReadImp.initialize (BlobStoreRecoveryTest.java:79-182): six messages -- at header
    V2 / V3 PUT (ttl 9999), PUT, PUT without an encryption key, TTL update, delete, TTL update; at V1, which has
    neither encryption keys nor TTL updates, PUTs in the updates' places -- and with `partial` a seventh PUT
    cut at half its size."""
    rng = np.random.default_rng(seed)
    enc, um, blob = (rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (256, 2000, 4000))
    keys = [MF.store_key("id%d" % i) for i in range(1, 7)]
    now = 1_700_000_123_456

    def put(k, with_enc=True, ttl=-1):
        return put_message(keys[k], blob, hv=hv, um=um, enc_key=enc if with_enc else None, ttl=ttl, account=k + 10,
                           container=k + 20, creation_ms=now, service_id="test", owner_id="mem1", content_type="img")

    def ttl_update(k):
        return update_message(keys[k], hv=hv, life=0, uv=3, kind="ttl", account=k + 10, container=k + 20, when=now + 7)

    msgs = [put(0, ttl=ttl), put(1), put(2, with_enc=False),
            ttl_update(1) if hv >= 2 else put(3),
            update_message(keys[1], hv=hv, life=0, uv=3 if hv >= 2 else 2, kind="delete", account=11, container=21,
                           when=now + 7),
            ttl_update(0) if hv >= 2 else put(4)]
    if partial:
        last = put(5)
        msgs.append(last[:len(last) // 2])
    region, offs = join(msgs)
    return region, offs, [len(m) for m in msgs], now


# (name, BlobProperties fields, the status recover gives): the expiry arithmetic's edges and a creation time below -1
INFO_CASES = [
    ("ttl-forever", dict(ttl=-1), 0), ("creation-forever", dict(creation_ms=-1, ttl=50), 0),
    ("ttl-negative", dict(ttl=-5), 0), ("ttl-saturates", dict(ttl=1 << 62), 0),
    ("wraps", dict(creation_ms=(1 << 62) + 1, ttl=1 << 62), 0), ("creation-bad", dict(creation_ms=-2), BAD_INFO),
    ("ttl-min", dict(ttl=-(1 << 63)), 0), ("edge-over", dict(ttl=LONG_MAX // 1000 + 1, creation_ms=5), 0),
    ("edge-at", dict(ttl=LONG_MAX // 1000, creation_ms=900), 0),
]
