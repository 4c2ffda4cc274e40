"""Expected results for batches far larger than the Python oracle can walk: one tile of T mixed messages, judged by
the oracle once, and the expectation for K back-to-back copies of it derived with numpy. Every message operation
is position-independent per message, so over K copies the statuses, lengths and output bytes repeat and the
offsets shift by k tile lengths (or k packed output lengths). test_scale_tiles.py proves each derivation here
against the oracle itself on two concatenated tiles; test_gpu_scale.py uses them at K in the hundreds.

T is prime, so no grid stride of a thread-per-message kernel is a multiple of it: a thread's second and later
messages are never the same tile message as its first."""
import functools
import struct
from types import SimpleNamespace

import numpy as np

import hard_delete_oracle as HD
import rekey_oracle as RK
from msgfmt import MF
from regions import put_expected

T = 1201
NOWHERE = -1  # out_off of a message not written, as the int64 the device returns


# ---------------------------------------------------------------- the tile and the oracle over a region
@functools.lru_cache(maxsize=None)
def tile():
    """The tile: region bytes, message offsets (int64 array), metadata-blob flags, re-key descriptors and their
    aux bytes. Every stored format of RK.build_region, 10 % corrupted, about 1 KiB per message."""
    region, offs, meta = RK.build_region(n=T, seed=1, corrupt_frac=0.1, big_every=10**9, max_blob=1000,
                                         max_usermeta=400)
    descs, aux = RK.build_descs(offs, meta, seed=1)
    return SimpleNamespace(region=region, offs=np.asarray(offs, dtype=np.int64), meta=meta, descs=descs, aux=aux,
                           life=np.random.default_rng(5).integers(0, 9, size=T).astype(np.int16))


def header_versions(region: bytes, offs) -> np.ndarray:
    """The version field each message starts with (0 when it is none of 1, 2, 3)."""
    v = np.array([struct.unpack_from(">h", region, int(o))[0] for o in offs], dtype=np.int64)
    return np.where((v >= 1) & (v <= 3), v, 0)


def verify_oracle(region: bytes, offs):
    """(status uint32[m], msg_end int64[m])."""
    res = [MF.verify_message(region, int(o)) for o in offs]
    return np.array([s for s, _ in res], dtype=np.uint32), np.array([e for _, e in res], dtype=np.int64)


def transform_oracle(region: bytes, offs, life=None, version: int = 3):
    """(status uint32[m], out_off int64[m] (-1: refused), out_len int64[m], the packed output)."""
    st, off, ln, packed = [], [], [], bytearray()
    for i, o in enumerate(offs):
        s, b = MF.transform_message(region, int(o), life=None if life is None else int(life[i]), version=version)
        st.append(s)
        off.append(NOWHERE if b is None else len(packed))
        ln.append(0 if b is None else len(b))
        packed += b or b""
    return np.array(st, dtype=np.uint32), np.array(off, dtype=np.int64), np.array(ln, dtype=np.int64), bytes(packed)


def hard_delete_oracle(region: bytes, offs, recovery=None):
    """(status uint32[m], info HD.INFO[m], the region after)."""
    st, info, out = HD.hard_delete(region, [int(o) for o in offs], recovery)
    return np.array(st, dtype=np.uint32), info, out


def rekey_oracle(region: bytes, offs, descs, aux: bytes, life=None, version: int = 3, out_cap=None):
    """(status uint32[m], out_off int64[m] (-1: not written), out_len int64[m], the packed output)."""
    st, off, ln, packed = RK.expected(region, [int(o) for o in offs], descs, aux, life=life, version=version,
                                      out_cap=out_cap)
    return (np.array(st, dtype=np.uint32), np.array(off, dtype=np.uint64).view(np.int64),
            np.array(ln, dtype=np.int64), packed)


def clean_puts(region: bytes, offs, status):
    """The PutMessage of every message of the region that verifies clean and is a PUT: what a serializer would
    have been handed for it (its blob record is written as Blob_Format_V3 whatever version stored it)."""
    from ambry_amd.messages import PutMessage

    out = []
    for o, s in zip(offs, status):
        o = int(o)
        if s:
            continue
        v, total, (enc, bp, upd, um, blob) = MF.parse_header(region, o)
        if upd != MF.INVALID:
            continue
        first = enc if enc != MF.INVALID else bp
        bv = MF._be16(region, o + blob)
        head = HD.BLOB_HEAD[bv]
        out.append(PutMessage(
            key=region[o + MF.HEADER_SIZE[v]:o + first],
            enckey=None if enc == MF.INVALID else region[o + enc + 6:o + bp - 8],
            props=region[o + bp + 2:o + um - 8], usermeta=region[o + um + 6:o + blob - 8],
            blob=region[o + blob + head:o + first + total - 8], header_version=v,
            life_version=MF._be16(region, o + 2) if v == 3 else 0,
            blob_type=0 if bv == 1 else MF._be16(region, o + blob + 2),
            compressed=bool(bv == 3 and region[o + blob + 4] == 1)))
    return out


def serialize_oracle(msgs):
    """(descriptor array, fields, blobs, total output bytes, msg_len int64[n], the output): messages packed back
    to back by messages.pack_batch, every byte from oracle/message_format.py."""
    from ambry_amd.messages import pack_batch

    descs, fields, blobs, offs, total = pack_batch(msgs)
    outs = [put_expected(m) for m in msgs]
    assert offs == [int(x) for x in np.cumsum([0] + [len(b) for b in outs[:-1]])] and total == sum(map(len, outs))
    return descs, fields, blobs, total, np.array([len(b) for b in outs], dtype=np.int64), b"".join(outs)


# ---------------------------------------------------------------- K copies, by numpy alone
def tiled_offsets(offs, length: int, k: int) -> np.ndarray:
    """Message offsets of k back-to-back copies of a tile of `length` bytes."""
    return (np.arange(k, dtype=np.int64)[:, None] * length + np.asarray(offs, dtype=np.int64)[None, :]).reshape(-1)


def tiled_verify(status, end, length: int, k: int):
    """Statuses repeat; a message end shifts with its copy, and stays 0 where the header was refused."""
    end = np.asarray(end, dtype=np.int64)
    shift = np.arange(k, dtype=np.int64)[:, None] * length
    return np.tile(status, k), np.where(end[None, :] != 0, end[None, :] + shift, 0).reshape(-1)


def tiled_packed(status, out_off, out_len, packed_len: int, k: int):
    """Transform and uncapped re-key: statuses and lengths repeat, a written message's offset shifts by its
    copy's k packed lengths, an unwritten one stays at -1."""
    off = np.asarray(out_off, dtype=np.int64)
    shift = np.arange(k, dtype=np.int64)[:, None] * packed_len
    return (np.tile(status, k), np.where(off[None, :] != NOWHERE, off[None, :] + shift, NOWHERE).reshape(-1),
            np.tile(out_len, k))


def tiled_rekey_capped(status, out_len, k: int, out_cap: int):
    """Re-key into out_cap bytes, from the tile's uncapped statuses and lengths: the running offset is the
    exclusive sum of the uncapped lengths (it advances past a refused message too), a message that would end
    past out_cap is refused with NO_ROOM and written nowhere. Returns (status, out_off, out_len)."""
    st, ln = np.tile(status, k), np.tile(np.asarray(out_len, dtype=np.int64), k)
    pos = np.cumsum(ln) - ln
    refused = (ln > 0) & (pos + ln > out_cap)
    written = (ln > 0) & ~refused
    return (np.where(refused, np.uint32(RK.NO_ROOM), st).astype(np.uint32), np.where(written, pos, NOWHERE),
            np.where(written, ln, 0))


def tiled_recv_capped(status, info, k: int, out_cap: int):
    """The packed receive of k copies of a tile's payloads into out_cap bytes, from recv_oracle.expected's
    uncapped statuses and infos over one tile: a payload the rules accept (out_off set) takes the exclusive
    running sum of the accepted lengths -- which advances past a payload without room too -- and is placed there
    if it fits as recv_fits has it (at <= out_cap and len <= out_cap - at: an empty slice at out_cap fits, one past
    it does not); otherwise it is refused with NO_ROOM, its info zero and out_off nowhere. A payload refused by
    an earlier rule keeps its status and does not advance the sum. Returns (status, info, the end of the last
    placed non-empty slice)."""
    from oracle_common import NO_ROOM, NOWHERE as NOWHERE_U64

    st, out = np.tile(np.asarray(status, dtype=np.uint32), k), np.tile(info, k)
    accepted = out["out_off"] != np.uint64(NOWHERE_U64)
    ln = np.where(accepted, out["out_len"], 0).astype(np.uint64)
    pos = np.cumsum(ln, dtype=np.uint64) - ln
    cap = np.uint64(out_cap)
    fits = accepted & (pos <= cap) & (ln <= cap - np.minimum(pos, cap))
    refused = accepted & ~fits
    st[refused] = NO_ROOM
    out[refused] = np.zeros((), dtype=out.dtype)
    out["out_off"] = np.where(fits, pos, np.uint64(NOWHERE_U64))
    return st, out, int((pos + ln)[fits & (ln > 0)].max(initial=0))


def tiled_put_descs(descs, k: int, total: int, fields_len: int, blobs_len: int):
    """Serialize descriptors for k copies: out_off shifts by the tile's output bytes, the four field sources by
    the tile's field bytes, the blob source by its blob bytes (the source buffers are repeated too)."""
    out = np.tile(descs, k)
    c = np.repeat(np.arange(k, dtype=np.uint64), len(descs))
    out["out_off"] += c * np.uint64(total)
    for name in ("key_src", "enckey_src", "props_src", "usermeta_src"):
        out[name] += c * np.uint64(fields_len)
    out["blob_src"] += c * np.uint64(blobs_len)
    return out


def copies_above_caps(cus: int) -> int:
    """K such that m = K * T is at least 2 x 4 x 256 x CUs + 1: more than twice the widest capped grid."""
    return -(-(2 * 4 * 256 * cus + 1) // T)


def stride_mix(status, versions, cus: int, blocks_per_cu: int):
    """For a grid of blocks_per_cu x CUs blocks of 256 threads over copies_above_caps(cus) * T messages: among
    the pairs of messages (i, i + grid threads) one thread takes in successive trips, (the fraction whose
    (status, header version) differ, the number that go clean -> refused, the number refused -> clean)."""
    m, s = copies_above_caps(cus) * T, blocks_per_cu * 256 * cus
    i = np.arange(m - s, dtype=np.int64)
    a, b = i % T, (i + s) % T
    status, versions = np.asarray(status), np.asarray(versions)
    differ = (status[a] != status[b]) | (versions[a] != versions[b])
    return (float(differ.mean()), int(((status[a] == 0) & (status[b] != 0)).sum()),
            int(((status[a] != 0) & (status[b] == 0)).sum()))
