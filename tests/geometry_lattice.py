"""Record geometry by construction: inputs that put a CRC span on every start residue, length and size class at
which the CRC kernels change their case split, and cells(), the classifier the tests assert that coverage with.

The kernels split a span [pa, pa + length) by where it starts and ends on the 64-B run grid (region_crc.h
record_crc, record_crc_runs_wave), by its end's offset in a 16-B block and its count of 64-run rounds
(region_proc.h record_crc_direct), by its 64 KiB pieces (message_kernels.hip region_long_kernel) and, in the
batch engine's group phase, by its size class (crc32_kernels.hip small_class). cells() restates that split from
those files; it shares no code with kernel_model.py.

message_lattice() is one log region of clean PUT messages stored back to back from offset 0: probes, each with one
probed record (its user-metadata or its blob record) whose CRC span has a wanted residue and length, and before
each probe a spacer, a clean PUT whose user-metadata size (0..63) moves the probe's record onto that residue.
flipped() is the same region with one bit flipped inside every probed span. chunk_lattice() is the same idea for
the batch engine: (off, len) pairs over one buffer. Every user-metadata, blob and buffer byte is nonzero, so a
byte that a mask wrongly drops or keeps changes the CRC."""
import functools
import struct
import zlib
from types import SimpleNamespace

import numpy as np

from msgfmt import MF

RUN = 64                 # region_crc.h: the run grid
LONG_RUNS = 512          # region_crc.h kLongRuns: more runs than this go to the whole wave / the grid
LONG_PIECE = 64 << 10    # crc32_kernels.h kLongPiece
CLASS_CUTS = (256, 1024, 4096, 16384)  # crc32_kernels.hip small_class; kGroupSmallMax = 16384

SHORT_U = range(0, 321)  # user-metadata sizes of the short probes: spans of 6 + u bytes
HORNER_N = (16, 17, 18, 19, 20, 21, 32, 33, 34, 35, 36, 37)
HORNER_LO = (0, 1, 61, 62, 63)
END_RES = (0, 1, 63)
CUT_LENGTHS = tuple(c + k for c in CLASS_CUTS for k in (-1, 0, 1, 2))  # 255..258, ..., 16383..16386
THRESHOLD_N = (511, 512, 513)
THRESHOLD_LO = (0, 1, 63)
PIECE_K = (1, 2, 64)
PIECE_LO = (0, 1, 63)

USERMETA_HEAD = 6        # UserMetadata_Format_V1: version, int size; the span is 6 + u bytes
BLOB_HEAD = 13           # Blob_Format_V3: version, type, isCompressed, long size; the span is 13 + c bytes


def cells(pa: int, length: int):
    """The kernels' case split for the CRC span [pa, pa + length), pa relative to a 64-aligned base.

    record_crc / record_crc_runs_wave (region_crc.h): A0 = pa rounded down, B1 = pb rounded up to 64 B; lo = pa - A0,
    n = (B1 - A0) / 64 runs; tin = record bytes in the head run (under 4: the initial register is split across
    the run end); tail_bytes = the last run is taken from the bytes (n >= 2 and pb off the grid); ng = ceil(n / 4)
    run groups, rb = n - 4 ng (-3..0) the first group's padding, prefetch = ng > 4 (the next 16 sums are loaded
    inside the loop); d = B1 - pb the un-shift; bytewise = length < 4 (no runs at all).
    record_crc_direct (region_proc.h): sh = pb & 15 the funnel shift, R = ceil(length / 64) runs aligned to the
    record's end, V = ceil(R / 64) rounds.
    long = n > 512: the whole wave (record_crc_runs_wave), or region_long_kernel's pieces = ceil(length / 64 KiB),
    the last of last_piece bytes, folded in rounds = ceil((pieces - 1) / 64) rounds of 64 full pieces.
    cls: the group phase's size class (None: empty, or above 16 KiB and left to the sweep)."""
    pb = pa + length
    a0, b1 = pa & ~63, (pb + 63) & ~63
    n = (b1 - a0) >> 6
    lo = pa - a0
    hi = min(pb - a0, 64)
    ng = (n + 3) >> 2
    r = (length + 63) >> 6
    pieces = -(-length // LONG_PIECE)
    if length == 0 or length > CLASS_CUTS[-1]:
        cls = None
    else:
        cls = sum(1 for c in CLASS_CUTS[:-1] if length > c)
    return SimpleNamespace(
        pa=pa, length=length, lo=lo, n=n, tin=hi - lo, tail_bytes=n >= 2 and (pb & 63) != 0, ng=ng, rb=n - 4 * ng,
        prefetch=ng > 4, d=b1 - pb, bytewise=length < 4, sh=pb & 15, R=r, V=(r + 63) >> 6, long=n > LONG_RUNS,
        pieces=pieces, last_piece=length - (pieces - 1) * LONG_PIECE if pieces else 0,
        rounds=(max(pieces, 1) - 1 + 63) // 64, cls=cls)


def nonzero_bytes(seed: int, n: int) -> bytes:
    """n bytes in 1..255, different for different seeds."""
    if n == 0:
        return b""
    return np.random.default_rng(seed).integers(1, 256, size=n, dtype=np.uint8).tobytes()


def span_length(lo: int, n: int, end_res: int) -> int:
    """The length of the span that starts at residue lo, covers n runs and ends at residue end_res (0: on the
    run grid)."""
    return 64 * (n - 1) + (end_res or 64) - lo


def probe_specs():
    """(kind, record, lo, span length) of every probe, in region order. record: 3 user metadata, 4 blob (the
    header's slot numbers)."""
    specs = [("short", 3, lo, USERMETA_HEAD + u) for lo in range(64) for u in SHORT_U]
    specs += [("horner", 4, lo, span_length(lo, n, e)) for n in HORNER_N for lo in HORNER_LO for e in END_RES]
    specs += [("cut", 4, lo, ln) for ln in CUT_LENGTHS for lo in range(64)]
    specs += [("threshold", 4, lo, span_length(lo, n, e)) for n in THRESHOLD_N for lo in THRESHOLD_LO for e in END_RES]
    specs += [("pieces", 4, lo, LONG_PIECE * k + dk) for k in PIECE_K for dk in (-1, 0, 1) for lo in PIECE_LO]
    return specs


KEY_DIGITS = 7


def _message(i: int, usermeta: bytes, content: bytes) -> bytes:
    """A clean PUT the transform's fast path accepts: header V3, canonical VERSION_5 ASCII properties, a
    Blob_Format_V3 record. Everything before the user-metadata record has the same length in every message."""
    return MF.put_message(MF.store_key("g%0*d" % (KEY_DIGITS, i)), MF.blob_properties_bytes(len(content)), usermeta,
                          content, version=3, life=i % 3)


@functools.lru_cache(maxsize=None)
def message_lattice():
    """region (bytes), offs (int64[m]), probe (bool[m]), and per message the probed span: rec_pa (its offset in
    the region), rec_len, rec_bit (its status bit), kind; zeros and "spacer" for the spacers. Messages alternate
    spacer, probe from offset 0; the region starts 64-aligned in cells()' terms (a test that shifts it adds the
    shift to rec_pa)."""
    pre = len(_message(0, b"", b"x")) - len(MF.usermeta_record(b"")) - len(MF.blob_record(b"x"))  # to the um record
    spacer_fixed = pre + len(MF.usermeta_record(b"")) + len(MF.blob_record(b"x"))
    parts, offs, probe, rec_pa, rec_len, rec_bit, kind = [], [], [], [], [], [], []
    pos = 0

    def put(msg, is_probe, pa, ln, bit, what):
        nonlocal pos
        offs.append(pos)
        probe.append(is_probe)
        rec_pa.append(pa)
        rec_len.append(ln)
        rec_bit.append(bit)
        kind.append(what)
        parts.append(msg)
        pos += len(msg)

    for j, (what, rec, lo, ln) in enumerate(probe_specs()):
        if rec == 3:
            um, content = nonzero_bytes(2 * j, ln - USERMETA_HEAD), nonzero_bytes(2 * j + 1, 1 + j % 5)
            rel = pre  # the span's start in its message
        else:
            um, content = nonzero_bytes(2 * j, 1 + j % 7), nonzero_bytes(2 * j + 1, ln - BLOB_HEAD)
            rel = pre + len(um) + 14
        # the spacer ends where the probe starts: its user-metadata size makes that start + rel = lo mod 64
        s = (lo - rel - pos - spacer_fixed) % 64
        put(_message(2 * j, nonzero_bytes(3 * j + 7, s), nonzero_bytes(3 * j + 8, 1)), False, 0, 0, 0, "spacer")
        msg = _message(2 * j + 1, um, content)
        put(msg, True, pos + rel, ln, MF.USERMETA_CRC if rec == 3 else MF.BLOB_CRC, what)
    region = b"".join(parts)
    return SimpleNamespace(region=region, offs=np.asarray(offs, dtype=np.int64), probe=np.asarray(probe),
                           rec_pa=np.asarray(rec_pa, dtype=np.int64), rec_len=np.asarray(rec_len, dtype=np.int64),
                           rec_bit=np.asarray(rec_bit, dtype=np.uint32), kind=kind)


def flip_position(j: int, pa: int, length: int) -> int:
    """Where probe j's span gets its flipped bit: by turns its first byte, its fourth and its fifth (either side
    of the initial register folded into the first four), the last byte of its head run and the first of its second
    run, the first byte of its tail run, its last byte and, for a span of several 64 KiB pieces, the last byte of
    one piece and the first byte of the next. A span too short for a position gets its last byte."""
    pb = pa + length
    pieces = -(-length // LONG_PIECE)
    choices = [pa, pa + 3, pa + 4, pa | 63, (pa | 63) + 1, max(pa, (pb - 1) & ~63), pb - 1]
    if pieces > 1:
        p = 1 + (j // 9) % (pieces - 1)  # the cut between pieces p - 1 and p
        choices += [pa + LONG_PIECE * p - 1, pa + LONG_PIECE * p]
    return min(choices[j % len(choices)], pb - 1)


@functools.lru_cache(maxsize=None)
def flipped():
    """message_lattice() with exactly one bit flipped in every probe's probed span (flip_position; the bit cycles
    too), the spacers untouched: the lattice's fields, with its region replaced, plus flip_at (the flipped byte's
    offset in the region, -1 for a spacer)."""
    lat = message_lattice()
    region = bytearray(lat.region)
    flip_at = np.full(len(lat.offs), -1, dtype=np.int64)
    for j, i in enumerate(np.nonzero(lat.probe)[0]):
        at = flip_position(j, int(lat.rec_pa[i]), int(lat.rec_len[i]))
        region[at] ^= 1 << (j % 8)
        flip_at[i] = at
    out = SimpleNamespace(**vars(lat))
    out.region = bytes(region)
    out.flip_at = flip_at
    return out


def field_bytes(bit: int) -> int:
    """Bytes at the start of a probed span that its deserializer reads as fields (a flip there may add
    BAD_VERSION or BAD_RECORD to the record's CRC bit)."""
    return USERMETA_HEAD if bit == MF.USERMETA_CRC else BLOB_HEAD


CRC_BITS = MF.HEADER_CRC | MF.ENCKEY_CRC | MF.PROPS_CRC | MF.UPDATE_CRC | MF.USERMETA_CRC | MF.BLOB_CRC


@functools.lru_cache(maxsize=None)
def verify_oracle(which: str):
    """(status uint32[m], msg_end int64[m]) of MF.verify_message over message_lattice() ("clean") or flipped()
    ("flipped"); the region is bytes already, so no call converts it."""
    lat = message_lattice() if which == "clean" else flipped()
    res = [MF.verify_message(lat.region, int(o)) for o in lat.offs]
    return np.array([s for s, _ in res], dtype=np.uint32), np.array([e for _, e in res], dtype=np.int64)


EDGE_SHIFTS = (0, 1, 15, 16, 63)


@functools.lru_cache(maxsize=None)
def edge_region():
    """A small back-to-back region for record_crc_direct's clamp at the region's first 16-B block (RegionArgs
    lo16): region, offs, status, end (the oracle's), and first_pa, first_len, the first message's first CRC span
    (its properties record). No record can start inside the region's first 16-B block -- a V3 header is 40 bytes
    and a key at least 2 -- but the direct form hashes 64-B runs aligned to a span's END, so the first span's
    first run starts before the region when the span's length is a little over a multiple of 64: here 43 bytes
    in and 67 long, it ends at byte 110 and its two runs start at byte -18 (low_load_below_region() for the exact
    condition on the 16-B loads). The last message ends at the region's last byte. No load of a well-formed
    message passes the last 16-B block (hi16): the highest is the block of pb, and pb is followed by the
    8-B stored CRC, so floor16(pb) <= floor16(region end - 1). Sizes step through every end residue of a 16-B
    block; every third message has a flipped bit in its blob span's last byte."""
    parts, offs, pos = [], [], 0
    for i in range(48):
        props = MF.blob_properties_bytes(1 + i % 17, content_type="x", owner_id="ow") if i == 0 else \
            MF.blob_properties_bytes(1 + i % 17)
        msg = bytearray(MF.put_message(MF.store_key("e" if i == 0 else "e%d" % i), props, nonzero_bytes(500 + i, i % 23),
                                       nonzero_bytes(600 + i, 1 + i % 17), version=3))
        if i % 3 == 2:
            msg[-9] ^= 1 << (i % 8)
        offs.append(pos)
        parts.append(bytes(msg))
        pos += len(msg)
    region = b"".join(parts)
    res = [MF.verify_message(region, o) for o in offs]
    _, _, rel = MF.parse_header(region, 0)
    return SimpleNamespace(region=region, offs=np.asarray(offs, dtype=np.int64),
                           status=np.array([s for s, _ in res], dtype=np.uint32),
                           end=np.array([e for _, e in res], dtype=np.int64),
                           first_pa=rel[1], first_len=rel[3] - 8 - rel[1])


def low_load_below_region(shift: int, pa: int, length: int) -> bool:
    """record_crc_direct's lowest 16-B load for the span [pa, pa + length) of a region placed `shift` bytes past
    a run boundary: block 0 of run 0, at floor16(pb) - 64 R from the base. True when that is below lo16, the
    first 16-B block holding region bytes, so the clamp moves it."""
    reg0 = shift % 64
    c = cells(reg0 + pa, length)
    return ((reg0 + pa + length) & ~15) - 64 * c.R < (reg0 & ~15)


CHUNK_BUFFER = 256 << 10


@functools.lru_cache(maxsize=None)
def chunk_lattice():
    """mem (uint8[CHUNK_BUFFER], nonzero), off, length (int64[n]), crc_in (uint32[n], one third 0): every
    off mod 64 for every length 0..320, and the class-cut lengths at every residue. The chunks overlap in one
    small buffer; each starts at its residue from a 64-aligned place that moves with its index."""
    mem = np.frombuffer(nonzero_bytes(99, CHUNK_BUFFER), dtype=np.uint8)
    pairs = [(r, ln) for r in range(64) for ln in range(0, 321)] + [(r, ln) for ln in CUT_LENGTHS for r in range(64)]
    slots = (CHUNK_BUFFER - CUT_LENGTHS[-1] - 64) // 64
    off = np.array([64 * ((i * 977) % slots) + r for i, (r, _) in enumerate(pairs)], dtype=np.int64)
    length = np.array([ln for _, ln in pairs], dtype=np.int64)
    crc_in = np.random.default_rng(7).integers(0, 1 << 32, size=len(pairs), dtype=np.uint64).astype(np.uint32)
    crc_in[::3] = 0
    assert int((off + length).max()) <= CHUNK_BUFFER
    return SimpleNamespace(mem=mem, off=off, length=length, crc_in=crc_in)


def chunk_crcs(lat, seeded: bool = True) -> np.ndarray:
    """zlib's CRC of every chunk, continued from crc_in when seeded."""
    mem = lat.mem.tobytes()
    return np.array([zlib.crc32(mem[o:o + n], int(c) if seeded else 0)
                     for o, n, c in zip(lat.off.tolist(), lat.length.tolist(), lat.crc_in.tolist())], dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def trailed_lattice():
    """The chunk lattice as CRC-trailered items: every chunk followed by the big-endian long of its CRC, packed
    into one buffer with padding that keeps each chunk's residue. Every seventh trailer has one flipped bit, by
    turns in its high word (always a mismatch: a CRC-32 has no upper bits) and in its low word.
    mem (uint8), off, length (int64[n], trailer included), bad (bool[n])."""
    lat = chunk_lattice()
    src = lat.mem.tobytes()
    crcs = chunk_crcs(lat, seeded=False)
    out, offs = bytearray(), []
    bad = np.zeros(len(lat.off), dtype=bool)
    for i, (o, n) in enumerate(zip(lat.off.tolist(), lat.length.tolist())):
        out += nonzero_bytes(i, (o - len(out)) % 64)
        offs.append(len(out))
        trailer = bytearray(struct.pack(">q", int(crcs[i])))
        if i % 7 == 0:
            bad[i] = True
            word = 0 if (i // 7) % 2 == 0 else 4
            trailer[word + (i // 14) % 4] ^= 1 << (i % 8)
        out += src[o:o + n] + trailer
    return SimpleNamespace(mem=np.frombuffer(bytes(out), dtype=np.uint8), off=np.asarray(offs, dtype=np.int64),
                           length=lat.length + 8, bad=bad)
