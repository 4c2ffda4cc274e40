"""An independent model of how the host-staged GPU legs (ambrycrc_host.cpp: batch, message verify,
transform) cut host memory into staging slabs, and the case tables that place those cuts on purpose.

The model is written from the rules ambrycrc_host.cpp states, not from its loops, and takes the four
geometry numbers as arguments (Geometry). HEADER_GEOMETRY is what ambrycrc_ctx.h states; the tables
are built for it, test_host_slab_model.py pins it against the header's text, and the GPU tests compare
the library's own report (ambrycrc_last_host_slabs) with both.

The rules:

* Batch leg. A slab holds at most slab_bytes bytes and slab_chunks pieces. Every piece starts at a
  multiple of 16 in its slab. A chunk that does not fit the room left is cut there and goes on at the
  start of the next slab; its pieces are combined in order. A slab is closed once its pieces and
  their padding reach slab_bytes or it holds slab_chunks pieces; a zero-length chunk is a piece of no
  bytes in whatever slab is open.
* Verify leg. Messages go in offset order (a stable sort), offsets clamped to the region's end. A slab
  stages one span [lo, hi) that covers the extent of every message it holds: at most slab_bytes
  bytes, at most slab_msgs messages. A message whose own extent exceeds slab_bytes takes the oversize
  path alone and ends the slab before it.
* Transform leg. Runs of consecutive messages in index order; a run's span [lo, hi) is the hull of
  its messages' extents (a later message at a lower offset pulls lo down). A run ends where the span
  would pass slab_bytes, where it holds slab_msgs messages, or where the summed extents + GROWTH per
  message would pass xform_out_bytes (a run always takes its first message); an oversize message goes
  alone between two runs.
* extent: the header window of min(rem, 40) bytes, or first record offset + total size when the
  header's sizes fit the bytes that remain.

Every case names its family (the cut it aims at) and the side of the cut it is on, and states what
the plan must be (`expect`); check_plan holds a model plan against that.
"""
from __future__ import annotations

import contextlib
import functools
import struct
import zlib
from typing import NamedTuple

import numpy as np

from datagen import stream_bytes
from msgfmt import MF

GROWTH = 26  # AMBRYCRC_TRANSFORM_GROWTH_MAX
MSG_NO_ROOM = 1 << 12


class Geometry(NamedTuple):
    slab_bytes: int
    slab_chunks: int
    slab_msgs: int
    xform_out_bytes: int


HEADER_GEOMETRY = Geometry(64 << 20, 1 << 14, 1 << 16, (64 << 20) + GROWTH * (1 << 16))
S = HEADER_GEOMETRY.slab_bytes
C = HEADER_GEOMETRY.slab_chunks
M = HEADER_GEOMETRY.slab_msgs
X = HEADER_GEOMETRY.xform_out_bytes


# ------------------------------------------------------------------ the model
def plan_batch(lens, geo: Geometry):
    """Per slab, the list of (chunk, piece length, offset in slab)."""
    assert geo.slab_bytes % 16 == 0
    slabs, used = [], 0
    for chunk, n in enumerate(lens):
        left = n
        while True:
            if not slabs or used >= geo.slab_bytes or len(slabs[-1]) == geo.slab_chunks:
                slabs.append([])
                used = 0
            piece = min(left, geo.slab_bytes - used)
            slabs[-1].append((chunk, piece, used))
            used += -(-piece // 16) * 16
            left -= piece
            if not left:
                break
    return slabs


def plan_verify(offs, exts, region_len, geo: Geometry):
    """(slabs, oversize): slabs as dicts of lo, hi and members (message indices, in staging order);
    oversize the indices that take the oversize path."""
    slabs, oversize, open_slab = [], [], None
    for i in sorted(range(len(offs)), key=lambda j: offs[j]):
        if exts[i] > geo.slab_bytes:
            oversize.append(i)
            open_slab = None
            continue
        o = min(offs[i], region_len)
        e = o + exts[i]
        if open_slab is None or len(open_slab["members"]) == geo.slab_msgs or \
                max(open_slab["hi"], e) - open_slab["lo"] > geo.slab_bytes:
            open_slab = {"lo": o, "hi": o, "members": []}
            slabs.append(open_slab)
        open_slab["hi"] = max(open_slab["hi"], e)
        open_slab["members"].append(i)
    return slabs, oversize


def plan_transform(offs, exts, region_len, geo: Geometry, growth: int = GROWTH):
    """(runs, oversize): runs as dicts of i0, n, lo, hi and outs (the summed output bound)."""
    runs, oversize, run = [], [], None
    for i in range(len(offs)):
        if exts[i] > geo.slab_bytes:
            oversize.append(i)
            run = None
            continue
        o = min(offs[i], region_len)
        e = o + exts[i]
        if run is not None:
            lo, hi, outs = min(run["lo"], o), max(run["hi"], e), run["outs"] + exts[i] + growth
            if run["n"] == geo.slab_msgs or hi - lo > geo.slab_bytes or outs > geo.xform_out_bytes:
                run = None
        if run is None:
            run = {"i0": i, "n": 0, "lo": o, "hi": e, "outs": 0}
            runs.append(run)
            lo, hi, outs = o, e, exts[i] + growth
        run.update(n=run["n"] + 1, lo=lo, hi=hi, outs=outs)
    return runs, oversize


def extent(region, off: int) -> int:
    """Bytes from `off` that a verify or transform of the message there may read (0 past the end)."""
    n = len(region)
    if off > n:
        return 0
    rem = n - off
    window = min(rem, 40)
    if rem < 2:
        return rem
    v = struct.unpack_from(">h", region, off)[0]
    h = MF.HEADER_SIZE.get(v, 0)
    if not h or rem < h:
        return window
    _, total, rel = MF.parse_header(region, off)
    first = next((r for r in rel if r != MF.INVALID), -1)
    if total <= 0 or first < 0 or total > rem or first > rem - total:
        return window
    return max(window, first + total)


def extents(region, offs):
    """extent() of every offset, each distinct one read once."""
    seen = {o: extent(region, o) for o in set(offs)}
    return [seen[o] for o in offs]


def check_plan(case, geo: Geometry):
    """The model's plan of `case` under `geo` is what the case states (so the cut it names happens, on
    the side it names), and no slab exceeds the geometry. Returns (slabs or runs, oversize) counts."""
    want = case["expect"]
    if case["leg"] == "batch":
        slabs = plan_batch(case["lens"], geo)
        got = {}
        for w, pieces in enumerate(slabs):
            assert len(pieces) <= geo.slab_chunks
            for chunk, n, at in pieces:
                assert at % 16 == 0 and at + n <= geo.slab_bytes, (case["name"], w, chunk)
                got.setdefault(chunk, []).append((w, at, n))
        for chunk, n in enumerate(case["lens"]):
            assert sum(p[2] for p in got[chunk]) == n, (case["name"], chunk)
            assert [p[0] for p in got[chunk]] == sorted(p[0] for p in got[chunk])
        assert len(slabs) == want["slabs"], (case["name"], len(slabs))
        for chunk, pieces in want["pieces"].items():
            assert got[chunk] == pieces, (case["name"], chunk, got[chunk])
        return len(slabs), 0
    with region_for(case) as region:
        exts = extents(region, case["offs"])
    if case["leg"] == "verify":
        slabs, oversize = plan_verify(case["offs"], exts, case["region_len"], geo)
        for s in slabs:
            assert s["hi"] - s["lo"] <= geo.slab_bytes and 0 < len(s["members"]) <= geo.slab_msgs
        assert [s["hi"] - s["lo"] for s in slabs] == want["spans"], (case["name"], [s["hi"] - s["lo"] for s in slabs])
        if "members" in want:
            assert [len(s["members"]) for s in slabs] == want["members"], case["name"]
        assert sorted(oversize) == want["oversize"], case["name"]
        return len(slabs), len(oversize)
    runs, oversize = plan_transform(case["offs"], exts, case["region_len"], geo)
    for r in runs:
        assert r["hi"] - r["lo"] <= geo.slab_bytes and 0 < r["n"] <= geo.slab_msgs
        assert r["n"] == 1 or r["outs"] <= geo.xform_out_bytes
    assert [(r["i0"], r["n"], r["hi"] - r["lo"]) for r in runs] == want["runs"], \
        (case["name"], [(r["i0"], r["n"], r["hi"] - r["lo"]) for r in runs])
    assert oversize == want["oversize"], case["name"]
    return len(runs), len(oversize)


# ------------------------------------------------------------------ batch leg: data and tables
DATA_BYTES = 3 * S + (64 << 10)
ALIGNMENTS = (0, 5)


@functools.lru_cache(maxsize=None)
def batch_data() -> np.ndarray:
    """Seeded bytes the batch cases' chunks point into: DATA_BYTES at each base alignment."""
    return stream_bytes(0x51AB, 0, DATA_BYTES + 16)


class CrcRef:
    """zlib CRCs of ranges of one buffer; a range that starts where an earlier one did (the filler,
    the long chunks) is hashed once and extended."""

    def __init__(self, data):
        self.data = data
        self.seen = {}

    def crc(self, off: int, n: int, crc_in: int = 0) -> int:
        best, acc = 0, crc_in
        for (o, c, length), v in self.seen.items():
            if o == off and c == crc_in and best < length <= n:
                best, acc = length, v
        out = zlib.crc32(self.data[off + best:off + n], acc) if n > best else acc
        if n >= (1 << 20):
            self.seen[(off, crc_in, n)] = out
        return out


FILL = S - 4096     # the filler chunk
ADJ_AT = FILL + 7   # where the adjuster chunk's bytes lie in the buffer
PROBE_AT = S + 4097


def _batch_case(name, family, side, chunks, slabs, pieces, crc_in=None, pinned=False, entry="batch", **more):
    return dict(more, leg="batch", entry=entry, name=name, family=family, side=side, chunks=chunks,
                lens=[n for _, n in chunks], crc_in=crc_in, pinned=pinned,
                expect={"slabs": slabs, "pieces": pieces})


def _end_of_slab_cases():
    """Filler + adjuster bring `used` to S - r; with an adjuster of 1..15 mod 16 bytes only the padding
    does. The probe chunk then lies inside the slab, ends on the cut, is split by it (first piece r
    bytes, second 1, 15, 16 or 17) or starts the next slab."""
    out = []
    for r in (0, 16, 32):
        for k in (0, 1, 15):
            adj = 4096 - r - k
            probes = sorted(x for x in {0, 1, 15, 16, 17, r - 1, r, r + 1, r + 15, r + 16, r + 17} if x >= 0)
            for n in probes:
                if r == 0:
                    side, slabs, pieces = "next", 2, [(1, 0, n)]
                elif n <= r:
                    side, slabs, pieces = ("on_cut" if n == r else "inside"), 1, [(0, S - r, n)]
                else:
                    side, slabs, pieces = "split", 2, [(0, S - r, r), (1, 0, n - r)]
                out.append(_batch_case(f"end_r{r}_adj{adj % 16}_probe{n}", "end_of_slab", side,
                                       [(0, FILL), (ADJ_AT, adj), (PROBE_AT, n)], slabs,
                                       {0: [(0, 0, FILL)], 1: [(0, FILL, adj)], 2: pieces}, pinned=True))
    return out


def _other_batch_cases():
    ones = [(3 + 7 * i, 1) for i in range(C - 1)]  # C - 1 one-byte chunks: pieces at 16 * i
    full = 16 * (C - 1)
    c = _batch_case
    return [
        # long chunks, each continuing a running CRC
        c("long_S", "long_chunk", "at", [(3, S)], 1, {0: [(0, 0, S)]}, crc_in=[0xDEADBEEF], pinned=True),
        c("long_2S", "long_chunk", "at_twice", [(3, 2 * S)], 2, {0: [(0, 0, S), (1, 0, S)]}, crc_in=[0x00C0FFEE],
          pinned=True),
        c("long_2S_17", "long_chunk", "over", [(3, 2 * S + 17)], 3, {0: [(0, 0, S), (1, 0, S), (2, 0, 17)]},
          crc_in=[0xDEADBEEF], pinned=True),
        c("long_2S_17_shifted", "long_chunk", "shifted", [(1, 5), (3, 2 * S + 17)], 3,
          {0: [(0, 0, 5)], 1: [(0, 16, S - 16), (1, 0, S), (2, 0, 33)]}, crc_in=[0x12345678, 0x9ABCDEF0], pinned=True),
        # a chunk that ends exactly at S, then a zero-length chunk and a one-byte chunk
        c("exact_end", "after_exact_end", "exact", [(0, S), (100, 0), (200, 1)], 2,
          {0: [(0, 0, S)], 1: [(1, 0, 0)], 2: [(1, 0, 1)]}),
        c("padded_end", "after_exact_end", "padded", [(0, S - 16), (50, 1), (100, 0), (200, 1)], 2,
          {1: [(0, S - 16, 1)], 2: [(1, 0, 0)], 3: [(1, 0, 1)]}),
        c("short_of_end", "after_exact_end", "under", [(0, S - 16), (100, 0), (200, 1)], 1,
          {1: [(0, S - 16, 0)], 2: [(0, S - 16, 1)]}),
        # zero-length chunks as the last piece of a slab and as the first piece of the next
        c("zero_last_and_first", "zero_length", "last_and_first", ones + [(9, 0), (9, 0), (11, 5)], 2,
          {C - 1: [(0, full, 0)], C: [(1, 0, 0)], C + 1: [(1, 0, 5)]}, crc_in=list(range(1, C + 3))),
        c("zero_last_of_batch", "zero_length", "last_of_batch", [(0, 100), (0, 0)], 1, {1: [(0, 112, 0)]},
          crc_in=[7, 0xFFFFFFFF]),
        # only zero-length chunks (one with no address at all): one slab of no bytes, out == crc_in
        c("all_zero", "all_zero", "only", [(0, 0), (17, 0), (None, 0), (5, 0), (DATA_BYTES, 0)], 1,
          {i: [(0, 0, 0)] for i in range(5)}, crc_in=[0, 1, 0xFFFFFFFF, 0x80000000, 0x1234ABCD]),
        # the count cut and the byte cut in the same piece, and the count cut alone
        c("count_and_bytes", "count_and_bytes", "both", ones + [(1, S + 1)], 2,
          {C - 1: [(0, full, S - full), (1, 0, full + 1)]}),
        c("count_at", "count", "at", ones + [(1, 1)], 1, {C - 1: [(0, full, 1)]}),
        c("count_over", "count", "over", ones + [(1, 1), (2, 1)], 2, {C - 1: [(0, full, 1)], C: [(1, 0, 1)]}),
    ]


def _trailed_cases():
    """ambrycrc_verify_trailed_host: item = body + 8-byte trailer, the body goes through the batch leg.
    A good item, a short one (under 8 bytes: no body), the big body that ends at S - r, then two
    items of 100-byte bodies, the first of which the cut splits (r > 0), starts the next slab
    (r = 0) or leaves whole (r = 128)."""
    out = []
    area = S + 8192
    for r in (0, 16, 32, 128):
        for variant, kinds in (("wrong_after", ("good", "good", "wrong")), ("wrong_on_cut", ("good", "wrong", "good")),
                               ("wrong_big", ("wrong", "good", "good"))):
            items = [(area, 100, "good"), (area + 512, 5, "short"), (0, S - r - 112, kinds[0]),
                     (area + 1024, 100, kinds[1]), (area + 1536, 100, kinds[2])]
            if r == 0:
                side, x = "next", [(1, 0, 100)]
            elif r >= 100:
                side, x = "inside", [(0, S - r, 100)]
            else:
                side, x = "split", [(0, S - r, r), (1, 0, 100 - r)]
            chunks = [(o, 0 if kind == "short" else n) for o, n, kind in items]
            out.append(_batch_case(f"trailed_r{r}_{variant}", "trailed", side, chunks, 2,
                                   {0: [(0, 0, 100)], 1: [(0, 112, 0)], 2: [(0, 112, S - r - 112)], 3: x},
                                   entry="trailed", items=items, pinned=(variant == "wrong_on_cut")))
    return out


def _range_cases():
    """ambrycrc_range_checksums_host: [first, second) ranges of a file of file_len bytes, clipped at
    its end, through the batch leg in the order given."""
    flen = S + 4099

    def case(name, side, ranges, slabs, pieces):
        clip = [(min(a, flen), min(b, flen)) for a, b in ranges]
        return _batch_case(name, "ranges", side, [(a, b - a) for a, b in clip], slabs, pieces, entry="ranges",
                           ranges=ranges, file_len=flen)
    return [
        case("ranges_split", "split", [(0, S - 32), (S - 1, S + 1), (S - 8, S + 24), (flen - 10, flen + 100),
                                       (flen, flen + 5), (flen + 7, flen + 9), (5, 6)], 2,
             {1: [(0, S - 32, 2)], 2: [(0, S - 16, 16), (1, 0, 16)], 3: [(1, 16, 10)], 4: [(1, 32, 0)], 5: [(1, 32, 0)],
              6: [(1, 32, 1)]}),
        case("ranges_next", "next", [(0, S), (S - 1, S + 1), (flen - 3, flen + 3)], 2,
             {0: [(0, 0, S)], 1: [(1, 0, 2)], 2: [(1, 16, 3)]}),
        case("ranges_padded", "padded", [(1, S - 1), (S - 1, S + 1)], 2, {0: [(0, 0, S - 2)], 1: [(1, 0, 2)]}),
        case("ranges_clipped_long", "clipped_long", [(0, flen + 1000)], 2, {0: [(0, 0, S), (1, 0, 4099)]}),
    ]


@functools.lru_cache(maxsize=None)
def batch_cases():
    return _end_of_slab_cases() + _other_batch_cases() + _trailed_cases() + _range_cases()


# the sides every family must have a case on
BATCH_SIDES = {
    "end_of_slab": {"inside", "on_cut", "split", "next"}, "long_chunk": {"at", "at_twice", "over", "shifted"},
    "after_exact_end": {"exact", "padded", "under"}, "zero_length": {"last_and_first", "last_of_batch"},
    "all_zero": {"only"}, "count_and_bytes": {"both"}, "count": {"at", "over"},
    "trailed": {"inside", "split", "next"}, "ranges": {"split", "next", "padded", "clipped_long"},
}


# ------------------------------------------------------------------ message legs: data and tables
REGION_BYTES = S + (1 << 20)
JUNK = 0xA5


@functools.lru_cache(maxsize=None)
def _region_buffer() -> np.ndarray:
    return np.full(REGION_BYTES, JUNK, dtype=np.uint8)


@contextlib.contextmanager
def region_for(case):
    """The case's region: junk with the case's messages patched in (and taken out again afterwards)."""
    buf = _region_buffer()
    spans = []
    try:
        for off, msg in case["patches"]:
            buf[off:off + len(msg)] = np.frombuffer(msg, dtype=np.uint8)
            spans.append((off, len(msg)))
        for pos in case.get("flips", ()):
            buf[pos] ^= 1
        yield buf[:case["region_len"]]
    finally:
        for off, n in spans:
            buf[off:off + n] = JUNK


def _put(name, blob, version=3, **kw):
    content = stream_bytes(0xB10B, 0, blob).tobytes() if isinstance(blob, int) else blob
    return MF.put_message(MF.store_key(name), MF.blob_properties_bytes(len(content)), b"um-" + name.encode(), content,
                          version=version, **kw)


@functools.lru_cache(maxsize=None)
def small():
    """The small messages the cases place: PUTs of the three header versions, an update, a PUT whose
    extent is above 1 KiB, and a header that claims 1 GiB of records."""
    m = {
        "p0": _put("p0", 100, enc_key=b"k" * 32, life=2),
        "p1": _put("p1", 300, version=2),
        "p2": _put("p2", 57, version=1),
        "p3": _put("p3", 1, compressed=True),
        "u0": MF.update_message(MF.store_key("u0")),
        "k1": _put("k1", 1000),
        "claim": MF.header(3, 1 << 30, MF.INVALID, 50, MF.INVALID, 90, 120, 1),
    }
    assert len(m["k1"]) > 1024 > max(len(m[k]) for k in ("p0", "p1", "p2", "p3", "u0")) and len(m["claim"]) == 40
    return m


@functools.lru_cache(maxsize=None)
def big(total: int) -> bytes:
    """A clean V3 PUT of exactly `total` bytes (the blob record is its last)."""
    content = stream_bytes(0xB16, 0, total)
    n = total - len(_put("big", b""))
    msg = _put("big", content[:n].tobytes())
    assert len(msg) == total
    return msg


def _msg_case(leg, name, family, side, region_len, patches, offs, expect, **more):
    assert region_len <= REGION_BYTES
    return dict(more, leg=leg, name=name, family=family, side=side, region_len=region_len, patches=patches,
                offs=offs, expect=expect)


def _side(d):
    return "under" if d < 0 else "at" if d == 0 else "over"


@functools.lru_cache(maxsize=None)
def verify_cases():
    sm = small()
    out = []
    for lo in (0, 4099):
        # A at lo, B ends at lo + S + d
        for order in ("sorted", "reversed", "dups"):
            a, b = (sm["p0"], sm["p1"]) if order != "reversed" else (sm["u0"], sm["p2"])
            for d in range(-2, 3):
                bo = lo + S + d - len(b)
                offs = {"sorted": [lo, bo], "reversed": [bo, lo], "dups": [bo, lo, lo, bo, bo]}[order]
                exp = {"spans": [S + d], "members": [len(offs)]} if d <= 0 else \
                    {"spans": [len(a), len(b)], "members": [offs.count(lo), offs.count(bo)]}
                out.append(_msg_case("verify", f"span_lo{lo}_{order}_d{d}", "end_of_span", _side(d), lo + S + d + 977,
                                     [(lo, a), (bo, b)], offs, dict(exp, oversize=[])))
        # d = 0 and the region ends with B: one offset equal to region_len, one beyond, in the same slab
        bo = lo + S - len(sm["p3"])
        out.append(_msg_case("verify", f"span_lo{lo}_past_end_slots", "end_of_span", "at", lo + S,
                             [(lo, sm["u0"]), (bo, sm["p3"])], [bo, lo + S, lo, lo + S + 7],
                             {"spans": [S], "members": [4], "oversize": []}))
        # B is a header that claims more than the region holds: its extent is the 40-byte window
        for d in (-1, 0, 1):
            bo = lo + S + d - 40
            exp = {"spans": [S + d]} if d <= 0 else {"spans": [len(sm["p1"]), 40]}
            out.append(_msg_case("verify", f"claim_lo{lo}_d{d}", "truncated_header", _side(d), lo + S + d + 500,
                                 [(lo, sm["p1"]), (bo, sm["claim"])], [lo, bo], dict(exp, oversize=[])))
    # B starts t < 40 bytes before the region's end, which is at lo + S + d
    lo = 4099
    for t, key in ((1, "p0"), (2, "p0"), (33, "p0"), (39, "p0"), (39, "p2")):
        for d in (0, 1):
            end = lo + S + d
            exp = {"spans": [S]} if d == 0 else {"spans": [len(sm["p1"]), t]}
            out.append(_msg_case("verify", f"tail_{key}_t{t}_d{d}", "region_tail", _side(d), end,
                                 [(lo, sm["p1"]), (end - t, sm[key][:t])], [end - t, lo], dict(exp, oversize=[])))
    # the largest message that fits a slab (extent S) and the smallest that does not (S + 1),
    # between small messages, listed out of order; clean, and with a bit of the last blob byte flipped
    for total, side in ((S, "at"), (S + 1, "over")):
        for flip in (False, True):
            m = big(total)
            at = 4099
            p1 = at + total + 5
            u0 = p1 + len(sm["p1"]) + 3
            tail = u0 + len(sm["u0"]) - p1
            exp = {"spans": [len(sm["p0"]), S, tail], "oversize": []} if total == S else \
                {"spans": [len(sm["p0"]), tail], "oversize": [1]}
            out.append(_msg_case("verify", f"largest_{side}{'_flipped' if flip else ''}", "largest_message", side,
                                 u0 + len(sm["u0"]) + 11, [(61, sm["p0"]), (at, m), (p1, sm["p1"]), (u0, sm["u0"])],
                                 [p1, at, u0, 61], exp, flips=[at + total - 9] if flip else []))
    # every offset at or past the region's end: one slab of span 0
    out.append(_msg_case("verify", "past_end_only", "past_end_only", "only", 1000, [(100, sm["p0"])],
                         [1000, 1001, 10 ** 15], {"spans": [0], "members": [3], "oversize": []}))
    # the message count cuts: slab_msgs copies of one offset, and one more
    for n, side in ((M, "at"), (M + 1, "over")):
        out.append(_msg_case("verify", f"count_{side}", "count", side, 3 + len(sm["p0"]) + 10, [(3, sm["p0"])], [3] * n,
                             {"spans": [len(sm["p0"])] * (1 if n == M else 2), "members": [M] if n == M else [M, 1],
                              "oversize": []}))
    return out


VERIFY_SIDES = {"end_of_span": {"under", "at", "over"}, "truncated_header": {"under", "at", "over"},
                "region_tail": {"at", "over"}, "largest_message": {"at", "over"}, "past_end_only": {"only"},
                "count": {"at", "over"}}


def _lives(n):
    """A life version of its own for every message (distinct below 251 messages)."""
    return [(3 + i) % 251 for i in range(n)]


def _xform_case(*a, **kw):
    case = _msg_case("transform", *a, **kw)
    case.setdefault("lives", _lives(len(case["offs"])))
    case.setdefault("out_cap", None)
    return case


def transformed_len(msg: bytes, life: int) -> int:
    st, out = MF.transform_message(msg, 0, life=life, version=3)
    return len(out) if st == 0 else 0


@functools.lru_cache(maxsize=None)
def transform_cases():
    sm = small()
    out = []
    a, b, c = sm["p0"], sm["p1"], sm["p2"]
    for lo in (0, 4099):
        for d in range(-2, 3):
            end = lo + S + d
            bo = end - len(b)
            co = bo - len(c) - 9
            near = end - co
            patches = [(lo, a), (bo, b), (co, c)]
            # the end of a run in index order: A at lo, B ends at lo + S + d, C next to B
            out.append(_xform_case(f"run_lo{lo}_d{d}", "end_of_run", _side(d), end + 977, patches, [lo, bo, co],
                                   {"runs": [(0, 3, S + d)] if d <= 0 else [(0, 1, len(a)), (1, 2, near)], "oversize": []}))
            # the mirror: B and C first, then A at a lower offset pulls lo down
            out.append(_xform_case(f"lower_lo{lo}_d{d}", "lower_offset", _side(d), end + 977, patches, [bo, co, lo],
                                   {"runs": [(0, 3, S + d)] if d <= 0 else [(0, 2, near), (2, 1, len(a))], "oversize": []}))
    # a capacity that runs out across two runs: run 1 = p0, u0 (refused: it adds nothing), p1; run 2 = p3, p2
    lo = 4099
    names = ["p0", "u0", "p1", "p3", "p2"]
    offs = [lo, lo + 400, lo + 600, lo + S + 5000, lo + S + 5400]
    patches = [(o, sm[k]) for o, k in zip(offs, names)]
    lens = [transformed_len(sm[k], life) for k, life in zip(names, _lives(5))]
    assert lens[1] == 0 and all(lens[i] for i in (0, 2, 3, 4))
    run1 = offs[2] + len(sm["p1"]) - lo
    run2 = offs[4] + len(sm["p2"]) - offs[3]
    sum3, sum4 = sum(lens[:3]), sum(lens[:4])
    for side, cap in (("last_of_run1_out", sum3 - 1), ("run1_fits", sum3), ("first_of_run2_out", sum4 - 1),
                      ("first_of_run2_fits", sum4), ("first_of_run2_fits_1_spare", sum4 + 1), ("ample", sum(lens) + 100)):
        out.append(_xform_case(f"capacity_{side}", "capacity", side, offs[4] + len(sm["p2"]) + 33, patches, offs,
                               {"runs": [(0, 3, run1), (3, 2, run2)], "oversize": []}, out_cap=cap))
    # an oversize message between two runs (S + 1), its neighbour that still fits a slab (S); the
    # oversize one also refused (a flipped blob byte)
    for total, side, flip in ((S, "at", False), (S + 1, "over", False), (S + 1, "over", True)):
        m = big(total)
        at = 4099
        p2 = at + total + 5
        p3 = p2 + len(sm["p2"]) + 3
        offs = [61, 61 + len(sm["p0"]) + 1, at, p2, p3]
        head = offs[1] + len(sm["p1"]) - 61
        tail = p3 + len(sm["p3"]) - p2
        exp = {"runs": [(0, 2, head), (2, 1, S), (3, 2, tail)], "oversize": []} if total == S else \
            {"runs": [(0, 2, head), (3, 2, tail)], "oversize": [2]}
        out.append(_xform_case(f"oversize_between_{side}{'_refused' if flip else ''}", "oversize_between", side,
                               p3 + len(sm["p3"]) + 11,
                               [(offs[0], sm["p0"]), (offs[1], sm["p1"]), (at, m), (p2, sm["p2"]), (p3, sm["p3"])], offs,
                               exp, flips=[at + total - 9] if flip else []))
    # duplicates of one offset: the summed output bound cuts the run (extent above 1 KiB) ...
    e = len(sm["k1"])
    n0 = X // (e + GROWTH) + 1  # the first n with n * (e + GROWTH) > X
    assert (n0 - 1) * (e + GROWTH) <= X < n0 * (e + GROWTH) and n0 <= M and (n0 - 1) % 251
    for n, side in ((n0 - 1, "at"), (n0, "over")):
        out.append(_xform_case(f"dup_out_{side}", "dup_output_cut", side, 7 + e + 13, [(7, sm["k1"])], [7] * n,
                               {"runs": [(0, n, e)] if n < n0 else [(0, n0 - 1, e), (n0 - 1, 1, e)], "oversize": []},
                               out_cap=n * (e + GROWTH)))
    # ... or the message count does (under 1 KiB)
    e = len(sm["p0"])
    assert M % 251
    for n, side in ((M, "at"), (M + 1, "over")):
        out.append(_xform_case(f"dup_count_{side}", "dup_count_cut", side, 7 + e + 13, [(7, sm["p0"])], [7] * n,
                               {"runs": [(0, M, e)] if n == M else [(0, M, e), (M, 1, e)], "oversize": []},
                               out_cap=n * (e + GROWTH)))
    return out


TRANSFORM_SIDES = {"end_of_run": {"under", "at", "over"}, "lower_offset": {"under", "at", "over"},
                   "capacity": {"last_of_run1_out", "run1_fits", "first_of_run2_out", "first_of_run2_fits",
                                "first_of_run2_fits_1_spare", "ample"},
                   "oversize_between": {"at", "over"}, "dup_output_cut": {"at", "over"},
                   "dup_count_cut": {"at", "over"}}


def families(cases):
    out = {}
    for c in cases:
        out.setdefault(c["family"], []).append(c)
    return out


# ------------------------------------------------------------------ what the oracle says of a case
SMALL_MESSAGE = 1 << 20  # the GPU tests hold messages up to this size against the oracle's bytes


def oracle_verify(region, offs):
    """(status, end) lists by MF.verify_message; each distinct offset judged once."""
    seen = {}
    for o in offs:
        if o not in seen:
            seen[o] = MF.verify_message(region, o)
    return [seen[o][0] for o in offs], [seen[o][1] for o in offs]


def oracle_messages(region, offs, lives, version=3, largest=None):
    """(status, transformed bytes or None) per message by MF.transform_message; each distinct (offset,
    life version) judged once. largest: a clean message above that many bytes is left to the caller
    (status None)."""
    seen = {}
    for o, life in zip(offs, lives):
        if (o, life) in seen:
            continue
        st, end = MF.verify_message(region, o)
        if st:
            seen[(o, life)] = (st, None)
        elif largest is not None and end - o > largest:
            seen[(o, life)] = (None, None)
        else:
            seen[(o, life)] = MF.transform_message(bytes(region[o:end]), 0, life=life, version=version)
    return [seen[(o, life)] for o, life in zip(offs, lives)]


def pack(messages, out_cap):
    """The packing rule over oracle_messages' list: message i's bytes go at the sum of the transformed
    lengths of the messages before it, or it gets MSG_NO_ROOM when they would pass out_cap (the sum
    grows all the same). Returns (status, out_off (-1: none), out_len) lists."""
    pos = 0
    status, off_out, len_out = [], [], []
    for st, body in messages:
        fits = st == 0 and pos + len(body) <= out_cap
        status.append(st if st else 0 if fits else MSG_NO_ROOM)
        off_out.append(pos if fits else -1)
        len_out.append(len(body) if fits else 0)
        if st == 0:
            pos += len(body)
    return status, off_out, len_out


def ample_cap(case, region) -> int:
    """An output capacity no message of the case runs out of: the summed extents + GROWTH each."""
    return sum(e + GROWTH for e in extents(region, case["offs"]))


def check_transform(case, region, got, messages):
    """A transform's outputs (out bytes, out_off, out_len, status) against oracle_messages' list."""
    out, oo, ol, st = got
    cap = case["out_cap"] if case["out_cap"] is not None else ample_cap(case, region)
    status, off_out, len_out = pack(messages, cap)
    assert st.tolist() == status and oo.tolist() == off_out and ol.tolist() == len_out, case["name"]
    view = memoryview(out)
    for (_, body), at in zip(messages, off_out):
        if at >= 0:
            assert view[at:at + len(body)] == body, case["name"]
