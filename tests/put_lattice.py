"""Write-side geometry by construction: inputs that put a copied field on every destination phase, source residue
and length at which the write-side kernels change their case split, and put_cells(), the classifier the tests
assert that coverage with.

Three kernels produce the output bytes of serialize, transform, re-key and send:

  put_stream_kernel (put_kernels.hip), copy-mode messages of at most 6,144 B: the output is cut into 16-B
      pieces on the destination's grid; a piece wholly inside a data segment is one 16-B load and store, every
      other segment byte goes through the segment's 32 edge slots. stream_cells().
  the copy-through sweep (SweepArgs::copy_dst, crc32_kernels.hip): every 16-B piece read for a job's CRC is
      stored at dst - src past its source; the source residue picks the case. through_cells(), sweep_cuts().
  gather_copy_kernel (put_kernels.hip): copy_range's head / 16-B pieces / tail split on the destination's grid,
      the pieces built from two aligned source loads. range_cells(), gather_ranges().

put_cells() restates those splits from the kernel sources; it shares no code with kernel_model.py.

stream_lattice() is a batch of PutMessages with explicit descriptors, source buffers and output offsets;
copy_lattice() the same for the job path's copy-through sweep, below and above the group phase's job count;
stored_lattice() a log region of clean stored PUTs of every header, properties and blob-record version for the
re-key's gather copy, the transform's general path and send. Every key, encryption-key, user-metadata and blob
byte is nonzero (a properties source is real BlobPropertiesSerDe bytes, which the round trip parses, so it holds
zero bytes); padding between sources is nonzero too, and the output's filler is 0xAA.

What cannot be reached is stated in the tests that run into it: kCopySkip through serialize, the
gather copy under a clean transform, and missing_pairings() for copy_range."""
import functools
from types import SimpleNamespace

import numpy as np

import geometry_lattice as G
import rekey_oracle as RK
from msgfmt import MF

STREAM_MAX = 6144            # crc32_kernels.h kStreamPutMax
SUPER_BLOCK = 4096           # crc32_kernels.h kSuperBlock: 64 runs
FILL = 0xAA
SRC_PAD = 0x77               # between sources in the fields / blobs buffers
SEGMENTS = ("key", "enckey", "props", "usermeta", "blob")
KEY, ENC, PROPS, UM, BLOB = range(5)
GROUP_MIN_JOBS = 16384       # crc32_kernels.h kGroupMinChunks
GROUP_SMALL_MAX = G.CLASS_CUTS[-1]  # kGroupSmallMax
SHARE_QUANTUM, MIN_SHARE = 1024, 16384  # crc32_kernels.h kShareQuantum, kMinShare
COPY_JOB_COST = 2048         # crc32_kernels.h kCopyJobCost
GATHER_MIN_SHARE = 4096      # gather_copy_kernel: S is a multiple of 256 and at least this
DELTAS = (0, 1, 8, 15)


# ---------------------------------------------------------------- the classifier
def stream_cells(m0: int, lo: int, hi: int, src: int, length: int = 0):
    """put_stream_kernel's split for the data segment [lo, hi) (message-relative) of a message that starts m0
    bytes past a 64-aligned base, the segment's source at address src; length: the message's.

    mis = m0 & 15 the destination grid's phase, m63 = m0 & 63; span = m0 - S0 + length (S0 = m0 rounded down to
    64), nruns = ceil(span / 64) hashed runs, two_sb = more than 64 of them (a second super-block); streamed =
    length <= 6,144. up / dn: the first piece boundary at or above lo / the last at or below hi; inside = the
    16-B pieces between them (inside_class 0, 1 or 2 for more); head = edge bytes below up (slots 0..15), tail =
    edge bytes from max(up, dn) (slots 16..31); within = a nonempty segment inside one piece, straddle = one
    across a boundary that fills no piece. phase = (m0 + lo) & 15, src16 = src & 15."""
    mis = m0 & 15
    up = ((lo + mis + 15) & ~15) - mis
    dn = ((hi + mis) & ~15) - mis
    inside = max(0, (dn - up) >> 4)
    head = max(0, min(up, hi) - lo)
    tail = max(0, hi - max(up, dn))
    span = (m0 & 63) + length
    return SimpleNamespace(
        mis=mis, m63=m0 & 63, span=span, nruns=(span + 63) >> 6, two_sb=span > SUPER_BLOCK, streamed=length <= STREAM_MAX,
        up=up, dn=dn, inside=inside, inside_class=min(inside, 2), head=head, tail=tail,
        within=hi > lo and inside == 0 and ((lo + mis) >> 4) == ((hi - 1 + mis) >> 4),
        straddle=hi > lo and inside == 0 and ((lo + mis) >> 4) != ((hi - 1 + mis) >> 4),
        phase=(m0 + lo) & 15, src16=src & 15, length=hi - lo)


def range_cells(dst: int, src: int, n: int):
    """copy_range (put_kernels.hip) for one wave's n bytes src -> dst. head = min((16 - dst & 15) & 15, n)
    bytewise lanes, capped = n ended the head before the boundary; n16 = 16-B pieces; shift = (src + head) & 15
    = 4 Q + r picks copy_pieces<Q> and shift_pair's r (r == 0: whole dwords, shift == 0: one load a piece);
    unrolled / remainder = the most iterations any lane makes of the four-piece loop (p + 192 < n16, p from
    the lane in steps of 256) and of the one-piece loop after it; tail = (n - head) & 15 bytewise lanes."""
    head0 = (16 - (dst & 15)) & 15
    head = min(head0, n)
    body = n - head
    n16 = body >> 4
    shift = (src + head) & 15
    unrolled = remainder = 0
    for lane in range(64):
        p, u, r = lane, 0, 0
        while p + 192 < n16:
            p, u = p + 256, u + 1
        while p < n16:
            p, r = p + 64, r + 1
        unrolled, remainder = max(unrolled, u), max(remainder, r)
    return SimpleNamespace(head=head, capped=head0 > n, n16=n16, shift=shift, Q=shift >> 2, r=shift & 3,
                           aligned=shift == 0, unrolled=unrolled, remainder=remainder, tail=body & 15, n=n)


def through_cells(src: int, length: int, dst: int):
    """The copy-through sweep's split for a job of `length` bytes at source address src, stored at dst. cls: the
    group phase's size class by G.CLASS_CUTS (None: empty, or above 16 KiB and the sweep's in any batch); the
    group phase takes a classed job only in a batch of at least 16,384 jobs. The source picks the case: the body
    ends at cb = max(src, floor16(src + length)); with a body, the first piece is the 16-B block at floor16(src)
    and lead = src & 15 of its bytes are dropped (copy_piece stores the rest bytewise); t = src + length - cb
    trailing bytes go one lane each (st8g). delta = (dst - src) & 15: every 16-B store is that far off the
    destination's grid."""
    ce = src + length
    cb = max(src, ce & ~15)
    body = cb > src
    if length == 0 or length > G.CLASS_CUTS[-1]:
        cls = None
    else:
        cls = sum(1 for c in G.CLASS_CUTS[:-1] if length > c)
    return SimpleNamespace(cls=cls, src16=src & 15, src64=src & 63, body=body, lead=(src & 15) if body else 0,
                           t=ce - cb, delta=(dst - src) & 15, length=length)


def put_cells(form: str, *args):
    """The write side's case split: put_cells("stream", m0, lo, hi, src, length), put_cells("range", dst, src, n),
    put_cells("through", src, length, dst)."""
    return {"stream": stream_cells, "range": range_cells, "through": through_cells}[form](*args)


def snap_cut(cs: int, length: int, r: int) -> int:
    """crc32_kernels.hip snap_cut: the chunk-relative cut r moved up to a 16-B aligned address, capped."""
    return min(((cs + r + 15) & ~15) - cs, length)


def sweep_share(total: int, grid: int) -> int:
    """crc32_sweep_kernel's byte share of one wave: 16 waves a workgroup."""
    nwaves = 16 * grid
    share = ((total + nwaves - 1) // nwaves + SHARE_QUANTUM - 1) & ~(SHARE_QUANTUM - 1)
    return max(share, MIN_SHARE)


def sweep_cuts(lens, small_max: int, grid: int):
    """{job: [raw cut r, ...]}: where the sweep's share boundaries fall strictly inside a job. The stream is the
    concatenation of the jobs longer than small_max (the others are the group phase's and take no share)."""
    spans = [n if n > small_max else 0 for n in lens]
    share = sweep_share(sum(spans), grid)
    cuts, pos = {}, 0
    for j, n in enumerate(spans):
        if n:
            first = (pos // share + 1) * share
            rs = list(range(first - pos, n, share))
            if rs:
                cuts[j] = rs
        pos += n
    return cuts


def gather_ranges(jobs, share: int = GATHER_MIN_SHARE):
    """gather_copy_kernel's copy_range calls, [(dst, src, n, job)]: job j's bytes are the first len units of its
    cost range [start, start + len + 2048) (an empty job costs nothing), wave w takes cost units [w S, (w + 1) S),
    so a job is cut wherever a multiple of S falls inside its bytes. jobs: [(dst, src, n)] in job order. S is
    `share` as long as the summed cost is at most share * (waves in the grid), which gather_cost() lets a test
    check."""
    out, start = [], 0
    for j, (dst, src, n) in enumerate(jobs):
        if n:
            cuts = [0] + list(range((start // share + 1) * share - start, n, share)) + [n]
            out += [(dst + a, src + a, b - a, j) for a, b in zip(cuts, cuts[1:])]
            start += n + COPY_JOB_COST
    return out


def gather_cost(jobs) -> int:
    return sum(n + COPY_JOB_COST for _, _, n in jobs if n)


# ---------------------------------------------------------------- PUT messages with explicit descriptors
def segment_bounds(v: int, key_len: int, enc_len, props_len: int, um_len: int, blob_len: int):
    """(message length, lo[5], hi[5]) of a PUT's data segments, restated from PutMessageFormatInputStream's
    layout: header (34 / 38 / 40 B), key, [encryption-key record: 6 B head, key, CRC], properties record (2 B
    head), user-metadata record (6 B head), blob record (13 B head), each record closed by an 8-B CRC. An absent
    encryption key is the empty segment at the key's end."""
    pos = MF.HEADER_SIZE[v]
    lo, hi = [pos], [pos + key_len]
    pos += key_len
    if enc_len is not None and v >= 2:
        lo.append(pos + 6)
        hi.append(pos + 6 + enc_len)
        pos += 6 + enc_len + 8
    else:
        lo.append(pos)
        hi.append(pos)
    for head, n in ((2, props_len), (6, um_len), (13, blob_len)):
        lo.append(pos + head)
        hi.append(pos + head + n)
        pos += head + n + 8
    return pos, lo, hi


def expected_bytes(m) -> bytes:
    """The oracle's layout of PutMessage m (blob type 0, as every lattice message)."""
    return MF.put_message(m.key, m.props, m.usermeta, m.blob, version=m.header_version, enc_key=m.enckey,
                          life=m.life_version, compressed=m.compressed)


class _Batch:
    """Accumulates messages, their sources in the two buffers at chosen residues, and their output offsets."""

    def __init__(self):
        from ambry_amd.messages import PUT_DESC_DTYPE

        self.dtype = PUT_DESC_DTYPE
        self.msgs, self.kind, self.probe, self.out_off, self.src, self.lo, self.hi, self.length = [], [], [], [], [], [], [], []
        self.fields, self.blobs = bytearray(), bytearray()
        self.pos = 0

    def _place(self, buf: bytearray, data: bytes, res: int, mod: int) -> int:
        buf += bytes([SRC_PAD]) * ((res - len(buf)) % mod)
        at = len(buf)
        buf += data
        return at

    def add(self, m, kind: str, probe: int, out_off: int, res, mod: int = 16):
        """res[k]: the wanted residue mod `mod` of segment k's source offset (the buffers are 64-aligned)."""
        assert out_off >= self.pos
        src = [self._place(self.blobs if k == BLOB else self.fields, getattr(m, name) or b"", res[k], mod)
               for k, name in enumerate(SEGMENTS)]
        n, lo, hi = segment_bounds(m.header_version, len(m.key), None if m.enckey is None else len(m.enckey),
                                   len(m.props), len(m.usermeta), len(m.blob))
        self.msgs.append(m)
        self.kind.append(kind)
        self.probe.append(probe)
        self.out_off.append(out_off)
        self.src.append(src)
        self.lo.append(lo)
        self.hi.append(hi)
        self.length.append(n)
        self.pos = out_off + n

    def finish(self, **extra):
        n = len(self.msgs)
        descs = np.zeros(n, dtype=self.dtype)
        src = np.asarray(self.src, dtype=np.int64)
        descs["out_off"] = self.out_off
        for k, name in enumerate(SEGMENTS):
            descs[name + "_src"] = src[:, k]
        descs["blob_len"] = [len(m.blob) for m in self.msgs]
        descs["key_len"] = [len(m.key) for m in self.msgs]
        descs["enckey_len"] = [-1 if m.enckey is None else len(m.enckey) for m in self.msgs]
        descs["props_len"] = [len(m.props) for m in self.msgs]
        descs["usermeta_len"] = [len(m.usermeta) for m in self.msgs]
        descs["life_version"] = [m.life_version for m in self.msgs]
        descs["header_version"] = [m.header_version for m in self.msgs]
        total = self.pos + 16
        image = np.full(total, FILL, dtype=np.uint8)
        for m, o, ln in zip(self.msgs, self.out_off, self.length):
            e = expected_bytes(m)
            assert len(e) == ln
            image[o:o + ln] = np.frombuffer(e, dtype=np.uint8)
        return SimpleNamespace(
            msgs=self.msgs, kind=self.kind, probe=np.asarray(self.probe), out_off=np.asarray(self.out_off, dtype=np.int64),
            src=src, lo=np.asarray(self.lo, dtype=np.int64), hi=np.asarray(self.hi, dtype=np.int64),
            length=np.asarray(self.length, dtype=np.int64), descs=descs,
            fields=np.frombuffer(bytes(self.fields) or b"\x77", dtype=np.uint8),
            blobs=np.frombuffer(bytes(self.blobs) or b"\x77", dtype=np.uint8), total=total, image=image, **extra)


def _message(j: int, v: int, key_len: int, enc_len, um_len: int, blob_len: int):
    from ambry_amd.messages import PutMessage

    enc = None if enc_len is None or v == 1 else G.nonzero_bytes(5 * j + 1, enc_len)
    return PutMessage(key=G.nonzero_bytes(5 * j, key_len), props=MF.blob_properties_bytes(blob_len, service_id="s%d" % j),
                      usermeta=G.nonzero_bytes(5 * j + 2, um_len), blob=G.nonzero_bytes(5 * j + 3, blob_len), enckey=enc,
                      header_version=v, life_version=j % 5 if v == 3 else 0)


PHASE_LENGTHS = range(0, 49)
REPEAT_LENGTHS = (1, 16, 17, 33, 47)
KEY_LENGTHS = range(2, 20)
ENC_LENGTHS = (None,) + tuple(range(0, 18))
SPAN_EDGES = (4095, 4096, 4097)
LENGTH_EDGES = (6143, 6144, 6145)
EDGE_M63 = (0, 1, 63)
BACK_TO_BACK = 128


def stream_specs():
    """(kind, probed segment, header version, key length, enc length or None, um length, blob length, placement)
    of every message, in batch order. placement: ("phase", p): the probed segment starts at destination phase p;
    ("m63", r): the message starts r past a 64-B boundary; ("span", r, s) / ("len", r, n): as m63, the blob sized
    so that r + length = s / length = n; ("next",): back to back with its predecessor."""
    specs, j = [], 0
    for seg in (UM, BLOB):
        for p in range(16):
            for n in PHASE_LENGTHS:
                v = 1 + j % 3
                enc = j % 18 if j % 4 == 0 else None
                specs.append(("phase", seg, v, 3 + j % 17, enc, n if seg == UM else j % 7, n if seg == BLOB else j % 5,
                              ("phase", p)))
                j += 1
    for r in range(64):
        for s16 in range(16):
            seg = UM if (r + s16) % 2 else BLOB
            n = REPEAT_LENGTHS[(r + 3 * s16) % len(REPEAT_LENGTHS)]
            specs.append(("repeat", seg, 1 + j % 3, 3 + j % 11, None if j % 3 else j % 9, n if seg == UM else 2,
                          n if seg == BLOB else 1, ("m63", r)))
            j += 1
    for p in range(16):
        for n in KEY_LENGTHS:
            specs.append(("key", KEY, 1 + j % 3, n, None, j % 4, j % 6, ("phase", p)))
            j += 1
        for n in ENC_LENGTHS:
            specs.append(("enckey", ENC, 2 + j % 2, 3 + j % 5, n, j % 4, j % 6, ("phase", p)))
            j += 1
    for r in EDGE_M63:
        for s in SPAN_EDGES:
            specs.append(("span", BLOB, 1 + j % 3, 9, None, 11, None, ("span", r, s)))
            j += 1
    for r in EDGE_M63:
        for n in LENGTH_EDGES:
            specs.append(("length", BLOB, 1 + j % 3, 9, 5 if j % 2 else None, 11, None, ("len", r, n)))
            j += 1
    for i in range(BACK_TO_BACK):
        specs.append(("packed", UM if i % 2 else BLOB, 1 + j % 3, 3 + i % 13, None if i % 3 else i % 6, i % 23, i % 19,
                      ("next",)))
        j += 1
    return specs


@functools.lru_cache(maxsize=None)
def stream_lattice():
    """The streamed form's batch: msgs, kind, probe (the probed segment), out_off, src [m, 5] (offsets into the
    fields buffer, the blob's into the blobs buffer), lo / hi [m, 5], length, descs (PUT_DESC_DTYPE), fields,
    blobs (uint8), total, image (the expected output, 0xAA between the messages). The probed segment's source
    sits at residue (7 j) mod 16 for message j, except in the "repeat" family, which steps through all 16 at
    every m0 & 63; the other sources take whatever residue follows."""
    b = _Batch()
    for j, (kind, seg, v, klen, enc, um, blen, place) in enumerate(stream_specs()):
        if blen is None:  # sized by the message's length
            base, _, _ = segment_bounds(v, klen, enc if v >= 2 else None, len(MF.blob_properties_bytes(0, service_id="s%d" % j)),
                                        um, 0)
            blen = (place[2] - place[1] if place[0] == "span" else place[2]) - base
        m = _message(j, v, klen, enc, um, blen)
        _, lo, _ = segment_bounds(v, klen, None if m.enckey is None else len(m.enckey), len(m.props), um, blen)
        if place[0] == "phase":
            off = b.pos + ((place[1] - b.pos - lo[seg]) & 15)
        elif place[0] == "next":
            off = b.pos
        else:
            off = b.pos + ((place[1] - b.pos) & 63)
        res = [(3 * j + 5 * k) % 16 for k in range(5)]
        res[seg] = (j % 16) if kind == "repeat" else (7 * j) % 16
        b.add(m, kind, seg, off, res)
    return b.finish()


def segment_cells(lat, i: int, k: int, shift: int = 0):
    """stream_cells of segment k of lattice message i, the output view `shift` bytes past a 64-B boundary (the
    source buffers 64-aligned)."""
    return stream_cells(shift % 64 + int(lat.out_off[i]), int(lat.lo[i, k]), int(lat.hi[i, k]), int(lat.src[i, k]),
                        int(lat.length[i]))


# ---------------------------------------------------------------- the copy-through sweep
COPY_GRID = 64
BIG_BLOBS = tuple(65536 * k + d for k in (1, 2) for d in (-1, 0, 1)) + ((1 << 20) + 4109,)
BIG_RES = (0, 1, 15, 63)
CUT_TARGET = 40000 + 3   # the three blobs a share cut is steered into; ends 3 past a 16-B boundary
CUT_WANT = ("first16", "last16", "mid")
CLASS0_LENGTHS = range(0, 81)


def copy_specs(jobs: str):
    """(kind, probed slot, probe length, source residue mod 64, delta) of every copy-lattice message but the cut
    targets. "wave": under 16,384 jobs; "group": class 0 at all four deltas, which takes it past 16,384."""
    specs, j = [], 0
    for d in (DELTAS if jobs == "group" else (None,)):
        for r in range(16):
            for n in CLASS0_LENGTHS:
                specs.append(("class0", UM if (r + n) % 2 else BLOB, n, r + 16 * (j % 4), DELTAS[j % 4] if d is None else d))
                j += 1
    for n in G.CUT_LENGTHS:
        for r in range(64):
            specs.append(("cut", UM if (r + n) % 2 else BLOB, n, r, DELTAS[j % 4]))
            j += 1
    for n in BIG_BLOBS:
        for r in BIG_RES:
            specs.append(("big", BLOB, n, r, DELTAS[j % 4]))
            j += 1
    return specs


@functools.lru_cache(maxsize=None)
def copy_lattice(jobs: str):
    """The job path's batch, as stream_lattice() plus grid (the workgroups the share cuts below were computed
    for), small_max, job_len (the 5 m job lengths in the sweep's order, slot-major) and cut (message index of
    the blob each of CUT_WANT's cuts falls in). One slot a message is the probe: user metadata for a
    fields-buffer source, the blob for a blobs-buffer source, at source residue r mod 64 and with the output
    placed so that (dst - src) & 15 is the wanted delta. Job lengths are the field lengths themselves (the record
    prefix is hashed as the job's seed and written by the layout kernel), so G.CUT_LENGTHS apply unreduced.

    The last six messages are three (pad, target) pairs: each pad's blob (over 16 KiB, so it takes a share in
    both sizes) is sized so that a share boundary falls 5 bytes into its target's blob, 5 bytes before its end
    (the snapped cut leaves the last 3 bytes to the next wave), and 20,000 bytes in."""
    b = _Batch()
    specs = copy_specs(jobs)

    def add(j, kind, slot, n, r, delta, um=None, blob=None):
        um = (n if slot == UM else 1 + j % 5) if um is None else um
        blob = (n if slot == BLOB else 1 + j % 3) if blob is None else blob
        m = _message(j, 1 + j % 3, 3 + j % 9, None if j % 5 else j % 7, um, blob)
        _, lo, _ = segment_bounds(m.header_version, len(m.key), None if m.enckey is None else len(m.enckey),
                                  len(m.props), um, blob)
        res = [(3 * j + 5 * k) % 64 for k in range(5)]
        res[slot] = r
        off = b.pos + ((r + delta - b.pos - lo[slot]) & 15)  # dst = off + lo, src = r (mod 16)
        b.add(m, kind, slot, off, res, mod=64)

    for j, (kind, slot, n, r, delta) in enumerate(specs):
        add(j, kind, slot, n, r, delta)
    m_all = len(specs) + 6
    small_max = GROUP_SMALL_MAX if 5 * m_all >= GROUP_MIN_JOBS else 0
    span = lambda n: n if n > small_max else 0  # noqa: E731
    fixed_um = 9
    # every job before the blobs' slot, the pads' and targets' own fields included: their lengths are fixed
    j0 = len(specs)
    tail_msgs = [_message(j0 + t, 1 + (j0 + t) % 3, 3 + (j0 + t) % 9, None if (j0 + t) % 5 else (j0 + t) % 7, fixed_um, 0)
                 for t in range(6)]
    before = sum(span(len(getattr(m, name) or b"")) for name in SEGMENTS[:4] for m in b.msgs + tail_msgs)
    before += sum(span(len(m.blob)) for m in b.msgs)
    share, cut = MIN_SHARE, {}  # the total stays under 16 waves x COPY_GRID x 16 KiB: asserted below
    for t, want in enumerate(CUT_WANT):
        r = {"first16": 5, "last16": CUT_TARGET - 5, "mid": 20000}[want]
        pad = GROUP_SMALL_MAX + 1
        pad += -(before + pad + r) % share  # the pad blob starts at stream position `before`
        j = j0 + 2 * t
        add(j, "pad", BLOB, pad, (5 * t) % 64, DELTAS[t % 4], um=fixed_um)
        add(j + 1, "target", BLOB, CUT_TARGET, (16 + 3 - CUT_TARGET) % 16 + 16 * t, DELTAS[(t + 1) % 4], um=fixed_um)
        cut[want] = len(b.msgs) - 1
        before += pad + CUT_TARGET
    lat = b.finish(grid=COPY_GRID, small_max=small_max, cut=cut)
    m = len(lat.msgs)
    assert m == m_all
    lat.job_len = np.concatenate([lat.hi[:, k] - lat.lo[:, k] for k in range(5)])
    assert sweep_share(int(sum(n for n in lat.job_len.tolist() if n > small_max)), COPY_GRID) == MIN_SHARE == share
    return lat


def job_through_cells(lat, i: int, k: int, in_place=()):
    """through_cells of slot k of copy-lattice message i: the source in its buffer, or where it lies in the output
    when its slot is in place (the two buffers and the output 64-aligned)."""
    dst = int(lat.out_off[i] + lat.lo[i, k])
    src = dst if SEGMENTS[k] in in_place else int(lat.src[i, k])
    return through_cells(src, int(lat.hi[i, k] - lat.lo[i, k]), dst)


# ---------------------------------------------------------------- stored PUTs
STORED_LENGTHS = tuple(range(0, 49)) + (63, 64, 65, 4095, 4096, 4097)
STORED_BIG = 300000
STORED_MID = tuple(8200 + 7 * t for t in range(24))  # two shares and a little: one range of a whole share each
STORED_HEAD = {1: 10, 2: 12, 3: 13}  # Blob_Format_V1 / V2 / V3: the bytes before the content


def _stored(i: int, um: bytes, content: bytes, hv: int, sv: int, bv: int) -> bytes:
    enc = G.nonzero_bytes(11 * i + 5, 1 + i % 21) if hv >= 2 and i % 3 == 0 else None
    props = MF.blob_properties_bytes(len(content), serde_version=sv, service_id="s%d" % (i % 11),
                                     owner_id="o" * (i % 6), filename="f.bin" if i % 2 else None)
    return RK.stored_put(MF.store_key("p%05d" % i), props, um, content, hv=hv, enc_key=enc, life=i % 3, bv=bv)


@functools.lru_cache(maxsize=None)
def stored_lattice():
    """region (bytes), offs (int64[m]), probe (bool[m]), blob_src / blob_len (the content's offset in the region
    and its length). Messages alternate spacer, probe from offset 0; header versions 1-3, properties versions 1-5
    and blob-record versions 1-3 cycle with different periods, so a transform to header V3 grows the messages by
    different amounts and dst - src steps through the residues. A spacer's user-metadata size (0..15) puts its
    probe's content on source residue j mod 16 (the region 16-aligned). Probe content lengths: STORED_LENGTHS at
    every residue, STORED_MID (a gather-copy range of one whole wave share, 4,096 B, exists only inside a longer job;
    with 24 of them one such range starts on a 16-B boundary of the output, which test_gather_copy_coverage
    asserts) and one STORED_BIG blob."""
    parts, offs, probe, blob_src, blob_len = [], [], [], [], []
    pos = 0

    def put(msg, is_probe):
        nonlocal pos
        _, total, rel = MF.parse_header(msg, 0)
        first = next(r for r in rel if r != MF.INVALID)
        bv = MF._be16(msg, rel[4])
        offs.append(pos)
        probe.append(is_probe)
        blob_src.append(pos + rel[4] + STORED_HEAD[bv])
        blob_len.append(first + total - 8 - rel[4] - STORED_HEAD[bv])
        parts.append(msg)
        pos += len(msg)

    spec = [(n, r) for n in STORED_LENGTHS for r in range(16)] + [(n, t % 16) for t, n in enumerate(STORED_MID)] + \
        [(STORED_BIG, 5)]
    for j, (n, r) in enumerate(spec):
        hv, sv, bv = 1 + j % 3, 1 + j % 5, 1 + (j // 2) % 3
        msg = _stored(2 * j + 1, G.nonzero_bytes(7 * j, j % 29), G.nonzero_bytes(7 * j + 1, n), hv, sv, bv)
        _, _, rel = MF.parse_header(msg, 0)
        content_rel = rel[4] + STORED_HEAD[bv]
        shv, ssv, sbv = 1 + (j // 3) % 3, 1 + (j // 2) % 5, 1 + j % 3
        s0 = _stored(2 * j, b"", G.nonzero_bytes(7 * j + 2, 1 + j % 9), shv, ssv, sbv)
        s = (r - content_rel - pos - len(s0)) % 16
        put(_stored(2 * j, G.nonzero_bytes(7 * j + 3, s), G.nonzero_bytes(7 * j + 2, 1 + j % 9), shv, ssv, sbv), False)
        put(msg, True)
    return SimpleNamespace(region=b"".join(parts), offs=np.asarray(offs, dtype=np.int64), probe=np.asarray(probe),
                           blob_src=np.asarray(blob_src, dtype=np.int64), blob_len=np.asarray(blob_len, dtype=np.int64))


@functools.lru_cache(maxsize=None)
def rekey_inputs():
    """(descs, aux) that re-key every stored-lattice message: new keys of 1 + (5 i) mod 16 bytes, so the packed
    output's offsets step through all 16 residues; the stored content, account and container kept apart from
    the ids the descriptor always sets."""
    lat = stored_lattice()
    descs, aux = np.zeros(len(lat.offs), dtype=RK.DESC), bytearray()
    for i in range(len(lat.offs)):
        d = descs[i]
        klen = 1 + (5 * i) % 16
        d["key_src"], d["key_len"] = len(aux), klen
        d["content_src"], d["props_blob_size"] = RK.KEEP, -1
        d["account_id"], d["container_id"] = 100 + i % 50, 7 + i % 9
        aux += G.nonzero_bytes(13 * i + 9, klen)
    return descs, bytes(aux)


@functools.lru_cache(maxsize=None)
def rekey_expected():
    lat = stored_lattice()
    descs, aux = rekey_inputs()
    return RK.expected(lat.region, lat.offs.tolist(), descs, aux, None, 3)


@functools.lru_cache(maxsize=None)
def transform_expected(corrupt: bool = False):
    """(status, out_off (-1: not placed), out_len, the packed output) of MF.transform_message to header V3 over
    stored_lattice(), or over corrupted_region()."""
    lat = stored_lattice()
    region = corrupted_region() if corrupt else lat.region
    st, off, ln, out, pos = [], [], [], [], 0
    for i, o in enumerate(lat.offs.tolist()):
        s, b = MF.transform_message(region, o, life=i % 7, version=3)
        st.append(s)
        off.append(pos if b is not None else -1)
        ln.append(len(b) if b is not None else 0)
        if b is not None:
            out.append(b)
            pos += len(b)
    return np.asarray(st, dtype=np.uint32), np.asarray(off, dtype=np.int64), np.asarray(ln, dtype=np.int64), b"".join(out)


@functools.lru_cache(maxsize=None)
def send_expected(flag: int):
    """(status list, info array, the packed body) of send_oracle over stored_lattice() under `flag`, every
    message at its header's own length."""
    import send_oracle as SO

    lat = stored_lattice()
    return SO.expected(lat.region, lat.offs.tolist(), None, flag)


CORRUPT_PROBE = 101 # the probe whose content gets one flipped bit in corrupted_region()


@functools.lru_cache(maxsize=None)
def corrupted_region() -> bytes:
    """stored_lattice()'s region with one bit flipped in one probe's content: the transform's speculative pass
    fails, and its fallback pass rebuilds the whole output with the gather copy."""
    lat = stored_lattice()
    i = int(np.nonzero(lat.probe)[0][CORRUPT_PROBE])
    assert lat.blob_len[i] > 0
    region = bytearray(lat.region)
    region[int(lat.blob_src[i])] ^= 0x10
    return bytes(region)


def rekey_jobs(region_base: int = 0, aux_base: int = 0, out_base: int = 0):
    """The re-key's gather-copy jobs [(dst, src, n)] in the kernel's order (slot-major: the new key from aux, the
    encryption-key record whole, the user-metadata record whole, the blob content), from the oracle's output
    offsets and the two headers alone. Addresses from the given bases (any 16-aligned bases give the same
    cells)."""
    lat = stored_lattice()
    descs, _ = rekey_inputs()
    _, out_off, _, packed = rekey_expected()
    slots = [[], [], [], []]
    for i, off in enumerate(lat.offs.tolist()):
        _, total, rel = MF.parse_header(lat.region, off)
        at = out_off[i]
        _, ototal, orel = MF.parse_header(packed, at)
        slots[0].append((out_base + at + MF.HEADER_SIZE[3], aux_base + int(descs[i]["key_src"]), int(descs[i]["key_len"])))
        if rel[0] != MF.INVALID:
            slots[1].append((out_base + at + orel[0], region_base + off + rel[0], rel[1] - rel[0]))
        else:
            slots[1].append((0, 0, 0))
        slots[2].append((out_base + at + orel[3], region_base + off + rel[3], rel[4] - rel[3]))
        slots[3].append((out_base + at + orel[4] + 13, region_base + int(lat.blob_src[i]), int(lat.blob_len[i])))
    return [j for s in slots for j in s]


def missing_pairings(ranges):
    """The (head, shift) pairings no range with pieces hits. A range with pieces has a head that runs to the
    16-B boundary, so its shift is (src + head) & 15 = (src - dst) & 15 (asserted here): the pairing is the
    destination's residue with the job's delta, which a share cut keeps. Nothing ties the two, so no pairing is
    unreachable in principle; the caller pins how few the lattice misses and asserts every single value."""
    hit = set()
    for dst, src, n, _ in ranges:
        c = range_cells(dst, src, n)
        if c.n16:
            assert not c.capped and c.shift == (src - dst) & 15
            hit.add((c.head, c.shift))
    return {(h, s) for h in range(16) for s in range(16)} - hit


def describe_packed(what: str, at: int, flag: int = 0) -> str:
    """Where byte `at` of a packed output of the stored lattice lies: the message, the record of the stored
    message it came from, and through_cells of that record's copy (its CRC span, from where it is stored to where
    it is placed). what: "transform" (clean, to header V3), "rekey" or "send" (under `flag`)."""
    lat = stored_lattice()
    names = ("enckey", "props", "update", "usermeta", "blob")
    if what == "send":
        info = send_expected(flag)[1]
        placed, rel_off = info["out_off"].astype(np.int64), info["rel_off"].astype(np.int64)
    else:
        placed = np.asarray(transform_expected()[1] if what == "transform" else rekey_expected()[1], dtype=np.int64)
        rel_off = None
    i = int(np.searchsorted(placed, at, side="right")) - 1
    off = int(lat.offs[i])
    _, total, rel = MF.parse_header(lat.region, off)
    if rel_off is None:  # a rebuilt message: find the record in the output's own header
        out = transform_expected()[3] if what == "transform" else rekey_expected()[3]
        _, ototal, orel = MF.parse_header(out, int(placed[i]))
        ostart = [r for r in orel if r != MF.INVALID] + [next(r for r in orel if r != MF.INVALID) + ototal]
        pos = at - int(placed[i])
        if pos < ostart[0]:
            return "message %d, byte %d: header or key (computed)" % (i, pos)
        k = [k for k, r in enumerate(orel) if r != MF.INVALID and r <= pos][-1]
        dst = int(placed[i]) + orel[k]
    else:
        pos = int(rel_off[i]) + at - int(placed[i])
        if pos < next(r for r in rel if r != MF.INVALID):
            return "message %d, byte %d: header or key (moved whole)" % (i, pos)
        k = [k for k, r in enumerate(rel) if r != MF.INVALID and r <= pos][-1]
        dst = int(placed[i]) + rel[k] - int(rel_off[i])
    starts = [r for r in rel if r != MF.INVALID] + [next(r for r in rel if r != MF.INVALID) + total]
    end = starts[starts.index(rel[k]) + 1]
    return "message %d, byte %d: %s record; cells %s" % (
        i, pos, names[k], vars(through_cells(off + rel[k], end - rel[k] - 8, dst)))


# ---------------------------------------------------------------- comparing an output image
def describe_byte(lat, at: int, shift: int = 0, form: str = "stream", in_place=()):
    """Where output byte `at` of a put lattice lies: (message index or None for filler, segment name, "gap" for
    computed bytes or "filler", the cells of that segment or of the nearest message's probed segment)."""
    i = int(np.searchsorted(lat.out_off, at, side="right")) - 1
    if i < 0 or at >= lat.out_off[i] + lat.length[i]:
        nxt = min(i + 1, len(lat.out_off) - 1)
        near = nxt if i < 0 or lat.out_off[nxt] - at <= at - (lat.out_off[i] + lat.length[i] - 1) else i
        k = int(lat.probe[near])
        cell = segment_cells(lat, near, k, shift) if form == "stream" else job_through_cells(lat, near, k, in_place)
        return None, "filler", near, cell
    rel = at - int(lat.out_off[i])
    for k in range(5):
        if lat.lo[i, k] <= rel < lat.hi[i, k]:
            cell = segment_cells(lat, i, k, shift) if form == "stream" else job_through_cells(lat, i, k, in_place)
            return i, SEGMENTS[k], i, cell
    k = int(lat.probe[i])
    cell = segment_cells(lat, i, k, shift) if form == "stream" else job_through_cells(lat, i, k, in_place)
    return i, "gap", i, cell


def compare_image(lat, got, shift: int = 0, form: str = "stream", in_place=(), exp=None):
    """None when `got` (uint8 array) equals the lattice's expected image, else a message that names the first
    differing byte, the message and segment it belongs to, and that segment's put_cells."""
    exp = lat.image if exp is None else exp
    got = np.asarray(got)
    if got.shape == exp.shape and np.array_equal(got, exp):
        return None
    if got.shape != exp.shape:
        return "output of %d bytes, expected %d" % (got.size, exp.size)
    diff = np.nonzero(got != exp)[0]
    at = int(diff[0])
    i, what, near, cell = describe_byte(lat, at, shift, form, in_place)
    where = "filler next to message %d (%s)" % (near, lat.kind[near]) if i is None else \
        "message %d (%s) byte %d, %s" % (i, lat.kind[i], at - int(lat.out_off[i]), what)
    return "%d bytes differ; first byte %d: %#x, expected %#x; %s; cells %s" % (
        len(diff), at, got[at], exp[at], where, vars(cell))

