"""The write-side lattices (put_lattice.py) on the CPU: that they hit every cell of the write-side kernels' case
split, by construction and asserted through put_cells(); the pure-Python restatements of the stream kernel's
partition rule and of copy_range (kernel_model.py), exhaustively; the library's CPU serializer, re-key and
transform over the lattices against the oracle; and the comparison helper's sensitivity to one changed byte."""
import itertools

import numpy as np
import pytest

import geometry_lattice as G
import kernel_model as KM
import put_lattice as P
from msgfmt import MF


@pytest.fixture(scope="module")
def stream():
    return P.stream_lattice()


@pytest.fixture(scope="module")
def probed(stream):
    """(kind, cells of the probed segment) of every stream-lattice message."""
    return [(stream.kind[i], P.segment_cells(stream, i, int(stream.probe[i]))) for i in range(len(stream.msgs))]


# ---------------------------------------------------------------- put_cells() itself
def test_put_cells_restates_the_split():
    c = P.put_cells("stream", 64 + 5, 40, 40 + 30, 7, 200)  # mis 5: boundaries at 43, 59, 75
    assert (c.mis, c.m63, c.up, c.dn, c.inside, c.head, c.tail, c.phase, c.src16) == (5, 5, 43, 59, 1, 3, 11, 13, 7)
    assert not c.within and not c.straddle and (c.span, c.nruns, c.two_sb) == (205, 4, False)
    c = P.put_cells("stream", 5, 44, 50, 0, 100)  # inside the piece [43, 59)
    assert c.within and (c.up, c.dn, c.inside, c.head, c.tail) == (59, 43, 0, 6, 0)
    c = P.put_cells("stream", 5, 55, 62, 0, 100)  # across 59, filling nothing
    assert c.straddle and (c.up, c.dn, c.inside, c.head, c.tail) == (59, 59, 0, 4, 3)
    c = P.put_cells("stream", 5, 43, 50, 0, 100)  # from a boundary: no head, the tail slots take it
    assert c.within and (c.head, c.tail) == (0, 7)
    assert P.put_cells("stream", 5, 43, 43, 0, 100).length == 0
    assert [P.put_cells("stream", 63, 0, 0, 0, n).nruns for n in (4032, 4033, 4034)] == [64, 64, 65]
    assert [P.put_cells("stream", 63, 0, 0, 0, n).two_sb for n in (4032, 4033, 4034)] == [False, False, True]
    assert [P.put_cells("stream", 0, 0, 0, 0, n).streamed for n in (6144, 6145)] == [True, False]
    c = P.put_cells("range", 0x1003, 0x2009, 100)  # head 13 to the boundary, then from 0x2016: shift 6
    assert (c.head, c.capped, c.n16, c.shift, c.Q, c.r, c.tail, c.unrolled, c.remainder) == (13, False, 5, 6, 1, 2, 7, 0, 1)
    c = P.put_cells("range", 0x1003, 0x2009, 7)
    assert (c.head, c.capped, c.n16, c.tail) == (7, True, 0, 0)
    assert [(P.put_cells("range", 0, 0, 16 * n).unrolled, P.put_cells("range", 0, 0, 16 * n).remainder)
            for n in (192, 193, 255, 256, 257)] == [(0, 3), (1, 3), (1, 3), (1, 0), (1, 1)]
    c = P.put_cells("through", 0x1009, 30, 0x5008)  # body to 0x1020, 7 trailing bytes
    assert (c.cls, c.src16, c.body, c.lead, c.t, c.delta) == (0, 9, True, 9, 7, 15)
    c = P.put_cells("through", 0x1009, 5, 0x5009)  # no 16-B boundary inside: all trailing
    assert (c.body, c.lead, c.t, c.delta) == (False, 0, 5, 0)
    assert [P.put_cells("through", 0, n, 0).cls for n in (0, 1, 256, 257, 1025, 4097, 16384, 16385)] == \
        [None, 0, 0, 1, 2, 3, 3, None]
    assert P.snap_cut(0x1009, 100, 5) == 7 and P.snap_cut(0x1009, 100, 99) == 100
    assert P.sweep_share(1 << 20, 64) == 16384 and P.sweep_share(1 << 30, 64) == 1 << 20
    # a 10,000-byte job after 3,000 cost units: cut where 4,096 and 8,192 fall inside it
    assert [(d, s, n) for d, s, n, _ in P.gather_ranges([(0, 0, 952), (100, 200, 10000)])] == \
        [(0, 0, 952), (100, 200, 1096), (1196, 1296, 4096), (5292, 5392, 4096), (9388, 9488, 712)]


# ---------------------------------------------------------------- the stream lattice
def test_stream_probes_sit_where_they_were_asked(stream, probed, ambry):
    from ambry_amd.messages import layout

    specs = P.stream_specs()
    assert len(specs) == len(stream.msgs)
    for i, ((kind, seg, v, _, _, _, _, place), (k2, c)) in enumerate(zip(specs, probed)):
        m = stream.msgs[i]
        assert kind == k2 and m.header_version == v
        if place[0] == "phase":
            assert c.phase == place[1]
        elif place[0] == "next":
            assert stream.out_off[i] == stream.out_off[i - 1] + stream.length[i - 1]
        else:
            assert c.m63 == place[1]
            if place[0] == "span":
                assert c.span == place[2]
            if place[0] == "len":
                assert stream.length[i] == place[2]
    # the restated layout against the oracle's header and against the library's own
    for i in range(0, len(stream.msgs), 7):
        e = P.expected_bytes(stream.msgs[i])
        v, total, rel = MF.parse_header(e, 0)
        lo = stream.lo[i]
        assert len(e) == stream.length[i] and lo[0] == MF.HEADER_SIZE[v]
        assert (rel[1] + 2, rel[3] + 6, rel[4] + 13) == (lo[2], lo[3], lo[4])
        assert (rel[0] == MF.INVALID and lo[1] == stream.hi[i, 0]) or rel[0] + 6 == lo[1]
        n, fo = layout(stream.msgs[i])
        assert n == stream.length[i] and [fo[s] for s in ("key", "props", "usermeta", "blob")] == [lo[0], lo[2], lo[3], lo[4]]
    ends = stream.out_off + stream.length
    assert (stream.out_off[1:] >= ends[:-1]).all() and stream.total == ends[-1] + 16


def test_stream_sources_are_nonzero_and_placed(stream):
    for i, m in enumerate(stream.msgs):
        for k, name in enumerate(P.SEGMENTS):
            b = getattr(m, name) or b""
            buf = stream.blobs if k == P.BLOB else stream.fields
            s = int(stream.src[i, k])
            assert buf[s:s + len(b)].tobytes() == b
            assert k == P.PROPS or all(b)
    assert P.SRC_PAD != 0 and (stream.fields == P.SRC_PAD).any() and (stream.blobs == P.SRC_PAD).any()
    img = stream.image
    inside = np.zeros(stream.total, dtype=bool)
    for o, n in zip(stream.out_off.tolist(), stream.length.tolist()):
        inside[o:o + n] = True
    assert (img[~inside] == P.FILL).all() and (~inside).sum() > 1000


def test_stream_every_phase_meets_every_length(probed):
    for seg_kind, seg in (("usermeta", P.UM), ("blob", P.BLOB)):
        hit = {(c.phase, c.length) for (k, c), (_, s, *_) in zip(probed, P.stream_specs()) if k == "phase" and s == seg}
        assert hit == set(itertools.product(range(16), P.PHASE_LENGTHS)), seg_kind
    phase = [c for k, c in probed if k == "phase"]
    assert {(c.head, c.inside_class) for c in phase} >= set(itertools.product(range(16), (0, 1, 2)))
    assert {(c.tail, c.inside_class) for c in phase} >= set(itertools.product(range(16), (0, 1, 2)))
    assert {(c.head, c.tail) for c in phase if c.inside} == set(itertools.product(range(16), range(16)))
    assert {(c.head, c.tail) for c in phase if c.straddle} == set(itertools.product(range(1, 16), range(1, 16)))
    assert {(c.phase, c.length) for c in phase if c.within} == \
        {(p, n) for p in range(16) for n in range(1, 16) if p + n <= 16}
    assert {c.src16 for c in phase} == set(range(16)) and {c.length for c in phase if c.length == 0} == {0}


def test_stream_repeats_at_every_run_residue_and_source_residue(probed):
    rep = [c for k, c in probed if k == "repeat"]
    assert {(c.m63, c.src16) for c in rep} == set(itertools.product(range(64), range(16)))
    assert {c.length for c in rep} == set(P.REPEAT_LENGTHS)
    for n in P.REPEAT_LENGTHS:
        assert {c.mis for c in rep if c.length == n} == set(range(16)), n
    assert {c.m63 for _, c in probed} == set(range(64))


def test_stream_key_and_encryption_key_segments(stream, probed):
    key = [c for k, c in probed if k == "key"]
    assert {(c.phase, c.length) for c in key} == set(itertools.product(range(16), P.KEY_LENGTHS))
    enc = [(i, c) for i, (k, c) in enumerate(probed) if k == "enckey"]
    present = {(c.phase, c.length) for i, c in enc if stream.msgs[i].enckey is not None}
    assert present == set(itertools.product(range(16), range(0, 18)))
    absent = [c for i, c in enc if stream.msgs[i].enckey is None]
    assert {c.phase for c in absent} == set(range(16)) and {c.length for c in absent} == {0}
    for i, c in enc:  # an absent key is the empty segment at the key's end; one of length 0 has its record
        gap = stream.lo[i, 1] - stream.hi[i, 0]
        assert gap == (0 if stream.msgs[i].enckey is None else 6)
        assert stream.lo[i, 2] - stream.hi[i, 1] == (2 if stream.msgs[i].enckey is None else 8 + 2)


def test_stream_run_counts_and_the_length_cut(stream, probed):
    span = [c for k, c in probed if k == "span"]
    assert {(c.m63, c.span) for c in span} == set(itertools.product(P.EDGE_M63, P.SPAN_EDGES))
    assert {(c.span, c.nruns, c.two_sb) for c in span} == {(4095, 64, False), (4096, 64, False), (4097, 65, True)}
    ln = [(i, c) for i, (k, c) in enumerate(probed) if k == "length"]
    assert {(c.m63, int(stream.length[i])) for i, c in ln} == set(itertools.product(P.EDGE_M63, P.LENGTH_EDGES))
    assert {(int(stream.length[i]), c.streamed) for i, c in ln} == {(6143, True), (6144, True), (6145, False)}
    assert sorted(np.nonzero(stream.length > P.STREAM_MAX)[0].tolist()) == [i for i, c in ln if not c.streamed]
    assert (stream.length > P.STREAM_MAX).sum() == 3  # the job path and clear_short run beside the streamed form
    assert max(c.nruns for _, c in probed if c.streamed) == 97
    assert 5 * len(stream.msgs) >= P.GROUP_MIN_JOBS  # with streaming off, the job path's group phase takes them


def test_stream_versions_neighbours_and_filler(stream, probed):
    for kind in ("phase", "repeat", "key", "span", "length", "packed"):
        assert {stream.msgs[i].header_version for i, (k, _) in enumerate(probed) if k == kind} == {1, 2, 3}, kind
    assert {stream.msgs[i].header_version for i, (k, _) in enumerate(probed) if k == "enckey"} == {2, 3}
    ends = stream.out_off + stream.length
    gap = stream.out_off[1:] - ends[:-1]
    assert (gap == 0).sum() >= P.BACK_TO_BACK and set(range(16)) <= set(gap.tolist()) and gap.max() >= 48
    touching = np.nonzero(gap == 0)[0]
    assert ((ends[touching] & 15) != 0).sum() >= 100  # neighbours that share a 16-B piece
    assert ((ends[touching] & 63) != 0).sum() >= 100  # ... and a 64-B run
    assert {int(e) & 15 for e in ends[touching]} == set(range(16))


# ---------------------------------------------------------------- the stream kernel's partition rule
@pytest.mark.parametrize("mis", range(16))
def test_stream_partition_writes_every_segment_byte_once(mis):
    """kernel_model's restatement of put_stream_kernel's stores: the inside pieces of stream_piece_src and the 32
    edge slots write every byte of the segment exactly once and nothing else, for every lo 0..63 and length
    0..128 at this destination phase, the segment in table slot 0, 2 and 4 (the others empty, before and after
    it), the message starting in each quarter of a 64-B run."""
    lens = np.arange(129)
    for lo in range(64):
        for slot in (0, 2, 4):
            los = np.zeros((len(lens), 5), dtype=np.int64)
            his = np.zeros((len(lens), 5), dtype=np.int64)
            los[:, slot], his[:, slot] = lo, lo + lens
            los[:, slot + 1:] = his[:, slot + 1:] = (lo + lens + 8)[:, None]
            m0 = np.full(len(lens), mis + 16 * (lo % 4), dtype=np.int64)
            count, owner = KM.stream_store_counts(m0, los, his, 64 + 128 + 64)
            x = np.arange(-64, 64 + 128 + 64)[None, :]
            want = (x >= lo) & (x < (lo + lens)[:, None])
            assert np.array_equal(count, want.astype(np.int32)), (mis, lo, slot)
            assert np.array_equal(owner, np.where(want, slot, -1)), (mis, lo, slot)


def test_stream_partition_over_the_lattice(stream):
    """The same rule over every segment of every streamed lattice message, at output shifts 0 and 37: each data
    byte written once by its own segment, no gap byte and no byte outside the message written."""
    sel = np.nonzero(stream.length <= P.STREAM_MAX)[0]
    for shift in (0, 37):
        for c0 in range(0, len(sel), 256):
            ix = sel[c0:c0 + 256]
            width = int(stream.length[ix].max()) + 64
            count, owner = KM.stream_store_counts(shift + stream.out_off[ix], stream.lo[ix], stream.hi[ix], width)
            want = np.full(count.shape, -1, dtype=np.int8)
            x = np.arange(-64, width)[None, :]
            for k in range(5):
                want[(x >= stream.lo[ix, k:k + 1]) & (x < stream.hi[ix, k:k + 1])] = k
            bad = np.nonzero((count != (want >= 0)) | (owner != want))
            assert len(bad[0]) == 0, (shift, int(ix[bad[0][0]]), int(bad[1][0]) - 64)


def test_stream_partition_agrees_with_put_cells(stream):
    """The two restatements (put_cells: counts; kernel_model: slots) agree on every lattice segment."""
    for i in range(0, len(stream.msgs), 3):
        if stream.length[i] > P.STREAM_MAX:
            continue
        for k in range(5):
            c = P.segment_cells(stream, i, k)
            e, live = KM.stream_edge_slots(c.mis, stream.lo[i, k], stream.hi[i, k])
            assert (int(live[:16].sum()), int(live[16:].sum())) == (c.head, c.tail), (i, k)
            dd = -(c.m63) + 16 * np.arange(KM.STREAM_PIECES)
            seg = KM.stream_piece_segment(stream.lo[i], stream.hi[i], dd)
            assert int((seg == k).sum()) == (c.inside if c.length else 0), (i, k)


# ---------------------------------------------------------------- copy_range
def _check_range(mem, dst, src, n):
    r = KM.copy_range_model(dst, src, n, mem)
    c = P.range_cells(dst, src, n)
    assert (r.head[2], r.n16, r.shift if r.n16 else c.shift, r.tail[2]) == (c.head, c.n16, c.shift, c.tail)
    assert sorted(r.out) == list(range(dst, dst + n)), (dst, src, n)  # every byte once, nothing outside
    assert bytes(r.out[a] for a in range(dst, dst + n)) == mem[src:src + n], (dst, src, n)
    lo16, hi16 = src & ~15, (src + n + 15) & ~15
    assert all(lo16 <= a and a + 16 <= hi16 for a in r.loads), (dst, src, n)  # copy_pieces' claim
    assert all(d % 16 == 0 for d, _, _ in r.pieces)
    assert all((b is None) == (c.shift == 0) for _, _, b in r.pieces)


def test_copy_range_model_every_residue_and_length():
    mem = G.nonzero_bytes(3, 8192)
    for d16 in range(16):
        for s16 in range(16):
            for n in itertools.chain(range(0, 81), (255, 256, 257)):
                _check_range(mem, 0x1000 + d16, 64 + s16, n)
    for d16, s16 in ((0, 0), (0, 5), (9, 0), (15, 1), (1, 15), (7, 7)):
        for n in (4095, 4096, 4097, 4111):
            _check_range(mem, 0x2000 + d16, 128 + s16, n)


# ---------------------------------------------------------------- the copy lattices
@pytest.mark.parametrize("jobs", ["wave", "group"])
def test_copy_lattice_coverage(jobs):
    lat = P.copy_lattice(jobs)
    m = len(lat.msgs)
    assert (5 * m < P.GROUP_MIN_JOBS) == (jobs == "wave") and lat.small_max == (0 if jobs == "wave" else 16384)
    cells = [(lat.kind[i], int(lat.probe[i]), P.job_through_cells(lat, i, int(lat.probe[i]))) for i in range(m)]
    c0 = [(s, c) for k, s, c in cells if k == "class0"]
    assert {(c.src16, c.length) for _, c in c0} == set(itertools.product(range(16), P.CLASS0_LENGTHS))
    assert {c.delta for _, c in c0} == set(P.DELTAS) and {s for s, _ in c0} == {P.UM, P.BLOB}
    if jobs == "group":
        assert {(c.src16, c.length, c.delta) for _, c in c0} == \
            set(itertools.product(range(16), P.CLASS0_LENGTHS, P.DELTAS))
    assert {c.lead for _, c in c0 if c.body} == set(range(16)) and {c.t for _, c in c0} == set(range(16))
    assert {(c.src16, c.length) for _, c in c0 if not c.body} >= {(r, n) for r in range(1, 16) for n in range(1, 16 - r)}
    cut = [(s, c) for k, s, c in cells if k == "cut"]
    assert {(c.src64, c.length) for _, c in cut} == set(itertools.product(range(64), G.CUT_LENGTHS))
    assert {c.cls for _, c in cut} == {0, 1, 2, 3, None} and {c.delta for _, c in cut} == set(P.DELTAS)
    for cls in (1, 2, 3):
        assert {c.src64 for _, c in cut if c.cls == cls} == set(range(64)), cls
        assert {s for s, c in cut if c.cls == cls} == {P.UM, P.BLOB}, cls
    big = [c for k, _, c in cells if k == "big"]
    assert {(c.src64, c.length) for c in big} == set(itertools.product(P.BIG_RES, P.BIG_BLOBS))
    assert {c.delta for c in big} == set(P.DELTAS)
    for i in range(m):  # the wanted delta really is the distance between the two 64-aligned buffers' bytes
        k = int(lat.probe[i])
        assert (lat.out_off[i] + lat.lo[i, k] - lat.src[i, k]) % 16 == cells[i][2].delta
    assert {lat.msgs[i].header_version for i in range(m)} == {1, 2, 3}


@pytest.mark.parametrize("jobs", ["wave", "group"])
def test_copy_lattice_share_cuts(jobs):
    """At lat.grid workgroups the sweep's share is its minimum, 16 KiB, and a share boundary falls 5 bytes into
    the first target blob, 5 bytes before the end of the second (snapped to the last 16-B boundary inside it, so
    the next wave's segment is the blob's trailing 3 bytes alone) and in the third's mid-body. In-place slots
    leave the job lengths, and so the raw cuts, as they are."""
    lat = P.copy_lattice(jobs)
    m = len(lat.msgs)
    lens = lat.job_len.tolist()
    assert len(lens) == 5 * m
    assert P.sweep_share(sum(n for n in lens if n > lat.small_max), lat.grid) == P.MIN_SHARE
    cuts = P.sweep_cuts(lens, lat.small_max, lat.grid)
    n = P.CUT_TARGET
    src = {w: int(lat.src[i, P.BLOB]) for w, i in lat.cut.items()}
    r = {w: cuts[4 * m + i] for w, i in lat.cut.items()}
    assert r["first16"][0] == 5 and P.snap_cut(src["first16"], n, 5) == 16 - src["first16"] % 16
    assert r["last16"][-1] == n - 5 and P.snap_cut(src["last16"], n, n - 5) == n - 3
    assert (src["last16"] + n) % 16 == 3
    assert 16 < r["mid"][1] == 20000 < n - 16 and P.snap_cut(src["mid"], n, 20000) % 16 == (-src["mid"]) % 16
    # every big blob is cut many times, at both sizes
    for i in np.nonzero(np.asarray(lat.kind) == "big")[0].tolist():
        assert len(cuts[4 * m + i]) >= 3


def test_copy_through_cells_not_reached_by_serialize():
    """kCopySkip (a job hashed and not stored) has no serialize form: put_layout_kernel gives every job of a
    copy-through batch a destination (cp_dst = out_off + field offset). Send reaches it: under BLOB every record
    but the blob's is hashed only, which the send test over the stored lattice runs."""
    import send_oracle as SO

    lat = P.stored_lattice()
    st, info, packed = P.send_expected(SO.BLOB)
    assert not any(st) and int(info["send_len"].sum()) == len(packed) < len(lat.region) // 2 + P.STORED_BIG


# ---------------------------------------------------------------- the library's CPU serializer
@pytest.mark.parametrize("which", ["stream", "wave", "group"])
def test_serialize_host_over_the_lattices(ambry, which):
    from ambry_amd.messages import serialize_host

    lat = P.stream_lattice() if which == "stream" else P.copy_lattice(which)
    step = 1 if which != "group" else 3  # the group lattice repeats the wave lattice's fields at more deltas
    for i in range(0, len(lat.msgs), step):
        m = lat.msgs[i]
        out, _ = serialize_host(m)
        o, n = int(lat.out_off[i]), int(lat.length[i])
        assert out == lat.image[o:o + n].tobytes(), (i, lat.kind[i])
        if n < 70000:
            assert MF.verify_message(out, 0) == (0, n), i


# ---------------------------------------------------------------- the stored lattice
def test_stored_lattice_is_clean_and_placed():
    lat = P.stored_lattice()
    ends = np.append(lat.offs[1:], len(lat.region))
    for i, o in enumerate(lat.offs.tolist()):
        assert MF.verify_message(lat.region, o) == (0, int(ends[i])), i
    pr = lat.probe
    assert not pr[0::2].any() and pr[1::2].all()
    spec = {(int(n), int(s) % 16) for n, s in zip(lat.blob_len[pr], lat.blob_src[pr])}
    assert spec >= set(itertools.product(P.STORED_LENGTHS, range(16))) and (P.STORED_BIG, 5) in spec
    reg = np.frombuffer(lat.region, dtype=np.uint8)
    assert all(reg[s:s + n].all() for s, n in zip(lat.blob_src.tolist(), lat.blob_len.tolist()))
    hv = [MF.parse_header(lat.region, o)[0] for o in lat.offs.tolist()]
    sv = [MF._be16(lat.region, o + MF.parse_header(lat.region, o)[2][1] + 2) for o in lat.offs.tolist()]
    bv = [MF._be16(lat.region, o + MF.parse_header(lat.region, o)[2][4]) for o in lat.offs.tolist()]
    assert set(itertools.product((1, 2, 3), (1, 2, 3, 4, 5))) == set(zip(hv, sv)) and set(bv) == {1, 2, 3}
    # not the fast path's batch: it takes header V3 with canonical VERSION_5 properties only
    assert sum(1 for h, s in zip(hv, sv) if h != 3 or s != 5) > len(hv) // 2


def test_stored_lattice_oracles():
    import send_oracle as SO

    lat = P.stored_lattice()
    m = len(lat.offs)
    st, off, ln, packed = P.transform_expected()
    assert not st.any() and off[0] == 0 and np.array_equal(off[1:], np.cumsum(ln)[:-1]) and ln.sum() == len(packed)
    grow = ln - np.diff(np.append(lat.offs, len(lat.region)))
    assert set(grow.tolist()) >= {0, 6, 17, 26} and len(set(grow.tolist())) >= 16  # dst - src steps by many amounts
    st2, off2, ln2, packed2 = P.transform_expected(True)
    bad = int(np.nonzero(lat.probe)[0][P.CORRUPT_PROBE])
    assert np.nonzero(st2)[0].tolist() == [bad] and st2[bad] == MF.BLOB_CRC and off2[bad] == -1
    assert len(packed2) == len(packed) - ln[bad]
    rst, roff, rln, rpacked = P.rekey_expected()
    assert rst == [0] * m and sum(rln) == len(rpacked)
    assert {o % 16 for o in roff} == set(range(16))
    for flag in (SO.BLOB, SO.ALL, SO.BLOB_INFO):
        s, info, body = P.send_expected(flag)
        assert s == [0] * m and not info["check"].any() and int(info["send_len"].sum()) == len(body)
    assert P.send_expected(SO.ALL)[2] == lat.region


def test_stored_lattice_cpu_entries(ambry):
    """The library's CPU transform and re-key over the stored lattice (the CPU leg of both)."""
    from ambry_amd import messages as M

    lat = P.stored_lattice()
    reg = np.frombuffer(lat.region, dtype=np.uint8)
    st, off, ln, packed = P.transform_expected()
    descs, aux = P.rekey_inputs()
    ax = np.frombuffer(aux, dtype=np.uint8)
    _, roff, rln, rpacked = P.rekey_expected()
    for i, o in enumerate(lat.offs.tolist()):
        s, b = M.transform_message_cpu(reg, o, header_version=3, life=i % 7)
        assert s == 0 and b == packed[off[i]:off[i] + ln[i]], i
        s, b = M.rekey_message_cpu(reg, o, descs[i], ax, header_version=3)
        assert s == 0 and b == rpacked[roff[i]:roff[i] + rln[i]], i


GATHER_WAVES = 256 * 8 * 4  # gather_copy_kernel's grid on an MI355X: 8 workgroups of 4 waves a CU, 256 CUs


def test_gather_copy_coverage():
    """copy_range's cells over the re-key's jobs, cut at the waves' cost shares: every head count, every shift,
    r = 0 and r != 0 under each Q, both loops, every tail count, n16 at the unrolled loop's bounds."""
    jobs = P.rekey_jobs()
    assert P.gather_cost(jobs) <= P.GATHER_MIN_SHARE * GATHER_WAVES  # so S is 4,096
    ranges = P.gather_ranges(jobs)
    assert sum(n for _, _, n, _ in ranges) == sum(n for _, _, n in jobs)
    cells = [P.range_cells(d, s, n) for d, s, n, _ in ranges]
    pieces = [c for c in cells if c.n16]
    assert {c.head for c in cells} == set(range(16)) and {c.head for c in pieces} == set(range(16))
    assert {c.shift for c in pieces} == set(range(16))
    assert {(c.Q, c.r == 0) for c in pieces} == set(itertools.product(range(4), (False, True)))
    assert {c.tail for c in cells} == set(range(16)) and {c.tail for c in pieces} == set(range(16))
    assert any(c.capped for c in cells) and any(c.n16 == 0 and c.tail for c in cells)
    assert any(c.unrolled for c in pieces) and any(c.remainder and not c.unrolled for c in pieces)
    assert any(c.unrolled and c.remainder for c in pieces)
    whole = [P.range_cells(d, s, n) for d, s, n in jobs if n]
    assert {c.n16 for c in whole} >= {0, 1, 2, 3, 255, 256}  # the job lengths, before the share cuts
    cut_jobs = {j for _, _, _, j in ranges}
    assert len(ranges) - len(cut_jobs) >= 70  # the 300,000-byte blob is cut at every 4,096 cost units
    assert {255, 256} <= {c.n16 for c in pieces} and max(c.n16 for c in pieces) == 256  # a share is 4,096 B
    # the content's source residues, as the spacers steered them
    lat = P.stored_lattice()
    content = jobs[3 * len(lat.offs):]
    assert {(n, s % 16) for (_, s, n), p in zip(content, lat.probe) if p} >= \
        set(itertools.product(P.STORED_LENGTHS, range(16)))


def test_gather_copy_pairings():
    """Which (head, shift) pairings the re-key's ranges miss. With pieces the head runs to the boundary, so
    shift = (src + head) & 15 = (src - dst) & 15: the pairing is (destination residue, the job's delta), and a
    cut keeps its job's delta. Nothing ties the two, so none is unreachable in principle; the lattice reaches
    nearly all of them, and the test pins how many it does not (singles are asserted in
    test_gather_copy_coverage)."""
    ranges = P.gather_ranges(P.rekey_jobs())
    missing = P.missing_pairings(ranges)
    assert len(missing) <= 2, sorted(missing)


# ---------------------------------------------------------------- the comparison helper
def test_compare_image_names_the_byte_and_its_cell(stream):
    assert P.compare_image(stream, stream.image.copy()) is None
    i = next(i for i in range(len(stream.msgs)) if stream.kind[i] == "phase" and stream.probe[i] == P.BLOB
             and P.segment_cells(stream, i, P.BLOB).head == 5 and P.segment_cells(stream, i, P.BLOB).tail == 9
             and P.segment_cells(stream, i, P.BLOB).inside == 1)
    c = P.segment_cells(stream, i, P.BLOB)
    o, lo, hi = int(stream.out_off[i]), int(stream.lo[i, P.BLOB]), int(stream.hi[i, P.BLOB])
    before = int(stream.out_off[i - 1] + stream.length[i - 1])
    assert before < o  # filler in front of it
    cases = {"head edge": (o + lo + 2, "blob"), "tail edge": (o + hi - 1, "blob"),
             "inside piece": (o + c.up, "blob"), "filler": (o - 1, "filler next to message %d" % i)}
    for what, (at, word) in cases.items():
        got = stream.image.copy()
        got[at] ^= 0x01
        msg = P.compare_image(stream, got)
        assert msg is not None and "first byte %d:" % at in msg and word in msg, (what, msg)
        assert ("message %d " % i in msg) and "'head': 5" in msg and "'tail': 9" in msg and "'mis': %d" % c.mis in msg, msg
    wave = P.copy_lattice("wave")
    j = wave.cut["last16"]
    at = int(wave.out_off[j] + wave.hi[j, P.BLOB]) - 1  # the last of the 3 bytes the next wave stores
    got = wave.image.copy()
    got[at] = 0
    msg = P.compare_image(wave, got, form="through")
    assert "first byte %d:" % at in msg and "message %d (target)" % j in msg and "'t': 3" in msg, msg


def test_describe_packed_names_the_record():
    """The packed outputs' failure text: a byte of a probe's placed blob record maps back to that message's
    blob record and the cells of its copy, under the transform, the re-key and send."""
    import send_oracle as SO

    lat = P.stored_lattice()
    i = int(np.nonzero(lat.probe & (lat.blob_len == 33))[0][3])
    off = int(lat.offs[i])
    _, total, rel = MF.parse_header(lat.region, off)
    span = next(r for r in rel if r != MF.INVALID) + total - 8 - rel[4]
    for what, placed, flag in (("transform", P.transform_expected()[1], 0), ("rekey", P.rekey_expected()[1], 0),
                               ("send", P.send_expected(SO.BLOB)[1]["out_off"], SO.BLOB),
                               ("send", P.send_expected(SO.ALL)[1]["out_off"], SO.ALL)):
        out_len = {"transform": P.transform_expected()[2], "rekey": P.rekey_expected()[2]}.get(
            what, P.send_expected(flag)[1]["send_len"])
        at = int(placed[i]) + int(out_len[i]) - 9  # the blob content's last byte, before the record's CRC
        msg = P.describe_packed(what, at, flag)
        assert msg.startswith("message %d," % i) and "blob record" in msg, (what, msg)
        assert "'src16': %d" % ((off + rel[4]) & 15) in msg, (what, msg)
        if what == "send":
            assert "'length': %d" % span in msg, msg
