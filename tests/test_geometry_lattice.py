"""The geometry lattices (geometry_lattice.py) on the CPU: that they hit every cell of the kernels' case split, by
construction and asserted through cells(); that they are eligible for the forms the GPU tests ask for; what the
oracle says of them; and the library's CPU entries over them (ambrycrc_verify_message_cpu, ambrycrc_batch_cpu:
the CLMUL host loop at every alignment and length)."""
import itertools
import zlib

import numpy as np
import pytest

import geometry_lattice as G
from msgfmt import MF


@pytest.fixture(scope="module")
def probed():
    """cells() of every probe's probed span, with its kind."""
    lat = G.message_lattice()
    idx = np.nonzero(lat.probe)[0]
    return [(lat.kind[i], G.cells(int(lat.rec_pa[i]), int(lat.rec_len[i]))) for i in idx]


# ---------------------------------------------------------------- cells() itself
def test_cells_restates_the_split():
    c = G.cells(61, 6)  # three bytes in the head run, three in the tail run
    assert (c.lo, c.n, c.tin, c.tail_bytes, c.ng, c.rb, c.d, c.sh, c.R, c.V) == (61, 2, 3, True, 1, -2, 61, 3, 1, 1)
    assert not c.long and c.pieces == 1 and c.last_piece == 6 and c.cls == 0 and not c.bytewise
    c = G.cells(64 * 5, 64 * 512)  # on the grid at both ends, the most runs one lane takes
    assert (c.lo, c.n, c.tin, c.tail_bytes, c.ng, c.rb, c.d, c.prefetch) == (0, 512, 64, False, 128, 0, 0, True)
    assert not c.long and c.cls is None and (c.R, c.V) == (512, 8)
    c = G.cells(1, 64 * 512)
    assert c.n == 513 and c.long and c.tail_bytes and c.d == 63
    c = G.cells(7, 64 * G.LONG_PIECE + 1)
    assert (c.pieces, c.last_piece, c.rounds) == (65, 1, 1)
    assert G.cells(7, 65 * G.LONG_PIECE + 1).rounds == 2
    assert [G.cells(0, n).cls for n in (0, 1, 256, 257, 1024, 1025, 4096, 4097, 16384, 16385)] == \
        [None, 0, 0, 1, 1, 2, 2, 3, 3, None]
    assert G.cells(9, 3).bytewise and G.cells(9, 4097).V == 2 and G.cells(9, 4096).V == 1


def test_probes_sit_where_they_were_asked(probed):
    """Every probe's span has the residue and length of its specification, and is the record the header names."""
    lat = G.message_lattice()
    specs = G.probe_specs()
    assert len(specs) == len(probed) == int(lat.probe.sum()) and len(lat.offs) == 2 * len(specs)
    assert not lat.probe[0::2].any() and lat.probe[1::2].all()  # spacer, probe, spacer, probe
    for (what, rec, lo, ln), (kind, c), i in zip(specs, probed, np.nonzero(lat.probe)[0]):
        assert (kind, c.lo, c.length) == (what, lo, ln)
        off = int(lat.offs[i])
        _, total, rel = MF.parse_header(lat.region, off)
        end = rel[rec + 1] if rec == 3 else rel[1] + total
        assert (off + rel[rec], off + end - 8) == (c.pa, c.pa + c.length)
    ends = np.append(lat.offs[1:], len(lat.region))
    assert lat.offs[0] == 0 and (np.diff(lat.offs) > 0).all()
    sp = ~lat.probe
    um = np.array([MF._be32(lat.region, int(o) + MF.parse_header(lat.region, int(o))[2][3] + 2) for o in lat.offs[sp]])
    assert um.min() >= 0 and um.max() <= 63 and len(set(um.tolist())) == 64  # the steering sizes
    assert int(ends[-1]) == len(lat.region)


def test_content_bytes_are_nonzero():
    lat = G.message_lattice()
    reg = np.frombuffer(lat.region, dtype=np.uint8)
    for off in lat.offs.tolist():  # every user-metadata and blob byte of every probe and spacer
        _, total, rel = MF.parse_header(lat.region, off)
        assert reg[off + rel[3] + 6:off + rel[4] - 8].all() and reg[off + rel[4] + 13:off + rel[1] + total - 8].all()
    assert G.chunk_lattice().mem.all()


def test_edge_region_reaches_below_the_first_block():
    """The direct form's lowest 16-B load for the first message's first span lies below lo16 at every tested
    shift (so the clamp moves it), its first run starts before the region, and no span's highest load lies past
    hi16: the clamp there is unreachable for a well-formed message."""
    e = G.edge_region()
    assert e.status[0] == 0 and (e.status != 0).sum() == 16 and e.end[-1] == len(e.region)
    assert (e.first_pa, e.first_len) == (43, 67)
    assert e.first_pa + e.first_len - 64 * G.cells(e.first_pa, e.first_len).R < 0
    for shift in G.EDGE_SHIFTS:
        assert G.low_load_below_region(shift, e.first_pa, e.first_len), shift
        reg0 = shift % 64
        hi16 = (reg0 + len(e.region) - 1) & ~15
        for off in e.offs.tolist():
            _, total, rel = MF.parse_header(e.region, off)
            starts = [r for r in rel if r != MF.INVALID] + [rel[1] + total]
            for s, t in zip(starts, starts[1:]):
                assert ((reg0 + off + t - 8) & ~15) <= hi16
    # the main lattice's first span does not reach below the region, which is why this region exists
    lat = G.message_lattice()
    _, _, rel = MF.parse_header(lat.region, 0)
    assert not G.low_load_below_region(0, rel[1], rel[3] - 8 - rel[1])


# ---------------------------------------------------------------- coverage
def test_every_head_residue_meets_every_unshift(probed):
    hit = {(c.lo, c.d) for _, c in probed}
    assert hit == set(itertools.product(range(64), range(64)))
    short = [c for k, c in probed if k == "short"]
    assert len(short) == 64 * 321 and {c.n for c in short} == set(range(1, 8))


def test_split_initial_register_at_every_lane(probed):
    """A head run of fewer than four record bytes (lanes 61..63, the record going on), at every un-shift."""
    for lo in (61, 62, 63):
        assert {c.d for _, c in probed if c.lo == lo and c.tin < 4} == set(range(64))
        assert {c.tin for _, c in probed if c.lo == lo} == {64 - lo}


def test_horner_groups(probed):
    """Every first-group padding with the tail run from the bytes and from its sum, in records of at most four
    groups (loaded before the loop) and of more (the prefetch inside it), and the group counts around both."""
    hit = {(c.rb, c.tail_bytes, c.prefetch) for _, c in probed if c.n >= 2 and not c.long}
    assert hit == set(itertools.product((-3, -2, -1, 0), (False, True), (False, True)))
    horner = [c for k, c in probed if k == "horner"]
    assert {c.ng for c in horner} >= {4, 5, 8, 9, 10}
    assert {(c.n, c.lo, c.d) for c in horner} == \
        set(itertools.product(G.HORNER_N, G.HORNER_LO, (0, 63, 1)))  # end residues 0, 1, 63
    for n in G.HORNER_N:
        assert {(c.rb, c.tail_bytes) for c in horner if c.n == n} == {(n - 4 * ((n + 3) // 4), False),
                                                                      (n - 4 * ((n + 3) // 4), True)}


def test_long_record_threshold(probed):
    for n in (511, 512, 513):
        assert {(c.tail_bytes, c.long) for _, c in probed if c.n == n} == {(False, n > 512), (True, n > 512)}
        assert {c.lo for _, c in probed if c.n == n} >= {0, 1, 63}
    assert {c.pieces for _, c in probed if c.n == 513} == {1}  # long spans of one piece


def test_pieces(probed):
    pieces = [c for k, c in probed if k == "pieces"]
    assert all(c.long for c in pieces)
    assert {c.pieces for c in pieces} == {1, 2, 3, 64, 65}
    assert {c.last_piece for c in pieces} == {1, 65535, 65536}
    assert {(c.pieces, c.last_piece) for c in pieces} == {(1, 65535), (1, 65536), (2, 1), (2, 65535), (2, 65536),
                                                          (3, 1), (64, 65535), (64, 65536), (65, 1)}
    assert {c.rounds for c in pieces} == {0, 1}  # 64 full pieces fill long_fold's round exactly
    assert {c.lo for c in pieces if c.last_piece == 1} == set(G.PIECE_LO)


def test_direct_form_shifts_and_rounds(probed):
    hit = {(c.sh, c.V) for _, c in probed}
    assert hit >= set(itertools.product(range(16), (1, 2)))
    assert {c.length for _, c in probed if c.V == 1} >= {4095, 4096}  # either side of the second round
    assert {c.length for _, c in probed if c.V == 2} >= {4097, 4098}


def test_class_cuts_at_every_residue(probed):
    for ln in G.CUT_LENGTHS:
        assert {c.lo for k, c in probed if k == "cut" and c.length == ln} == set(range(64)), ln
    assert {c.cls for k, c in probed if k == "cut"} == {0, 1, 2, 3, None}
    ch = G.chunk_lattice()
    cells = [G.cells(int(o), int(n)) for o, n in zip(ch.off, ch.length)]
    for ln in itertools.chain(range(0, 321), G.CUT_LENGTHS):
        assert {c.lo for c in cells if c.length == ln} == set(range(64)), ln
    assert {c.cls for c in cells} == {0, 1, 2, 3, None}


def test_flips_land_on_every_position():
    """One flipped bit per probe, inside its span, on each of the positions flip_position() names."""
    lat, bad = G.message_lattice(), G.flipped()
    a, b = np.frombuffer(lat.region, dtype=np.uint8), np.frombuffer(bad.region, dtype=np.uint8)
    diff = np.nonzero(a != b)[0]
    assert np.array_equal(diff, np.sort(bad.flip_at[lat.probe]))
    assert all(bin(int(x)).count("1") == 1 for x in (a[diff] ^ b[diff]))
    at, pa, ln = bad.flip_at[lat.probe], lat.rec_pa[lat.probe], lat.rec_len[lat.probe]
    assert ((at >= pa) & (at < pa + ln)).all() and (bad.flip_at[~lat.probe] == -1).all()
    rel = at - pa
    assert (rel == 0).sum() > 2000 and (rel == 3).sum() > 2000 and (rel == 4).sum() > 2000
    multi = ln > 64
    assert ((at[multi] & 63) == 63).sum() > 2000 and ((at[multi] & 63) == 0).sum() > 2000  # around a run boundary
    assert (rel == ln - 1).sum() > 2000
    assert (at == ((pa + ln - 1) & ~63))[multi].sum() > 2000  # the tail run's first byte
    long = ln > G.LONG_PIECE
    assert (rel[long] % G.LONG_PIECE == G.LONG_PIECE - 1).any() and (rel[long & (rel > 4)] % G.LONG_PIECE == 0).any()


# ---------------------------------------------------------------- eligibility
def test_lattices_are_eligible():
    lat = G.message_lattice()
    m = len(lat.offs)
    assert len(lat.region) <= 6144 * m  # region mode (kRegionMaxPerMessage)
    assert len(lat.region) <= 40960 * m  # the transform's fast path (kXformFastMaxPerMessage)
    assert 5 * m >= 16384  # CRC jobs: the group phase (kGroupMinChunks)
    n = len(G.chunk_lattice().off)
    assert n >= 16384 and (n + 1) // 2 <= 16383  # one batch in the group phase, two halves in wave mode
    assert len(G.trailed_lattice().off) == n


# ---------------------------------------------------------------- the oracle
def test_oracle_over_the_lattices():
    lat, bad = G.message_lattice(), G.flipped()
    st, end = G.verify_oracle("clean")
    ends = np.append(lat.offs[1:], len(lat.region))
    assert not st.any() and np.array_equal(end, ends)
    st, end = G.verify_oracle("flipped")
    assert np.array_equal(end, ends)
    assert not st[~lat.probe].any()
    # Exactly the probed record's CRC bit. A flip inside the bytes the record's deserializer reads as fields
    # (its version, sizes, blob type) may add what that reader says, BAD_VERSION or BAD_RECORD, and nothing else.
    assert np.array_equal(st[lat.probe] & G.CRC_BITS, lat.rec_bit[lat.probe])
    extra = st & ~np.uint32(G.CRC_BITS)
    fields = np.array([G.field_bytes(int(b)) for b in lat.rec_bit])
    in_fields = lat.probe & (bad.flip_at - lat.rec_pa < fields)
    assert not extra[~in_fields].any()
    assert not (extra & ~np.uint32(MF.BAD_VERSION | MF.BAD_RECORD)).any()
    assert (extra[in_fields] != 0).sum() > 2000 and (st[lat.probe] == lat.rec_bit[lat.probe]).sum() > 10000


# ---------------------------------------------------------------- the library's CPU entries
@pytest.mark.parametrize("which", ["clean", "flipped"])
def test_verify_message_cpu_over_the_lattice(ambry, which):
    from ambry_amd.messages import verify_message_cpu

    lat = G.message_lattice() if which == "clean" else G.flipped()
    reg = np.frombuffer(lat.region, dtype=np.uint8)
    st, end = G.verify_oracle(which)
    for i, o in enumerate(lat.offs.tolist()):
        got = verify_message_cpu(reg, o)
        if got != (int(st[i]), int(end[i])):
            raise AssertionError("message %d (%s): %s, expected %s; %s" % (
                i, lat.kind[i], got, (int(st[i]), int(end[i])), vars(G.cells(int(lat.rec_pa[i]), int(lat.rec_len[i])))))


@pytest.mark.parametrize("threads", [1, 3])
def test_batch_cpu_over_the_chunk_lattice(ambry, threads):
    from ambry_amd import device as D

    ch = G.chunk_lattice()
    mem = np.ascontiguousarray(ch.mem)
    base = mem.ctypes.data
    chunks = [(base + o, n) for o, n in zip(ch.off.tolist(), ch.length.tolist())]
    got = np.array(D.crc32_batch_cpu(chunks, crc_in=ch.crc_in.tolist(), threads=threads), dtype=np.uint32)
    exp = G.chunk_crcs(ch)
    if not np.array_equal(got, exp):
        i = int(np.nonzero(got != exp)[0][0])
        raise AssertionError("chunk %d: %#x, expected %#x; %s" % (
            i, got[i], exp[i], vars(G.cells(int(ch.off[i]), int(ch.length[i])))))
    assert (ch.crc_in == 0).sum() >= len(chunks) // 3 and (ch.crc_in != 0).sum() >= len(chunks) // 2


def test_trailed_lattice_keeps_the_residues():
    ch, tr = G.chunk_lattice(), G.trailed_lattice()
    assert np.array_equal(tr.off % 64, ch.off % 64) and np.array_equal(tr.length, ch.length + 8)
    assert (np.diff(tr.off) >= tr.length[:-1]).all() and int(tr.off[-1] + tr.length[-1]) == len(tr.mem)
    mem = tr.mem.tobytes()
    for i in range(0, len(tr.off), 61):
        o, n = int(tr.off[i]), int(tr.length[i])
        stored = int.from_bytes(mem[o + n - 8:o + n], "big")
        assert (zlib.crc32(mem[o:o + n - 8]) != stored) == bool(tr.bad[i])
    assert tr.bad.sum() == -(-len(tr.off) // 7)
    # the stored long's start falls on every residue of the run grid in every size class
    trailer = [G.cells(int(o + n - 8), 8).lo for o, n in zip(tr.off, tr.length)]
    for cls in (0, 1, 2, 3):
        assert {t for t, n in zip(trailer, ch.length) if G.cells(0, int(n)).cls == cls} == set(range(64))
