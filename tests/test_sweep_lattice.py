"""The sweep lattices (sweep_lattice.py) on the CPU: that the classifier's constants are the sources', that every
lattice hits every cell of crc32_sweep_kernel's case split by construction (a missing cell fails by name), that
each chunk's segments tile it, what cannot be reached and why, the CPU legs over the lattices, and that the
lattices are sensitive: one-line mutants of a plain restatement of the segment composition change a probe's CRC."""
import bisect
import itertools
import os
import re
import zlib

import numpy as np
import pytest

import sweep_lattice as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ambry_amd", "csrc")
LATTICES = [("wave", 16384), ("wave", 21504), ("wave", 24576), ("group", 16384)]
IDS = ["%s-%d" % ls for ls in LATTICES]
assert {S for _, S in LATTICES} == set(L.SHARES)


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def missing(want, hit, what):
    """Fails naming the cells of `want` that `hit` lacks."""
    lack = sorted(set(want) - set(hit), key=repr)
    assert not lack, "%s: %d cells not covered, first %s" % (what, len(lack), lack[:8])


@pytest.fixture(scope="module", params=LATTICES, ids=IDS)
def lw(request):
    """(the lattice, its walk, its segments by chunk)."""
    lat = L.sweep_lattice(*request.param)
    walk = L.lattice_walk(*request.param)
    return lat, walk, L.by_chunk(walk.segments)


def probes(lat, kind):
    return [(i, sp) for k, i, sp in lat.probes if k == kind]


def cut_of(lat, i, sp):
    return L.cut_cells(int(lat.off[i]), int(lat.length[i]), sp["r"])


# ---------------------------------------------------------------- the classifier against the sources
def test_constants_match_the_sources():
    kh, kern, lay = source("crc32_kernels.h"), source("crc32_kernels.hip"), source("crc32_layout.h")
    const = lambda text, name: int(re.search(r"constexpr \w+ %s = (\d+);" % name, text).group(1))  # noqa: E731
    assert const(kh, "kShareQuantum") == L.SHARE_QUANTUM and const(kh, "kMinShare") == L.MIN_SHARE
    assert const(kh, "kGroupMinChunks") == L.GROUP_MIN_CHUNKS and const(kh, "kGroupSmallMax") == L.GROUP_SMALL_MAX
    assert const(lay, "kBlockBytes") == L.BLOCK
    assert "constexpr uint64_t SB = 4 * (uint64_t)kBlockBytes;" in kern and L.SUPER_BLOCK == 4 * L.BLOCK
    # the sweep's instantiations: one super-block in flight, eight 1 KiB blocks in flight
    assert "body_crc_t4<1, true, true, COPY>(a.base, sa, be" in kern
    assert "body_crc<%d, true, DIAG>(a.base, sa, be" % L.PREFETCH_U in kern
    # 16 waves a workgroup, 64 descriptors a fetch
    assert "crc32_sweep_kernel<true, true>), dim3(grid), dim3(%d)" % (64 * L.WAVES) in kern
    assert "crc32_sweep_kernel<false, false>), dim3(grid), dim3(%d)" % (64 * L.WAVES) in kern
    assert "const uint32_t cnt = a.n - c < %du ? a.n - c : %du;" % (L.WINDOW, L.WINDOW) in kern
    assert const(kh, "kVariantPieces") == 0 and const(kh, "kVariantDefault") == 29


def test_classifier_restates_the_split():
    assert L.share_size(16 * 16384, 1) == (16384, 1) and L.share_size(16 * 16384 + 1, 1) == (17408, 1)
    assert L.share_size(5, 3) == (16384, 1)
    assert L.share_size(256 * 20000, 4, 64 * 20000) == (20480, 4)  # 4 rounds of 64 shares
    assert L.share_size(256 * 20000, 4, 256 * 20000) == (80896, 1)  # total == window: one round
    assert [L.snap_cut(3, 100, r) for r in (1, 13, 14, 29, 90, 99)] == [13, 13, 29, 29, 93, 100]
    c = L.cut_cells(3, 100, 5)
    assert (c.kind, c.a, c.rr, c.t, c.ce16) == ("first16", 8, 13, 7, False)
    assert L.cut_cells(3, 100, 98).kind == "last16" and L.cut_cells(3, 100, 93).kind == "mid"
    assert L.cut_cells(3, 109, 100).kind == "last16" and L.cut_cells(3, 109, 100).ce16  # rr == length exactly
    assert L.cut_cells(3, 100, 0).kind == "start"
    s = L._segment(5000 + 3, 9000, 0, 8189)  # from an unaligned start to an aligned cut: 8,189 body bytes
    assert (s.sa, s.be, s.body, s.nb, s.nb1k, s.path, s.lead, s.final) == (5003, 13192, 8189, 2, 8, "prime", 11, False)
    assert (s.sb_off, s.blk, s.lane) == (3, 0, 0) and not s.v0neg
    s = L._segment(3, 9000, 0, 4077)  # be = 4,080: one super-block, four blocks, both from 16 bytes below the buffer
    assert (s.nb, s.nb1k, s.sb_off) == (1, 4, 19) and s.v0neg and s.v0neg1k
    s = L._segment(64, 4096 + 16 + 5, 16, 4096 + 16 + 5)  # a last segment: 4,096 body bytes and 5 tail bytes
    assert (s.final, s.final_body, s.t, s.nb, s.tail_only, s.whole) == (True, 4096, 5, 1, False, False)
    s = L._segment(64, 37, 32, 37)
    assert (s.final_body, s.t, s.tail_only, s.body, s.nb) == (0, 5, True, 0, 0)
    assert L._segment(64, 37, 37, 37).empty
    assert [L._segment(0, 1 << 20, 0, n * 1024).path for n in (8, 9, 15, 16, 17, 23, 24)] == \
        ["prime", "drain-refill", "drain-refill", "roll-dry", "roll-refill", "roll-refill", "roll2"]


def test_walk_restates_find_start_and_the_jump():
    """Three span-0 chunks at a boundary, then a chunk: the share starts at the chunk. A share whose second
    descriptor window holds span-0 chunks only jumps to the run's end."""
    lens = [16384, 0, 0, 0, 16384] + [1] * 63 + [0] * 70 + [300]
    w = L.sweep_walk(lens, [64] * len(lens), 0, 1)
    assert w.S == 16384 and [x.c for x in w.windows if x.share == 1][0] == 4
    third = [x for x in w.windows if x.share == 2]
    assert [(x.c, x.work, x.jump, x.far) for x in third] == [(5, True, False, None), (69, False, True, 138), (138, True, False, None)]
    assert [s.chunk for s in w.segments if s.share == 2] == list(range(5, 68)) + [138]


# ---------------------------------------------------------------- the lattices are what they say
def test_every_data_byte_is_nonzero(lw):
    lat = lw[0]
    assert lat.mem.all() and lat.mem.size == L.BUFFER
    assert int(lat.off.min()) >= 0 and int((lat.off + lat.length).max()) <= L.BUFFER


def test_geometry_is_the_forms(lw):
    lat, walk, _ = lw
    n = len(lat.off)
    assert (n < L.GROUP_MIN_CHUNKS) == (lat.form == "wave") and lat.small_max == (0 if lat.form == "wave" else 16384)
    assert (walk.S, walk.R, walk.nwaves, walk.total) == (lat.S, 1, 16 * lat.grid, lat.total)
    assert lat.nwaves * (lat.S - 1024) < lat.total <= lat.nwaves * lat.S
    assert lat.total <= 32 << 20 and int(lat.length.sum()) <= 32 << 20
    if lat.form == "group":  # every probe and pad above 16 KiB, everything else the group phase's
        swept = np.array([k not in ("span0",) for k in lat.kind])
        assert (lat.length[swept] > L.GROUP_SMALL_MAX).all() and (lat.length[~swept] <= L.GROUP_SMALL_MAX).all()
        assert int((~swept).sum()) > 15000
    assert (lat.crc_in == 0).sum() > n // 8 and (lat.crc_in != 0).sum() > n // 2


def test_probes_sit_where_they_were_asked(lw):
    lat, walk, _ = lw
    for kind, i, sp in lat.probes:
        assert lat.kind[i] == kind and int(lat.off[i]) & 63 == sp["c64"] and int(lat.length[i]) == sp["length"]
        assert (int(lat.off[i]) < 64) == bool(sp.get("low"))
        if sp["r"] is not None and not sp.get("chain"):
            assert (walk.byte_start[i] + sp["r"]) % lat.S == 0, (kind, i)


def test_segments_tile_every_chunk(lw):
    """No gap, no overlap: a chunk that takes share bytes has segments from 0 to its length, each starting where
    the one before ended; an empty segment sits at the chunk's end only; a span-0 chunk has none."""
    lat, _, segs = lw
    walks = [segs] + ([L.by_chunk(L.lattice_walk(lat.form, lat.S, True).segments)] if lat.rounds and lat.form == "wave" else [])
    for by in walks:
        for i, ln in enumerate(lat.length.tolist()):
            if ln <= lat.small_max:
                assert i not in by
                continue
            at = 0
            for s in sorted(by[i], key=lambda s: (s.r0, s.r1)):
                assert s.r0 == at and (s.r1 > s.r0 or s.r0 == ln), (i, lat.kind[i], s.r0, s.r1, at)
                at = s.r1
            assert at == ln, (i, lat.kind[i])


# ---------------------------------------------------------------- coverage: the share cuts
def test_mid_cuts_at_every_residue(lw):
    lat, _, segs = lw
    hit = set()
    for i, sp in probes(lat, "mid"):
        c = cut_of(lat, i, sp)
        assert c.kind == "mid"
        hit.add((c.a, int(lat.off[i]) & 63))
        first, second = sorted(segs[i], key=lambda s: s.r0)[:2]
        assert first.r1 == second.r0 == c.rr and first.lead == int(lat.off[i]) & 15 and second.lead == 0
    missing(itertools.product(range(16), L.MID_START), hit, "mid cut (address residue, start residue)")


def test_first16_cuts(lw):
    """Every head length 1..16, from the cut one byte in and from the cut on the snapped place itself: the
    earlier wave's segment is that many bytes from the chunk's own start, one super-block whose virtual start
    lies 4 KiB - h before it."""
    lat, _, segs = lw
    hit = set()
    for i, sp in probes(lat, "first16"):
        c = cut_of(lat, i, sp)
        assert c.kind == "first16"
        head = min(segs[i], key=lambda s: s.r0)
        assert (head.r0, head.r1, head.body, head.nb, head.nb1k) == (0, c.rr, c.rr, 1, 1) and head.be == head.se
        assert head.sb_off == L.SUPER_BLOCK - c.rr and head.lead == (16 - c.rr) & 15
        hit.add((c.rr, sp["r"] == c.rr))
    missing([(h, ripe) for h in range(1, 17) for ripe in (False, True) if h > 1 or ripe], hit, "first16 (bytes, cut on the snap)")


def test_last16_cuts(lw):
    """The snap reaches the chunk's end: the earlier wave has the whole chunk (a plain store), the later an empty
    segment (it XORs 0). Every t = ce & 15 but 1: the raw cut must lie past floor16(ce) and before ce, and with
    t == 1 no byte does; there the cut one byte before the end is a mid cut whose last segment is the one tail
    byte, which test_final_segments covers."""
    lat, _, segs = lw
    hit = set()
    for i, sp in probes(lat, "last16"):
        c = cut_of(lat, i, sp)
        assert c.kind == "last16" and c.rr == int(lat.length[i])
        a, b = sorted(segs[i], key=lambda s: s.r0)[-2:]
        assert a.r1 == int(lat.length[i]) and not a.empty and a.whole == (lat.form == "wave")  # group form: cut before too
        assert b.empty and b.r0 == b.r1 == int(lat.length[i]) and b.share == a.share + 1
        hit.add((c.t, c.dist))
    want = [(0, 1), (0, 15)] + [(t, d) for t in range(2, 16) for d in {1, t - 1}]
    missing(want, hit, "last16 (t, bytes from the raw cut to the end)")
    assert {t == 0 for t, _ in hit} == {True, False}  # ce 16-aligned (rr == length) and not
    for cs in range(16):  # t == 1: no raw cut snaps to the end
        ln = 64 + (1 - cs) % 16
        assert (cs + ln) & 15 == 1 and all(L.cut_cells(cs, ln, ln - d).kind != "last16" for d in range(1, 16))


def test_boundary_on_a_chunk_start(lw):
    """r == 0: the share's first byte is the probe's first byte, with and without span-0 chunks at that stream
    position before the probe, and with the next boundary on the probe's end where span-0 chunks sit too. The
    share's walk starts at the probe: find_start lands on the chunk that holds the byte."""
    lat, walk, segs = lw
    hit = set()
    for i, sp in probes(lat, "start"):
        k = walk.byte_start[i] // lat.S
        assert walk.byte_start[i] == k * lat.S
        assert [x.c for x in walk.windows if x.share == k][0] == i
        head = min(segs[i], key=lambda s: s.r0)
        assert head.share == k and head.r0 == 0
        before = i > 0 and lat.kind[i - 1] == "span0"
        ends_on = walk.byte_start[i + 1] % lat.S == 0
        after = lat.kind[i + 1] == "span0"
        assert (before, ends_on and after) == (sp["form"] in ("before", "both"), sp["form"] in ("after", "both"))
        if ends_on:  # the next share starts at the pad behind the span-0 chunks
            nxt = [x.c for x in walk.windows if x.share == walk.byte_start[i + 1] // lat.S][0]
            assert nxt == i + 1 + len(sp["after"]) and lat.kind[nxt] == "pad"
        hit.add((sp["form"], int(lat.off[i]) & 15 != 0))
    missing(itertools.product(L.START_FORMS, (False, True)), hit, "start (form, unaligned)")


# ---------------------------------------------------------------- coverage: the segment bodies
def test_body_super_blocks(lw):
    """body_crc_t4<1>: nb = 1 (super-block 0 only), 2 (one turn of the tail loop), 3 and 4 (the pipelined loop,
    then its drain), 5 and more; where the body starts in super-block 0: every block, the first and last two
    lanes, and lead bytes that end the mask in dword 0 (1, 3), on its edge (4), in dword 1 (5) and in dword 3
    (15); a virtual start below the buffer."""
    lat, walk, _ = lw
    firsts = [s for s in walk.segments if not s.empty and s.first and not s.whole and lat.kind[s.chunk] == "head"]
    hit = {(s.nb, s.blk, s.lane, s.lead) for s in firsts}
    missing(itertools.product((1, 2, 3, 4), range(4), L.HEAD_LANES, L.HEAD_LEADS), hit, "head (nb, block, lane, lead)")
    assert {min(s.nb, 5) for s in walk.segments if not s.empty} == {0, 1, 2, 3, 4, 5}
    assert {(s.nb, s.lead != 0) for s in firsts if s.v0neg} >= set(itertools.product((1, 2, 3, 4), (False, True)))
    full = [s for s in walk.segments if not s.empty and s.body == lat.S and s.lead == 0 and not s.first and not s.final]
    assert full and {s.nb for s in full} == {-(-lat.S // 4096)} and {lat.kind[s.chunk] for s in full} >= {"long"}
    assert {s.sb_off for s in full} == {-lat.S % 4096}  # 21,504: a first super-block of 1 KiB


def test_body_pieces(lw):
    """body_crc<8> (variant 0) over the same segments: the prime alone, the drain with refills, one rolling
    iteration with a dry drain, one with refills. A second rolling iteration needs 24 blocks, a body above
    23 KiB; a segment lies inside one share plus the snap, so none exists at 16 KiB and 21 KiB shares, which the
    last line asserts; the 24 KiB lattice is there for it (a full share is 24 blocks, one from an unaligned start
    25)."""
    lat, walk, _ = lw
    n1k = {s.nb1k for s in walk.segments if not s.empty}
    missing(range(0, 17), n1k, "nb1k")
    paths = {s.path for s in walk.segments if not s.empty}
    missing(["prime", "drain-refill", "roll-dry", "roll-refill"], paths, "body_crc path")
    if lat.S > 16384:
        assert {lat.S // 1024, lat.S // 1024 + 1} <= n1k  # a full share, and one from an unaligned start
    else:
        assert 17 in n1k  # a share and the snap, from an unaligned start
    assert {s.lead for s in walk.segments if not s.empty and s.path == "roll-refill"} - {0}
    assert any(s.v0neg1k for s in walk.segments if not s.empty)
    assert ("roll2" in paths) == (lat.S == 24576) and max(n1k) == -(-(lat.S + 15) // 1024)
    assert lat.S < 24576 or {s.lead != 0 for s in walk.segments if not s.empty and s.path == "roll2"} == {False, True}


def test_final_segments(lw):
    """A chunk's last segment after a cut: cb - sa body bytes in {0, 16, 4080, 4096, 4112} at every t = ce & 15;
    at 0 the segment is the tail alone (sa == cb < ce). (0, 0) is no segment: that cut is a last16."""
    lat, walk, _ = lw
    finals = [s for s in walk.segments if not s.empty and s.final and not s.first and lat.kind[s.chunk] == "final"]
    hit = {(s.final_body, s.t) for s in finals}
    missing([(b, t) for b in L.FINAL_BODY for t in range(16) if b or t], hit, "final (body bytes, t)")
    assert all(s.tail_only == (s.final_body == 0) and s.sa == s.cb - s.final_body for s in finals)
    assert not any(s.final_body == 0 and s.t == 0 for s in walk.segments if not s.empty)
    # the kernel's t0 = sa > cb ? sa : cb always takes cb: a cut is 16-aligned and below ce, so sa <= cb
    assert all(s.sa <= s.cb for s in walk.segments if not s.empty and s.final)


def test_init_term_cases(lw):
    """The init term of a segment with r0 == 0: crc_in == 0 with the one-entry length cache hit and missed, and a
    seeded chunk between two cached ones (the cache must survive it). A hit needs two whole chunks of one length
    in one share; in group form every swept chunk is longer than the share, so none exists there."""
    lat, walk, _ = lw
    inits = {s.init for s in walk.segments if not s.empty and s.first}
    if lat.form == "group":
        assert inits == {"miss", "seeded"} and lat.S <= L.GROUP_SMALL_MAX
        return
    assert inits == {"hit", "miss", "seeded"}
    by_share = {}
    for s in walk.segments:
        if not s.empty and s.first:
            by_share.setdefault(s.share, []).append(s)
    found = 0
    for row in by_share.values():
        seq = [(s.init, s.length) for s in row]
        for q in range(len(seq) - 4):
            if [x for x, _ in seq[q:q + 5]] == ["miss", "hit", "seeded", "hit", "miss"] and len({n for _, n in seq[q:q + 4]}) == 1:
                found += 1
    assert found == 2  # the 70- and the 140-chunk share


# ---------------------------------------------------------------- coverage: the descriptor windows
def test_descriptor_windows(lw):
    """Shares of 70 and 140 whole chunks (two and three windows with work); runs of 63, 64, 65 and 200 span-0
    chunks inside a share, at a share boundary, at stream position 0 and after the last swept chunk.

    Inside a share in wave form the windows count from the anchor chunk, 63 short chunks fill the first, and the
    run starts the second: 63 leave it one chunk with work; 64 empty it and the jump lands on its own end (no
    chunk skipped); 65 skip one chunk; 200 skip 136. In group form nothing that takes share bytes fits between
    the anchor and the run (every such chunk is longer than the share), so the run starts in the anchor's window
    and only the run of 200 empties a window. A run at a boundary, at position 0 or behind the last swept chunk
    is never walked: the wave before it is done when its bytes end and find_start puts the wave behind it on the
    chunk that holds its first byte. Every empty chunk carries a nonzero crc_in and expects it back."""
    lat, walk, segs = lw
    wave = lat.form == "wave"
    whole = {}
    for s in walk.segments:
        if s.whole:
            whole[s.share] = whole.get(s.share, 0) + 1
    if wave:
        heads = [i for i, sp in probes(lat, "many") if not sp.get("chain")]
        shares = [walk.byte_start[i] // lat.S for i in heads]
        assert [walk.byte_start[i] % lat.S for i in heads] == [0, 0]
        assert [whole[k] for k in shares] == [71, 141]  # the chunks and the pad behind them: >= 65 and >= 129
        assert [sum(1 for x in walk.windows if x.share == k and x.work) for k in shares] == [2, 3]
    else:
        assert max(whole.values(), default=0) <= 1  # a swept chunk is longer than the share
    jumps = {x.c: x for x in walk.windows if x.jump}
    at = lat.run_at
    for n_run in L.RUN_LENGTHS:
        start = at[("inside", n_run)]
        assert all(lat.kind[i] == "span0" for i in range(start, start + n_run)) and lat.kind[start + n_run] == "run-after"
        anchor = start - (64 if wave else 1)
        assert lat.kind[anchor] == "run-inside"
        share = max(s.share for s in segs[anchor])
        assert [x.c for x in walk.windows if x.share == share][0] == anchor  # the windows count from the anchor
        assert min(s.share for s in segs[start + n_run]) == share  # the chunk behind the run starts in that share
        x = jumps.pop(anchor + 64, None)
        if wave:
            assert (x is not None) == (n_run >= 64), n_run
            assert x is None or (x.far, x.far - x.c - x.cnt) == (start + n_run, n_run - 64)
        else:
            assert (x is not None) == (n_run == 200) and (x is None or x.far == start + n_run)
        start = at[("boundary", n_run)]
        assert walk.byte_start[start] % lat.S == 0 and lat.kind[start + n_run] == "run-boundary"
        k = walk.byte_start[start] // lat.S
        assert [y.c for y in walk.windows if y.share == k][0] == start + n_run
        assert [y.done for y in walk.windows if y.share == k - 1][-1]
    assert not jumps  # no other window is empty
    assert at[("head", 65)] == 0 and walk.byte_start[65] == 0 and walk.windows[0].c == 65
    tail = at[("tail", 63)]
    assert walk.byte_start[tail] == lat.total and max(y.c + y.cnt for y in walk.windows if not y.done) <= tail
    empty = lat.length == 0
    assert empty.sum() >= 60 and (lat.crc_in[empty] != 0).all() and np.array_equal(lat.expect[empty], lat.crc_in[empty])


def test_rounds_geometry():
    """The 16 KiB wave lattice under rounds: a quarter of the workgroups and a window that makes four rounds of
    the same 16 KiB shares. The cuts k S are unchanged; wave w owns shares w, w + nwaves, ...; a probe crosses
    from a round's last share into the next round's first; the last round is part full; a wave's init cache
    lives across its rounds."""
    lat = L.sweep_lattice("wave", 16384)
    one, four = L.lattice_walk("wave", 16384), L.lattice_walk("wave", 16384, True)
    assert lat.grid % 4 == 0 and (four.S, four.R, four.nwaves) == (one.S, 4, one.nwaves // 4)
    key = lambda w: sorted((s.chunk, s.r0, s.r1, s.share) for s in w.segments)  # noqa: E731
    assert key(one) == key(four)
    assert all(s.wave == s.share % four.nwaves and s.round == s.share // four.nwaves for s in four.segments)
    by = L.by_chunk(four.segments)
    crossing = [i for _, i, _ in lat.probes
                if any(a.wave == four.nwaves - 1 and b.wave == 0 and b.round == a.round + 1 and not a.empty and not b.empty
                       for a in by[i] for b in by[i])]
    assert crossing, "no probe crosses from one round into the next"
    last = {s.wave for s in four.segments if s.round == 3}
    assert last and max(last) < four.nwaves - 1
    assert {s.round for s in four.segments} == {0, 1, 2, 3}


# ---------------------------------------------------------------- the CPU legs
@pytest.mark.parametrize("threads", [1, 3])
def test_cpu_legs_over_the_lattices(lw, oracle, ambry, threads):
    """The oracle's batch leg and the library's host batch entry over every lattice: both equal zlib."""
    from ambry_amd import device as D

    lat = lw[0]
    assert np.array_equal(oracle.batch(lat.mem, lat.off, lat.length, crc_in=lat.crc_in, threads=threads), lat.expect)
    mem = np.ascontiguousarray(lat.mem)
    chunks = [(mem.ctypes.data + o, n) for o, n in zip(lat.off.tolist(), lat.length.tolist())]
    got = np.array(D.crc32_batch_cpu(chunks, crc_in=lat.crc_in.tolist(), threads=threads), dtype=np.uint32)
    assert np.array_equal(got, lat.expect)


# ---------------------------------------------------------------- sensitivity
def raw_crc(data: bytes) -> int:
    """The CRC register run over `data` from 0 with no final XOR: what a segment's body and tail contribute."""
    return zlib.crc32(data, 0xFFFFFFFF) ^ 0xFFFFFFFF


def compose(lat, mutant=None):
    """Every chunk's CRC from its segments: a plain restatement of the kernel's composition, sharing no code with
    sweep_walk(). A segment's term is zlib over its body [sa, be) advanced to the chunk's end, plus zlib over its
    tail, plus the init term ~crc_in advanced over the chunk from the segment with r0 == 0; terms combine by XOR;
    ambry_amd.combine(v, 0, n) advances v over n bytes. `mutant` changes one line."""
    from ambry_amd import combine

    shift = lambda v, nbytes: combine(v, 0, nbytes)  # noqa: E731
    mem = lat.mem.tobytes()
    lens, offs, cins = lat.length.tolist(), lat.off.tolist(), lat.crc_in.tolist()
    n = len(lens)
    start = [0]
    for ln in lens:
        start.append(start[-1] + (ln if ln > lat.small_max else 0))
    total, S = start[n], lat.S

    def snap(cs, ln, r, side):
        down = mutant == "snap-down" or (mutant == "snap-disagrees" and side == 0)
        rr = ((cs + r + (0 if down else 15)) & ~15) - cs
        if mutant == "no-cap":
            return rr
        return rr if (rr <= ln if mutant == "rr-le-len" else rr < ln) else ln

    out = [c if ln == 0 else 0 for ln, c in zip(lens, cins)]
    for k in range(-(-total // S)):
        g0, g1 = k * S, min((k + 1) * S, total)
        c = bisect.bisect_right(start, g0, 0, n) - 1
        while c < n and start[c] < g1:
            ln, cs, bsc = lens[c], offs[c], start[c]
            c += 1
            if ln <= lat.small_max:
                continue
            ce = cs + ln
            cb = max(cs, ce & ~15)
            r0 = snap(cs, ln, g0 - bsc, 0) if g0 > bsc else 0
            r1 = snap(cs, ln, g1 - bsc, 1) if g1 - bsc < ln else ln
            init = (r1 == ln) if mutant in ("init-by-last", "init-by-every-last") else (r0 == 0)
            term = 0
            if mutant == "init-by-every-last" and init:  # before the empty segment's return
                term, init = shift(~cins[c - 1] & 0xFFFFFFFF, ln) ^ 0xFFFFFFFF, False
            if r0 >= r1:
                out[c - 1] ^= term
                continue
            sa, se = cs + r0, cs + r1
            be = cb if se == ce else se
            if sa < be:
                term ^= shift(raw_crc(mem[max(sa, 0):be]), ce - be)
            if se == ce and ce > cb and not (mutant == "tail-needs-body" and sa >= be):
                t0 = cb if mutant == "tail-from-cb" else max(sa, cb)
                term ^= raw_crc(mem[t0:ce])
            if init:
                term ^= shift(~cins[c - 1] & 0xFFFFFFFF, ln) ^ 0xFFFFFFFF
            out[c - 1] ^= term
    return np.array(out, dtype=np.uint64).astype(np.uint32)


# mutant -> the probe kinds that must catch it; an empty set: the mutant computes the same function (see below)
MUTANTS = {
    "snap-down": {"first16"},
    "snap-disagrees": {"mid", "first16", "final"},
    "rr-le-len": set(),
    "no-cap": {"last16"},
    "init-by-last": set(),
    "init-by-every-last": {"last16"},
    "tail-from-cb": set(),
    "tail-needs-body": {"final"},
}


def test_composition_restates_the_kernel(lw):
    lat = lw[0]
    swept = lat.length > lat.small_max
    assert np.array_equal(compose(lat)[swept | (lat.length == 0)], lat.expect[swept | (lat.length == 0)])


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutants_change_a_probe(lw, mutant):
    """One-line mutants of compose(), run on the CPU only: each must change a probe's CRC in every lattice, and
    the kinds of probe that catch it are asserted.

      snap-down            snap_cut rounds down. In Python's signed arithmetic a cut below the chunk's own start
                           comes out negative, and the first16 probes whose raw cut lies before the snapped
                           place catch it. (In the kernel's unsigned arithmetic the same cut wraps, exceeds the
                           length and is capped to it: both waves then agree on the chunk's end and the CRC is
                           right; a cut that rounds down inside the chunk moves both waves alike.)
      snap-disagrees       the earlier wave snaps up, the later down: the two overlap by 16 bytes at every cut
                           whose address is off the 16-B grid.
      no-cap               snap_cut without the cap at the length: the earlier wave runs past an unaligned end.
      init-by-every-last   the init term from every wave with r1 == len, the empty segment's included: a last16
                           chunk gets it twice.
      tail-needs-body      the tail only from a segment that has a body: the tail-only segments lose theirs.

    Three mutants as first proposed compute the same function as the kernel and can change nothing; the test
    asserts that, and their effective neighbours above stand in for them:
      rr-le-len            rr <= len ? rr : len equals rr < len ? rr : len at rr == len, the only place they differ.
      init-by-last         exactly one non-empty segment of a chunk has r0 == 0 and exactly one has r1 == len (an
                           empty one returns before the init term), and XOR does not care which wave adds it.
      tail-from-cb         t0 = sa > cb ? sa : cb: a cut is 16-aligned and below ce, so sa <= cb in every segment
                           that has a tail (test_final_segments asserts it over every lattice); the arm is dead."""
    lat, walk, segs = lw
    got = compose(lat, mutant)
    swept = lat.length > lat.small_max
    caught = {lat.kind[i] for i in np.nonzero((got != lat.expect) & swept)[0]}
    want = MUTANTS[mutant]
    if not want:
        assert not caught, "%s is no longer equivalent: it changes %s" % (mutant, sorted(caught))
        if mutant == "init-by-last":
            for i, row in segs.items():
                live = [s for s in row if not s.empty]
                assert sum(s.r0 == 0 for s in live) == 1 and sum(s.r1 == s.length for s in live) == 1
        if mutant == "rr-le-len":
            assert all(min(rr, ln) == (rr if rr <= ln else ln) for ln in range(1, 40) for rr in range(0, 60))
        return
    missing(want, caught, "mutant %s, probe kinds that catch it" % mutant)
    if mutant == "snap-down":
        assert "mid" not in caught and "last16" not in caught
    if mutant == "no-cap":
        bad = [i for i, _ in probes(lat, "last16") if got[i] != lat.expect[i]]
        assert bad and all((int(lat.off[i]) + int(lat.length[i])) & 15 for i in bad)  # the unaligned ends


def test_reduced_lattice_through_the_kernel_model():
    """The first16 and last16 probes of the 16 KiB wave lattice, each behind its pad, through KernelModel.batch
    (kernel_model.py: the kernels' arithmetic step by step) with body_crc_t4 (run=-4) and body_crc (run=1), at the
    lattice's share size. Measured where this was written: both runs together take 0.8 s on one core."""
    from kernel_model import KernelModel

    lat = L.sweep_lattice("wave", 16384)
    walk = L.lattice_walk("wave", 16384)
    keep = [i for k, i, _ in lat.probes if k in ("first16", "last16")]
    idx = sorted(set(keep) | {i - 1 for i in keep})
    assert all(lat.kind[i - 1] == "pad" for i in keep)
    # a leading chunk puts the first kept pad where it lies in the lattice (mod S); each pad then keeps its cut
    lens, offs, cins, at = [], [], [], {}
    pos = 0
    for i in idx:
        if lat.kind[i] == "pad":
            lead = (walk.byte_start[i] - pos) % lat.S
            if lead:
                lens.append(lead)
                offs.append(64)
                cins.append(0)
                pos += lead
        at[i] = pos
        lens.append(int(lat.length[i]))
        offs.append(int(lat.off[i]))
        cins.append(int(lat.crc_in[i]))
        pos += lens[-1]
    raw = lat.mem.tobytes()
    exp = [zlib.crc32(raw[o:o + n], c) for o, n, c in zip(offs, lens, cins)]
    r = {i: sp["r"] for _, i, sp in lat.probes}
    assert len(keep) == 60 and all((at[i] + r[i]) % lat.S == 0 for i in keep)  # every probe keeps its cut
    km = KernelModel()
    for run in (-4, 1):
        assert km.batch(lat.mem, offs, lens, crc_in=cins, nwaves=lat.nwaves, run=run, min_share=16384) == exp, run


def test_a_failure_names_the_segments():
    """What the GPU tests print for a wrong chunk: every segment with its wave, round and cells."""
    lat = L.sweep_lattice("wave", 16384)
    i = probes(lat, "last16")[0][0]
    text = L.describe_segments(L.by_chunk(L.lattice_walk("wave", 16384, True).segments)[i])
    assert text.count("{") == 2 and "wave=" in text and "round=" in text and "whole=True" in text and "empty=True" in text
