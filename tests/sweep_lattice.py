"""Sweep geometry by construction: batches that put a share boundary of the batch sweep (crc32_kernels.hip
crc32_sweep_kernel) on every cut residue, segment shape and descriptor-window case at which the kernel changes its
case split, and sweep_cells(), the classifier the tests assert that coverage with.

The sweep views a batch as one stream, the concatenation of its chunks longer than small_max, and gives wave w of
16 * grid the stream bytes [w S, (w + 1) S). Where a share boundary falls r bytes into a chunk, snap_cut moves it
up to a 16-B aligned address, and the chunk's CRC is the XOR of its segments' terms. sweep_cells() restates that
split from crc32_kernels.hip (the sweep kernel, snap_cut, body_crc_t4, body_crc) and wave_tools.h (find_start); it
shares no code with kernel_model.py.

sweep_lattice(form, S) is one stream of probes, each preceded by a pad chunk sized so that the next multiple of S
falls exactly r bytes into the probe. The chunks overlap in one small buffer of nonzero bytes, each at a chosen
offset mod 64, so a byte that a mask wrongly drops or keeps, or a cut taken 16 bytes off, changes the CRC.
form "wave": fewer than 16,384 chunks, so every non-empty chunk takes share bytes; form "group": at least 16,384
chunks, every probe and pad above 16 KiB, the rest chunks of at most 16 KiB that the group phase takes whole and
the sweep walks past."""
import bisect
import functools
import zlib
from types import SimpleNamespace

import numpy as np

import geometry_lattice as G

SHARE_QUANTUM = 1024         # crc32_kernels.h kShareQuantum
MIN_SHARE = 16384            # crc32_kernels.h kMinShare
GROUP_MIN_CHUNKS = 16384     # crc32_kernels.h kGroupMinChunks
GROUP_SMALL_MAX = G.CLASS_CUTS[-1]  # crc32_kernels.h kGroupSmallMax
SUPER_BLOCK = 4096           # body_crc_t4: four 1 KiB blocks a step
BLOCK = 1024                 # crc32_layout.h kBlockBytes: body_crc's step, 16 B a lane
PREFETCH_U = 8               # body_crc<8, ...>: blocks in flight
WAVES = 16                   # waves of one 1,024-thread workgroup
WINDOW = 64                  # descriptors a wave fetches at a time
DEFAULT_WINDOW_BYTES = 32 << 30  # ambrycrc_set_window's setting outside the tests
BUFFER = 256 << 10
FILLER_PIECE = 128 << 10
SHARES = (MIN_SHARE, 21504, 24576)  # 21 KiB: a partial first super-block; 24 KiB: body_crc's second rolling turn

MID_START = (0, 1, 15, 16, 17, 63)
HEAD_LANES = (0, 1, 62, 63)
HEAD_LEADS = (0, 1, 3, 4, 5, 15)
FINAL_BODY = (0, 16, 4080, 4096, 4112)
RUN_LENGTHS = (63, 64, 65, 200)
START_FORMS = ("plain", "before", "after", "both")


# ---------------------------------------------------------------- the classifier
def snap_cut(cs: int, length: int, r: int) -> int:
    """crc32_kernels.hip snap_cut: the chunk-relative cut r moved up to a 16-B aligned address, capped at the
    chunk's length."""
    rr = ((cs + r + 15) & ~15) - cs
    return rr if rr < length else length


def share_size(total: int, grid: int, window: int = 0):
    """(S, R): the byte share of one wave and the number of rounds. One round of 16 * grid shares unless `window`
    is set and the stream is longer: then R = ceil(total / window) rounds, wave w taking shares w, w + nwaves, ..."""
    nwaves = WAVES * grid
    rounds = -(-total // window) if window and total > window else 1
    share = (-(-total // (rounds * nwaves)) + SHARE_QUANTUM - 1) & ~(SHARE_QUANTUM - 1)
    return max(share, MIN_SHARE), rounds


def cut_cells(cs: int, length: int, r: int):
    """A share boundary r bytes into the chunk (cs, length), 0 <= r < length. a = (cs + r) & 15 picks the snap
    distance (16 - a) & 15; rr is the snapped cut. kind: "start" (r == 0: the boundary is the chunk's start, no
    cut), "last16" (the snap reaches the chunk's end: the earlier wave has the whole chunk, the later an empty
    segment), "first16" (the earlier wave's segment is 1..16 bytes), else "mid". t = ce & 15; ce16 = the chunk ends
    16-aligned (rr == length exactly, the equality of snap_cut's rr < length)."""
    rr = snap_cut(cs, length, r)
    kind = "start" if r == 0 else "last16" if rr == length else "first16" if rr <= 16 else "mid"
    return SimpleNamespace(kind=kind, a=(cs + r) & 15, rr=rr, t=(cs + length) & 15, ce16=(cs + length) & 15 == 0,
                           dist=length - r)


def _segment(cs, length, r0, r1):
    """One (share, chunk) intersection [r0, r1) after the snap, as crc32_sweep_kernel's `segment` lambda splits it.

    empty: r0 >= r1 (the later wave of a last16 cut: it XORs 0 into out). whole: r0 == 0 and r1 == length (a
    plain store, no atomic). Body [sa, be): be = cb at the chunk's last segment, else se (16-aligned); body = its
    bytes. body_crc_t4 (variant 29): nb = ceil(body / 4096) super-blocks, v0 = be - 4096 nb the virtual start,
    sb_off = sa - v0 where the body starts in super-block 0, blk = sb_off >> 10 the first block loaded, lane =
    (sb_off & 1023) >> 4 the first lane that forms an address, lead = sa & 15 bytes of its piece masked off, v0neg
    = the virtual start lies below the buffer. body_crc<8> (variant 0): nb1k = ceil(body / 1024) blocks, path =
    "prime" (1..8), "drain-refill" (9..15), "roll-dry" (16), "roll-refill" (17..23) or "roll2" (24 and up, two
    rolling iterations); v0neg1k as v0neg for its 1 KiB steps. final: the chunk's last segment; final_body = cb -
    sa (0: tail only) and t = bytes of the lane-parallel tail."""
    ce = cs + length
    cb = max(cs, ce & ~15)
    s = SimpleNamespace(r0=r0, r1=r1, empty=r0 >= r1, whole=r0 == 0 and r1 == length, first=r0 == 0, cs=cs, ce=ce, cb=cb)
    if s.empty:
        return s
    sa, se = cs + r0, cs + r1
    be = cb if se == ce else se
    body = max(be - sa, 0)
    nb = -(-body // SUPER_BLOCK)
    nb1k = -(-body // BLOCK)
    sb_off = sa - (be - nb * SUPER_BLOCK)
    final = se == ce
    s.__dict__.update(
        sa=sa, se=se, be=be, body=body, nb=nb, nb1k=nb1k, sb_off=sb_off, blk=sb_off >> 10, lane=(sb_off & 1023) >> 4,
        lead=sa & 15, v0neg=body > 0 and be - nb * SUPER_BLOCK < 0, v0neg1k=body > 0 and be - nb1k * BLOCK < 0,
        path=None if nb1k == 0 else "prime" if nb1k <= PREFETCH_U else "drain-refill" if nb1k < 2 * PREFETCH_U else
        "roll-dry" if nb1k == 2 * PREFETCH_U else "roll-refill" if nb1k < 3 * PREFETCH_U else "roll2",
        final=final, final_body=cb - sa if final else None, t=ce - max(sa, cb) if final and ce > cb else 0,
        tail_only=final and body == 0)
    return s


def sweep_walk(lens, offs, small_max: int, grid: int, window: int = 0, crc_in=None):
    """The sweep's walk over a batch: S, R, nwaves, total, byte_start, segments and windows.

    segments: _segment() of every (share, chunk) intersection the kernel evaluates, with share (k: stream bytes
    [k S, (k + 1) S)), wave = k mod nwaves, round = k div nwaves, chunk, and for a segment with r0 == 0 its init
    case: "seeded" (crc_in != 0), else "hit" / "miss" of the wave's one-entry init_len cache, which it keeps from
    chunk to chunk and from round to round.
    windows: every 64-descriptor fetch: share, wave, round, c (its first chunk), cnt, work (a chunk of it took
    share bytes), done (it reached the share's end), jump (no work and not done: the find_start jump is taken) and
    far (where the jump lands; at most c + cnt means the window was walked for nothing and no chunk skipped)."""
    lens = [int(x) for x in lens]
    offs = [int(x) for x in offs]
    n = len(lens)
    spans = [ln if ln > small_max else 0 for ln in lens]
    byte_start = [0] * (n + 1)
    for i, sp in enumerate(spans):
        byte_start[i + 1] = byte_start[i] + sp
    total = byte_start[n]
    share, rounds = share_size(total, grid, window)
    nwaves = WAVES * grid
    find_start = lambda g: bisect.bisect_right(byte_start, g, 0, n) - 1  # noqa: E731  largest c < n, start[c] <= g
    segments, windows, init_len = [], [], {}
    for k in range(-(-total // share)):
        wave, rnd = k % nwaves, k // nwaves
        assert rnd < rounds
        g0, g1 = k * share, min((k + 1) * share, total)
        c, done = find_start(g0), False
        while not done and c < n:
            cnt = min(n - c, WINDOW)
            bsc, work = byte_start[c], False
            for j in range(cnt):
                if bsc >= g1:
                    done = True
                    break
                i = c + j
                if spans[i]:
                    work = True
                    r0 = snap_cut(offs[i], lens[i], g0 - bsc) if g0 > bsc else 0
                    r1 = snap_cut(offs[i], lens[i], g1 - bsc) if g1 - bsc < lens[i] else lens[i]
                    s = _segment(offs[i], lens[i], r0, r1)
                    s.init = None
                    if not s.empty and r0 == 0:
                        if crc_in is not None and int(crc_in[i]) != 0:
                            s.init = "seeded"
                        else:
                            s.init = "hit" if init_len.get(wave) == lens[i] else "miss"
                            init_len[wave] = lens[i]
                    s.__dict__.update(share=k, wave=wave, round=rnd, chunk=i, length=lens[i])
                    segments.append(s)
                bsc += spans[i]
            nxt = c + cnt
            jump = not work and not done and nxt < n
            far = find_start(bsc) if jump else None
            windows.append(SimpleNamespace(share=k, wave=wave, round=rnd, c=c, cnt=cnt, work=work, done=done, jump=jump,
                                           far=far))
            c = max(nxt, far) if jump else nxt
    return SimpleNamespace(S=share, R=rounds, nwaves=nwaves, total=total, byte_start=byte_start, segments=segments,
                           windows=windows)


def sweep_cells(lens, offs, small_max: int, grid: int, window: int = 0, crc_in=None):
    """The segments of sweep_walk(): one per (wave, round, chunk) the kernel evaluates, with r0, r1 and the cells
    of _segment(). The same split serves both variants: nb, blk, lane, lead, v0neg are body_crc_t4's (variant
    29), nb1k, path, v0neg1k body_crc<8>'s (variant 0)."""
    return sweep_walk(lens, offs, small_max, grid, window, crc_in).segments


def by_chunk(segments):
    out = {}
    for s in segments:
        out.setdefault(s.chunk, []).append(s)
    return out


def describe_segments(segs) -> str:
    """The cells of one chunk's segments for a failure message, in stream order."""
    keys = ("wave", "round", "share", "r0", "r1", "empty", "whole", "init", "body", "nb", "nb1k", "path", "blk", "lane",
            "lead", "v0neg", "final_body", "t")
    return "; ".join("{" + ", ".join("%s=%s" % (k, getattr(s, k)) for k in keys if hasattr(s, k)) + "}" for s in segs)


# ---------------------------------------------------------------- the probes
def _fit(r_base: int, cs: int, a: int) -> int:
    """The smallest r >= r_base with (cs + r) & 15 == a."""
    return r_base + ((a - cs - r_base) & 15)


def probe_specs(form: str, S: int):
    """Every probe in stream order: dicts of kind, c64 (the chunk's offset mod 64), r (where the share boundary
    falls in it), length, and optionally low (the chunk sits in the buffer's first 64 bytes), cin (0: crc_in
    forced to 0, 1: forced nonzero), before / after (span-0 chunks at the probe's start / end position: a list of
    lengths) and lead_in (chunks that take share bytes between the probe and its `after` run)."""
    wave = form == "wave"
    rest = 3000 if wave else 12000     # bytes after the cut: a group-form probe is above 16 KiB
    floor = 0 if wave else GROUP_SMALL_MAX + 1
    specs = []

    def add(kind, c64, r, length, **kw):
        assert (r is None or 0 <= r < length) and (wave or length > GROUP_SMALL_MAX), (kind, r, length)
        specs.append(dict(kind=kind, c64=c64, r=r, length=length, **kw))

    def spanless(count, seed):
        """`count` chunks that take no share bytes: empty in wave form; in group form of 0..16 KiB, mostly short."""
        if wave:
            return [0] * count
        cycle = (0, 1, 15, 16, 17, 100, 255, 256, 257, 1000, 1024, 1025, 40, 4096, 64, 4097, 3, 16383, 7, 16384)
        return [cycle[(seed + 7 * q) % len(cycle)] if q % 16 == 0 else cycle[(seed + q) % 13] for q in range(count)]

    # mid: every address residue of the cut at six start residues; a first segment from an unaligned start, a
    # last one from an aligned one
    for a in range(16):
        for c64 in MID_START:
            r = _fit(5000 + 16 * a, c64, a)
            add("mid", c64, r, r + rest + 37 * a + c64)
    # long: a cut, a whole share, a cut: the full-share segment between them (S bytes from an aligned start)
    for q, c64 in enumerate((0, 7, 16, 63)):
        r = 2000 + 16 * q + q
        add("long", c64, r, r + S + max(1500 + q, floor - S))
    # first16: the earlier wave's segment is h bytes, from the cut one byte in and from the cut on the snapped place
    for h in range(1, 17):
        for r in sorted({1, h}):
            add("first16", ((16 - h) & 15) + 16 * (h % 4), r, max(2500 + 41 * h, floor + h))
    # last16: the snap reaches the chunk's end t bytes past a 16-B boundary; t == 0: from 1 and 15 bytes before
    # the end; t >= 2: from 1 and t - 1 (the raw cut must lie past floor16(ce)); t == 1 has no such cut
    for t in range(16):
        for dist in sorted({1, 15} if t == 0 else {1, t - 1} if t >= 2 else ()):
            c64 = (7 * t + 3) % 64
            length = _fit(max(2800 + 16 * t, floor + 16), c64, t)
            add("last16", c64, length - dist, length)
    # start: the boundary on the chunk's first byte; with span-0 chunks at that position before it, and with the
    # next boundary on its end and span-0 chunks there
    for form_ in START_FORMS:
        for c64 in (0, 5, 59):
            ends = form_ in ("after", "both")
            add("start", c64, 0, (S if wave else 2 * S) if ends else S + 40 + c64,
                before=spanless(3, c64) if form_ in ("before", "both") else [], after=spanless(3, c64 + 1) if ends else [],
                form=form_)
    # head: where the first segment's body starts in super-block 0, and how many super-blocks it has
    q = 0
    for nb in (1, 2, 3, 4):
        for blk in range(4):
            for lane in HEAD_LANES:
                for lead in HEAD_LEADS:
                    length = nb * SUPER_BLOCK - (BLOCK * blk + 16 * lane + lead)  # the first segment's bytes
                    add("head", lead + 16 * ((blk + lane + nb) % 4), length,
                        max(length + 40 + (7 * q) % 50, floor + q % 40), low=q % 8 == 0)
                    q += 1
    # final: the chunk's last segment has cb - sa body bytes and t tail bytes
    for body in FINAL_BODY:
        for t in range(16):
            if body or t:
                c64 = (11 * t + body // 16) % 64
                r = 3000 + 16 * t + body % 7 if wave else S
                add("final", c64, r, ((c64 + r + 15) & ~15) - c64 + body + t)
    if wave:
        # many: 70 and 140 whole chunks in one share (two and three descriptor windows), with the init cache's
        # cases: miss, hit, a seeded chunk between, hit again, miss
        for count in (70, 140):
            for q in range(count):
                length = 96 if q < 4 else 40 + (q * 29) % 90
                add("many", (5 * q + count) % 64, 0, length, cin=1 if q == 2 else 0 if q < 6 else None, chain=q > 0)
    # runs of span-0 chunks: at stream position 0 (set by the builder), at a share boundary, inside a share
    for n_run in RUN_LENGTHS:
        add("run-boundary", (3 * n_run) % 64, 0, max(700 + n_run, floor + n_run), before=spanless(n_run, n_run), run=n_run)
    for n_run in RUN_LENGTHS:
        # wave form: the anchor holds the share's first byte, so the descriptor windows count from it; 63 chunks
        # of 20 bytes fill the first window and the run starts the second. Group form: nothing that takes share
        # bytes fits between, so the run follows the anchor.
        add("run-inside", (5 * n_run) % 64, 16, 48 + floor, lead_in=[20] * 63 if wave else [],
            after=spanless(n_run, n_run + 1), run=n_run)
        add("run-after", (7 * n_run) % 64, None, max(500 + n_run, floor + n_run))
    return specs


def _rounds_cross(probe_cuts, nwaves4: int) -> bool:
    """A probe holds boundary j * nwaves4 (the first share of round j under a quarter of the waves)."""
    return any(j * nwaves4 in probe_cuts for j in (1, 2, 3))


@functools.lru_cache(maxsize=None)
def sweep_lattice(form: str, S: int):
    """mem (uint8[BUFFER], nonzero), off, length (int64[n]), crc_in (uint32[n]), grid, window (0: one round),
    small_max, S, nwaves, total, kind (per chunk: a probe's kind, "pad", "span0" for a chunk that takes no share
    bytes, "lead-in" or "filler"), probes ([(kind, chunk, spec)]), run_at ({(placement, run length): first chunk
    of the run}), expect (zlib's CRCs) and rounds (grid, window: a quarter of the workgroups and a window that
    makes four rounds of the same shares).

    The builder asserts that crc32_sweep_kernel's share formula gives exactly S at the returned grid, and under
    `rounds` too: closing filler chunks bring the stream's length into (nwaves (S - 1024), nwaves S], so that the
    last of the four rounds is part full, and the grid is the smallest multiple of four at which a probe holds a
    boundary between two rounds."""
    assert form in ("wave", "group") and S % SHARE_QUANTUM == 0 and S >= MIN_SHARE
    wave = form == "wave"
    small_max = 0 if wave else GROUP_SMALL_MAX
    span = lambda ln: ln if ln > small_max else 0  # noqa: E731
    length, c64s, low, kind, cin_force, probes, run_at, probe_cuts = [], [], [], [], [], [], {}, set()
    pos = 0

    def put(what, ln, c64, lo=False, cin=None):
        nonlocal pos
        length.append(ln)
        c64s.append(c64)
        low.append(lo)
        kind.append(what)
        cin_force.append(cin)
        pos += span(ln)
        return len(length) - 1

    def put_run(lens, key=None):
        for q, ln in enumerate(lens):
            i = put("span0", ln, (11 * q + len(lens)) % 64, cin=1 if ln == 0 else None)
            if q == 0 and key:
                run_at[key] = i

    specs = probe_specs(form, S)
    bulk = 0 if wave else max(0, GROUP_MIN_CHUNKS + 64 - 2 * len(specs) - sum(
        len(sp.get("before", ())) + len(sp.get("after", ())) for sp in specs) - 65 - 63)
    put_run([0 if wave else (1 + 9 * q) % 300 for q in range(65)], ("head", 65))  # stream position 0
    for j, sp in enumerate(specs):
        if sp["r"] is not None and not sp.get("chain"):
            pad = -(pos + sp["r"]) % S  # the next multiple of S falls r bytes into the probe
            pad = (pad or S) if wave else pad + S if pad else 2 * S  # group form: above 16 KiB
            put("pad", pad, (13 * j) % 64)
            assert (pos + sp["r"]) % S == 0
        if sp.get("before"):
            put_run(sp["before"], ("boundary", sp["run"]) if "run" in sp else None)
        at = pos
        i = put(sp["kind"], sp["length"], sp["c64"], sp.get("low", False), sp.get("cin"))
        probes.append((sp["kind"], i, sp))
        probe_cuts.update(k for k in range(at // S + 1, -(-pos // S)) if at < k * S < pos)
        for ln in sp.get("lead_in", ()):
            put("lead-in", ln, (3 * len(length)) % 64)
        if sp.get("after"):
            put_run(sp["after"], ("inside", sp["run"]) if "run" in sp else None)
    # the closing filler and the grid
    grid = 4 * -(-(pos + GROUP_SMALL_MAX + 1) // (4 * WAVES * (S - SHARE_QUANTUM)))
    while wave and S == MIN_SHARE and not _rounds_cross(probe_cuts, 4 * grid):
        grid += 4
    nwaves = WAVES * grid
    need = nwaves * (S - SHARE_QUANTUM) + 1017 - pos
    assert need > GROUP_SMALL_MAX
    while need > FILLER_PIECE + 2 * GROUP_SMALL_MAX:
        put("filler", FILLER_PIECE, (len(length) * 9) % 64)
        need -= FILLER_PIECE
    put("filler", need, 21)
    total = pos
    put_run([0 if wave else (3 + 5 * q) % 200 for q in range(63)], ("tail", 63))  # after the last swept chunk
    if bulk:
        put_run([(0, 1, 15, 16, 17, 100, 255, 256, 257, 33)[q % 10] for q in range(bulk)])
    n = len(length)
    assert (n < GROUP_MIN_CHUNKS) == wave
    assert nwaves * (S - SHARE_QUANTUM) < total <= nwaves * S and share_size(total, grid) == (S, 1)
    window4 = -(-total // 4)
    assert grid % 4 == 0 and share_size(total, grid // 4, window4) == (S, 4) and window4 >= 1 << 20
    assert -(-total // S) < nwaves and -(-total // S) > 3 * nwaves // 4  # the fourth round is part full

    mem = np.frombuffer(G.nonzero_bytes(4242, BUFFER), dtype=np.uint8)
    slots = (BUFFER - max(length) - 64) // 64
    assert slots > 64
    off = np.array([c + (0 if lo else 64 * (1 + (i * 977) % (slots - 1))) for i, (c, lo) in enumerate(zip(c64s, low))],
                   dtype=np.int64)
    length = np.asarray(length, dtype=np.int64)
    assert int((off + length).max()) <= BUFFER
    crc_in = np.random.default_rng(17).integers(1, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    crc_in[::3] = 0
    for i, f in enumerate(cin_force):
        if f == 0:
            crc_in[i] = 0
        elif f == 1:
            crc_in[i] |= 1
    raw = mem.tobytes()
    expect = np.array([zlib.crc32(raw[o:o + ln], int(c)) for o, ln, c in zip(off.tolist(), length.tolist(), crc_in.tolist())],
                      dtype=np.uint32)
    return SimpleNamespace(form=form, mem=mem, off=off, length=length, crc_in=crc_in, grid=grid, window=0,
                           small_max=small_max, S=S, nwaves=nwaves, total=total, kind=kind, probes=probes, run_at=run_at,
                           expect=expect, rounds=SimpleNamespace(grid=grid // 4, window=window4))


@functools.lru_cache(maxsize=None)
def lattice_walk(form: str, S: int, rounds: bool = False):
    """sweep_walk() of a lattice at its own grid, or at its `rounds` geometry."""
    lat = sweep_lattice(form, S)
    geo = lat.rounds if rounds else lat
    return sweep_walk(lat.length, lat.off, lat.small_max, geo.grid, geo.window, lat.crc_in)
