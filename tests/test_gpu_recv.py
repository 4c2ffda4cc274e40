"""GPU parity for ambrycrc_receive_blobs_dev against the oracle (tests/recv_oracle.py: oracle/message_format.py,
struct and zlib) and against the CPU entry: status, every info field and every delivered byte. Bodies are the send
oracle's packed spans. The body and the output each sit inside a larger tensor with 64 guard bytes of 0xA5 on
both sides, which must survive; the body must be unchanged, and output bytes outside the delivered spans must
stay 0xA5 -- only the bytes inside the span of a payload that failed on a CRC alone are unspecified."""
import functools

import numpy as np
import pytest

import recv_oracle as RO
import rekey_oracle as RK
import send_oracle as SO
from datagen import stream_bytes
from gpu_buffers import assert_guards, dev, guarded, guarded_workspace, guards_intact, host, u64_dev
from gpu_calls import assert_same, copies
from msgfmt import MF

pytestmark = pytest.mark.gpu

FLAG_NAMES = {RO.BLOB: "blob", RO.ALL: "all"}
GROUP_MIN_CHUNKS = 16384  # kGroupMinChunks: from this many jobs on, the CRC pass runs its group phase
JOBS = {RO.BLOB: 3, RO.ALL: 6}  # jobs a payload: content before the slice, the slice, after it; ALL: + three records


@pytest.fixture(scope="module")
def messages(gpu):
    from ambry_amd import messages as M

    assert M.RECV_INFO_DTYPE == RO.INFO
    return M


def run_gpu(messages, body: bytes, offs, sizes, flag, ranges=None, dst_off=None, shift=0, oshift=0, out_cap=64,
            workspace=None):
    """(status list, INFO array, the output view's bytes): guards checked around the body (which must be
    unchanged) and the output."""
    import torch

    rw, r = guarded(body, shift)
    ow, o = guarded(b"", oshift, out_cap)
    _, info, status = messages.receive_blobs_dev(r, u64_dev(offs), flag, pay_size=None if sizes is None else u64_dev(sizes),
                                                 ranges=None if ranges is None else u64_dev(ranges),
                                                 dst_off=None if dst_off is None else u64_dev(dst_off), out=o,
                                                 workspace=workspace)
    torch.cuda.synchronize()
    assert guards_intact(rw, shift, len(body)).tobytes() == body
    return (status.cpu().numpy().view(np.uint32).tolist(), info.cpu().numpy().view(RO.INFO),
            guards_intact(ow, oshift, out_cap))


def check(messages, body, offs, sizes, flag, ranges=None, dst_off=None, shift=0, oshift=0, out_cap=None, cpu=False,
          workspace=None, exp=None):
    """The batch on the device against the oracle (out_cap None: exactly the packed need); cpu: and the CPU
    entry against both."""
    if exp is None:
        exp = RO.expected(body, offs, sizes, flag, ranges=ranges, dst_off=dst_off, out_cap=out_cap)
        if len(exp[2]) == 0:  # nothing to deliver: one byte of output, which must stay untouched
            exp = RO.expected(body, offs, sizes, flag, ranges=ranges, dst_off=dst_off, out_cap=1)
    got = run_gpu(messages, body, offs, sizes, flag, ranges, dst_off, shift, oshift, len(exp[2]), workspace)
    RO.assert_outputs(got, exp)
    if cpu:
        assert dst_off is None
        RO.assert_outputs(RO.run_cpu(messages, body, offs, sizes, flag, ranges=ranges, out_cap=len(exp[2])), exp)
    return exp


@functools.lru_cache(maxsize=None)
def region_expected(flag, sized):
    body, offs, sizes = RO.sent_region(flag)
    return RO.expected(body, offs, sizes if sized else None, flag)


# ---------------------------------------------------------------- 1. parity on the mixed region
@pytest.mark.parametrize("shift,oshift,sized", [(0, 0, False), (1, 5, True), (17, 0, True), (63, 5, False)])
@pytest.mark.parametrize("flag", [RO.BLOB, RO.ALL], ids=FLAG_NAMES.get)
def test_region_matches_oracle_and_cpu(messages, flag, shift, oshift, sized):
    """Every stored format (headers V1-V3, blob records V1-V3, MetadataBlobs, update messages, 10 % corrupted,
    blobs up to 300 KB: one record across waves) sent under `flag` by the send oracle; the body at four offsets
    from a 64-B boundary and the output at two, with the sender's sizes and without (each payload then runs to
    the body's end, what follows its record ignored). A message the send refused arrives as (UINT64_MAX, 0)."""
    body, offs, sizes = RO.sent_region(flag)
    exp = check(messages, body, offs, sizes if sized else None, flag, shift=shift, oshift=oshift, cpu=shift in (0, 1),
                exp=region_expected(flag, sized))
    clean, crc, refused = RO.mix(exp[0])
    assert clean >= 100 and crc >= 1 and refused >= 1, (clean, crc, refused)


# ---------------------------------------------------------------- 2. content length ladder
LADDER = list(range(131)) + [4095, 4096, 4097, 16383, 16384, 16385, 65535, 65536, 65537, 300000]


@functools.lru_cache(maxsize=None)
def ladder_case():
    """One bare blob record per content length of LADDER (16,383-16,385: kGroupSmallMax either side) and record
    version (heads of 10, 12 and 13 bytes: three source / destination misalignments), packed back to back."""
    recs = [RO._blob(stream_bytes(300 + bv, n, n).tobytes(), bv) for n in LADDER for bv in (1, 2, 3)]
    offs = [int(x) for x in np.cumsum([0] + [len(b) for b in recs[:-1]])]
    body, sizes = b"".join(recs), [len(b) for b in recs]
    return body, offs, sizes, RO.expected(body, offs, sizes, RO.BLOB)


@pytest.mark.parametrize("shift,oshift", [(0, 0), (63, 5)])
def test_content_length_ladder(messages, shift, oshift):
    body, offs, sizes, exp = ladder_case()
    assert exp[0] == [0] * (3 * len(LADDER)) and len(exp[2]) == 3 * sum(LADDER)
    check(messages, body, offs, sizes, RO.BLOB, shift=shift, oshift=oshift, exp=exp)


# ---------------------------------------------------------------- 3. ranges
def _edges(n):
    return sorted({v for v in (0, 1, 63, 64, 65, n - 65, n - 64, n - 1, n) if 0 <= v <= n})


@functools.lru_cache(maxsize=None)
def range_case():
    """Records of 1, 2, 63, 64 and 65 content bytes under every (lo, hi), lo <= hi <= len; of 200, 5,000 and
    70,000 under lo and hi from the edges of 64 either end, and to the end. Every payload of one length reads the
    same record of the body. 6,607 payloads, 19,821 jobs: the CRC pass runs its group phase."""
    lens = (1, 2, 63, 64, 65, 200, 5000, 70000)
    recs = [RO._blob(stream_bytes(500 + n, 1, n).tobytes(), 1 + k % 3) for k, n in enumerate(lens)]
    starts = [int(x) for x in np.cumsum([0] + [len(b) for b in recs[:-1]])]
    offs, sizes, ranges = [], [], []
    for n, at, b in zip(lens, starts, recs):
        if n <= 65:
            pairs = [(lo, hi) for lo in range(n + 1) for hi in range(lo, n + 1)]
        else:
            pairs = [(lo, hi) for lo in _edges(n) for hi in _edges(n) if lo <= hi] + [(lo, RO.TO_END) for lo in _edges(n)]
        for lo, hi in pairs:
            offs.append(at)
            sizes.append(len(b))
            ranges.append((lo, hi))
    body = b"".join(recs)
    return body, offs, sizes, ranges, RO.expected(body, offs, sizes, RO.BLOB, ranges=ranges)


def test_ranges(messages):
    body, offs, sizes, ranges, exp = range_case()
    assert len(offs) == 6607 and JOBS[RO.BLOB] * len(offs) >= GROUP_MIN_CHUNKS and exp[0] == [0] * len(offs)
    check(messages, body, offs, sizes, RO.BLOB, ranges=ranges, shift=3, oshift=1, exp=exp)


@pytest.mark.parametrize("n", [5000, 70000])
def test_a_flipped_bit_in_any_piece_is_found(messages, n):
    """The record is hashed as its head and three pieces around [lo, hi): one flipped bit in turn in the head, in
    the content before lo, inside [lo, hi), after hi, in the trailer's low word and in its high word -- each must
    report BLOB_CRC, so a piece dropped from the combine, or shifted by the wrong length, cannot pass."""
    rec = RO._blob(stream_bytes(77, 2, n).tobytes(), 3)
    lo, hi = 65, n - 65
    places = {"head": 4, "before": 13 + 10, "inside": 13 + lo + 100, "after": 13 + n - 3, "trailer-low": len(rec) - 1,
              "trailer-high": len(rec) - 6}
    recs = [rec] + [RO._flip(rec, at, 0x02) for at in places.values()]
    offs = [i * len(rec) for i in range(len(recs))]
    body = b"".join(recs)
    exp = check(messages, body, offs, [len(rec)] * len(recs), RO.BLOB, ranges=[(lo, hi)] * len(recs), shift=5, oshift=2)
    assert exp[0] == [0] + [MF.BLOB_CRC] * len(places)


ALL_LENS = (1, 2, 63, 64, 65, 200)


@functools.lru_cache(maxsize=None)
def range_case_all():
    """Stored V3 PUTs with an encryption-key record (slot 3 filled) and without (slot 3 empty) for each content
    length of ALL_LENS, as payloads under ALL: every (lo, hi), lo <= hi <= len, for the first five lengths, and
    for 200 lo and hi from the edges of 64 either end, and to the end. 12,998 payloads, 77,988 jobs."""
    msgs = [RK.stored_put(MF.store_key("range-%d-%d" % (n, e)), MF.blob_properties_bytes(n), b"um" * (n % 7),
                          stream_bytes(600 + n, e, n).tobytes(), hv=3, enc_key=b"k" * 24 if e else None, bv=1 + k % 3)
            for k, n in enumerate(ALL_LENS) for e in (0, 1)]
    starts = [int(x) for x in np.cumsum([0] + [len(b) for b in msgs[:-1]])]
    offs, sizes, ranges = [], [], []
    for (n, e), at, b in zip([(n, e) for n in ALL_LENS for e in (0, 1)], starts, msgs):
        if n <= 65:
            pairs = [(lo, hi) for lo in range(n + 1) for hi in range(lo, n + 1)]
        else:
            pairs = [(lo, hi) for lo in _edges(n) for hi in _edges(n) if lo <= hi] + [(lo, RO.TO_END) for lo in _edges(n)]
        for lo, hi in pairs:
            offs.append(at)
            sizes.append(len(b))
            ranges.append((lo, hi))
    body = b"".join(msgs)
    return body, offs, sizes, ranges, RO.expected(body, offs, sizes, RO.ALL, ranges=ranges)


def test_ranges_all(messages):
    """test_ranges under ALL: the six-slot form, its slot 3 (the encryption-key record) filled and empty by
    turns, the three content pieces at every cut of the short contents. Every 41st payload through the CPU
    entry too."""
    body, offs, sizes, ranges, exp = range_case_all()
    assert len(offs) == 12998 and exp[0] == [0] * len(offs)
    assert {int(x) != 0 for x in exp[1]["enckey_len"]} == {False, True}
    check(messages, body, offs, sizes, RO.ALL, ranges=ranges, shift=3, oshift=1, exp=exp)
    pick = slice(0, None, 41)
    check(messages, body, offs[pick], sizes[pick], RO.ALL, ranges=ranges[pick], shift=5, oshift=2, cpu=True)


@pytest.mark.parametrize("n", [5000, 70000])
def test_a_flipped_bit_in_any_record_is_found(messages, n):
    """A stored PUT with all four records under ALL with a range: one flipped bit in turn in the content, the
    trailer's low word and its high word of the encryption-key, properties and user-metadata records, and in
    each of the blob record's three content pieces -- each reports exactly its own record's bit, so slots 3-5
    are each held to their own stored long. One in the header reports HEADER_CRC."""
    put = RK.stored_put(MF.store_key("flip-%d" % n), MF.blob_properties_bytes(n), stream_bytes(78, 1, 300).tobytes(),
                        stream_bytes(78, 2, n).tobytes(), hv=3, enc_key=stream_bytes(78, 3, 40).tobytes(), bv=3)
    _, _, rel = MF.parse_header(put, 0)
    lo, hi = 65, n - 65
    places = []
    for name, start, end, content, bit in (("enckey", rel[0], rel[1], rel[0] + 6 + 20, MF.ENCKEY_CRC),
                                           ("props", rel[1], rel[3], rel[1] + 15, MF.PROPS_CRC),
                                           ("usermeta", rel[3], rel[4], rel[3] + 6 + 150, MF.USERMETA_CRC)):
        places += [(name + "-content", content, bit), (name + "-trailer-low", end - 1, bit),
                   (name + "-trailer-high", end - 6, bit)]
    c = rel[4] + 13
    places += [("blob-before", c + 10, MF.BLOB_CRC), ("blob-inside", c + lo + 100, MF.BLOB_CRC),
               ("blob-after", c + n - 3, MF.BLOB_CRC), ("header", 5, MF.HEADER_CRC)]
    msgs = [put] + [RO._flip(put, at, 0x02) for _, at, _ in places]
    offs = [i * len(put) for i in range(len(msgs))]
    exp = check(messages, b"".join(msgs), offs, [len(put)] * len(msgs), RO.ALL, ranges=[(lo, hi)] * len(msgs), shift=5,
                oshift=2)
    assert exp[0] == [0] + [bit for _, _, bit in places], [name for (name, _, bit), s in zip(places, exp[0][1:]) if s != bit]


# ---------------------------------------------------------------- 4. counts and workspace
@functools.lru_cache(maxsize=None)
def small_case(m, flag):
    """m payloads of small messages of every stored format (content <= 600 B), 10 % corrupted, sent under `flag`
    by the send oracle."""
    region, offs, _ = RK.build_region(n=m, seed=2000 + m, corrupt_frac=0.1 if m > 1 else 0.0, big_every=10**9,
                                      max_blob=600, max_usermeta=300)
    _, sinfo, body = SO.expected(region, offs, None, flag)
    po, ps = [int(x) for x in sinfo["out_off"]], [int(x) for x in sinfo["send_len"]]
    return body, po, ps, RO.expected(body, po, ps, flag)


@pytest.mark.parametrize("m", [1, 2048, 2049])
@pytest.mark.parametrize("flag", [RO.BLOB, RO.ALL], ids=FLAG_NAMES.get)
def test_exact_workspace_between_guards(messages, flag, m):
    """A caller workspace of exactly ambrycrc_receive_workspace_size(m) between two guards, 0xA5 throughout: one
    payload, and the counts on either side of one plan block of the placement scan (2,048 entries)."""

    body, offs, sizes, exp = small_case(m, flag)
    if m > 1:
        clean, crc, refused = RO.mix(exp[0])
        assert clean >= 1000 and crc >= 20 and refused >= 20, (clean, crc, refused)
    whole, ws = guarded_workspace(messages.receive_workspace_bytes(m))
    check(messages, body, offs, sizes, flag, shift=17, oshift=5, workspace=ws, exp=exp)
    assert_guards(whole, ws)


@pytest.mark.parametrize("flag,side", [(RO.BLOB, "below"), (RO.BLOB, "above"), (RO.ALL, "below"), (RO.ALL, "above")])
def test_either_side_of_the_group_phase(messages, flag, side):
    """The CRC pass takes the sweep for every job below kGroupMinChunks jobs and its group phase from there on. The
    receive emits 3 jobs a payload under BLOB and 6 under ALL: m = 5,461 / 5,462 and 2,730 / 2,731 put the job
    count at 16,383 / 16,386 and 16,380 / 16,386."""
    per = JOBS[flag]
    m = (GROUP_MIN_CHUNKS - 1) // per + (1 if side == "above" else 0)
    assert (per * m >= GROUP_MIN_CHUNKS) == (side == "above") and abs(per * m - GROUP_MIN_CHUNKS) <= per
    body, offs, sizes, _ = small_case((GROUP_MIN_CHUNKS - 1) // per + 1, flag)
    exp = check(messages, body, offs[:m], sizes[:m], flag, shift=9, oshift=3)
    clean, crc, refused = RO.mix(exp[0])
    assert clean >= 2000 and crc >= 20 and refused >= 20, (clean, crc, refused)


# ---------------------------------------------------------------- 5. explicit destinations
def test_reverse_order(messages):
    """Every payload's slice where the caller says: the packed layout of the reversed batch."""
    body, offs, sizes, exp = small_case(2049, RO.BLOB)
    lens = [int(f["out_len"]) if int(f["out_off"]) != RO.NOWHERE else 0 for f in exp[1]]
    total = sum(lens)
    dst = [total - sum(lens[:i + 1]) for i in range(len(lens))]
    e2 = check(messages, body, offs, sizes, RO.BLOB, dst_off=dst, shift=1, oshift=7, out_cap=total)
    assert e2[0] == exp[0] and not (e2[2] == 0xA5).all()


def test_chunk_assembly(messages):
    """Five 4,096-byte data chunks of a composite blob, a byte range over the blob: dst_off = i * 4096 - lo0, the
    first chunk sliced to [lo0, 4096) and the last to [0, hi4). The output is blob[lo0 : 4 * 4096 + hi4]."""
    blob = stream_bytes(4242, 0, 5 * 4096).tobytes()
    recs = [RO._blob(blob[i * 4096:(i + 1) * 4096], 3) for i in range(5)]
    offs = [i * len(recs[0]) for i in range(5)]
    lo0, hi4 = 1000, 77
    ranges = [(lo0, 4096)] + [(0, RO.TO_END)] * 3 + [(0, hi4)]
    dst = [0] + [i * 4096 - lo0 for i in range(1, 5)]
    want = blob[lo0:4 * 4096 + hi4]
    got = run_gpu(messages, b"".join(recs), offs, [len(r) for r in recs], RO.BLOB, ranges=ranges, dst_off=dst, shift=2,
                  oshift=3, out_cap=len(want))
    assert got[0] == [0] * 5 and got[2].tobytes() == want
    assert [int(x) for x in got[1]["out_off"]] == dst and int(got[1]["out_len"].sum()) == len(want)
    RO.assert_outputs(got, RO.expected(b"".join(recs), offs, [len(r) for r in recs], RO.BLOB, ranges=ranges, dst_off=dst,
                                       out_cap=len(want)))


@pytest.mark.parametrize("explicit", [False, True], ids=["packed", "explicit"])
def test_no_room_at_exactly_the_need_and_one_less(messages, explicit):
    """out_cap exactly the need: everything fits. One byte less: the last slice is refused, its info zero, and
    no byte of it is written."""
    body, offs, sizes, exp = small_case(2048, RO.BLOB)
    need = len(exp[2])
    last = max(i for i, f in enumerate(exp[1]) if int(f["out_off"]) != RO.NOWHERE and int(f["out_len"]) > 0)
    assert int(exp[1][last]["out_off"]) + int(exp[1][last]["out_len"]) == need
    dst = [0 if int(f["out_off"]) == RO.NOWHERE else int(f["out_off"]) for f in exp[1]] if explicit else None
    e1 = check(messages, body, offs, sizes, RO.BLOB, dst_off=dst, oshift=1, out_cap=need)
    assert e1[0] == exp[0]
    e2 = check(messages, body, offs, sizes, RO.BLOB, dst_off=dst, oshift=1, out_cap=need - 1)
    diff = [i for i, (a, b) in enumerate(zip(e2[0], exp[0])) if a != b]  # (and empty slices placed at the very end)
    assert diff and diff[0] == last and all(e2[0][i] == RO.NO_ROOM and int(exp[1][i]["out_len"]) == 0 for i in diff[1:])
    assert e2[0][last] == RO.NO_ROOM


def test_no_room_advances_the_running_offset(messages):
    """out_cap ends inside a slice: that payload and every later one that does not fit are refused, the running
    offset advances past them, and nothing is written past the last placed slice."""
    body, offs, sizes = RO.sent_region(RO.ALL)
    cap = len(region_expected(RO.ALL, True)[2]) // 2 + 1
    exp = check(messages, body, offs, sizes, RO.ALL, shift=1, oshift=3, out_cap=cap, cpu=True)
    assert sum(1 for s in exp[0] if s == RO.NO_ROOM) >= 50


# ---------------------------------------------------------------- the rule table on the device
@pytest.mark.parametrize("flag", [RO.BLOB, RO.ALL], ids=FLAG_NAMES.get)
def test_each_rule(messages, flag):
    """recv_oracle.rule_cases() as one batch a flag (the cases with an output capacity of their own: one call
    each), then rule 1's cases that only a body has: an offset at and past the body's end, a size of 0, a size
    past the body -- and with a bad record there too, which rule 1 wins."""
    cases = [c for c in RO.rule_cases() if c[2] == flag]
    free = [c for c in cases if c[5] is None and len(c[1])]
    offs = [int(x) for x in np.cumsum([0] + [len(c[1]) for c in free[:-1]])]
    body = b"".join(c[1] for c in free)
    exp = check(messages, body, offs, [len(c[1]) for c in free], flag, ranges=[(c[3], c[4]) for c in free], shift=1, oshift=2)
    assert exp[0] == [c[6] for c in free]
    for c in cases:
        if c[5] is not None:
            e = check(messages, c[1], [0], [len(c[1])], flag, ranges=[(c[3], c[4])], out_cap=max(c[5], 1), oshift=1)
            assert e[0] == [c[6]], c[0]
    good = next(c[1] for c in free if c[6] == 0)
    bad = b"\x00\x09" + good[2:]
    body = good + bad
    n = len(good)
    offs = [0, 0, 0, n, 2 * n, 2 * n + 1, RO.NOWHERE, 0, n]
    sizes = [n, 0, 2 * n + 1, 0, 1, 1, 0, n - 1, n + 1]
    exp = check(messages, body, offs, sizes, flag, shift=7)
    assert exp[0][0] == 0 and exp[0][1:7] == [MF.BAD_LAYOUT] * 6 and exp[0][7] == MF.BAD_LAYOUT and exp[0][8] == MF.BAD_LAYOUT
    exp = check(messages, body, [0, n, 2 * n, RO.NOWHERE], None, flag, shift=7)
    assert exp[0] == [0, MF.BAD_VERSION, MF.BAD_LAYOUT, MF.BAD_LAYOUT]


def test_every_payload_refused_writes_nothing(messages):
    body, offs, sizes = RO.sent_region(RO.BLOB)
    st, info, out = run_gpu(messages, body, offs[:40], [0] * 40, RO.BLOB, shift=1, oshift=1, out_cap=4096)
    assert st == [MF.BAD_LAYOUT] * 40 and (info["out_off"] == RO.NOWHERE).all() and (out == 0xA5).all()
    assert not any(info[n].any() for n in RO.INFO.names[1:])


def test_invalid_arguments(messages):
    import torch

    body = torch.zeros(64, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    for flag in (0, 1, 4, 7):
        with pytest.raises(Exception):
            messages.receive_blobs_dev(body, offs, flag)
    with pytest.raises(Exception):
        messages.receive_blobs_dev(body, offs, RO.BLOB, workspace=torch.zeros(16, dtype=torch.uint8, device="cuda"))


# ---------------------------------------------------------------- 6. graph
@pytest.mark.parametrize("flag", [RO.BLOB, RO.ALL], ids=FLAG_NAMES.get)
def test_graph_capture_and_replay(messages, flag):
    """The call only enqueues work, so with a caller workspace it can be captured into a HIP graph and replayed:
    twice, over a body changed between the replays (one more payload corrupted), each with the eager result."""
    import torch

    body, offs, sizes = RO.sent_region(flag)
    ranges = RO.some_ranges(body, offs, sizes, flag)
    exp = RO.expected(body, offs, sizes, flag, ranges=ranges)
    victim = next(i for i, s in enumerate(exp[0]) if s == 0 and int(exp[1][i]["blob_size"]) > 100)
    at = offs[victim] + int(exp[1][victim]["content_rel"]) + 50
    body2 = RO._flip(body, at)
    exp2 = RO.expected(body2, offs, sizes, flag, ranges=ranges, out_cap=len(exp[2]))
    assert exp2[0][victim] == MF.BLOB_CRC and exp2[0] != exp[0]
    cap = len(exp[2])
    rw, r = guarded(body, 0)
    ow, o = guarded(b"", 3, cap)
    fresh_o = ow.clone()
    mo, ms, mr = u64_dev(offs), u64_dev(sizes), u64_dev(ranges)
    ws = torch.empty(messages.receive_workspace_bytes(len(offs)), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _, info0, st0 = messages.receive_blobs_dev(r, mo, flag, pay_size=ms, ranges=mr, out=o, workspace=ws)  # loads the kernels
        torch.cuda.synchronize()
        RO.assert_outputs((st0.cpu().numpy().view(np.uint32).tolist(), info0.cpu().numpy().view(RO.INFO),
                           guards_intact(ow, 3, cap).copy()), exp)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            _, info, st = messages.receive_blobs_dev(r, mo, flag, pay_size=ms, ranges=mr, out=o, workspace=ws)
    torch.cuda.synchronize()
    for b, e in ((body2, exp2), (body, exp)):
        r.copy_(torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda())
        ow.copy_(fresh_o)
        st.fill_(-1)
        info.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert guards_intact(rw, 0, len(b)).tobytes() == b
        RO.assert_outputs((st.cpu().numpy().view(np.uint32).tolist(), info.cpu().numpy().view(RO.INFO),
                           guards_intact(ow, 3, cap)), e)


# ---------------------------------------------------------------- 7. above the capped grids
@functools.lru_cache(maxsize=None)
def caps_tile(flag, layout):
    """scale_tiles.tile() sent under `flag` by the send oracle, and recv_oracle.expected over that one tile for
    the layout: (body, pay_off, pay_size, ranges or None, dst_off or None, the oracle's answers)."""
    import scale_tiles as S

    t = S.tile()
    _, sinfo, body = SO.expected(t.region, [int(o) for o in t.offs], None, flag)
    po, ps = [int(x) for x in sinfo["out_off"]], [int(x) for x in sinfo["send_len"]]
    ranges = dst = None
    if layout == "reversed-ranges":
        ranges = RO.some_ranges(body, po, ps, flag)
        free = RO.expected(body, po, ps, flag, ranges=ranges)
        lens = [int(f["out_len"]) if int(f["out_off"]) != RO.NOWHERE else 0 for f in free[1]]
        dst = [sum(lens) - sum(lens[:i + 1]) for i in range(len(lens))]
        exp = RO.expected(body, po, ps, flag, ranges=ranges, dst_off=dst, out_cap=sum(lens))
    else:
        exp = RO.expected(body, po, ps, flag)
    return body, po, ps, ranges, dst, exp


@pytest.mark.parametrize("layout", ["packed", "reversed-ranges", "capped"])
@pytest.mark.parametrize("flag", [RO.BLOB, RO.ALL], ids=FLAG_NAMES.get)
def test_receive_above_the_caps(gpu, messages, flag, layout):
    """The send oracle's body of tests/scale_tiles.py's tile, K times, at this device's m (more than twice the
    capped grid of 4 blocks a CU): every thread of recv_plan_kernel, recv_place_kernel and recv_finish_kernel
    takes a second and a third payload, a different tile message each trip, over slot-major arrays indexed
    k * m + i. The oracle judges one tile; statuses and infos are tiled with numpy and the output is compared
    on the device. packed: no ranges. reversed-ranges: a range for every payload and explicit destinations,
    the whole batch in reverse payload order. capped: packed into half the need -- NO_ROOM from the first slice
    that ends past the cap on, and no byte past the last placed slice changed."""
    import torch

    import scale_tiles as S

    k = S.copies_above_caps(torch.cuda.get_device_properties(0).multi_processor_count)
    body, po, ps, ranges, dst, (est, einfo, eout, loose) = caps_tile(flag, layout)
    clean, crc, refused = RO.mix(est)
    assert clean >= 100 and crc >= 10 and refused >= 100, (clean, crc, refused)
    p, nb = len(eout), np.uint64(len(body))
    copy = np.repeat(np.arange(k, dtype=np.uint64), S.T)
    sent = np.tile(np.array(po, dtype=np.uint64) != np.uint64(RO.NOWHERE), k)
    offs = np.where(sent, np.tile(np.array(po, dtype=np.uint64), k) + copy * nb, np.uint64(RO.NOWHERE))
    placed = np.tile(einfo["out_off"] != np.uint64(RO.NOWHERE), k)
    want_st, want_info, cap, end = np.tile(np.array(est, dtype=np.uint32), k), np.tile(einfo, k), k * p, k * p
    dst_dev = None
    if layout == "reversed-ranges":  # copy c lands at (k - 1 - c) * p
        back = (np.uint64(k - 1) - copy) * np.uint64(p)
        dst_dev = u64_dev(np.tile(np.array(dst, dtype=np.uint64), k) + back)
        want_info["out_off"] = np.where(placed, np.tile(einfo["out_off"], k) + back, np.uint64(RO.NOWHERE))
    elif layout == "capped":
        cap = k * p // 2
        want_st, want_info, end = S.tiled_recv_capped(est, einfo, k, cap)
        assert (want_st == RO.NO_ROOM).sum() >= 100 * (k // 2) and cap - end < 4096
    else:
        want_info["out_off"] = np.where(placed, np.tile(einfo["out_off"], k) + copy * np.uint64(p), np.uint64(RO.NOWHERE))
    tile_dev, out_tile, keep = dev(body), dev(eout), dev(~loose).bool()
    whole, region = copies(tile_dev, k)
    owhole, out = guarded(cap)
    _, info, status = messages.receive_blobs_dev(region, u64_dev(offs), flag, pay_size=u64_dev(np.tile(ps, k)),
                                                 ranges=None if ranges is None else u64_dev(np.tile(np.array(ranges, dtype=np.uint64), (k, 1))),
                                                 dst_off=dst_dev, out=out)
    torch.cuda.synchronize()
    assert_same(host(status, np.uint32), want_st, "status")
    got = host(info, np.uint8).view(RO.INFO)
    for name in RO.INFO.names:
        assert_same(got[name], want_info[name], name)
    assert_guards(owhole, out.numel())
    assert_guards(whole, region.numel())
    full, part = end // p, end % p  # whole copies of the tile's output, then the placed part of one more
    ne = (out[:full * p].view(full, p) != out_tile) & keep
    assert not bool(ne.any()), "output: copy %d, byte %d differs" % tuple(int(x) for x in ne.nonzero()[0])
    assert not bool(((out[full * p:end] != out_tile[:part]) & keep[:part]).any()), "the last, partial copy differs"
    assert bool((out[end:] == 0xA5).all()), "bytes written past the last placed slice"
    assert torch.equal(region.view(k, -1), tile_dev.expand(k, -1)), "the body changed"


# ---------------------------------------------------------------- 8. send -> receive on the device
def test_send_then_receive_on_the_device(messages):
    """ambrycrc_send_messages_dev(BLOB) over a stored region, its output fed to the receive with the info columns
    converted on the host: every message the verify finds clean delivers exactly the oracle's blob content."""
    import torch

    region, offs, _ = RK.build_region(n=300, seed=4)
    rw, r = guarded(region, 0)
    sent, sinfo, sst = messages.send_messages_dev(r, u64_dev(offs), SO.BLOB)
    torch.cuda.synchronize()
    si = sinfo.cpu().numpy().view(SO.INFO)
    body = sent[:max(int(si["send_len"].sum()), 1)]
    out, info, status = messages.receive_blobs_dev(body, u64_dev(si["out_off"]), RO.BLOB, pay_size=u64_dev(si["send_len"]))
    torch.cuda.synchronize()
    st, ri, host = status.cpu().numpy().view(np.uint32), info.cpu().numpy().view(RO.INFO), out.cpu().numpy()
    clean = 0
    for i, off in enumerate(offs):
        vst, vend = MF.verify_message(region, off)
        if vst or MF.parse_header(region, off)[2][2] != MF.INVALID:
            assert st[i] != 0 or vst & ~MF.BLOB_CRC, i  # a bad blob record never arrives clean
            continue
        clean += 1
        blob_rel = MF.parse_header(region, off)[2][4]
        est, ef, content = RO.receive_payload(region[off + blob_rel:vend], RO.BLOB)
        assert st[i] == 0 and est == 0
        assert (int(ri[i]["blob_size"]), int(ri[i]["out_len"])) == (len(content), len(content))
        assert host[int(ri[i]["out_off"]):int(ri[i]["out_off"]) + len(content)].tobytes() == content
    assert clean >= 200
    # and the whole batch as the oracle judges the body the device sent
    RO.assert_outputs((st.tolist(), ri, host[:int(ri["out_len"].sum())]),
                      RO.expected(sent.cpu().numpy().tobytes()[:body.numel()], [int(x) for x in si["out_off"]],
                                  [int(x) for x in si["send_len"]], RO.BLOB))
