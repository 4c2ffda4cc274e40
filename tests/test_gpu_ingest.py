"""GPU parity for ambrycrc_ingest_put_requests_dev against the oracle (tests/ingest_oracle.py:
oracle/message_format.py and zlib) and against the CPU entry: status, placement, every output byte, the wire
CRC, the MessageInfo and the packed length. The wire buffer and the output each sit inside a larger tensor with
64 guard bytes of 0xA5 on both sides, which must survive; the wire buffer must be unchanged."""
import functools

import numpy as np
import pytest

import ingest_oracle as IO
from gpu_buffers import assert_guards, guarded, guarded_workspace, guards_intact
from gpu_calls import assert_ingest_outputs, fetch_ingest, refs_tensor, run_ingest
from msgfmt import MF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def messages(gpu):
    from ambry_amd import messages as M

    assert M.PUT_REQUEST_REF_DTYPE == IO.REF
    return M


@functools.lru_cache(maxsize=None)
def case(seed, version=3):
    wire, refs, _ = IO.build_wire(300, seed)
    return wire, refs, IO.expected(wire, refs, version)


@pytest.mark.parametrize("shift,oshift", [(0, 0), (1, 7), (13, 0), (63, 7)])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_wire_matches_oracle_and_cpu(messages, seed, shift, oshift):
    """Every request version, SerDe V1-V5, keys and encryption keys absent and present, blobs up to 70 KB, 10 %
    refused over every status; the wire buffer at four offsets from a 64-B boundary and the output at two."""
    wire, refs, exp = case(seed)
    IO.assert_mix(wire, refs, exp[0])
    got = run_ingest(messages, wire, refs, shift, oshift)
    assert_ingest_outputs(got, exp)
    if shift == 0:
        buf = np.frombuffer(wire, dtype=np.uint8)
        for i, r in enumerate(refs):
            st, msg, crc, info = messages.ingest_put_request_cpu(buf, int(r["off"]), int(r["key_len"]),
                                                                 reserved=int(r["reserved"]))
            assert (st, crc) == (got[0][i], got[3][i])
            if st == 0:
                o, n = int(got[1][i]), int(got[2][i])
                assert msg == got[6][o:o + n].tobytes()
                assert info.tolist()[1:] == got[4][i].tolist()[1:]


@pytest.mark.parametrize("version", [1, 2])
def test_header_versions(messages, version):
    wire, refs, exp = case(2, version)
    assert_ingest_outputs(run_ingest(messages, wire, refs, shift=3, oshift=1, version=version), exp)


def test_two_refusal_causes_in_one_frame(messages):
    """IO.pair_wire() as one batch (test_ingest.py says what it holds, test_refusal_order's pairs among them):
    status, the wire CRC (0 where the parse refused), info, and nothing written for any of them. Then the same
    frames between clean ones, so refused requests sit among placed messages: every output byte."""
    wire, refs, pairs, _ = IO.pair_wire()
    exp = IO.expected(wire, refs)
    assert exp[0].all() and exp[6] == 0
    got = run_ingest(messages, wire, refs, shift=5, oshift=3)
    assert_ingest_outputs(got, exp)
    assert (got[1] == IO.NOWHERE).all() and not got[2].any() and not got[4].view(np.uint8).any()
    assert (got[6] == 0xA5).all()
    buf = np.frombuffer(wire, dtype=np.uint8)
    for i, r in enumerate(refs):
        st, msg, crc, _ = messages.ingest_put_request_cpu(buf, int(r["off"]), int(r["key_len"]),
                                                         reserved=int(r["reserved"]))
        assert (st, crc, msg) == (got[0][i], got[3][i], None), pairs[i]
    wire2, refs2, pairs2, _ = IO.pair_wire(clean_between=True)
    exp2 = IO.expected(wire2, refs2)
    assert all((p is None) == (st == 0) for p, st in zip(pairs2, exp2[0])) and len(pairs2) == 2 * len(pairs)
    assert_ingest_outputs(run_ingest(messages, wire2, refs2, shift=1, oshift=7), exp2)


# ---------------------------------------------------------------- the segment lattice
LENS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65)
BLOB_LENS = (255, 256, 257, 258, 4095, 4096, 4097, 4098, 16383, 16384, 16385, 16386, 65535, 65536, 65537, 131071,
             131072, 131073)


def lattice_frame(k, seg, n):
    """A V5 frame whose segment `seg` (0 blob id, 1 properties, 2 user metadata, 3 encryption key, 4 blob) has
    length n (the properties: their smallest, 39, plus n) and the others their fixed lengths; every content byte
    nonzero. Returns (frame, key_len, the segment's start in the frame)."""
    lens = [24, 0, 100, 32, 300]
    lens[seg] = n
    key, um, enc, blob = (IO.nonzero_bytes(7000 + k, j, lens[j]) for j in (0, 2, 3, 4))
    props = MF.blob_properties_bytes(lens[4], content_type="c" * lens[1], owner_id="", service_id="",
                                     serde_version=1 + k % 5, private=k % 3)
    fr = IO.frame(5, key, props, um, blob, blob_type=k % 2, enc_key=enc, compressed=k % 2, client_id=b"cl")
    starts = [IO.FIXED + 2]
    starts.append(starts[0] + lens[0])
    starts.append(starts[1] + len(props) + 4)
    starts.append(starts[2] + lens[2] + 4)
    starts.append(starts[3] + lens[3] + 9)
    return fr, lens[0], starts[seg]


@functools.lru_cache(maxsize=None)
def lattice(fill):
    """Each segment at every length of LENS and every wire residue mod 16, the blob also at BLOB_LENS and once at
    1 MiB + 4,109; then `fill` small clean frames, which lift the batch over the group phase's threshold."""
    cells = [(seg, n, r) for seg in range(5) for n in LENS for r in range(16)]
    cells += [(4, n, r) for n in BLOB_LENS for r in range(16)] + [(4, (1 << 20) + 4109, 11)]
    parts, refs, pos = [], [], 0
    for k, (seg, n, r) in enumerate(cells):
        fr, key_len, at = lattice_frame(k, seg, n)
        pad = (r - (pos + at)) % 16
        parts += [bytes(pad), fr]
        refs.append((pos + pad, key_len, 0))
        pos += pad + len(fr)
    for k in range(fill):
        fr, key_len, _ = lattice_frame(len(cells) + k, 4, 10 + k % 90)
        parts.append(fr)
        refs.append((pos, key_len, 0))
        pos += len(fr)
    wire, refs = b"".join(parts), np.array(refs, dtype=IO.REF)
    return wire, refs, IO.expected(wire, refs)


@pytest.mark.parametrize("fill", [0, 2100])
def test_segment_lattice(messages, fill):
    """The combination of the wire CRC and of each record CRC from the segment CRCs: the shift exponents and the
    empty-segment cases are per segment, so each varies on its own. Fewer than 16,384 jobs: every job in wave
    mode; at least 16,384: the small ones in the group phase."""
    wire, refs, exp = lattice(fill)
    assert (5 * len(refs) >= 16384) == (fill > 0)
    assert not exp[0].any()
    assert_ingest_outputs(run_ingest(messages, wire, refs, shift=0, oshift=5), exp)


# ---------------------------------------------------------------- workspaces, room, refused runs
@functools.lru_cache(maxsize=None)
def small_case(m):
    wire, refs, _ = IO.build_wire(m, 800 + m, refused=0.1 if m > 1 else 0.0, blobs=(0, 1, 63, 300, 600))
    return wire, refs, IO.expected(wire, refs)


@pytest.mark.parametrize("m", [1, 409, 410])
def test_exact_workspace_between_guards(messages, m):
    """A caller workspace of exactly ambrycrc_ingest_puts_workspace_size(m) between two guards, 0xA5 throughout:
    one request, and the counts on either side of one plan block (5 CRC jobs a request: 2,045 / 2,050 jobs)."""

    wire, refs, exp = small_case(m)
    whole, ws = guarded_workspace(messages.ingest_workspace_size(m))
    got = run_ingest(messages, wire, refs, shift=13, oshift=7, workspace=ws)
    assert_guards(whole, ws)
    assert_ingest_outputs(got, exp)


def test_no_room_in_the_middle(messages):
    wire, refs, full = case(3)
    cap = int(full[3].sum()) // 2 + 1
    exp = IO.expected(wire, refs, out_cap=cap)
    assert (exp[0] == IO.NO_ROOM).sum() >= 50 and exp[3].any() and exp[6] <= cap
    ends = full[2][full[3] > 0] + full[3][full[3] > 0]
    assert cap not in ends.tolist()  # the capacity ends inside a message
    assert_ingest_outputs(run_ingest(messages, wire, refs, shift=1, oshift=3, out_cap=cap), exp)


@pytest.mark.parametrize("where", ["start", "middle", "end"])
@pytest.mark.parametrize("run", [40, 64, 200])
def test_runs_of_refused_requests(messages, run, where):
    """`run` consecutive refused requests (every wire refusal by turns): their CRC jobs and copy jobs are empty,
    so every slot of the slot-major job arrays holds a run of empty jobs at one start."""
    rng = np.random.default_rng(run)
    clean = [IO.one_frame(rng, i, 31, None, 10 + i % 700) for i in range(300)]
    bad = [IO.one_frame(rng, 1000 + i, 31, IO.REFUSALS[i % len(IO.REFUSALS)], 50) for i in range(run)]
    first = {"start": 0, "middle": 150, "end": 300}[where]
    frames = clean[:first] + bad + clean[first:]
    refs, pos = np.zeros(len(frames), dtype=IO.REF), 0
    for i, (fr, key_len, reserved, delta) in enumerate(frames):
        refs[i] = (pos + delta, key_len, reserved)
        pos += len(fr)
    wire = b"".join(f[0] for f in frames)
    exp = IO.expected(wire, refs)
    assert exp[0][first:first + run].all() and (exp[0] != 0).sum() == run
    assert_ingest_outputs(run_ingest(messages, wire, refs, shift=1, oshift=7), exp)


def test_all_refused_writes_nothing(messages):
    wire, refs, exp = case(2)
    bad = np.nonzero(exp[0])[0]
    assert len(set(exp[0][bad].tolist())) == len(IO.WIRE_STATUSES)
    got = run_ingest(messages, wire, refs[bad], shift=1, oshift=1)
    assert np.array_equal(got[0], exp[0][bad]) and not got[2].any() and (got[1] == IO.NOWHERE).all()
    assert got[5] == 0 and (got[6] == 0xA5).all() and not got[4].view(np.uint8).any()


def test_empty_batch(messages):
    import torch

    wire = torch.full((256,), 0xA5, dtype=torch.uint8, device="cuda")
    refs = torch.empty(0, dtype=torch.uint8, device="cuda")
    junk = torch.full((1 << 16,), -1, dtype=torch.int64, device="cuda")  # what the next small allocations reuse
    del junk
    out = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
    res = messages.ingest_put_requests_dev(wire, refs, out=out)
    torch.cuda.synchronize()
    assert int(res[5].cpu()[0]) == 0 and res[1].numel() == 0 and res[6].numel() == 0
    assert bool((out == 0xA5).all()) and bool((wire == 0xA5).all())


# ---------------------------------------------------------------- round trip through recover
def test_round_trip_through_recover(messages):
    """ambrycrc_recover_messages_dev over d_out[0, total) chains exactly the clean requests, every status 0, and
    its MessageInfo equals the ingest's, entry for entry."""
    import torch

    from ambry_amd import device as D

    wire, refs, exp = case(1)
    ww, w = guarded(wire, 0)
    out, out_off, out_len, info, _, total, status = messages.ingest_put_requests_dev(w, refs_tensor(refs))
    torch.cuda.synchronize()
    n_total = int(total.cpu()[0])
    clean = np.nonzero(exp[0] == 0)[0]
    assert n_total == exp[6] and np.array_equal(status.cpu().numpy().view(np.uint32), exp[0])
    region = out[:n_total].clone()
    r_off, r_info, r_status, r_result = D.recover_messages(region, 0, max_messages=len(clean) + 8)
    torch.cuda.synchronize()
    res = D.recover_result(r_result)
    assert (int(res["chained"]), int(res["recovered"]), int(res["end_off"]), int(res["end_status"])) == \
        (len(clean), len(clean), n_total, 0)
    assert not r_status.cpu().numpy()[:len(clean)].any()
    assert np.array_equal(r_off.cpu().numpy()[:len(clean)].view(np.uint64), exp[2][clean])
    mine = np.frombuffer(info.cpu().numpy().tobytes(), dtype=IO.INFO)[clean]
    theirs = np.frombuffer(r_info.cpu().numpy().tobytes(), dtype=IO.INFO)[:len(clean)]
    assert np.array_equal(mine, theirs)


# ---------------------------------------------------------------- scale: past the capped grids
def test_scale_past_the_capped_grids(messages):
    """A tile of 1,201 mixed frames repeated on the device up to the smallest multiple past twice the widest capped
    grid of the per-request kernels (4 blocks a CU of 256 threads), so every thread loops; expectations derived
    per tile and compared on the device as (K, tile) views."""
    import torch

    wire, refs, exp = IO.tile_case()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    k = (2 * cus * 4 * 256) // IO.TILE + 1
    r, st, off, ln, crc, info = IO.tiled(refs, exp, k, len(wire))
    w = torch.from_numpy(np.frombuffer(wire, dtype=np.uint8).copy()).cuda().repeat(k)
    res = messages.ingest_put_requests_dev(w, refs_tensor(r))
    out, out_off, out_len, g_info, g_crc, total, status = res
    torch.cuda.synchronize()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    same = lambda t, a: bool(torch.equal(t.contiguous().view(torch.uint8).reshape(-1), dev(a)))  # noqa: E731
    assert same(status, st) and same(out_off, off) and same(out_len, ln) and same(g_crc, crc) and same(g_info, info)
    assert int(total.cpu()[0]) == k * exp[6]
    tile_out = torch.from_numpy(np.frombuffer(exp[1], dtype=np.uint8).copy()).cuda()
    assert bool((out[:k * exp[6]].view(k, exp[6]) == tile_out[None, :]).all())
    assert bool(torch.equal(w.view(k, len(wire))[k - 1], w[:len(wire)]))


# ---------------------------------------------------------------- graph capture
def test_graph_capture_and_replay(messages):
    """The call only enqueues work, so with a caller workspace it can be captured into a HIP graph and replayed
    after the wire bytes change, with the outputs of an uncaptured call over the new bytes."""
    import torch

    wire, refs, exp = case(1)
    wire2, refs2, exp2 = case(2)
    n = max(len(wire), len(wire2))
    m = len(refs)
    ww, w = guarded(wire, 0, n)
    cap = messages.ingest_out_bound(n, m)
    ow, o = guarded(b"", 3, cap)
    rt = refs_tensor(refs)
    ws = torch.empty(messages.ingest_workspace_size(m), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        first = messages.ingest_put_requests_dev(w, rt, out=o, workspace=ws)  # loads the kernels outside the capture
        torch.cuda.synchronize()
        assert_ingest_outputs(fetch_ingest(*first[1:]) + (guards_intact(ow, 3, cap),), exp)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            res = messages.ingest_put_requests_dev(w, rt, out=o, workspace=ws)
    torch.cuda.synchronize()
    for data, rr, want in ((wire2, refs2, exp2), (wire, refs, exp)):
        w.fill_(0xA5)
        w[:len(data)].copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
        rt.copy_(refs_tensor(rr))
        ow.fill_(0xA5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_ingest_outputs(fetch_ingest(*res[1:]) + (guards_intact(ow, 3, cap),), want)
