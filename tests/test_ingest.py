"""ambrycrc_ingest_put_request_cpu against the oracle (tests/ingest_oracle.py: oracle/message_format.py and zlib):
the oracle against the message-format oracle first, then status, every output byte, the wire CRC and the
MessageInfo over mixed wire buffers, each refusal on its own, the refusal order, the growth bound, the pinned
workspace size, and the wire parse and the workspace layout under ASan + UBSan as stand-alone programs."""
import functools
import shutil
import struct
import zlib

import numpy as np
import pytest

import ingest_oracle as IO
import native_build
from msgfmt import MF
from regions import put_request_fields
from workspace_sizes import M_VALUES, recorded

SEEDS = [1, 2, 3]


@pytest.fixture(scope="module")
def messages(ambry):
    from ambry_amd import messages as M

    assert M.PUT_REQUEST_REF_DTYPE == IO.REF
    assert (M.MSG_WIRE_CRC, M.INGEST_GROWTH_MAX) == (IO.WIRE_CRC, IO.GROWTH_MAX)
    return M


@functools.lru_cache(maxsize=None)
def case(seed):
    return IO.build_wire(300, seed)


def clean_frame(version=5, serde=3, key=b"K" * 24, um=b"u" * 100, blob=b"b" * 1000, enc=b"e" * 32, **kw):
    props = MF.blob_properties_bytes(len(blob), serde_version=serde)
    return IO.frame(version, key, props, um, blob, enc_key=enc if version >= 4 else b"", **kw), props


def run_cpu(M, wire, off, key_len, version=3, **kw):
    st, msg, crc, info = M.ingest_put_request_cpu(wire, off, key_len, header_version=version, **kw)
    return st, msg, crc, (tuple(info.tolist()) if st == 0 else None)


# ---------------------------------------------------------------- the oracle against itself
@pytest.mark.parametrize("version", [3, 4, 5])
@pytest.mark.parametrize("header", [1, 2, 3])
def test_oracle_message_is_put_message(version, header):
    key, um, blob, enc = b"K" * 24, b"u" * 100, bytes(range(1, 200)), b"e" * 32
    props = MF.blob_properties_bytes(len(blob), serde_version=2, private=2)
    fr = IO.frame(version, key, props, um, blob, blob_type=1, enc_key=enc if version >= 4 else b"", compressed=1)
    st, msg, crc, info = IO.ingest_request(fr, 0, len(key), header)
    assert st == 0
    f, _ = MF.parse_blob_properties(props, 0, len(props))
    want = MF.put_message(key, MF.serialize_blob_properties_v5(f), um, blob, version=header,
                          enc_key=enc if version >= 4 else None, compressed=version == 5, blob_type=1)
    assert msg == want
    assert MF.verify_message(msg, 0) == (0, len(msg))
    assert info[1] == len(msg) and info[4] == MF.HEADER_SIZE[header] and info[5] == len(key)
    if version == 5:
        assert crc == zlib.crc32(put_request_fields(key, props, um, 1, enc, True, len(blob)) + blob)


def test_oracle_mix():
    for seed in SEEDS:
        wire, refs, kinds = case(seed)
        st = IO.expected(wire, refs)[0]
        IO.assert_mix(wire, refs, st)
        assert all((k is None) == (s == 0) for k, s in zip(kinds, st))


# ---------------------------------------------------------------- the CPU entry
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("header", [1, 2, 3])
def test_cpu_matches_oracle(messages, seed, header):
    wire, refs, _ = case(seed)
    buf = np.frombuffer(wire, dtype=np.uint8)
    for r in refs:
        want = IO.ingest_request(wire, int(r["off"]), int(r["key_len"]), header, int(r["reserved"]))
        got = run_cpu(messages, buf, int(r["off"]), int(r["key_len"]), header, reserved=int(r["reserved"]))
        assert got == want
        if got[0] == 0:
            assert MF.verify_message(got[1], 0) == (0, len(got[1]))


EDITS = {  # a clean frame edited for each refusal: (frame keywords, expected status)
    "size_small": (dict(size=IO.MIN_FRAME - 1), IO.BAD_DESC),
    "size_negative": (dict(size=-1), IO.BAD_DESC),
    "size_past_wire": (dict(size=1 << 33), IO.BAD_DESC),
    "type": (dict(type_=1), IO.NOT_PUT),
    "version_2": (dict(wire_version=2), IO.BAD_VERSION),
    "version_6": (dict(wire_version=6), IO.BAD_VERSION),
    "client_negative": (dict(client_len=-1), IO.BAD_RECORD),
    "client_overrun": (dict(client_len=1 << 20), IO.BAD_RECORD),
    "um_negative": (dict(um_size=-1), IO.BAD_RECORD),
    "um_overrun": (dict(um_size=1 << 20), IO.BAD_RECORD),
    "blob_type_2": (dict(blob_type=2), IO.BAD_RECORD),
    "blob_type_negative": (dict(blob_type=-1), IO.BAD_RECORD),
    "enc_negative": (dict(enc_len=-1), IO.BAD_RECORD),
    "enc_overrun": (dict(enc_len=0x7FFF), IO.BAD_RECORD),
    "blob_negative": (dict(blob_size=-1), IO.BAD_RECORD),
    "blob_above_int": (dict(blob_size=IO.INT_MAX + 1), IO.BAD_RECORD),
    "blob_overrun": (dict(blob_size=1001), IO.BAD_RECORD),
    "crc_low": (dict(crc=0x12345678), IO.WIRE_CRC),
}


@pytest.mark.parametrize("name", sorted(EDITS))
def test_each_refusal(messages, name):
    kw, want = EDITS[name]
    fr, _ = clean_frame(**kw)
    assert IO.ingest_request(fr, 0, 24)[0] == want
    assert run_cpu(messages, fr, 0, 24) == IO.ingest_request(fr, 0, 24)


def test_reference_refusals(messages):
    fr, _ = clean_frame()
    wire = b"\0" * 7 + fr
    assert run_cpu(messages, wire, 7, 24)[0] == 0
    for off, key_len, reserved in [(len(wire) + 1, 24, 0), (len(wire) - 19, 24, 0), (8, 24, 0), (7, 24, 1)]:
        want = IO.ingest_request(wire, off, key_len, 3, reserved)
        assert want[0] == IO.BAD_DESC
        assert run_cpu(messages, wire, off, key_len, reserved=reserved) == want
    for key_len in (len(fr), 25, 23):  # the blob id overruns, or the properties start elsewhere
        want = IO.ingest_request(wire, 7, key_len)
        assert want[0] in (IO.BAD_RECORD, IO.WIRE_CRC)
        assert run_cpu(messages, wire, 7, key_len) == want
    assert IO.ingest_request(wire, 7, len(fr))[0] == IO.BAD_RECORD


def test_properties_refusals(messages):
    base = MF.blob_properties_bytes(10, serde_version=5)
    for props in (struct.pack(">h", 0) + base[2:], struct.pack(">h", 6) + base[2:],
                  base[:27] + struct.pack(">i", -1) + base[31:], base[:27] + struct.pack(">i", 1 << 24) + base[31:]):
        fr = IO.frame(5, b"K" * 24, props, b"um", b"0123456789")
        assert IO.ingest_request(fr, 0, 24)[0] == IO.BAD_RECORD
        assert run_cpu(messages, fr, 0, 24) == IO.ingest_request(fr, 0, 24)
    fr = IO.frame(5, b"K" * 24, MF.blob_properties_bytes(3, owner_id=b"\xc3\xa9"), b"um", b"abc")
    assert run_cpu(messages, fr, 0, 24)[0] == IO.NOT_ENCODABLE == IO.ingest_request(fr, 0, 24)[0]
    fr = IO.frame(5, b"K" * 24, MF.blob_properties_bytes(3, creation_ms=-2), b"um", b"abc")
    assert run_cpu(messages, fr, 0, 24)[0] == IO.BAD_INFO == IO.ingest_request(fr, 0, 24)[0]
    fr = IO.frame(5, b"K" * 24, MF.blob_properties_bytes(3, creation_ms=-1), b"um", b"abc")
    assert run_cpu(messages, fr, 0, 24)[0] == 0


@pytest.mark.parametrize("version", [3, 4, 5])
def test_flip_in_each_segment_is_wire_crc(messages, version):
    fr, props = clean_frame(version)
    body = IO.FIXED
    marks = {"key": body + 3, "props": body + 24 + 5, "um": body + 24 + len(props) + 4 + 50, "blob": len(fr) - 9,
             "crc_high": len(fr) - 8 + 1, "crc_low": len(fr) - 1}
    if version >= 4:
        marks["enc"] = body + 24 + len(props) + 4 + 100 + 4 + 9
    for name, at in marks.items():
        bad = fr[:at] + bytes([fr[at] ^ 1]) + fr[at + 1:]
        want = IO.ingest_request(bad, 0, 24)
        assert want[0] == IO.WIRE_CRC, name
        assert run_cpu(messages, bad, 0, 24) == want, name


def test_refusal_order(messages):
    # each frame qualifies for the two refusals named; the first in the reference's order wins
    pairs = [
        (dict(size=-1, type_=1), IO.BAD_DESC),                  # BAD_DESC before NOT_PUT
        (dict(type_=1, wire_version=9), IO.NOT_PUT),            # NOT_PUT before BAD_VERSION
        (dict(wire_version=9, client_len=-1), IO.BAD_VERSION),  # BAD_VERSION before BAD_RECORD
        (dict(um_size=-1, crc=1), IO.BAD_RECORD),               # BAD_RECORD before WIRE_CRC
    ]
    for kw, want in pairs:
        fr, _ = clean_frame(**kw)
        assert IO.ingest_request(fr, 0, 24)[0] == want
        assert run_cpu(messages, fr, 0, 24)[0] == want
    late = [
        (dict(owner_id=b"\xff", creation_ms=-2), dict(crc=1), IO.WIRE_CRC),  # WIRE_CRC before NOT_ENCODABLE
        (dict(owner_id=b"\xff", creation_ms=-2), {}, IO.NOT_ENCODABLE),      # NOT_ENCODABLE before BAD_INFO
    ]
    for pk, kw, want in late:
        fr = IO.frame(5, b"K" * 24, MF.blob_properties_bytes(3, **pk), b"um", b"abc", **kw)
        assert IO.ingest_request(fr, 0, 24)[0] == want
        assert run_cpu(messages, fr, 0, 24)[0] == want
    fr = IO.frame(5, b"K" * 24, MF.blob_properties_bytes(3, creation_ms=-2), b"um", b"abc")  # BAD_INFO before NO_ROOM
    assert run_cpu(messages, fr, 0, 24, out_cap=1)[0] == IO.BAD_INFO
    fr, _ = clean_frame()
    assert run_cpu(messages, fr, 0, 24, out_cap=1)[0] == IO.NO_ROOM


@functools.lru_cache(maxsize=None)
def single_refusal_status():
    """{cause: the oracle's status of a frame built with that cause alone}."""
    out = {}
    for a in IO.REFUSALS:
        fr, key_len, reserved, delta = IO.one_frame(np.random.default_rng(1), 7, 5, a, 50)
        out[a] = IO.ingest_request(fr, delta, key_len, 3, reserved)[0]
    return out


def test_two_refusal_causes_in_one_frame(messages):
    """IO.pair_wire(): every pair of REFUSALS one frame can hold (the five left out write one field twice). The
    oracle gives each frame the status of whichever of its two causes the reference reaches first (PutRequest
    .readFrom's order: WIRE_STATUSES), so every wire status wins a pair -- but BAD_INFO: it is the last check and
    has one cause (the creation time), so it loses all 23 of its pairs, which is asserted instead. The CPU entry
    against the oracle: status, the wire CRC (0 where the parse refused), no message and no info."""
    wire, refs, pairs, skipped = IO.pair_wire()
    assert len(pairs) + len(skipped) == len(IO.REFUSALS) * (len(IO.REFUSALS) - 1) // 2 and len(skipped) == 5
    single, order = single_refusal_status(), IO.WIRE_STATUSES.index
    assert set(single.values()) == set(IO.WIRE_STATUSES)
    buf = np.frombuffer(wire, dtype=np.uint8)
    winners, parsed = set(), 0
    for (a, b), r in zip(pairs, refs):
        want = IO.ingest_request(wire, int(r["off"]), int(r["key_len"]), 3, int(r["reserved"]))
        assert want[0] == min(single[a], single[b], key=order) and want[1] is None and want[3] is None, (a, b)
        assert (want[2] != 0) == (want[0] in (IO.WIRE_CRC, IO.NOT_ENCODABLE, IO.BAD_INFO)), (a, b)
        parsed += want[2] != 0
        winners.add(want[0])
        if "creation" in (a, b):
            assert want[0] == single[a if b == "creation" else b] != IO.BAD_INFO, (a, b)
        got = run_cpu(messages, buf, int(r["off"]), int(r["key_len"]), reserved=int(r["reserved"]))
        assert got == want, (a, b)
    assert winners == set(IO.WIRE_STATUSES) - {IO.BAD_INFO} and parsed >= 20


def test_trailing_slack_is_tolerated(messages):
    for version in (3, 4, 5):
        fr, _ = clean_frame(version, slack=11)
        plain, _ = clean_frame(version)
        want = IO.ingest_request(fr, 0, 24)
        assert want[0] == 0 and want[1:] == IO.ingest_request(plain, 0, 24)[1:]
        assert run_cpu(messages, fr, 0, 24) == want


def test_out_bound(messages):
    # the worst case, built explicitly: a V4 request, encryption key present, SerDe V1, empty client id
    props = MF.blob_properties_bytes(5, serde_version=1)
    fr = IO.frame(4, b"K" * 24, props, b"um", b"hello", enc_key=b"e" * 16, client_id=b"")
    st, msg, _, _ = IO.ingest_request(fr, 0, 24, 3)
    assert st == 0 and len(msg) - len(fr) == IO.GROWTH_MAX
    assert run_cpu(messages, fr, 0, 24, out_cap=len(fr) + IO.GROWTH_MAX)[1] == msg
    assert messages.ingest_out_bound(1000, 3) == 1000 + 3 * IO.GROWTH_MAX
    assert messages.ingest_out_bound((1 << 64) - 10, 1) == (1 << 64) - 1
    for seed in SEEDS:
        wire, refs, _ = case(seed)
        for header in (1, 2, 3):
            for r in refs:
                st, msg, _, _ = IO.ingest_request(wire, int(r["off"]), int(r["key_len"]), header)
                if st == 0:
                    size = struct.unpack_from(">q", wire, int(r["off"]))[0]
                    assert len(msg) - size <= IO.GROWTH_MAX


def test_workspace_size_is_pinned(messages):
    assert {str(m): messages.ingest_workspace_size(m) for m in M_VALUES} == recorded("ingest_workspace_size")


def _asan_program(tmp_path, name):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / name
    native_build.build_host_sanitized(name + ".cpp", exe, flags=native_build.HIP_HEADERS)
    return native_build.run_harness(exe, timeout=300)


def test_wire_parse_under_asan(tmp_path):
    """tests/native/put_request_asan.cpp: the wire parse, the verdict and the MessageInfo over exactly-sized
    malloc'ed frames -- every truncation length of a clean frame of each version, and seeded mutations."""
    out = _asan_program(tmp_path, "put_request_asan")
    assert "frames=" in out and "bad=0" in out


def test_ingest_layout_under_asan(tmp_path):
    """tests/native/ingest_ws_asan.cpp: the ingest workspace carved over exactly its measured size and written
    end to end."""
    out = _asan_program(tmp_path, "ingest_ws_asan")
    assert "layouts=" in out and "bad=0" in out


def test_tile_derivation():
    """What test_gpu_ingest's scale test derives per tile (IO.tiled) equals the oracle over two concatenated
    tiles."""
    wire, refs, exp = IO.tile_case()
    IO.assert_mix(wire, refs, exp[0])
    r2, st, off, ln, crc, info = IO.tiled(refs, exp, 2, len(wire))
    two = IO.expected(wire * 2, r2)
    assert np.array_equal(two[0], st) and np.array_equal(two[2], off) and np.array_equal(two[3], ln)
    assert np.array_equal(two[4], crc) and np.array_equal(two[5], info)
    assert two[1] == exp[1] * 2 and two[6] == 2 * exp[6]
