"""ambrycrc_receive_blob_cpu against the oracle (tests/recv_oracle.py: oracle/message_format.py, struct and zlib):
each rule of the entry once and which of two wins, status, info and every delivered byte over a region of every
stored format sent under BLOB and ALL, with and without ranges, the struct's layout, the pinned workspace size,
and recv.h -- the plan and the whole entry -- in a stand-alone program under ASan + UBSan."""
import os
import re
import shutil
import struct

import numpy as np
import pytest

import native_build
import recv_oracle as RO
import rekey_oracle as RK
from msgfmt import MF
from workspace_sizes import M_VALUES, recorded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_NAMES = {RO.BLOB: "blob", RO.ALL: "all"}


@pytest.fixture(scope="module")
def messages(ambry):
    from ambry_amd import messages as M

    assert M.RECV_INFO_DTYPE == RO.INFO
    assert (M.SEND_BLOB, M.SEND_ALL) == (RO.BLOB, RO.ALL)
    assert M.RECV_NOWHERE == RO.NOWHERE and M.RECV_TO_END == RO.TO_END
    assert M.MSG_NO_ROOM == RO.NO_ROOM and M.MSG_BAD_RANGE == RO.BAD_RANGE
    return M


def test_bad_range_is_a_bit_of_its_own():
    """No other AMBRYCRC_MSG_* bit of the header has BAD_RANGE's value."""
    text = open(os.path.join(ROOT, "include", "ambrycrc.h")).read()
    bits = re.findall(r"#define (AMBRYCRC_MSG_[A-Z_]+)\s+\(1u << (\d+)\)", text)
    assert ("AMBRYCRC_MSG_BAD_RANGE", "18") in bits
    assert [n for n, b in bits if int(b) == 18] == ["AMBRYCRC_MSG_BAD_RANGE"]
    assert len({b for _, b in bits}) == len(bits)


def _one(messages, case):
    name, payload, flag, lo, hi, cap, want = case
    st, info, got = messages.receive_blob_cpu(np.frombuffer(payload, dtype=np.uint8), flag, lo,
                                              None if hi == RO.TO_END else hi, out_cap=cap)
    return st, info, got


@pytest.mark.parametrize("case", RO.rule_cases(), ids=lambda c: c[0])
def test_each_rule(messages, case):
    """The status written out in the table, from the entry and from the oracle; then info and bytes as the
    oracle's. A refused payload reports nothing; one that fails only on CRCs still reports its info."""
    name, payload, flag, lo, hi, cap, want = case
    est, ef, eb = RO.receive_payload(payload, flag, lo, hi)
    if eb is not None and cap is not None and len(eb) > cap:
        est, ef, eb = RO.NO_ROOM, RO._zero_info(), None
    assert est == want, "the oracle gives %#x" % est
    st, info, got = _one(messages, case)
    assert st == want, "%#x" % st
    for n in RO.INFO.names:
        assert int(info[n]) == int(ef[n]), n
    if want & ~RO.CRC_BITS:
        assert got is None and int(info["out_off"]) == RO.NOWHERE
        assert not any(int(info[n]) for n in RO.INFO.names[1:])
    elif want == 0:
        assert got == eb
    else:
        assert got is not None and len(got) == len(eb)  # the bytes inside a CRC-failed span are unspecified


def test_the_table_covers_every_status(messages):
    seen = {c[6] for c in RO.rule_cases()}
    for bit in (MF.BAD_LAYOUT, MF.BAD_VERSION, MF.BAD_RECORD, MF.HEADER_CRC, MF.NOT_PUT, RO.BAD_RANGE, RO.NO_ROOM,
                MF.BLOB_CRC, MF.ENCKEY_CRC, MF.PROPS_CRC, MF.USERMETA_CRC, 0):
        assert bit in seen, hex(bit)


def test_delivered_fields_of_the_clean_shapes(messages):
    """What a caller reads out of info: the blob's type, the compressed byte, the versions, and under ALL the
    places of the key, the properties and the user metadata -- each checked against the payload's own bytes."""
    by = {c[0]: c for c in RO.rule_cases()}
    _, info, got = _one(messages, by["blob-metadata-type"])
    assert (int(info["blob_type"]), int(info["blob_version"]), int(info["content_rel"])) == (1, 2, 12)
    _, info, _ = _one(messages, by["blob-compressed"])
    assert (int(info["compressed"]), int(info["blob_version"]), int(info["header_version"])) == (1, 3, 0)
    _, info, got = _one(messages, by["blob-size-0-v1"])
    assert (int(info["out_len"]), int(info["blob_size"]), int(info["content_rel"]), got) == (0, 0, 10, b"")
    _, info, got = _one(messages, by["blob-range"])
    assert (int(info["out_len"]), int(info["blob_size"])) == (800, 1000) and got == by["blob-range"][1][113:913]
    payload = by["all-clean"][1]
    _, info, got = _one(messages, by["all-clean"])
    assert int(info["header_version"]) == 3 and int(info["blob_version"]) == 2
    key = payload[int(info["enckey_rel"]):int(info["enckey_rel"]) + int(info["enckey_len"])]
    assert key == b"k" * 32
    props = payload[int(info["props_rel"]):int(info["props_rel"]) + int(info["props_len"])]
    assert props == MF.blob_properties_bytes(1000)
    um = payload[int(info["usermeta_rel"]):int(info["usermeta_rel"]) + int(info["usermeta_len"])]
    assert len(um) == 50 and payload[int(info["usermeta_rel"]) - 4:int(info["usermeta_rel"])] == struct.pack(">i", 50)
    assert got == payload[int(info["content_rel"]):int(info["content_rel"]) + 1000]
    _, info, _ = _one(messages, by["all-clean-v1"])
    assert (int(info["header_version"]), int(info["enckey_rel"]), int(info["enckey_len"])) == (1, 0, 0)


@pytest.mark.parametrize("ranged", [False, True], ids=["whole", "ranges"])
@pytest.mark.parametrize("flag", [RO.BLOB, RO.ALL], ids=FLAG_NAMES.get)
def test_region_matches_oracle(messages, flag, ranged):
    """rekey_oracle.build_region(n=300) -- every stored format, update messages, 10 % corrupted, blobs to 300 KB --
    sent under `flag` by the send oracle and received payload by payload."""
    body, offs, sizes = RO.sent_region(flag)
    ranges = RO.some_ranges(body, offs, sizes, flag) if ranged else None
    exp = RO.expected(body, offs, sizes, flag, ranges=ranges)
    clean, crc, refused = RO.mix(exp[0])
    assert clean >= 100 and crc >= 1 and refused >= 1, (clean, crc, refused)
    if ranged:
        assert sum(1 for s in exp[0] if s == RO.BAD_RANGE) >= 5
    RO.assert_outputs(RO.run_cpu(messages, body, offs, sizes, flag, ranges=ranges), exp)


@pytest.mark.parametrize("flag", [RO.BLOB, RO.ALL], ids=FLAG_NAMES.get)
def test_no_room(messages, flag):
    """out_cap ends inside a slice: that payload and every later one that does not fit are refused."""
    body, offs, sizes = RO.sent_region(flag)
    full = RO.expected(body, offs, sizes, flag)
    cap = len(full[2]) // 2 + 1
    exp = RO.expected(body, offs, sizes, flag, out_cap=cap)
    assert sum(1 for s in exp[0] if s == RO.NO_ROOM) >= 50
    RO.assert_outputs(RO.run_cpu(messages, body, offs, sizes, flag, out_cap=cap), exp)


def test_invalid_arguments(messages):
    lib, buf = messages.lib(), np.zeros(64, dtype=np.uint8)
    info, st = np.zeros(1, dtype=RO.INFO), np.zeros(1, dtype=np.uint32)
    import ctypes

    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    for flag in (0, 1, 4, 5, -1):  # the metadata flags deliver no blob
        assert lib.ambrycrc_receive_blob_cpu(p(buf), 64, flag, 0, 0, p(buf), 64, p(info),
                                             st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))) != 0
    assert lib.ambrycrc_receive_blob_cpu(p(buf), 64, RO.BLOB, 0, 0, p(buf), 64, None,
                                         st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))) != 0


def test_workspace_size_is_pinned(messages):
    assert {str(m): messages.receive_workspace_bytes(m) for m in M_VALUES} == recorded("recv_workspace_size")


def _asan_payloads(path):
    """Clean payloads for tests/native/recv_asan.cpp: [u32 flag][u32 length][bytes] each."""
    from datagen import stream_bytes

    items = []
    for bv in (1, 2, 3):
        for n in (0, 1, 50, 300):
            items.append((RO.BLOB, RO._blob(stream_bytes(bv, n, n).tobytes(), bv, btype=n % 2 if bv > 1 else 0)))
    items.append((RO.BLOB, RO._blob(stream_bytes(9, 9, 5000).tobytes()) + b"\x77" * 19))  # trailing bytes
    for hv, bv, enc in ((1, 1, None), (2, 2, b"e" * 20), (3, 3, b"f" * 7), (3, 3, None)):
        items.append((RO.ALL, RK.stored_put(MF.store_key("asan-%d" % hv), MF.blob_properties_bytes(200, serde_version=1 + hv),
                                            stream_bytes(hv, 1, 33).tobytes(), stream_bytes(hv, 2, 200).tobytes(), hv=hv,
                                            enc_key=enc, bv=bv)))
    items.append((RO.ALL, items[-1][1] + b"\x55" * 11))
    with open(path, "wb") as f:
        for flag, b in items:
            assert RO.receive_payload(b, flag)[0] == 0
            f.write(struct.pack("<II", flag, len(b)) + b)
    return len(items)


@pytest.fixture(scope="module")
def asan_output(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("recv_asan")
    exe = tmp / "recv_asan"
    native_build.build_host_sanitized("recv_asan.cpp", exe, flags=native_build.HIP_HEADERS)
    n = _asan_payloads(tmp / "payloads.bin")
    out = native_build.run_harness(exe, [tmp / "payloads.bin"])
    return n, out


def test_plan_and_entry_under_asan(asan_output):
    """tests/native/recv_asan.cpp: recv.h's plan and the whole CPU entry over exactly-sized malloc'ed payloads --
    every truncation, single flipped bits, ranges and capacities -- and the workspace carved over its size."""
    n, out = asan_output
    runs = int(re.search(r"runs=(\d+)", out).group(1))
    assert runs > 1000 * n and "bad=0" in out and int(re.search(r"layouts=(\d+)", out).group(1)) >= 10


def test_struct_layout_matches_the_dtype(asan_output):
    """sizeof and every offsetof of ambrycrc_recv_info, printed by the native program, against RECV_INFO_DTYPE."""
    from ambry_amd import messages as M

    line = next(ln for ln in asan_output[1].splitlines() if ln.startswith("sizeof="))
    got = {k: int(v) for k, v in (kv.split("=") for kv in line.split())}
    assert got.pop("sizeof") == M.RECV_INFO_DTYPE.itemsize == 56
    assert got == {n: M.RECV_INFO_DTYPE.fields[n][1] for n in M.RECV_INFO_DTYPE.names}
