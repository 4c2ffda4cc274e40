"""ambrycrc_hard_delete_message_cpu against the oracle (tests/hard_delete_oracle.py: oracle/message_format.py
and zlib): status, recovery info and the whole region after the delete, the plan_only / recovery phases
of HardDeleter (HardDeleter.java:655-700), hand-assembled record versions, and the entry under ASan + UBSan."""
import os

import numpy as np
import pytest

import hard_delete_oracle as HD
from datagen import stream_bytes
from msgfmt import MF
from regions import join, verify_region

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def device(ambry):
    from ambry_amd import device as D

    assert D.HARD_DELETE_INFO == HD.INFO
    return D


@pytest.fixture(scope="module", params=[(1, 17), (2, 17), (3, 17), (1, 10**9), (2, 10**9), (3, 10**9)],
                ids=lambda p: "seed%d-big%d" % p)
def corrupt_case(request):
    seed, big = request.param
    region, offs, _ = verify_region(n=300, seed=seed, corrupt_frac=0.1, big_every=big)
    return region, offs, HD.hard_delete(region, offs)


def test_region_matches_oracle(device, corrupt_case):
    region, offs, (est, einfo, eout) = corrupt_case
    deleted, refused, not_put, other = HD.counts(region, offs, est)
    assert deleted >= 200 and refused >= 20 and not_put >= 20 and other >= 1, (deleted, refused, not_put, other)
    st, info, out = HD.run_cpu(device, region, offs)
    assert st == est
    assert np.array_equal(info, einfo)
    assert out == eout


def test_plan_only_writes_nothing(device, corrupt_case):
    region, offs, (est, einfo, _) = corrupt_case
    st, info, out = HD.run_cpu(device, region, offs, plan_only=True)
    assert st == est
    assert np.array_equal(info, einfo)
    assert out == region


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_replay_with_recovery_info(device, seed):
    """HardDeleter's two phases: plan_only on the clean region gives the recovery info; a replay with it
    skips the record CRCs, so blobs corrupted in between are still deleted, with the expected bytes."""
    region, offs, _ = verify_region(n=300, seed=seed, corrupt_frac=0.0, big_every=17)
    est, einfo, eout = HD.hard_delete(region, offs)
    st, info, out = HD.run_cpu(device, region, offs, plan_only=True)
    assert st == est and np.array_equal(info, einfo) and out == region
    damaged, flipped = HD.flip_blob_bodies(region, offs, info)
    assert flipped >= 50
    st0, _, _ = HD.run_cpu(device, damaged, offs)
    assert sum(1 for s in st0 if s == MF.BLOB_CRC) == flipped  # without the info they are refused
    st, info2, out = HD.run_cpu(device, damaged, offs, recovery=info)
    assert st == est and all(s in (0, MF.NOT_PUT) for s in st)
    assert np.array_equal(info2, einfo)
    assert out == eout
    assert (st, out) == HD.hard_delete(damaged, offs, info)[::2]


def test_bad_recovery_info_is_refused(device):
    region, offs, _ = verify_region(n=30, seed=4, corrupt_frac=0.0, big_every=10**9)
    _, info, _ = HD.run_cpu(device, region, offs, plan_only=True)
    tried = 0
    for i, off in enumerate(offs):
        if int(info[i]["header_version"]) == 0 or int(info[i]["usermeta_size"]) == 0 or int(info[i]["blob_size"]) == 0:
            continue
        for r in HD.bad_recoveries(info[i]):
            buf = np.frombuffer(region, dtype=np.uint8).copy()
            st, inf = device.hard_delete_message_cpu(buf, off, r)
            assert st == MF.BAD_RECORD == HD.one(region, off, r)[0]
            assert inf.tobytes() == bytes(32) and buf.tobytes() == region
            tried += 1
    assert tried >= 7 * 10


def assembled_cases():
    """Hand-assembled PUT messages: blob record V1 / V2 / V3, blob type 1, stored isCompressed = 1, header
    V1 / V2 / V3, empty user metadata and an empty blob."""
    key = MF.store_key("hd-key")
    content = stream_bytes(77, 0, 777).tobytes()
    um = stream_bytes(78, 0, 33).tobytes()
    cases = []
    for hv in (1, 2, 3):
        for bv, bt, comp in ((1, 0, False), (2, 0, False), (2, 1, False), (3, 0, False), (3, 1, True), (3, 0, True)):
            for um_b, blob_b in ((um, content), (b"", content), (um, b""), (b"", b"")):
                msg = MF.put_message(key, MF.blob_properties_bytes(len(blob_b)), um_b, blob_b, version=hv,
                                     enc_key=b"k" * 16 if hv >= 2 else None, blob_version=3, blob_type=bt,
                                     compressed=comp)
                if bv != 3:  # swap the blob record (the last) for a V1 / V2 one and re-seal the header
                    v, total, rel = MF.parse_header(msg, 0)
                    rec = MF.blob_record_v1(blob_b) if bv == 1 else MF.blob_record(blob_b, version=2, blob_type=bt)
                    total += len(rec) - (len(msg) - rel[4])
                    msg = MF.header(v, total, *rel) + msg[MF.HEADER_SIZE[v]:rel[4]] + rec
                cases.append(((hv, bv, bt, comp, len(um_b), len(blob_b)), msg))
    return cases


def test_assembled_record_versions(device):
    cases = assembled_cases()
    region, offs = join([m for _, m in cases])
    est, einfo, eout = HD.hard_delete(region, offs)
    assert all(s == 0 for s in est)
    for (tag, _), inf in zip(cases, einfo):
        assert (int(inf["header_version"]), int(inf["blob_version"]), int(inf["blob_type"])) == tag[:3]
    st, info, out = HD.run_cpu(device, region, offs)
    assert st == est and np.array_equal(info, einfo) and out == eout
    # stored isCompressed = 1 comes out 0; every deleted message still verifies clean
    assert all(MF.verify_message(out, o)[0] == 0 for o in offs)
    comp = [i for i, (tag, _) in enumerate(cases) if tag[1] == 3 and tag[3]]
    assert comp
    for i in comp:
        blob = offs[i] + int(einfo[i]["start"]) + 14 + int(einfo[i]["usermeta_size"])
        assert region[blob + 4] == 1 and out[blob + 4] == 0
    # the second phase over the same messages
    st, info, out = HD.run_cpu(device, region, offs, recovery=einfo)
    assert st == est and np.array_equal(info, einfo) and out == eout


def test_offsets_past_the_region_are_refused(device):
    region, offs, _ = verify_region(n=5, seed=9, corrupt_frac=0.0, big_every=10**9)
    buf = np.frombuffer(region, dtype=np.uint8).copy()
    for off in (len(region), len(region) + 1, len(region) - 1, 2**63):
        st, inf = device.hard_delete_message_cpu(buf, off)
        assert st == MF.BAD_LAYOUT and int(inf["header_version"]) == 0
    cut = np.frombuffer(region[:offs[-1] + 50], dtype=np.uint8).copy()  # the last message truncated
    st, _ = device.hard_delete_message_cpu(cut, offs[-1])
    assert st == MF.BAD_LAYOUT == HD.one(region[:offs[-1] + 50], offs[-1])[0]
    assert buf.tobytes() == region and cut.tobytes() == region[:offs[-1] + 50]


def test_hard_delete_cpu_under_asan(tmp_path):
    """The CPU entry parses untrusted bytes and writes in place: built with ASan + UBSan (host side) into a
    stand-alone program (tests/native/hard_delete_asan.cpp) that runs it over every message of a region, every
    tail truncation, byte flips in the header and the two record heads, and random recovery structs, and checks
    that no byte outside [start, start + size) ever changes."""
    import subprocess

    import native_build

    if not native_build.have_toolchain():
        pytest.skip("hipcc/g++ not available")
    region, _, _ = verify_region(n=24, seed=11, corrupt_frac=0.0, big_every=10**9)
    rf = tmp_path / "region.bin"
    rf.write_bytes(region)
    rf2 = tmp_path / "region2.bin"
    rf2.write_bytes(b"".join(m for _, m in assembled_cases()[::5]))
    exe = tmp_path / "hard_delete_asan"
    native_build.build_sanitized("hard_delete_asan.cpp", exe, tmp_path)
    for f in (rf, rf2):
        out = native_build.run_harness(exe, [f])
        assert "runs=" in out and "bad=0" in out
