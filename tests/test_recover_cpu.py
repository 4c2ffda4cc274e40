"""ambrycrc_recover_messages_cpu against the oracle (tests/recover_oracle.py: oracle/message_format.py, zlib and
Python integers), the oracle itself against BlobStoreRecoveryTest's scenarios, the properties of the regions
test_gpu_recover.py runs on the device, and the entry under ASan + UBSan."""
import functools

import numpy as np
import pytest

import recover_oracle as RO
from msgfmt import MF
from oracle_common import LONG_MAX, wrap64
from recover_oracle import INFO_CASES


@pytest.fixture(scope="module")
def dev(ambry):
    from ambry_amd import device as D

    assert D.MESSAGE_INFO == RO.INFO and D.RECOVER_RESULT == RO.RESULT
    assert D.MSG_BAD_INFO == RO.BAD_INFO and D.NO_MESSAGE == RO.NO_MESSAGE
    return D


@functools.lru_cache(maxsize=None)
def mixed():
    return RO.mixed_region()


def check(dev, region, start=0, max_m=64):
    got = dev.recover_messages_cpu(region, start, max_m)
    exp = RO.recover(region, start, max_m)
    RO.assert_call(got, exp, max_m)
    return exp


# ---------------------------------------------------------------- the oracle, pinned to the reference's test
@pytest.mark.parametrize("hv", [1, 2, 3])
def test_oracle_recovers_the_reference_scenarios(dev, hv):
    """BlobStoreRecoveryTest.java:203-315 at each header version."""
    region, offs, sizes, now = RO.recovery_test_region(hv)
    got_offs, sts, infos, res = RO.recover(region)
    assert got_offs == offs and sts == [0] * 6
    assert res == {"chained": 6, "recovered": 6, "end_off": len(region), "end_status": 0, "more": 0}
    assert [f["size"] for f in infos] == sizes
    assert infos[0]["expires_at_ms"] == now + 9999 * 1000  # the first PUT carries ttl 9999
    assert [f["expires_at_ms"] for f in infos[1:]] == [-1] * 5
    flags = [0, 0, 0, RO.TTL_UPDATED, RO.DELETED, RO.TTL_UPDATED] if hv >= 2 else [0, 0, 0, 0, RO.DELETED, 0]
    assert [f["flags"] for f in infos] == flags
    for i, f in enumerate(infos):
        key = region[offs[i] + f["key_rel"]:offs[i] + f["key_rel"] + f["key_len"]]
        assert key[2:].startswith(b"id") and len(key) == 5
    check(dev, region)
    # a seventh message cut at half its size: six infos, a stop at startOffsets[6], a failure
    region, offs, _, _ = RO.recovery_test_region(hv, partial=True)
    _, sts, _, res = RO.recover(region)
    assert sts == [0] * 6 and res["recovered"] == 6 and res["end_off"] == offs[6] and res["end_status"] != 0
    check(dev, region)
    # an unknown version in the second header; a flipped byte of the second message's last CRC
    for pos, val in ((offs[1], None), (offs[2] - 8, None)):
        b = bytearray(region)
        if pos == offs[1]:
            b[pos:pos + 2] = (100).to_bytes(2, "big")
        else:
            b[pos] ^= 0xFF
        _, sts, _, res = RO.recover(bytes(b))
        assert res["recovered"] == 1 and res["end_off"] == offs[1] and res["end_status"] != 0 and res["more"] == 0
        check(dev, bytes(b))


# ---------------------------------------------------------------- the CPU entry
def test_mixed_region_clean_and_corrupt(dev):
    (clean, offs, _), (dirty, doffs, _) = mixed()
    exp = check(dev, clean, 0, 400)
    assert exp[0] == offs and exp[3]["recovered"] == 300 and exp[3]["end_off"] == len(clean)
    assert check(dev, clean, offs[137], 400)[0] == offs[137:]
    # one message in ten corrupted: recovery stops at the first bad one; restart after it to cover the rest
    start, stops, covered = 0, 0, 0
    while start < len(dirty):
        offs_e, sts, _, res = check(dev, dirty, start, 400)
        covered += res["recovered"]
        if res["end_off"] == len(dirty):
            break
        stops += 1
        nxt = [o for o in doffs if o > res["end_off"]]
        if not nxt:
            break
        start = nxt[0]
    assert stops >= 20 and covered >= 200, (stops, covered)


def test_info_edge_cases(dev):
    key = MF.store_key
    msgs, want = [], []
    for sv in range(1, 6):
        for hv in (1, 2, 3):
            msgs.append(RO.put_message(key("p%d%d" % (sv, hv)), b"c" * (sv * 7), hv=hv, serde_version=sv, ttl=77 + sv,
                                       account=300 + sv, container=-7, life=hv, filename="f" if sv % 2 else None))
            want.append(0)
    for name, props, st in INFO_CASES:
        msgs.append(RO.put_message(key(name), b"content", hv=3, **props))
        want.append(st)
    for uv in (1, 2, 3):
        for kind in ("delete", "ttl", "undelete"):
            for hv in (1, 2, 3):
                msgs.append(RO.update_message(key("u"), hv=hv, life=4, uv=uv, kind=kind, account=-3, container=9))
                want.append(0)
    msgs.append(RO.update_message(key("late"), uv=3, kind="undelete", when=-2))
    want.append(RO.BAD_INFO)
    msgs.append(RO.update_message(key("never"), uv=2, when=-1, account=-3))
    want.append(0)
    for m, st in zip(msgs, want):  # each alone: a refused message ends the clean prefix
        offs, sts, infos, _ = check(dev, m)
        assert sts == [st], m[:60]
    region, offs = RO.join([m for m, st in zip(msgs, want) if st == 0])
    _, sts, infos, res = check(dev, region, 0, 128)
    assert res["recovered"] == len(offs) == want.count(0)
    by = {region[o + f["key_rel"] + 2:o + f["key_rel"] + f["key_len"]].decode(): f for o, f in zip(offs, infos)}
    assert by["p11"]["account_id"] == -1 and by["p11"]["container_id"] == -1 and by["p23"]["account_id"] == 302
    assert by["p23"]["life_version"] == 3 and by["p22"]["life_version"] == 0
    assert by["ttl-forever"]["expires_at_ms"] == -1 and by["creation-forever"]["expires_at_ms"] == -1
    assert by["ttl-negative"]["expires_at_ms"] == 1_700_000_000_000 - 5000
    assert by["ttl-saturates"]["expires_at_ms"] == wrap64(1_700_000_000_000 + LONG_MAX) < 0
    assert by["wraps"]["expires_at_ms"] == wrap64((1 << 62) + 1 + LONG_MAX) < 0
    assert by["never"]["flags"] == RO.DELETED and by["never"]["operation_time_ms"] == -1
    flags = sorted({(f["flags"], f["account_id"]) for f in infos if f["flags"]})
    assert flags == [(1, -3), (1, -1), (2, -3), (4, -3)]  # Update_Format_V1: a delete with -1, -1, -1


def test_stop_cases(dev):
    seen = {}
    for name, region in RO.stop_cases():
        _, sts, _, res = check(dev, region, 0, 16)
        seen[name] = (res["chained"], res["recovered"], res["end_status"], res["more"])
    L, V, H = MF.BAD_LAYOUT, MF.BAD_VERSION, MF.HEADER_CRC
    assert seen["clean"] == (5, 5, 0, 0)
    assert seen["version"] == (1, 1, V, 0) and seen["version-0"] == (3, 3, V, 0)
    assert seen["header-crc"] == (2, 2, H, 0) and seen["size-flip"] == (1, 1, H, 0)
    assert seen["size-zero"] == (3, 3, L, 0) and seen["size-over"] == (4, 4, L, 0) and seen["size-negative"] == (1, 1, L, 0)
    assert seen["one-byte-short"] == (4, 4, L, 0) and seen["one-trailing"] == (5, 5, L, 0)
    assert seen["trailing-header"] == (5, 5, L, 0) and seen["trailing-version"] == (5, 5, V, 0)
    assert seen["record-enckey"] == (5, 0, MF.ENCKEY_CRC, 0) and seen["record-props"] == (5, 0, MF.PROPS_CRC, 0)
    assert seen["record-usermeta"] == (5, 0, MF.USERMETA_CRC, 0) and seen["record-blob"] == (5, 0, MF.BLOB_CRC, 0)
    assert seen["record-update"] == (5, 2, MF.UPDATE_CRC, 0)


def test_max_m_and_repeated_calls(dev):
    (clean, offs, _), (dirty, _, _) = mixed()
    whole = dev.recover_messages_cpu(clean, 0, 512)
    for max_m in (1, 7, 299, 300, 301):
        start, parts = 0, []
        while True:
            got = dev.recover_messages_cpu(clean, start, max_m)
            RO.assert_call(got, RO.recover(clean, start, max_m), max_m)
            n = int(got[3]["chained"])
            parts.append((got[0][:n], got[1][:n], got[2][:n]))
            if not got[3]["more"]:
                break
            assert n == max_m
            start = int(got[3]["end_off"])
        assert int(got[3]["end_off"]) == len(clean) and got[3]["end_status"] == 0
        for k in range(3):
            assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k][:300]), (max_m, k)
    # the chain hops over messages whose records fail; the result stops at the first
    _, sts, _, res = RO.recover(dirty, 0, 512)
    assert res["chained"] > res["recovered"] and any(s for s in sts)


def test_arguments(dev):
    from ambry_amd import AmbryCrcError

    (clean, offs, _), _ = mixed()
    got = dev.recover_messages_cpu(clean, len(clean), 4)  # start == region_len: a clean empty result
    RO.assert_call(got, ([], [], [], {"chained": 0, "recovered": 0, "end_off": len(clean), "end_status": 0, "more": 0}), 4)
    RO.assert_call(dev.recover_messages_cpu(b"", 0, 2), RO.recover(b"", 0, 2), 2)
    for start, max_m in ((len(clean) + 1, 4), (0, 0), (0, 1 << 31)):
        with pytest.raises(AmbryCrcError):
            dev.recover_messages_cpu(clean, start, max_m)
    for m in (1, 1000, 1 << 20):
        chain, rec = dev.chain_workspace_bytes(1 << 30, m), dev.recover_workspace_bytes(1 << 30, m)
        assert chain >= 28 * m + (1 << 30) // RO.scan_geometry()[0] * 4 and rec >= chain + dev.messages_workspace_bytes(m)


# ---------------------------------------------------------------- what the device tests' regions hold
def test_lattice_regions_cover_every_residue_and_straddle(dev):
    block, wave = RO.scan_geometry()
    assert block % wave == 0 and wave % 64 == 0
    region, offs = RO.residue_region()
    assert {o % 64 for o in offs} == set(range(64))
    check(dev, region, 0, 80)
    seen = set()
    for d in range(-40, 2):
        region, offs = RO.straddle_region(d)
        seen |= {(b, o - b) for o in offs for b in (wave, block, 2 * block) if -40 <= o - b <= 1}
        exp = check(dev, region, 0, 8)
        assert exp[3]["recovered"] == 5
    assert seen == {(b, d) for b in (wave, block, 2 * block) for d in range(-40, 2)}
    # -1: the version pair straddles the boundary; -39 .. -1: the longest header does
    assert all((b, -1) in seen and (b, -39) in seen for b in (wave, block, 2 * block))


def test_false_nodes_are_accepted_headers(dev):
    region, offs, inside = RO.false_node_region()
    assert dev.chain_messages_host(region, 0) == offs
    assert len(inside["region"]) == 50
    for p in inside["region"] + inside["lands"]:
        assert dev.chain_messages_host(region, p, 1) == [p]
    p = inside["lands"][0]
    assert dev.chain_messages_host(region, p, 4)[1] == offs[4]  # ... and hops onto a real message's start
    q = inside["overruns"][0]
    assert dev.chain_messages_host(region, q, 1) == [] and dev.chain_messages_host(region + b"\x00", q, 1) == [q]
    assert all(offs[1] < x < offs[2] for x in inside["region"]) and offs[2] < p < q < offs[3]
    assert check(dev, region, 0, 8)[3]["recovered"] == 6


def test_dense_false_nodes_exceed_the_staged_count(dev):
    region, offs, inside = RO.dense_false_node_region()
    block, stage = RO.scan_geometry(("kScanBlock", "kStageMax"))
    assert dev.chain_messages_host(region, 0) == offs
    assert dev.chain_messages_host(region, inside[0], 400) == inside  # each hops onto the next; then the blob's CRC
    per_block = np.bincount(np.asarray(inside) // block)
    assert per_block.max() > stage and len(per_block) >= 3
    assert check(dev, region, 0, 8)[3]["recovered"] == 4
    assert check(dev, region, inside[7], 512)[3]["chained"] == 293


def test_decoys_are_dense(dev):
    region, offs = RO.decoy_region()
    for i in (1, 2):
        assert RO.candidates(region[offs[i]:offs[i + 1]]) >= 20000
    assert check(dev, region, 0, 8)[3]["recovered"] == 4


def test_update_chain_message(dev):
    region, one = RO.update_chain(9)
    assert 80 <= one <= 100
    assert check(dev, region, 0, 16)[0] == [i * one for i in range(9)]


# ---------------------------------------------------------------- under the sanitizers
def test_recover_cpu_under_asan(tmp_path):
    """The CPU entry walks untrusted bytes: built with ASan + UBSan (host side) into a stand-alone program
    (tests/native/recover_asan.cpp) that runs it over every stop case, a corrupted region and the info edge
    cases, each as an exactly sized heap copy, from every message start and on every tail truncation."""
    import native_build
    import rekey_oracle as RK

    if not native_build.have_toolchain():
        pytest.skip("hipcc/g++ not available")
    regions = [r for _, r in RO.stop_cases()]
    regions.append(RK.build_region(n=40, seed=11, corrupt_frac=0.3, big_every=10**9)[0])
    regions.append(RO.join([RO.put_message(MF.store_key(n), b"content", hv=3, **p) for n, p, _ in INFO_CASES])[0])
    args = []
    for i, r in enumerate(regions):
        (tmp_path / ("r%d.bin" % i)).write_bytes(r)
        args.append(str(tmp_path / ("r%d.bin" % i)))
    exe = tmp_path / "recover_asan"
    native_build.build_sanitized("recover_asan.cpp", exe, tmp_path)
    out = native_build.run_harness(exe, args)
    assert "runs=" in out and "bad=0" in out
