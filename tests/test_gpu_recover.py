"""GPU parity for ambrycrc_chain_messages_dev and ambrycrc_recover_messages_dev against the CPU entry and the
oracle (tests/recover_oracle.py), bit for bit: offsets, statuses, every info field, the result struct, the
UINT64_MAX fill and the zeroed infos. The region sits inside a larger tensor with 64 guard bytes of 0xA5 on
both sides. test_recover_cpu.py proves on the CPU what the lattice, false-node and decoy regions hold."""
import functools

import numpy as np
import pytest

import recover_oracle as RO
import rekey_oracle as RK
from gpu_buffers import assert_guards, dev as to_dev, guarded, guarded_workspace, guards_intact
from gpu_calls import assert_chain, copies, recover_to_numpy, run_recover
from msgfmt import MF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu):
    from ambry_amd import device as D

    assert D.MESSAGE_INFO == RO.INFO and D.RECOVER_RESULT == RO.RESULT
    return D


def same_as_cpu(got, cpu):
    assert np.array_equal(got[0], cpu[0]) and np.array_equal(got[2], cpu[2]) and got[3] == cpu[3]
    for name in RO.INFO.names:
        assert np.array_equal(got[1][name], cpu[1][name]), name


def check(dev, region, start=0, max_m=64, shift=0, oracle=True):
    """Chain and recover on the device against the CPU entry, and the oracle unless the region is large."""
    cpu = dev.recover_messages_cpu(region, start, max_m)
    got = run_recover(dev, region, start, max_m, shift)
    same_as_cpu(got, cpu)
    if oracle:
        RO.assert_call(got, RO.recover(region, start, max_m), max_m)
        assert_chain(run_recover(dev, region, start, max_m, shift, chain=True), *RO.chain_result(region, start, max_m),
                     max_m)
    return got


@functools.lru_cache(maxsize=None)
def mixed():
    return RO.mixed_region()


# ---------------------------------------------------------------- regions of every stored format
@pytest.mark.parametrize("shift", [0, 5])
def test_mixed_region(dev, shift):
    (clean, offs, _), (dirty, doffs, _) = mixed()
    got = check(dev, clean, 0, 400, shift)
    assert int(got[3]["recovered"]) == 300 and int(got[3]["end_off"]) == len(clean)
    check(dev, clean, offs[137], 200, shift)
    check(dev, clean, offs[299], 3, shift)
    check(dev, dirty, 0, 400, shift)
    check(dev, dirty, doffs[150], 400, shift)
    check(dev, clean, len(clean), 4, shift)  # start == region_len: a clean empty result


@functools.lru_cache(maxsize=None)
def exact_case(max_m):
    """Small messages of every stored format, one in twenty corrupted, ten more than max_m of them, and the
    oracle's recover and chain answers (this seed: no header among the first 410 is hit, so the chain fills
    every slot)."""
    region, _, _ = RK.build_region(n=max_m + 10, seed=1101, corrupt_frac=0.05, big_every=10**9, max_blob=600,
                                   max_usermeta=300)
    return region, RO.recover(region, 0, max_m), RO.chain_result(region, 0, max_m)


@pytest.mark.parametrize("max_m", [1, 409, 410])
def test_exact_workspace_between_guards(dev, max_m):
    """Caller workspaces of exactly ambrycrc_recover_workspace_bytes and ambrycrc_chain_workspace_bytes between
    two guards, 0xA5 throughout: one slot, and the counts on either side of one plan block of the verify
    (5 jobs a message: 2,045 / 2,050 jobs), every slot filled. Both calls against the oracle and recover
    against the CPU entry; the workspaces' guards intact."""

    region, exp, (coffs, cres) = exact_case(max_m)
    assert exp[3]["chained"] == cres["chained"] == max_m
    assert max_m == 1 or 10 <= sum(1 for s in exp[1] if s) <= max_m // 8  # refused and accepted messages both
    whole, ws = guarded_workspace(dev.recover_workspace_bytes(len(region), max_m))
    got = run_recover(dev, region, 0, max_m, shift=5, workspace=ws)
    assert_guards(whole, ws)
    same_as_cpu(got, dev.recover_messages_cpu(region, 0, max_m))
    RO.assert_call(got, exp, max_m)
    whole, ws = guarded_workspace(dev.chain_workspace_bytes(len(region), max_m))
    got = run_recover(dev, region, 0, max_m, shift=5, chain=True, workspace=ws)
    assert_guards(whole, ws)
    assert_chain(got, coffs, cres, max_m)


def test_reference_scenarios(dev):
    for hv in (1, 2, 3):
        for partial in (False, True):
            region = RO.recovery_test_region(hv, partial)[0]
            assert int(check(dev, region, 0, 8)[3]["recovered"]) == 6


def test_max_m_and_repeated_calls(dev):
    (clean, offs, _), _ = mixed()
    whole = dev.recover_messages_cpu(clean, 0, 512)
    for max_m in (7, 299, 300, 301):
        start, parts = 0, []
        while True:
            got = check(dev, clean, start, max_m, oracle=max_m >= 299)
            n = int(got[3]["chained"])
            parts.append((got[0][:n], got[1][:n], got[2][:n]))
            if not got[3]["more"]:
                break
            start = int(got[3]["end_off"])
        for k in range(3):
            assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k][:300]), (max_m, k)


# ---------------------------------------------------------------- where a message may start
def test_start_lattice(dev):
    region, offs = RO.residue_region()
    assert [int(x) for x in check(dev, region, 0, 80)[0][:65]] == offs
    for d in range(-40, 2):
        region, offs = RO.straddle_region(d)
        got = check(dev, region, 0, 8, oracle=d in (-40, -39, -2, -1, 0, 1))
        assert [int(x) for x in got[0][:5]] == offs and int(got[3]["recovered"]) == 5, d
        got = check(dev, region, offs[1], 8, shift=3, oracle=False)  # the blocks then count from another place
        assert [int(x) for x in got[0][:4]] == offs[1:], d


# ---------------------------------------------------------------- headers inside blob content
def test_false_nodes(dev):
    region, offs, inside = RO.false_node_region()
    got = check(dev, region, 0, 128)
    assert [int(x) for x in got[0][:6]] == offs and int(got[3]["chained"]) == 6
    embedded = set(inside["region"] + inside["lands"] + inside["overruns"])
    assert not embedded & {int(x) for x in got[0][:6]}
    # started inside the blob, the embedded headers are the chain
    p = inside["lands"][0]
    got = check(dev, region, p, 16)
    assert [int(x) for x in got[0][:3]] == [p, offs[4], offs[5]]
    check(dev, region, inside["region"][0], 64)
    check(dev, region, inside["overruns"][0], 4)
    # more false nodes before the chain's end than max_m: calls repeated while `more` is set make the same chain
    for max_m in (1, 4, 8, 51):
        start, chained, calls = 0, [], 0
        while True:
            msg_off, res = run_recover(dev, region, start, max_m, chain=True)
            chained += [int(x) for x in msg_off[:int(res["chained"])]]
            calls += 1
            assert all(int(x) == RO.NO_MESSAGE for x in msg_off[int(res["chained"]):])
            if not res["more"]:
                break
            assert int(res["end_off"]) > start and res["end_status"] == 0
            start = int(res["end_off"])
        assert chained == offs and int(res["end_off"]) == len(region) and res["end_status"] == 0, max_m
        assert calls <= 7  # every call chains at least the message it starts on


def test_dense_false_nodes(dev):
    """More nodes in a scan block than the scan stages: those blocks are read again."""
    region, offs, inside = RO.dense_false_node_region()
    for shift in (0, 9):
        got = check(dev, region, 0, 512, shift)
        assert [int(x) for x in got[0][:4]] == offs and int(got[3]["chained"]) == 4
        got = check(dev, region, inside[0], 512, shift)
        assert [int(x) for x in got[0][:300]] == inside and got[3]["end_status"] != 0
        got = check(dev, region, inside[150], 100, shift)  # max_m inside the dense blocks
        assert int(got[3]["chained"]) == 100 and got[3]["end_status"] != 0  # (no embedded header verifies)
        _, res = run_recover(dev, region, inside[150], 100, shift, chain=True)
        assert int(res["chained"]) == 100 and res["more"] == 1 and int(res["end_off"]) == inside[250]
    for max_m in (3, 70, 299):
        msg_off, res = run_recover(dev, region, 0, max_m, chain=True)
        assert [int(x) for x in msg_off[:int(res["chained"])]] == offs[:int(res["chained"])]
        assert (res["more"] == 1) == (int(res["chained"]) < 4)


def test_decoys(dev):
    region, offs = RO.decoy_region()
    got = check(dev, region, 0, 16)
    assert [int(x) for x in got[0][:4]] == offs and int(got[3]["recovered"]) == 4
    check(dev, region, 0, 16, shift=1)
    check(dev, region, offs[2], 2, shift=2)


# ---------------------------------------------------------------- the doubling rounds
@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 9, 4095, 4096, 4097, 65537])
def test_doubling_rounds(dev, n):
    import torch

    region, one = RO.update_chain(n)
    rw, r = guarded(region, 0)
    want = np.arange(n, dtype=np.uint64) * np.uint64(one)
    pow2 = 1 << max(n - 1, 1).bit_length()
    for max_m in sorted({n, n - 1, pow2} - {0}):
        msg_off, res = recover_to_numpy(dev.chain_messages(r, 0, max_m))
        k = min(n, max_m)
        assert int(res["chained"]) == k and np.array_equal(msg_off[:k], want[:k]), max_m
        assert (msg_off[k:] == np.uint64(RO.NO_MESSAGE)).all()
        if max_m < n:
            assert res["more"] == 1 and int(res["end_off"]) == k * one and res["end_status"] == 0
            tail, res2 = recover_to_numpy(dev.chain_messages(r, int(res["end_off"]), max_m))
            assert int(res2["chained"]) == 1 and int(tail[0]) == k * one  # the follow-up call completes it
            res = res2
        assert res["more"] == 0 and int(res["end_off"]) == len(region) and res["end_status"] == 0
    if n <= 4097:
        got = recover_to_numpy(dev.recover_messages(r, 0, n + 3))
        same_as_cpu(got, dev.recover_messages_cpu(region, 0, n + 3))
        assert int(got[3]["recovered"]) == n
    torch.cuda.synchronize()
    guards_intact(rw, 0, len(region))


# ---------------------------------------------------------------- where and why recovery stops
def test_stops(dev):
    for name, region in RO.stop_cases():
        for shift in (0, 7):
            got = check(dev, region, 0, 9, shift)
            n = int(got[3]["chained"])
            assert (got[0][n:] == np.uint64(RO.NO_MESSAGE)).all(), name
            zero = np.zeros(1, dtype=RO.INFO)[0]
            assert all(got[1][i] == zero for i in range(9) if i >= n or got[2][i] != 0), name
    from ambry_amd import AmbryCrcError

    _, r = guarded(b"\x00" * 64, 0)
    for start, max_m in ((65, 4), (0, 0), (0, 1 << 31)):
        for fn in (dev.chain_messages, dev.recover_messages):
            with pytest.raises(AmbryCrcError):
                fn(r, start, max_m, out=tuple([r] * (2 if fn is dev.chain_messages else 4)))


def test_info_edge_cases(dev):
    from recover_oracle import INFO_CASES

    key = MF.store_key
    msgs = [RO.put_message(key("p%d%d" % (sv, hv)), b"c" * (sv * 7), hv=hv, serde_version=sv, ttl=77 + sv,
                           account=300 + sv, container=-7, life=hv) for sv in range(1, 6) for hv in (1, 2, 3)]
    msgs += [RO.put_message(key(name), b"content", hv=3, **props) for name, props, st in INFO_CASES if st == 0]
    msgs += [RO.update_message(key("u"), hv=hv, life=4, uv=uv, kind=kind, account=-3, container=9)
             for uv in (1, 2, 3) for kind in ("delete", "ttl", "undelete") for hv in (1, 2, 3)]
    bad = [RO.put_message(key("creation-bad"), b"content", creation_ms=-2),
           RO.update_message(key("late"), uv=3, kind="undelete", when=-2)]
    region, offs = RO.join(msgs + bad + msgs[:3])
    got = check(dev, region, 0, 128)
    assert int(got[3]["recovered"]) == len(msgs) and got[3]["end_status"] == RO.BAD_INFO
    assert int(got[3]["chained"]) == len(offs) and list(got[2][len(msgs):len(msgs) + 2]) == [RO.BAD_INFO] * 2


# ---------------------------------------------------------------- the verify's unused slots
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_inert_slots(dev, mode):
    """An offset of UINT64_MAX is AMBRYCRC_MSG_BAD_LAYOUT with msg_end 0 in every verify form, reads nothing and
    leaves the real messages' results unchanged: what the recover entry's verify over max_m slots relies on."""
    import torch

    (clean, offs, _), (dirty, doffs, _) = mixed()
    before = dev.get_region_mode(0)
    try:
        dev.set_region_mode(0, mode)
        for region, real in ((dirty, doffs), (clean, offs[:40])):
            rw, r = guarded(region, 0)
            want_st, want_end = dev.verify_messages(r, torch.tensor(real, dtype=torch.int64, device="cuda"))
            for mix in (real + [-1] * 300, real + [-1], [-1] * 5):
                st, end = dev.verify_messages(r, torch.tensor(mix, dtype=torch.int64, device="cuda"))
                torch.cuda.synchronize()
                n = min(len(real), len(mix)) if mix[0] != -1 else 0
                assert torch.equal(st[:n], want_st[:n]) and torch.equal(end[:n], want_end[:n])
                assert bool((st[n:] == MF.BAD_LAYOUT).all()) and bool((end[n:] == 0).all())
            guards_intact(rw, 0, len(region))
            same_as_cpu(recover_to_numpy(dev.recover_messages(r, 0, 700)), dev.recover_messages_cpu(region, 0, 700))
    finally:
        dev.set_region_mode(0, before)


# ---------------------------------------------------------------- offsets past 2^32
def test_chain_past_4gib(dev):
    """Three PUTs with 1.5 GiB blobs of random bytes (never hashed: the chain reads headers only), then 100 small
    messages whose starts lie above 2^32. The blobs hold about 2 x 10^5 candidates, all rejected."""
    import torch

    blob = 3 << 29
    small, soffs = RO.join([RO.update_message(MF.store_key("s%03d" % i), kind=("delete", "ttl", "undelete")[i % 3])
                            if i % 2 else RO.put_message(MF.store_key("s%03d" % i), b"x" * i, hv=1 + i % 3)
                            for i in range(100)])
    heads = []
    for i in range(3):  # everything of the message before the content, from a PUT with an empty blob
        m = RO.put_message(MF.store_key("big%d" % i), b"", hv=3, um=b"u" * i)
        v, total, rel = MF.parse_header(m, 0)
        head = m[40:rel[4]] + b"\x00\x03\x00\x00\x00" + blob.to_bytes(8, "big")
        heads.append(MF.header(3, total + blob, *rel) + head)
    total_len = sum(len(h) + blob + 8 for h in heads) + len(small)
    region = torch.empty(total_len, dtype=torch.uint8, device="cuda")
    dev.fill_random(region, seed=77)  # the blobs' content and their CRCs; the rest is overwritten
    want, pos = [], 0
    for i, h in enumerate(heads):
        want.append(pos)
        region[pos:pos + len(h)] = torch.from_numpy(np.frombuffer(h, dtype=np.uint8).copy()).cuda()
        pos += len(h) + blob + 8
    region[pos:] = torch.from_numpy(np.frombuffer(small, dtype=np.uint8).copy()).cuda()
    want += [pos + o for o in soffs]
    assert want[3] > 1 << 32
    for start, first in ((0, 0), (want[2], 2), (want[50], 50)):
        msg_off, res = recover_to_numpy(dev.chain_messages(region, start, 128))
        n = len(want) - first
        assert [int(x) for x in msg_off[:n]] == want[first:] and (msg_off[n:] == np.uint64(RO.NO_MESSAGE)).all()
        assert {k: int(res[k]) for k in RO.RESULT.names} == {"chained": n, "recovered": n, "end_off": total_len,
                                                            "end_status": 0, "more": 0}
    # the small messages alone, recovered at their offsets above 2^32
    got = recover_to_numpy(dev.recover_messages(region, want[3], 100))
    cpu = dev.recover_messages_cpu(small, 0, 100)
    assert np.array_equal(got[0], cpu[0] + np.uint64(want[3])) and np.array_equal(got[2], cpu[2])
    assert np.array_equal(got[1]["msg_off"], cpu[1]["msg_off"] + np.uint64(want[3]))
    assert np.array_equal(got[1]["size"], cpu[1]["size"]) and int(got[3]["recovered"]) == 100


# ---------------------------------------------------------------- above the capped grids
def test_above_the_capped_grids(dev):
    """A clean tile of 1,201 mixed messages repeated on the device to the smallest multiple past 2 x 256 x CUs + 1
    messages: every thread of the thread-per-message kernels takes a second message. The oracle judges one
    tile; offsets and infos of the copies are derived with numpy and compared on the device."""
    import torch

    T = 1201
    tile, offs, _ = RK.build_region(n=T, seed=1, corrupt_frac=0.0, big_every=10**9, max_blob=1000, max_usermeta=400)
    _, sts, infos, res = RO.recover(tile, 0, T)
    assert res["recovered"] == T and sts == [0] * T
    k = -(-(2 * 256 * torch.cuda.get_device_properties(0).multi_processor_count + 1) // T)
    m = k * T
    whole, region = copies(to_dev(tile), k)
    max_m = m + 37
    msg_off, info, status, result = dev.recover_messages(region, 0, max_m)
    shift = np.repeat(np.arange(k, dtype=np.uint64) * np.uint64(len(tile)), T)
    want_off = np.full(max_m, RO.NO_MESSAGE, dtype=np.uint64)
    want_off[:m] = np.tile(np.asarray(offs, dtype=np.uint64), k) + shift
    want_info = np.zeros(max_m, dtype=RO.INFO)
    want_info[:m] = np.tile(RO.info_array(infos), k)
    want_info["msg_off"][:m] += shift
    want_st = np.full(max_m, MF.BAD_LAYOUT, dtype=np.uint32)
    want_st[:m] = 0
    assert torch.equal(msg_off, to_dev(want_off).view(torch.int64))
    assert torch.equal(info.reshape(-1), to_dev(want_info))
    assert torch.equal(status, to_dev(want_st).view(torch.int32))
    res = dev.recover_result(result)
    assert {n: int(res[n]) for n in RO.RESULT.names} == {"chained": m, "recovered": m, "end_off": k * len(tile),
                                                        "end_status": 0, "more": 0}
    sample = info[m - 1].cpu().numpy().view(RO.INFO)[0]
    assert int(sample["msg_off"]) == (k - 1) * len(tile) + offs[-1] and int(sample["size"]) == len(tile) - offs[-1]
    assert_guards(whole, region.numel())


# ---------------------------------------------------------------- no host synchronisation
def test_recover_in_a_graph(dev):
    """The call only enqueues, so with a caller workspace it is captured into a HIP graph and replayed after the
    region is replaced by a different one of the same length: the second region's result."""
    import torch

    (clean, _, _), (dirty, _, _) = mixed()
    n = min(len(clean), len(dirty))
    a, b = clean[:n], dirty[:n]
    rw, r = guarded(a, 0)
    max_m = 400
    ws = torch.empty(dev.recover_workspace_bytes(n, max_m), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = dev.recover_messages(r, 0, max_m, workspace=ws)  # loads the kernels first
        torch.cuda.synchronize()
        same_as_cpu(recover_to_numpy(out), dev.recover_messages_cpu(a, 0, max_m))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            dev.recover_messages(r, 0, max_m, workspace=ws, out=out)
    torch.cuda.synchronize()
    for data in (b, a, b):
        r.copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda())
        for t in out:
            t.fill_(0x5A if t.dtype == torch.uint8 else 7)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        same_as_cpu(recover_to_numpy(out), dev.recover_messages_cpu(data, 0, max_m))
    assert dev.recover_messages_cpu(a, 0, max_m)[3] != dev.recover_messages_cpu(b, 0, max_m)[3]
