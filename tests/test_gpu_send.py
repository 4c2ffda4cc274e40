"""GPU parity for ambrycrc_send_messages_dev against the oracle (tests/send_oracle.py: oracle/message_format.py
and zlib) and against the CPU entry: status, every info field and every output byte. The region and the output
each sit inside a larger tensor with 64 guard bytes of 0xA5 on both sides, which must survive; output bytes
outside the sent spans must stay 0xA5 too."""
import functools

import numpy as np
import pytest

import rekey_oracle as RK
import send_oracle as SO
from datagen import stream_bytes
from gpu_buffers import assert_guards, dev, guarded, guarded_workspace, guards_intact, host
from gpu_calls import assert_copies, assert_same, assert_send_outputs, check_send, copies, offsets_dev, run_send
from msgfmt import MF
from regions import join

pytestmark = pytest.mark.gpu

FLAG_NAMES = {SO.BLOB_PROPERTIES: "props", SO.BLOB_USER_METADATA: "usermeta", SO.BLOB: "blob", SO.ALL: "all",
              SO.BLOB_INFO: "info"}


@pytest.fixture(scope="module")
def messages(gpu):
    from ambry_amd import messages as M

    assert M.SEND_INFO_DTYPE == SO.INFO
    return M


@functools.lru_cache(maxsize=None)
def region_case(seed):
    region, offs, _ = RK.build_region(n=300, seed=seed)
    ends = offs[1:] + [len(region)]
    sizes = [SO.header_length(region, o) or e - o for o, e in zip(offs, ends)]
    return region, offs, sizes


@pytest.mark.parametrize("shift,oshift,sized", [(0, 0, False), (1, 5, True), (17, 0, True), (63, 5, False)])
@pytest.mark.parametrize("flag", SO.FLAGS, ids=FLAG_NAMES.get)
def test_region_matches_oracle_and_cpu(messages, flag, shift, oshift, sized):
    """Every stored format (headers V1-V3, blob records V1-V3, update messages, 10 % corrupted, blobs up to
    300 KB: one record across waves), the region at four offsets from a 64-B boundary and the output at two,
    with the header's sizes and with given ones; out_cap exactly the sum of the sent spans."""
    region, offs, sizes = region_case(1)
    exp = check_send(messages, region, offs, sizes if sized else None, flag, shift, oshift, cpu=shift in (0, 1))
    clean, found, refused = SO.mix(exp[0], exp[1])
    assert clean >= 1 and found >= 1 and (refused >= 1 or (flag == SO.ALL and sized))


@functools.lru_cache(maxsize=None)
def exact_case(m, flag):
    """m small messages of every stored format, 10 % corrupted, their sizes, and the oracle's answers under
    `flag`: sizes given under ALL (messages that go whole: the plain-copy scan), the headers' own otherwise."""
    region, offs, _ = RK.build_region(n=m, seed=1000 + m, corrupt_frac=0.1 if m > 1 else 0.0, big_every=10**9,
                                      max_blob=600, max_usermeta=300)
    ends = offs[1:] + [len(region)]
    sizes = [SO.header_length(region, o) or e - o for o, e in zip(offs, ends)] if flag == SO.ALL else None
    return region, offs, sizes, SO.expected(region, offs, sizes, flag)


@pytest.mark.parametrize("m", [1, 2048, 2049])
@pytest.mark.parametrize("flag", [SO.ALL, SO.BLOB], ids=FLAG_NAMES.get)
def test_exact_workspace_between_guards(messages, flag, m):
    """A caller workspace of exactly ambrycrc_send_workspace_bytes(m) between two guards, 0xA5 throughout: one
    message, and the counts on either side of one plan block of the per-message scans (2,048 entries). ALL
    with given sizes runs both scans (the placement and the plain copies), BLOB reads the encryption-key
    records first and refuses messages. Status, info and every output byte as the oracle's."""

    region, offs, sizes, exp = exact_case(m, flag)
    clean, found, refused = SO.mix(exp[0], exp[1])
    if m > 1:
        assert clean >= 1000 and found >= 100 and (refused >= 20 or flag == SO.ALL)
    whole, ws = guarded_workspace(messages.send_workspace_bytes(m))
    check_send(messages, region, offs, sizes, flag, shift=17, oshift=5, workspace=ws, exp=exp)
    assert_guards(whole, ws)


SIZES = [0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 16371, 16372, 16373, 70000, 300 * 1024]


@functools.lru_cache(maxsize=None)
def sized_messages():
    """One clean V3 PUT per blob size of SIZES (16,371-16,373 put the 13-B-headed record at the 16 KiB group
    cap; 300 KB is one record across waves), with and without an encryption key by turns."""
    return [MF.put_message(MF.store_key("size-%d" % n), MF.blob_properties_bytes(n), b"u" * (i % 9),
                           stream_bytes(900 + i, 0, n).tobytes(), version=3, enc_key=b"e" * 24 if i % 2 else None)
            for i, n in enumerate(SIZES)]


@pytest.mark.parametrize("flag", [SO.BLOB, SO.ALL, SO.BLOB_INFO], ids=FLAG_NAMES.get)
def test_blob_sizes_in_the_group_phase(messages, flag):
    """A batch of 3,286 messages (16,430 jobs >= 16,384: the copy-through runs its group phase): the sizes
    among 3,270 small messages, a tenth of them with a flipped bit."""
    rng = np.random.default_rng(77)
    small = []
    for k in range(3270):
        b = MF.put_message(MF.store_key("s%d" % k), MF.blob_properties_bytes(k % 300), b"m" * (k % 5),
                           stream_bytes(5000 + k, 0, k % 300).tobytes(), version=1 + k % 3,
                           enc_key=b"q" * 16 if k % 3 else None)
        if k % 10 == 3:
            at = int(rng.integers(0, len(b)))
            b = b[:at] + bytes([b[at] ^ 4]) + b[at + 1:]
        small.append(b)
    big = sized_messages()
    msgs = small[:1000] + big[:8] + small[1000:2500] + big[8:] + small[2500:]
    assert len(msgs) >= 3277
    region, offs = join(msgs)
    exp = check_send(messages, region, offs, None, flag, shift=3, oshift=5)
    assert sum(1 for s in exp[0] if s == 0) >= 3000


@pytest.mark.parametrize("part", [0, 1, 2])
@pytest.mark.parametrize("flag", [SO.BLOB, SO.ALL], ids=FLAG_NAMES.get)
def test_blob_sizes_in_a_batch_of_7(messages, flag, part):
    """The same sizes seven at a time: every job through the sweep's wave mode."""
    msgs = sized_messages()[[0, 7, 9][part]:][:7]
    assert len(msgs) == 7
    region, offs = join(msgs)
    exp = check_send(messages, region, offs, [len(b) for b in msgs] if part == 1 else None, flag, shift=part, oshift=5 * part)
    assert exp[0] == [0] * 7 and not exp[1]["check"].any()


@pytest.mark.parametrize("sized", [False, True], ids=["header-size", "given-size"])
@pytest.mark.parametrize("flag", SO.FLAGS, ids=FLAG_NAMES.get)
def test_each_rule(messages, flag, sized):
    """The fatal and the counted cases of test_send_cpu.py on the device, a size of 0 among them."""
    names, region, offs, sizes = SO.rule_cases()
    exp = check_send(messages, region, offs, sizes if sized else None, flag, shift=1, oshift=2, cpu=not sized)
    by = {n: i for i, n in enumerate(names)}
    if sized:
        assert exp[0][by["v3-size-0"]] == exp[0][by["past-region"]] == MF.BAD_LAYOUT
        whole = exp[0][by["v3-header"]] == 0
        assert whole == (flag == SO.ALL)  # an unparseable header goes whole under ALL with a size
    st, f = exp[0][by["v3-enckey"]], exp[1][by["v3-enckey"]]
    assert (st, int(f["check"])) == {SO.ALL: (0, MF.ENCKEY_CRC), SO.BLOB_PROPERTIES: (0, 0)}.get(flag, (MF.ENCKEY_CRC, 0))


@pytest.mark.parametrize("flag", [SO.BLOB_INFO, SO.BLOB_PROPERTIES, SO.BLOB_USER_METADATA], ids=FLAG_NAMES.get)
def test_blob_records_are_not_judged(messages, flag):
    """Every blob's content corrupted: the metadata flags neither report it nor refuse the message."""
    msgs = []
    for k in range(40):
        b = MF.put_message(MF.store_key("c%d" % k), MF.blob_properties_bytes(500 + k), b"meta" * k,
                           stream_bytes(70 + k, 0, 500 + 37 * k).tobytes(), version=2 + k % 2,
                           enc_key=b"k" * 20 if k % 2 else None)
        at = MF.parse_header(b, 0)[2][4] + 13 + k  # inside the content
        msgs.append(b[:at] + bytes([b[at] ^ 0x10]) + b[at + 1:])
    region, offs = join(msgs)
    assert all(MF.verify_message(region, o)[0] == MF.BLOB_CRC for o in offs)
    exp = check_send(messages, region, offs, None, flag, shift=5)
    assert exp[0] == [0] * 40 and not exp[1]["check"].any()


@pytest.mark.parametrize("flag", SO.FLAGS, ids=FLAG_NAMES.get)
def test_repeats_and_overlaps(messages, flag):
    """The same offset listed three times, and a message that lies inside another's blob content."""
    inner = MF.put_message(MF.store_key("inner"), MF.blob_properties_bytes(300), b"im", stream_bytes(1, 0, 300).tobytes(),
                           version=3, enc_key=b"i" * 16)
    outer = MF.put_message(MF.store_key("outer"), MF.blob_properties_bytes(len(inner) + 20), b"om",
                           b"\x01" * 9 + inner + b"\x02" * 11, version=2)
    other = MF.put_message(MF.store_key("other"), MF.blob_properties_bytes(77), b"", stream_bytes(2, 0, 77).tobytes())
    region = outer + other
    at = MF.parse_header(outer, 0)[2][4] + 13 + 9
    assert region[at:at + len(inner)] == inner
    offs = [0, at, len(outer), 0, at, 0]
    exp = check_send(messages, region, offs, None, flag, shift=7, oshift=1)
    assert exp[0] == [0] * 6 and not exp[1]["check"].any()


def test_single_message_and_one_past_a_block(messages):
    region, offs, sizes = region_case(1)
    for flag in SO.FLAGS:
        i = next(k for k, o in enumerate(offs) if SO.send_message(region, o, None, flag)[0] == 0)
        check_send(messages, region, [offs[i]], None, flag, shift=9)
    msgs = [RK.stored_put(MF.store_key("b%d" % k), MF.blob_properties_bytes(k, serde_version=1 + k % 5), b"u" * (k % 7),
                          stream_bytes(400 + k, 0, k).tobytes(), hv=1 + k % 3, bv=1 + k % 3,
                          enc_key=b"x" * (k % 30 + 1) if k % 4 == 0 else None) for k in range(257)]
    region2, offs2 = join(msgs)
    for flag in (SO.BLOB, SO.BLOB_INFO, SO.ALL):
        exp = check_send(messages, region2, offs2, None, flag, shift=5, oshift=2)
        assert exp[0] == [0] * 257


@pytest.mark.parametrize("flag", [SO.BLOB, SO.ALL, SO.BLOB_USER_METADATA], ids=FLAG_NAMES.get)
def test_every_message_refused_writes_nothing(messages, flag):
    region, offs, _ = region_case(2)
    if flag == SO.ALL:  # a size of 0 refuses any message
        bad, sizes = offs[:25], [0] * 25
    else:
        bad, sizes = [o for o in offs if SO.send_message(region, o, None, flag)[0] != 0][:25], None
    assert len(bad) >= 5
    st, info, out = run_send(messages, region, bad, sizes, flag, shift=1, oshift=1, out_cap=4096)
    assert all(st) and (info["out_off"] == SO.NOWHERE).all() and not info["send_len"].any()
    assert (out == 0xA5).all()
    assert_send_outputs((st, info, out), SO.expected(region, bad, sizes, flag))


@pytest.mark.parametrize("flag", SO.FLAGS, ids=FLAG_NAMES.get)
def test_no_room_advances_the_running_offset(messages, flag):
    """out_cap ends inside a message: that one and every later one that does not fit are refused, the running
    offset advances past them, and nothing is written past the last placed span."""
    region, offs, sizes = region_case(3)
    full = SO.expected(region, offs, None, flag)
    sent = [f for s, f in zip(full[0], full[1]) if s == 0]
    mid = sent[len(sent) // 2]
    cap = int(mid["out_off"]) + int(mid["send_len"]) // 2  # inside a message
    exp = check_send(messages, region, offs, None, flag, shift=1, oshift=3, out_cap=cap, cpu=True)
    assert sum(1 for s in exp[0] if s == SO.NO_ROOM) >= 50 and len(exp[2]) <= cap


@pytest.mark.parametrize("flag", [SO.BLOB, SO.BLOB_INFO], ids=FLAG_NAMES.get)
def test_graph_capture_and_replay(messages, flag):
    """The call only enqueues work, so with a caller workspace it can be captured into a HIP graph and replayed
    on fresh data, with the outputs of the uncaptured call."""
    import torch

    region, offs, _ = region_case(1)
    exp = SO.expected(region, offs, None, flag)
    cap = len(exp[2])
    rw, r = guarded(region, 0)
    ow, o = guarded(b"", 3, cap)
    fresh_r, fresh_o = rw.clone(), ow.clone()
    mo = torch.tensor(np.asarray(offs, dtype=np.int64), device="cuda")
    ws = torch.empty(messages.send_workspace_bytes(len(offs)), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _, info0, st0 = messages.send_messages_dev(r, mo, flag, out=o, workspace=ws)  # loads the kernels first
        torch.cuda.synchronize()
        assert_send_outputs((st0.cpu().numpy().view(np.uint32).tolist(), info0.cpu().numpy().view(SO.INFO),
                             guards_intact(ow, 3, cap).copy()), exp)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            _, info, st = messages.send_messages_dev(r, mo, flag, out=o, workspace=ws)
    torch.cuda.synchronize()
    for _ in range(2):
        rw.copy_(fresh_r)
        ow.copy_(fresh_o)
        st.fill_(-1)
        info.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_send_outputs((st.cpu().numpy().view(np.uint32).tolist(), info.cpu().numpy().view(SO.INFO),
                             guards_intact(ow, 3, cap)), exp)


@pytest.mark.parametrize("flag", [SO.BLOB, SO.BLOB_INFO], ids=FLAG_NAMES.get)
def test_send_above_the_caps(gpu, messages, flag):
    """tests/scale_tiles.py's tile at its m for this device (more than twice the widest capped grid): every
    thread of send_plan_kernel, send_jobs_kernel and send_finish_kernel takes a second message, a different
    tile message each trip. The oracle judges one tile; the K copies are compared on the device."""
    import torch

    import scale_tiles as S

    t = S.tile()
    k = S.copies_above_caps(torch.cuda.get_device_properties(0).multi_processor_count)
    est, einfo, packed = SO.expected(t.region, [int(o) for o in t.offs], None, flag)
    clean, found, refused = SO.mix(est, einfo)
    assert clean >= 100 and found >= 10 and refused >= 100
    tile_dev, packed_dev = dev(t.region), dev(packed)
    whole, region = copies(tile_dev, k)
    owhole, out = guarded(k * len(packed))
    _, info, status = messages.send_messages_dev(region, offsets_dev(t.offs, len(t.region), k), flag, out=out)
    torch.cuda.synchronize()
    assert_same(host(status, np.uint32), np.tile(np.array(est, dtype=np.uint32), k), "status")
    got = host(info, np.uint8).view(SO.INFO)
    shift = np.repeat(np.arange(k, dtype=np.uint64) * np.uint64(len(packed)), S.T)
    sent = np.tile(einfo["out_off"] != SO.NOWHERE, k)
    assert_same(got["out_off"], np.where(sent, np.tile(einfo["out_off"], k) + shift, np.uint64(SO.NOWHERE)), "out_off")
    for name in SO.INFO.names[1:]:
        assert_same(got[name], np.tile(einfo[name], k), name)
    assert_guards(owhole, out.numel())
    assert_guards(whole, region.numel())
    starts = np.sort(einfo["out_off"][einfo["out_off"] != SO.NOWHERE].astype(np.int64))
    assert_copies(out, packed_dev, k, "output", starts)
    assert_copies(region, tile_dev, k, "region after the send")
