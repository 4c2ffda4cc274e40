"""Every per-message device entry once with a blob of 2^24 - 1, 2^28 - 1 and 2^31 - 1 (Integer.MAX_VALUE) bytes:
the largest blob a stored message may hold, and two smaller ones that run the same code, so a failure at 2 GiB has
a 16 MiB and a 256 MiB case beside it. Every size has all its bits set, so each whole-length CRC combine reads
every word of the x^(8 * 2^k) table up to the size's top bit in one call.

The message is built on the device and judged by tests/big_message.py's streamed oracle (zlib as a running value
over the head and the tile; test_big_message.py proves it against the full oracles on the CPU). Each batch is the
big message between small ones of the existing builders -- a clean one (properties stored at SerDe V1), a
corrupted one, an update message -- at an offset that is not a multiple of 64. Regions and outputs sit between
64 guard bytes of 0xA5; every output byte, status, offset, length and info field is compared."""
import contextlib
import functools
import struct
from types import SimpleNamespace

import numpy as np
import pytest

import big_message as B
import hard_delete_oracle as HD
import ingest_oracle as IO
import recover_oracle as RC
import recv_oracle as RO
import rekey_oracle as RK
import send_oracle as SO
from datagen import stream_bytes
from gpu_buffers import assert_guards, dev, guarded, host, u64_dev
from gpu_calls import recover_to_numpy, recovery_dev, refs_tensor
from msgfmt import MF
from oracle_common import BAD_DESC, NOWHERE, flip, same
from regions import put_expected

pytestmark = pytest.mark.gpu

BIG = 2  # the big message's place in the batch: clean, corrupted, big, update
FLAG_NAMES = {SO.BLOB: "blob", SO.ALL: "all"}


@functools.lru_cache(maxsize=None)
def smalls():
    """(clean PUT with SerDe V1 properties, PUT with a flipped content bit, update message)."""
    clean = RC.put_message(MF.store_key("small-clean"), stream_bytes(41, 0, 777).tobytes(), hv=3, um=b"m" * 33,
                           enc_key=b"k" * 16, serde_version=1)
    bad = RC.put_message(MF.store_key("small-corrupted"), stream_bytes(42, 0, 1500).tobytes(), hv=2, um=b"n" * 7)
    return clean, flip(bad, len(bad) - 100), RC.update_message(MF.store_key("small-update"), kind="ttl")


def small_region():
    parts = smalls()
    return b"".join(parts), [0, len(parts[0]), len(parts[0]) + len(parts[1])]


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    """The module holds up to 12 GiB of device tensors at a time: when it is done, the allocator's cache goes back
    to the device, so the modules after it start from the memory they started from before."""
    yield
    import gc

    import torch

    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def tile_dev(gpu):
    return dev(B.tile())


@pytest.fixture(scope="module", params=B.SIZES, ids=lambda n: "%#x" % n)
def ctx(gpu, tile_dev, request):
    """The region [clean, corrupted, big, update] on the device, read-only: one copy serves every entry."""
    import torch

    b = B.big(request.param)
    clean, bad, upd = smalls()
    whole, region, offs = B.build_region([clean, bad, b.span, upd], tile_dev)
    torch.cuda.synchronize()
    assert region.data_ptr() % 64 == 0 and offs[BIG] % 64 != 0
    return SimpleNamespace(b=b, whole=whole, region=region, offs=offs, at=offs[BIG], tile=tile_dev, gpu=gpu,
                           offs_dev=u64_dev(offs), small_at=[offs[0], offs[1], offs[3]])


def in_batch(small, big):
    """Per-message values in batch order from the three small messages' and the big one's."""
    return [small[0], small[1], big, small[2]]


def fields(rec, names):
    return {k: int(rec[k]) for k in names}


def place(parts):
    """(offsets or None, total) of outputs packed in order; a part is bytes, a Span, or None."""
    at, pos = [], 0
    for p in parts:
        at.append(None if p is None else pos)
        pos += 0 if p is None else len(p) if isinstance(p, bytes) else B.span_len(p)
    return at, pos


def assert_parts(out, parts, at, tile_dev, what):
    for i, (p, o) in enumerate(zip(parts, at)):
        if p is not None:
            s = p if isinstance(p, B.Span) else B.Span(p, None, b"")
            B.assert_span(out[o:o + B.span_len(s)], s, tile_dev, "%s of message %d" % (what, i))


@contextlib.contextmanager
def flipped(view, at):
    """One bit of view[at] flipped for the block's duration."""
    view[at] ^= 0x10
    try:
        yield
    finally:
        view[at] ^= 0x10


# ---------------------------------------------------------------- verify
def verify_expected(c):
    sm, soffs = small_region()
    res = [MF.verify_message(sm, o) for o in soffs]
    st = in_batch([s for s, _ in res], 0)
    end = in_batch([e - o + a if e else 0 for (_, e), o, a in zip(res, soffs, c.small_at)], B.verify_expected(c.b, c.at)[1])
    assert st[1] == MF.BLOB_CRC and end[BIG] == c.at + c.b.length
    return st, end


def run_verify(c):
    import torch

    st, end = c.gpu.verify_messages(c.region, c.offs_dev)
    torch.cuda.synchronize()
    return host(st, np.uint32).tolist(), host(end, np.uint64).tolist()


def test_verify(ctx):
    """The job form: a batch of four messages with this region is far above region mode's 6 KiB per message."""
    got = run_verify(ctx)
    assert ctx.gpu.last_message_mode(0) == 0
    assert got == verify_expected(ctx)


def test_verify_finds_a_flipped_bit(ctx):
    st, end = verify_expected(ctx)
    for name, p in flip_places(ctx):
        with flipped(ctx.region, p):
            got = run_verify(ctx)
        assert got == (st[:BIG] + [MF.BLOB_CRC] + st[BIG + 1:], end), name
    assert run_verify(ctx) == (st, end)


def flip_places(c):
    b, at = c.b, c.at
    return (("first tile", at + b.content_rel + 1000), ("last content byte", at + b.content_rel + b.size - 1),
            ("trailer low word", at + b.length - 1), ("trailer high word", at + b.length - 6))


@pytest.mark.parametrize("mode", [1, 2])
def test_verify_in_region_mode(ctx, mode):
    """Region mode takes a region of at most 6 KiB per message, so the batch is followed by as many copies of
    scale_tiles.tile() (1,201 mixed messages of about 1 KiB) as bring the region's average below that: about
    2,700 messages at the smallest size and 400,000 at the largest. The big record then goes through region
    mode's long-record path (64 KiB pieces folded in rounds). Both region forms (asserted), the clean region and
    one flipped bit in turn in the first tile, the last content byte and either trailer word."""
    import torch

    import scale_tiles as S
    from gpu_calls import assert_copies

    t = S.tile()
    n0, length = ctx.region.numel(), len(t.region)
    k = -(-(n0 - 6144 * 4) // (6144 * S.T - length)) + 1
    assert n0 + k * length <= 6144 * (4 + k * S.T)
    tile_region = dev(t.region)
    whole, region = guarded(n0 + k * length, 0)
    region[:n0].copy_(ctx.region)
    region[n0:].copy_(tile_region.repeat(k))
    offs = np.concatenate([np.array(ctx.offs, dtype=np.int64), n0 + S.tiled_offsets(t.offs, length, k)])
    tst, tend = S.tiled_verify(*S.verify_oracle(t.region, t.offs), length, k)
    st, end = verify_expected(ctx)
    want_st = np.concatenate([np.array(st, dtype=np.uint32), tst])
    want_end = np.concatenate([np.array(end, dtype=np.int64), np.where(tend != 0, tend + n0, 0)])
    assert (tst == 0).sum() >= 900 * k and (tst != 0).sum() >= 80 * k
    offs_dev = torch.from_numpy(offs).cuda()

    def run(big_status):
        got_st, got_end = ctx.gpu.verify_messages(region, offs_dev)
        torch.cuda.synchronize()
        assert ctx.gpu.last_message_mode(0) == mode
        want_st[BIG] = big_status
        bad = np.nonzero(host(got_st, np.uint32) != want_st)[0]
        assert not len(bad), "status: %d differ, first message %d: %#x" % (len(bad), bad[0], host(got_st, np.uint32)[bad[0]])
        assert np.array_equal(host(got_end, np.int64), want_end)

    before = ctx.gpu.get_region_mode(0)
    try:
        ctx.gpu.set_region_mode(0, mode)
        run(0)
        for name, p in flip_places(ctx):
            with flipped(region, p):
                run(MF.BLOB_CRC)
        run(0)
    finally:
        ctx.gpu.set_region_mode(0, before)
    assert_guards(whole, region)
    assert_copies(region[n0:], tile_region, k, "the padding after the verify")


# ---------------------------------------------------------------- send
@pytest.mark.parametrize("flag", [SO.BLOB, SO.ALL], ids=FLAG_NAMES.get)
def test_send(ctx, flag):
    import torch

    from ambry_amd import messages as M

    sm, soffs = small_region()
    res = in_batch([SO.send_message(sm, o, None, flag) for o in soffs], B.send_expected(ctx.b, flag))
    parts = [p for _, _, p in res]
    at, total = place(parts)
    owhole, out = guarded(total, 5)
    _, info, status = M.send_messages_dev(ctx.region, ctx.offs_dev, flag, out=out)
    torch.cuda.synchronize()
    same(host(status, np.uint32).tolist(), [st for st, _, _ in res], "status")
    got = host(info, np.uint8).view(SO.INFO)
    for i, (st, f, p) in enumerate(res):
        assert fields(got[i], SO.INFO.names) == dict(f, out_off=NOWHERE if p is None else at[i]), i
    assert_guards(owhole, out, 5)
    assert_parts(out, parts, at, ctx.tile, "the sent span")
    assert int(got[BIG]["send_len"]) == (ctx.b.length if flag == SO.ALL else 13 + ctx.b.size + 8)


# ---------------------------------------------------------------- receive
BODY_LEN = (5 << 30) + (2 << 20)  # the largest message, from 3 GiB + 3 on, ends a few hundred bytes past 5 GiB
PAYLOAD_AT = (1 << 32) - (1 << 30) + 3
SMALL_AT = BODY_LEN - (1 << 20) + 1


@pytest.fixture(scope="module")
def body(ctx):
    """A GetResponse body of 5 GiB + 2 MiB of which only the payloads are ever written: the big message at
    3 GiB + 3 (at the largest size its record straddles 2^32) and the two small PUTs in the last MiB, wholly
    above 2^32."""
    import torch

    clean, bad, _ = smalls()
    t = torch.empty(BODY_LEN, dtype=torch.uint8, device="cuda")
    B.put_span(t[PAYLOAD_AT:PAYLOAD_AT + ctx.b.length], ctx.b.span, ctx.tile)
    for at, m in ((SMALL_AT, clean), (SMALL_AT + len(clean), bad)):
        t[at:at + len(m)] = dev(m)
    torch.cuda.synchronize()
    assert SMALL_AT > PAYLOAD_AT + ctx.b.length and SMALL_AT > 1 << 32
    return t


def cut(size):
    """(lo, hi): pieces of 0x15555555, 0x2AAAAAAA and 0x40000000 bytes at the largest size -- their set bits
    partition bits 0-30, so each piece's shift reads other table words -- and the same masks below the top bit
    of a smaller size."""
    top = 1 << (size.bit_length() - 1)
    lo, mid = 0x15555555 & (top - 1), 0x2AAAAAAA & (top - 1)
    assert lo + mid + top == size and lo & mid == 0
    return lo, lo + mid


def run_receive(c, body, flag, ranges):
    """The batch [clean, big, corrupted] against the oracle; returns the statuses."""
    import torch

    from ambry_amd import messages as M

    clean, bad, _ = smalls()
    b = c.b
    pay = []  # (offset, size, payload bytes or None)
    for at, m in ((SMALL_AT, clean), (PAYLOAD_AT, None), (SMALL_AT + len(clean), bad)):
        rel = 0 if flag == SO.ALL else (b.rel[4] if m is None else MF.parse_header(m, 0)[2][4])
        n = b.length if m is None else len(m)
        pay.append((at + rel, n - rel, None if m is None else m[rel:]))
    rng = [(0, None)] * 3 if ranges is None else ranges
    res = [B.recv_expected(b, flag, lo, hi) if p is None else RO.receive_payload(p, flag, lo, RO.TO_END if hi is None else hi)
           for (_, _, p), (lo, hi) in zip(pay, rng)]
    parts = [s if isinstance(s, B.Span) else None if s is None else bytes(s) for _, _, s in res]
    at, total = place(parts)
    owhole, out = guarded(total, 3)
    _, info, status = M.receive_blobs_dev(
        body, u64_dev([o for o, _, _ in pay]), flag, pay_size=u64_dev([n for _, n, _ in pay]),
        ranges=None if ranges is None else u64_dev([(lo, RO.TO_END if hi is None else hi) for lo, hi in ranges]), out=out)
    torch.cuda.synchronize()
    got_st = host(status, np.uint32).tolist()
    got = host(info, np.uint8).view(RO.INFO)
    assert_guards(owhole, out, 3)
    return got_st, got, out, res, parts, at


def check_receive(c, body, flag, ranges):
    got_st, got, out, res, parts, at = run_receive(c, body, flag, ranges)
    same(got_st, [st for st, _, _ in res], "status")
    assert got_st == [0, 0, MF.BLOB_CRC]
    for i, (st, f, p) in enumerate(res):
        assert fields(got[i], RO.INFO.names) == dict(f, out_off=at[i]), i
    assert_parts(out, parts[:2], at[:2], c.tile, "the delivered slice")  # (the CRC-failed payload's span is unspecified)


@pytest.mark.parametrize("flag", [SO.BLOB, SO.ALL], ids=FLAG_NAMES.get)
def test_receive(ctx, body, flag):
    check_receive(ctx, body, flag, None)
    B.assert_span(body[PAYLOAD_AT:PAYLOAD_AT + ctx.b.length], ctx.b.span, ctx.tile, "the body after the receive")


@pytest.mark.parametrize("flag", [SO.BLOB, SO.ALL], ids=FLAG_NAMES.get)
def test_receive_a_range(ctx, body, flag):
    """Three pieces whose lengths share no bit; then one bit flipped in each piece and in the trailer's high
    word, each a call of its own, each exactly BLOB_CRC."""
    b = ctx.b
    lo, hi = cut(b.size)
    ranges = [(0, None), (lo, hi), (1, 100)]
    check_receive(ctx, body, flag, ranges)
    content = PAYLOAD_AT + b.content_rel
    for name, p in (("before", content + lo // 2), ("inside", content + lo + (hi - lo) // 2), ("after", content + hi + 5),
                    ("trailer high word", PAYLOAD_AT + b.length - 6)):
        with flipped(body, p):
            got_st, got, _, res, _, at = run_receive(ctx, body, flag, ranges)
        assert got_st == [0, MF.BLOB_CRC, MF.BLOB_CRC], name
        assert fields(got[1], RO.INFO.names) == dict(res[1][1], out_off=at[1]), name


# ---------------------------------------------------------------- hard delete
def test_hard_delete(ctx):
    """On a clone: the full call, then plan_only over the result, then, on a fresh clone, a call with the plan's
    recovery info. The content becomes zeros, the trailer the streamed CRC of head plus zeros, the rest of the
    region stays, and the verify finds the message clean afterwards."""
    import torch

    gpu, b = ctx.gpu, ctx.b
    sm, soffs = small_region()
    bst, binfo, bspan = B.hard_delete_expected(b)
    n = ctx.region.numel()

    def expect(region_small, recovery=None):
        st, info, after = HD.hard_delete(region_small, soffs, recovery)
        einfo = np.zeros(4, dtype=HD.INFO)
        einfo[[0, 1, 3]], einfo[BIG] = info, binfo
        ends = soffs[1:] + [len(sm)]
        return in_batch(st, bst), einfo, in_batch([after[o:e] for o, e in zip(soffs, ends)], bspan)

    def check(whole, got, exp, what, parts=None):
        status, info = got
        torch.cuda.synchronize()
        same(host(status, np.uint32).tolist(), exp[0], "status, " + what)
        same(host(info, np.uint8).view(HD.INFO), exp[1], "info, " + what)
        assert_guards(whole, n)
        assert_parts(whole[64:64 + n], exp[2] if parts is None else parts, ctx.offs, ctx.tile, "the region after " + what)

    whole = ctx.whole.clone()
    region = whole[64:64 + n]
    first = expect(sm)
    assert first[0] == [0, MF.BLOB_CRC, 0, MF.NOT_PUT]
    check(whole, gpu.hard_delete_messages(region, ctx.offs_dev), first, "the delete")
    st, end = gpu.verify_messages(region, ctx.offs_dev)
    assert host(st, np.uint32).tolist() == [0, MF.BLOB_CRC, 0, 0] and int(end[BIG]) == ctx.at + b.length
    # the plan over the deleted region: the same infos, nothing written
    after_small = b"".join(p for p in (first[2][0], first[2][1], first[2][3]))
    plan = expect(after_small)
    got = gpu.hard_delete_messages(region, ctx.offs_dev, plan_only=True)
    check(whole, got, plan, "the plan", parts=first[2])
    same(plan[1], first[1], "the plan's info against the delete's")
    # a fresh clone, with the plan's info as recovery info: the record CRCs are not read
    whole.copy_(ctx.whole)
    rec = host(got[1], np.uint8).view(HD.INFO).copy()
    third = expect(sm, rec[[0, 1, 3]])
    check(whole, gpu.hard_delete_messages(region, ctx.offs_dev, recovery=recovery_dev(rec)), third, "the delete with recovery info")
    assert third[0] == first[0]


# ---------------------------------------------------------------- re-key
def key_descs(keys, m):
    d = np.zeros(m, dtype=RK.DESC)
    d["key_len"], d["content_src"], d["props_blob_size"] = len(keys) // m, RK.KEEP, -1
    d["key_src"] = np.arange(m) * (len(keys) // m)
    d["account_id"], d["container_id"] = 9, 77
    return d


def run_rekey(region, offs_dev, descs, aux, total, version=3):
    import torch

    from ambry_amd import messages as M

    owhole, out = guarded(total, 1)
    _, out_off, out_len, status = M.rekey_dev(region, offs_dev, dev(descs), aux, header_version=version, out=out)
    torch.cuda.synchronize()
    assert_guards(owhole, out, 1)
    return host(status, np.uint32).tolist(), host(out_off, np.uint64).tolist(), host(out_len, np.uint64).tolist(), out


def test_rekey_keeps_the_content(ctx):
    """A new key of another length for every message, the content kept."""
    keys = b"".join(MF.store_key("a-new-key-of-another-length-%d" % i) for i in range(4))
    descs = key_descs(keys, 4)
    sm, soffs = small_region()
    small = [RK.rekey_message(sm, o, descs[i], keys) for o, i in zip(soffs, (0, 1, 3))]
    res = in_batch(small, B.rekey_expected(ctx.b, descs[BIG], keys))
    parts = [p for _, p in res]
    at, total = place(parts)
    st, off, ln, out = run_rekey(ctx.region, ctx.offs_dev, descs, dev(keys), total)
    same(st, [s for s, _ in res], "status")
    assert st == [0, MF.BLOB_CRC, 0, MF.NOT_PUT]
    same(off, [NOWHERE if a is None else a for a in at], "out_off")
    same(ln, [0 if p is None else len(p) if isinstance(p, bytes) else B.span_len(p) for p in parts], "out_len")
    assert_parts(out, parts, at, ctx.tile, "the re-keyed message")


def test_rekey_replaces_a_content_of_max_int(gpu, tile_dev):
    """A MetadataBlob's content replaced by 0x7FFFFFFF bytes of aux; and a descriptor whose content_len is
    0x80000000, inside aux, which is refused (AMBRYCRC_MSG_BAD_DESC: content_len > Integer.MAX_VALUE)."""
    meta = B.big(5, blob_type=1)
    key = MF.store_key("the-metadata-blob-s-new-key")
    n = 0x7FFFFFFF
    rule = ("stream", 3, 3 + n)
    awhole, aux, _ = B.build_region([key, B.Span(b"", ("stream", 3, 4 + n), b"")], tile_dev)
    assert aux.numel() == len(key) + 0x80000000
    descs = key_descs(key, 1).repeat(2)
    descs["key_src"] = 0
    descs["content_src"], descs["props_blob_size"] = len(key), 1 << 33
    descs["content_len"] = [n, n + 1]
    st0, span = B.rekey_expected(meta, descs[0], key, rule)
    assert st0 == 0
    rwhole, region, offs = B.build_region([b"\xEE" * 5, meta.span, meta.span], tile_dev)
    st, off, ln, out = run_rekey(region, u64_dev(offs[1:]), descs, aux, B.span_len(span))
    assert (st, off, ln) == ([0, BAD_DESC], [0, NOWHERE], [B.span_len(span), 0])
    B.assert_span(out, span, tile_dev, "the re-keyed message")
    assert_guards(awhole, aux)


# ---------------------------------------------------------------- transform
@pytest.mark.parametrize("version", [1, 3])
def test_transform(ctx, version):
    """The general path (the batch holds a corrupted message and an update); the clean small message's
    properties are stored at SerDe V1, so props_v5_crc runs in the same batch."""
    import torch

    from ambry_amd import messages as M

    sm, soffs = small_region()
    res = in_batch([MF.transform_message(sm, o, version=version) for o in soffs], B.transform_expected(ctx.b, version))
    parts = [p for _, p in res]
    at, total = place(parts)
    assert [s for s, _ in res] == [0, MF.BLOB_CRC, 0, MF.NOT_PUT]
    owhole, out = guarded(total, 7)
    _, out_off, out_len, status = M.transform_dev(ctx.region, ctx.offs_dev, header_version=version, out=out)
    torch.cuda.synchronize()
    assert ctx.gpu.last_transform_path(0) == 0
    same(host(status, np.uint32).tolist(), [s for s, _ in res], "status")
    same(host(out_off, np.uint64).tolist(), [NOWHERE if a is None else a for a in at], "out_off")
    same(host(out_len, np.uint64).tolist(), [0 if p is None else len(p) if isinstance(p, bytes) else B.span_len(p) for p in parts],
         "out_len")
    assert_guards(owhole, out, 7)
    assert_parts(out, parts, at, ctx.tile, "the transformed message")


@functools.lru_cache(maxsize=None)
def dense_tile():
    """(region, offsets, life versions, the oracle's transformed bytes) of 1,201 clean dense V3 PUTs."""
    from regions import dense_v3_region

    region, offs = dense_v3_region(1201, seed=77)
    life = np.random.default_rng(7).integers(0, 9, size=len(offs)).astype(np.int16)
    ends = offs[1:] + [len(region)]
    out = [MF.transform_message(region, o, life=int(v))[1] for o, v in zip(offs, life)]
    assert all(len(b) == e - o for b, o, e in zip(out, offs, ends))  # the fast path's: the same bytes, new life versions
    return region, offs, life, b"".join(out)


def test_transform_on_the_fast_path(ctx):
    """Clean V3 PUTs with VERSION_5 properties back to back, the big message between the first two, followed by as
    many copies of a dense tile as bring the region to at most 40 KiB per message -- the fast path's cut-off
    (kXformFastMaxPerMessage): the one-pass kernel's copy form takes the batch alone (last_transform_path 1)."""
    import torch

    import scale_tiles as S
    from ambry_amd import messages as M
    from gpu_calls import assert_copies

    small = [RC.put_message(MF.store_key("dense-%d" % i), stream_bytes(50 + i, 0, 900 + i).tobytes(), hv=3, um=b"d" * i,
                            enc_key=b"k" * 16 if i else None, life=i) for i in range(2)]
    tregion, toffs, tlife, tout = dense_tile()
    n0, m = len(small[0]) + ctx.b.length + len(small[1]), len(toffs)
    k = -(-(n0 - 40960 * 3) // (40960 * m - len(tregion))) + 1
    assert n0 + k * len(tregion) <= 40960 * (3 + k * m)
    tile_region, tile_out = dev(tregion), dev(tout)
    rwhole, region = guarded(n0 + k * len(tregion), 9)
    stored = [small[0], ctx.b.span, small[1]]
    offs, _ = place(stored)
    for p, o in zip(stored, offs):
        sp = p if isinstance(p, B.Span) else B.Span(p, None, b"")
        B.put_span(region[o:o + B.span_len(sp)], sp, ctx.tile)
    region[n0:].copy_(tile_region.repeat(k))
    all_offs = np.concatenate([np.array(offs[:3], dtype=np.int64), n0 + S.tiled_offsets(toffs, len(tregion), k)])
    life = np.concatenate([np.array([4, 5, 6], dtype=np.int16), np.tile(tlife, k)])
    parts = [MF.transform_message(small[0], 0, life=4)[1], B.transform_expected(ctx.b, 3, life=5)[1],
             MF.transform_message(small[1], 0, life=6)[1]]
    at, total = place(parts)
    assert total == n0 and len(tout) == len(tregion)
    owhole, out = guarded(total + k * len(tout), 2)
    _, out_off, out_len, status = M.transform_dev(region, torch.from_numpy(all_offs).cuda(), header_version=3,
                                                  life_version=torch.from_numpy(life).cuda(), out=out)
    torch.cuda.synchronize()
    assert ctx.gpu.last_transform_path(0) == 1
    assert not host(status, np.uint32).any()
    assert np.array_equal(host(out_off, np.int64), all_offs)  # nothing grows: a message lands at its own offset
    ends = np.concatenate([all_offs[1:], [region.numel()]])
    assert np.array_equal(host(out_len, np.int64), ends - all_offs)
    assert_guards(owhole, out, 2)
    assert_guards(rwhole, region, 9)
    assert_parts(out, parts, at, ctx.tile, "the transformed message")
    assert_copies(out[n0:], tile_out, k, "the transformed padding")
    assert_copies(region[n0:], tile_region, k, "the padding after the transform")


@pytest.mark.parametrize("bv", [1, 2])
def test_transform_and_rekey_of_an_older_blob_record(ctx, bv):
    """The big message stored with a Blob_Format_V1 / V2 record (a 10- / 12-byte head): the transform and the
    kept-content re-key write it as V3, and get the new record's CRC from the stored one by shifting the heads'
    difference over the whole content (blob_crc_moved: one combine over `size` bytes)."""
    import torch

    from ambry_amd import messages as M

    b = B.big(ctx.b.size, bv=bv)
    rwhole, region, offs = B.build_region([b"\xEE" * 5, b.span], ctx.tile, shift=3)
    offs_dev = u64_dev(offs[1:])
    st, span = B.transform_expected(b, 3, life=6)
    assert st == 0 and MF._be16(b.head, b.rel[4]) == bv
    owhole, out = guarded(B.span_len(span), 7)
    _, out_off, out_len, status = M.transform_dev(region, offs_dev, header_version=3,
                                                  life_version=torch.tensor([6], dtype=torch.int16, device="cuda"), out=out)
    torch.cuda.synchronize()
    assert (host(status, np.uint32).tolist(), host(out_off, np.uint64).tolist(), host(out_len, np.uint64).tolist()) == \
        ([0], [0], [B.span_len(span)])
    assert_guards(owhole, out, 7)
    B.assert_span(out, span, ctx.tile, "the transformed message")
    key = MF.store_key("a-new-key-of-another-length")
    descs = key_descs(key, 1)
    st, span = B.rekey_expected(b, descs[0], key)
    assert st == 0
    got_st, off, ln, out = run_rekey(region, offs_dev, descs, dev(key), B.span_len(span))
    assert (got_st, off, ln) == ([0], [0], [B.span_len(span)])
    B.assert_span(out, span, ctx.tile, "the re-keyed message")
    assert_guards(rwhole, region, 3)
    B.assert_span(region[offs[1]:], b.span, ctx.tile, "the region afterwards")


# ---------------------------------------------------------------- serialize
def test_serialize(ctx):
    """serialize_dev in copy mode, the big blob between two small ones in the blobs buffer: put_stream_max keeps
    its default, so the big message goes by the job form."""
    import torch

    from ambry_amd.messages import PUT_DESC_DTYPE, PutMessage, serialize_dev

    b = ctx.b
    small = [PutMessage(key=MF.store_key("ser-%d" % i), props=MF.blob_properties_bytes(300 + i), usermeta=b"s" * (5 + i),
                        blob=stream_bytes(60 + i, 0, 300 + i).tobytes(), enckey=b"e" * 24 if i else None,
                        header_version=3 - i, life_version=1 - i) for i in range(2)]
    msgs = [small[0], B.put_message_of(b, b""), small[1]]
    blob_lens = [len(small[0].blob), b.size, len(small[1].blob)]
    parts = [put_expected(small[0]), B.serialize_expected(b)[1], put_expected(small[1])]
    assert B.serialize_expected(b)[0] == b.length
    at, total = place(parts)
    descs, fbytes, bpos = np.zeros(3, dtype=PUT_DESC_DTYPE), bytearray(), 0
    for i, m in enumerate(msgs):
        src = {}
        for name in ("key", "enckey", "props", "usermeta"):
            src[name] = len(fbytes)
            fbytes += getattr(m, name) or b""
        src["blob"] = bpos
        bpos += blob_lens[i]
        d = m.desc(at[i], src)
        d.blob_len = blob_lens[i]
        descs[i] = np.frombuffer(bytes(d), dtype=PUT_DESC_DTYPE)[0]
    bwhole, blobs, _ = B.build_region([small[0].blob, B.Span(b"", b.span.rule, b""), small[1].blob], ctx.tile, shift=11)
    owhole, out = guarded(total, 6)
    mlen = torch.empty(3, dtype=torch.int64, device="cuda")
    serialize_dev(dev(descs), out, dev(bytes(fbytes)), blobs, msg_len=mlen)
    torch.cuda.synchronize()
    assert host(mlen, np.int64).tolist() == [len(parts[0]), b.length, len(parts[2])]
    assert_guards(owhole, out, 6)
    assert_guards(bwhole, blobs, 11)
    assert_parts(out, parts, at, ctx.tile, "the serialized message")


# ---------------------------------------------------------------- ingest
def test_ingest(ctx):
    """A V5 PutRequest frame whose blob is the big content between a clean small frame and one whose blobSize
    field is 0x80000000 (rule 4: BAD_RECORD); the wire CRC is the streamed zlib value over the frame."""
    import torch

    from ambry_amd import messages as M

    b = ctx.b
    frame, key_len, crc = B.frame_of(b, 5)
    rng = np.random.default_rng(3)
    f0, k0, _, _ = IO.one_frame(rng, 1, 900, blob_len=5000)
    f2, k2, _, _ = IO.one_frame(rng, 2, 900, refusal="blob_huge", blob_len=300)
    wwhole, wire, woffs = B.build_region([b"\x5A" * 3, f0, frame, f2], ctx.tile)
    refs = np.zeros(3, dtype=IO.REF)
    refs["off"], refs["key_len"] = woffs[1:], [k0, key_len, k2]
    r0, r2 = IO.ingest_request(f0, 0, k0, 3), IO.ingest_request(f2, 0, k2, 3)
    rb = B.ingest_expected(b, frame, 3)
    assert (r0[0], r2[0]) == (0, MF.BAD_RECORD) and struct.pack(">q", 1 << 31) in f2
    parts = [r0[1], rb[1], None]
    at, total = place(parts)
    owhole, out = guarded(total, 4)
    res = M.ingest_put_requests_dev(wire, refs_tensor(refs), header_version=3, out=out)
    torch.cuda.synchronize()
    _, out_off, out_len, info, wire_crc, tot, status = res
    same(host(status, np.uint32).tolist(), [0, 0, MF.BAD_RECORD], "status")
    same(host(out_off, np.uint64).tolist(), [at[0], at[1], NOWHERE], "out_off")
    same(host(out_len, np.uint64).tolist(), [len(parts[0]), B.span_len(parts[1]), 0], "out_len")
    same(host(wire_crc, np.uint32).tolist(), [r0[2], crc, 0], "wire CRC")
    assert rb[2] == crc and int(tot.cpu()[0]) == total
    got = host(info, np.uint8).view(IO.INFO)
    assert fields(got[0], IO.INFO.names) == dict(zip(IO.INFO.names, (at[0],) + r0[3][1:]))
    assert fields(got[1], IO.INFO.names) == dict(rb[3], msg_off=at[1]) and int(got[1]["size"]) == B.span_len(parts[1])
    assert not any(int(got[2][k]) for k in IO.INFO.names)
    assert_guards(owhole, out, 4)
    assert_guards(wwhole, wire)
    assert_parts(out, parts, at, ctx.tile, "the ingested message")


# ---------------------------------------------------------------- chain and recover
def test_chain_and_recover(ctx):
    b = ctx.b
    total = ctx.region.numel()
    msg_off, res = recover_to_numpy(ctx.gpu.chain_messages(ctx.region, 0, 8))
    assert msg_off.tolist() == ctx.offs + [RC.NO_MESSAGE] * 4
    assert fields(res, RC.RESULT.names) == {"chained": 4, "recovered": 4, "end_off": total, "end_status": 0, "more": 0}
    sm, soffs = small_region()
    small = [RC.message_info(sm, o) for o in soffs]
    infos = in_batch([None if f is None else dict(f, msg_off=a) for (_, f), a in zip(small, ctx.small_at)],
                     B.recover_expected(b, ctx.at)[1])
    sts = in_batch([s for s, _ in small], 0)
    assert sts == [0, MF.BLOB_CRC, 0, 0] and infos[BIG]["size"] == b.length and (b.size < 0x7FFFFFFF or b.length > 1 << 31)
    # from the start: recovery stops at the corrupted message; from the big message on: two clean messages
    for first in (0, BIG):
        exp_res = {"chained": 4 - first, "recovered": 4 - first, "end_off": total, "end_status": 0, "more": 0}
        if first == 0:
            exp_res.update(recovered=1, end_off=ctx.offs[1], end_status=MF.BLOB_CRC)
        got = recover_to_numpy(ctx.gpu.recover_messages(ctx.region, ctx.offs[first], 8))
        RC.assert_call(got, (ctx.offs[first:], sts[first:], infos[first:], exp_res), 8)


def test_the_region_is_unchanged(ctx):
    """After every read-only entry above: the guards and every byte of the module's region."""
    clean, bad, upd = smalls()
    assert_guards(ctx.whole, ctx.region)
    assert_parts(ctx.region, [clean, bad, ctx.b.span, upd], ctx.offs, ctx.tile, "the region")


def test_ingest_refuses_a_record_offset_past_a_java_int(gpu, tile_dev):
    """Rule 8 of ambrycrc_ingest_put_requests_dev: a frame that parses, whose wire CRC holds and whose properties
    encode, but whose user metadata of 0x7FFFFFFF - 40 bytes would put the stored message's blob record past a
    relative offset of Integer.MAX_VALUE: AMBRYCRC_MSG_BAD_RECORD, nothing written, the computed wire CRC
    returned. Rule 5 comes first, so the whole frame is on the device and its CRC is the streamed zlib value.
    The same frame with 70,001 bytes of user metadata is accepted (and by the oracle: test_big_message.py)."""
    import torch

    from ambry_amd import messages as M

    key, props, blob = MF.store_key("past-a-java-int"), MF.blob_properties_bytes(9), b"blob bytes"
    um_len = 0x7FFFFFFF - 40
    far, far_crc = B.frame_with_usermeta(um_len, B.TILE_LEN, key, props, blob, enc_key=b"e" * 12)
    near, near_crc = B.frame_with_usermeta(70001, B.TILE_LEN, key, props, blob, enc_key=b"e" * 12)
    assert MF.HEADER_SIZE[3] + len(key) + 14 + um_len > 0x7FFFFFFF >= um_len  # umSize itself is a valid Java int
    st, msg, crc, info = IO.ingest_request(B.span_bytes(near, B.TILE_LEN), 0, len(key), 3)
    assert (st, crc) == (0, near_crc)
    wwhole, wire, woffs = B.build_region([b"\x5A" * 7, far, near], tile_dev)
    refs = np.zeros(2, dtype=IO.REF)
    refs["off"], refs["key_len"] = woffs[1:], len(key)
    owhole, out = guarded(len(msg) + 100, 4)
    _, out_off, out_len, dinfo, wire_crc, tot, status = M.ingest_put_requests_dev(wire, refs_tensor(refs), header_version=3, out=out)
    torch.cuda.synchronize()
    same(host(status, np.uint32).tolist(), [MF.BAD_RECORD, 0], "status")
    same(host(out_off, np.uint64).tolist(), [NOWHERE, 0], "out_off")
    same(host(out_len, np.uint64).tolist(), [0, len(msg)], "out_len")
    same(host(wire_crc, np.uint32).tolist(), [far_crc, near_crc], "wire CRC")
    got = host(dinfo, np.uint8).view(IO.INFO)
    assert not any(int(got[0][k]) for k in IO.INFO.names) and int(tot.cpu()[0]) == len(msg)
    assert fields(got[1], IO.INFO.names) == dict(zip(IO.INFO.names, info))
    assert_guards(owhole, out, 4)
    assert_guards(wwhole, wire)
    assert out[:len(msg)].cpu().numpy().tobytes() == msg and bool((out[len(msg):] == 0xA5).all())
