"""Mixed message batches above the capped grids, byte for byte. The thread-per-message kernels run a bounded
grid of 256-thread blocks and loop over messages past it:

    msg_parse_kernel                   AMBRY_PARSE_BPC = 2 blocks per CU
    region_msg_kernel                  AMBRY_REGION_BPC = AMBRY_REGION_BPC_SMALL = 2
    put_stream_seal_kernel             AMBRY_SEAL_BPC = 2
    rekey_plan_kernel, rekey_write_kernel   4 (their launchers, rekey_kernels.hip)

(build_knobs.h; the values are not readable at run time). The batches here hold m = K x T messages with
m > 2 x 4 x 256 x CUs, about 525,000 on 256 CUs: every thread of a grid capped at 4 blocks per CU takes at least
three messages, one capped at 2 takes five, and since T = 1,201 is prime they are different tile messages --
clean and refused ones, headers V1 to V3, PUTs and update messages by turns (test_scale_tiles.py asserts that
mix at these strides). State a thread carries from one message into the next shows as a wrong status or byte.

The expectation is scale_tiles.py's: the oracle's results for one tile, repeated by numpy. The tile is uploaded
once and repeated on the device, outputs are compared on the device as (K, tile bytes) views against the one
expected tile, and only statuses, offsets and lengths come back. Regions and outputs sit between 64 guard bytes
of 0xA5.

The ladder at the end runs hard delete and re-key at the smallest multiples of T past each size at which they
change mechanism, so that a failure of a big test has a small one beside it that names the mechanism."""
import functools

import numpy as np
import pytest

import scale_tiles as S
from gpu_buffers import assert_guards, dev, guarded, host
from gpu_calls import assert_copies, assert_same, copies, offsets_dev

pytestmark = pytest.mark.gpu

T = S.T


# ---------------------------------------------------------------- the tile, on the host and on the device
@pytest.fixture(scope="module")
def big(gpu):
    """K: copies of the tile in a batch above every capped grid of this device."""
    import torch

    k = S.copies_above_caps(torch.cuda.get_device_properties(0).multi_processor_count)
    assert k * T > 2 * 4 * 256 * torch.cuda.get_device_properties(0).multi_processor_count
    return k


@pytest.fixture(scope="module")
def tile(gpu):
    """The tile and its device copies: region, descriptors, aux, life versions."""
    import torch
    from types import SimpleNamespace

    t = S.tile()
    return SimpleNamespace(region_dev=dev(t.region), descs_dev=dev(t.descs), aux_dev=dev(t.aux),
                           life_dev=dev(t.life).view(torch.int16), **vars(t))


@functools.lru_cache(maxsize=None)
def expect_verify():
    t = S.tile()
    return S.verify_oracle(t.region, t.offs)


@functools.lru_cache(maxsize=None)
def expect_transform(version):
    t = S.tile()
    st, off, ln, packed = S.transform_oracle(t.region, t.offs, t.life, version)
    return st, off, ln, dev(packed)


@functools.lru_cache(maxsize=None)
def expect_hard_delete():
    t = S.tile()
    st, info, out = S.hard_delete_oracle(t.region, t.offs)
    return st, dev(info), dev(out)


@functools.lru_cache(maxsize=None)
def expect_rekey():
    t = S.tile()
    st, off, ln, packed = S.rekey_oracle(t.region, t.offs, t.descs, t.aux)
    return st, off, ln, dev(packed)


@functools.lru_cache(maxsize=None)
def expect_serialize():
    t = S.tile()
    msgs = S.clean_puts(t.region, t.offs, expect_verify()[0])
    descs, fields, blobs, total, mlen, out = S.serialize_oracle(msgs)
    return descs, dev(fields), dev(blobs), total, mlen, dev(out)


# ---------------------------------------------------------------- above the caps
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_verify_above_the_caps(gpu, tile, big, mode):
    """All three forms of the verify: CRC jobs (msg_parse_kernel's loop), region mode in one pass and in two
    (region_msg_kernel's)."""
    import torch

    st, end = expect_verify()
    est, eend = S.tiled_verify(st, end, len(tile.region), big)
    whole, region = copies(tile.region_dev, big)
    offs = offsets_dev(tile.offs, len(tile.region), big)
    gpu.set_region_mode(0, mode)
    try:
        status, msg_end = gpu.verify_messages(region, offs)
        torch.cuda.synchronize()
        assert gpu.last_message_mode(0) == mode
    finally:
        gpu.set_region_mode(0, 2)
    assert_same(host(status, np.uint32), est, "status")
    assert_same(host(msg_end, np.int64), eend, "msg_end")
    assert_guards(whole, region.numel())
    assert_copies(region, tile.region_dev, big, "region after the verify")


@pytest.mark.parametrize("version", [3, 1])
def test_transform_above_the_caps(gpu, tile, big, version):
    """The general path (the mixed tile is not the fast path's), with index life versions."""
    import torch

    from ambry_amd.messages import out_bound, transform_dev

    st, off, ln, packed = expect_transform(version)
    est, eoff, eln = S.tiled_packed(st, off, ln, packed.numel(), big)
    whole, region = copies(tile.region_dev, big)
    m = big * T
    owhole, out = guarded(out_bound(region.numel(), m))
    _, out_off, out_len, status = transform_dev(region, offsets_dev(tile.offs, len(tile.region), big),
                                                header_version=version, life_version=tile.life_dev.repeat(big), out=out)
    torch.cuda.synchronize()
    assert gpu.last_transform_path(0) == 0
    assert_same(host(status, np.uint32), est, "status")
    assert_same(host(out_off, np.int64), eoff, "out_off")
    assert_same(host(out_len, np.int64), eln, "out_len")
    assert_guards(owhole, out.numel())
    assert_guards(whole, region.numel())
    assert_copies(out[:big * packed.numel()], packed, big, "output", np.cumsum(ln) - ln)
    assert_copies(region, tile.region_dev, big, "region after the transform")


def test_serialize_copy_mode_above_the_caps(gpu, big):
    """The tile's clean PUTs serialized from both source buffers: the streamed form (every message is under its
    6 KiB cut-off) and put_stream_seal_kernel's loop."""
    import torch

    from ambry_amd.messages import serialize_dev

    descs, fields, blobs, total, mlen, out_tile = expect_serialize()
    n = len(descs)
    assert big * n > 2 * 2 * 256 * torch.cuda.get_device_properties(0).multi_processor_count  # three trips
    owhole, out = guarded(big * total)
    msg_len = torch.empty(big * n, dtype=torch.int64, device="cuda")
    prev = gpu.set_put_stream_max(0, 6144)
    try:
        serialize_dev(dev(S.tiled_put_descs(descs, big, total, fields.numel(), blobs.numel())), out,
                      fields.repeat(big), blobs.repeat(big), msg_len=msg_len)
        torch.cuda.synchronize()
    finally:
        gpu.set_put_stream_max(0, prev)
    assert_same(host(msg_len, np.int64), np.tile(mlen, big), "msg_len")
    assert_guards(owhole, out.numel())
    assert_copies(out, out_tile, big, "output", np.cumsum(mlen) - mlen)


def run_hard_delete(gpu, tile, k: int):
    """A full call over k copies, then plan_only on fresh copies and a second call with the info it returned:
    status, info and every region byte each time."""
    import torch

    st, info, out_tile = expect_hard_delete()
    est = np.tile(st, k)
    offs = offsets_dev(tile.offs, len(tile.region), k)

    def check(status, got_info, region_tile, what):
        torch.cuda.synchronize()
        assert_same(host(status, np.uint32), est, what + " status")
        assert_copies(got_info.view(-1), info, k, what + " info")
        assert_guards(whole, region.numel())
        assert_copies(region, region_tile, k, what + " region", tile.offs)

    whole, region = copies(tile.region_dev, k)
    check(*gpu.hard_delete_messages(region, offs), out_tile, "full call:")
    region.copy_(tile.region_dev.repeat(k))
    status, plan = gpu.hard_delete_messages(region, offs, plan_only=True)
    check(status, plan, tile.region_dev, "plan_only:")
    check(*gpu.hard_delete_messages(region, offs, recovery=plan), out_tile, "with recovery info:")


def run_rekey(tile, k: int, capped: bool):
    """Re-key of k copies, every copy's descriptors pointing at the one aux buffer: status, out_off, out_len,
    every written span, and 0xA5 still in every byte no message was placed at."""
    import torch

    from ambry_amd.messages import rekey_dev, rekey_out_bound

    st, off, ln, packed = expect_rekey()
    p = packed.numel()
    whole, region = copies(tile.region_dev, k)
    awhole, aux = copies(tile.aux_dev, 1)
    if capped:
        cap = k * p // 2
        est, eoff, eln = S.tiled_rekey_capped(st, ln, k, cap)
        assert (est == S.RK.NO_ROOM).sum() >= k * T // 4 and (eln > 0).sum() >= k * T // 4
    else:
        cap = rekey_out_bound(region.numel(), k * T, aux.numel())
        est, eoff, eln = S.tiled_packed(st, off, ln, p, k)
    owhole, out = guarded(cap)
    _, out_off, out_len, status = rekey_dev(region, offsets_dev(tile.offs, len(tile.region), k),
                                            tile.descs_dev.repeat(k), aux, out=out)
    torch.cuda.synchronize()
    assert_same(host(status, np.uint32), est, "status")
    assert_same(host(out_off, np.int64), eoff, "out_off")
    assert_same(host(out_len, np.int64), eln, "out_len")
    for w, v in ((whole, region), (awhole, aux), (owhole, out)):
        assert_guards(w, v.numel())
    # the running offset only grows, so the written messages are a prefix of the packed output
    used = int((eoff + eln).max())
    assert used == eln.sum() and used <= cap
    full, rest = divmod(used, p)
    starts = np.cumsum(ln) - ln
    assert_copies(out[:full * p], packed, full, "output", starts)
    assert_copies(out[full * p:used], packed[:rest], 1, "output, copy %d" % full, starts)
    assert bool((out[used:] == 0xA5).all()), "bytes written past the last placed message"
    assert_copies(region, tile.region_dev, k, "region after the re-key")
    assert_copies(aux, tile.aux_dev, 1, "aux after the re-key")


def test_hard_delete_above_the_caps(gpu, tile, big):
    run_hard_delete(gpu, tile, big)


@pytest.mark.parametrize("capped", [False, True])
def test_rekey_above_the_caps(gpu, tile, big, capped):
    """rekey_plan_kernel's and rekey_write_kernel's loops; capped: out_cap at half the packed output, so about
    half the batch is refused with NO_ROOM and must leave nothing written."""
    run_rekey(tile, big, capped)


# ---------------------------------------------------------------- the ladder
def above(threshold: int) -> int:
    """Copies of the tile in the smallest batch of more than `threshold` messages."""
    return threshold // T + 1


# ids: the number of messages the batch exceeds, and the mechanism that engages past it
@pytest.mark.parametrize("threshold", [
    pytest.param(2048, id="2048-fill-search-three-levels"),  # more than 4,096 fill jobs (two per message)
    pytest.param(8192, id="8192-check-batch-group-phase"),  # 16,384 record-check jobs, the refused ones empty
    pytest.param(131072, id="131072-fill-search-four-levels"),  # more than 262,144 fill jobs
])
def test_hard_delete_ladder(gpu, tile, threshold):
    assert above(threshold) * T > threshold >= (above(threshold) - 1) * T
    run_hard_delete(gpu, tile, above(threshold))


@pytest.mark.parametrize("threshold", [
    pytest.param(1024, id="1024-copy-search-three-levels"),
    pytest.param(2048, id="2048-placement-scan-across-planning-blocks"),
    pytest.param(3277, id="3277-verify-group-phase"),  # 5 m >= 16,384 CRC jobs
    pytest.param(16384, id="16384-content-batch-group-phase"),  # mostly empty jobs
    pytest.param(65536, id="65536-copy-search-four-levels"),
])
def test_rekey_ladder(gpu, tile, threshold):
    assert above(threshold) * T > threshold >= (above(threshold) - 1) * T
    run_rekey(tile, above(threshold), capped=False)
