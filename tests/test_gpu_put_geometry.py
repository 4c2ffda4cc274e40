"""The write-side lattices (put_lattice.py; test_put_lattice.py asserts what they cover) through the kernels that
produce output bytes: the streamed serialize (put_stream_kernel, put_stream_seal_kernel), the job path's
copy-through sweep in wave mode and in the group phase, with both source buffers and with slots in place, the
gather copy under the re-key and under the transform's fallback pass, the transform's general path and send
(the copy-through sweep at the deltas their packing gives). Every comparison is byte for byte against
oracle/message_format.py's layout, inside guards, with the sources checked unchanged and every serialize output
verified again by ambrycrc_verify_messages_dev. A failure names the first differing byte, its message and
segment, and that segment's put_cells()."""
import dataclasses

import numpy as np
import pytest

import geometry_lattice as G
import put_lattice as P
import send_oracle as SO
from gpu_buffers import assert_guards, assert_untouched, guarded

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, copy=True)).cuda()


def run_serialize(gpu, lat, form, shift=0, order=None, stream_max=P.STREAM_MAX, in_place=(), grid=None):
    """One ambrycrc_serialize_puts_dev call over a put lattice: the output view `shift` bytes past a 64-B boundary,
    the descriptors in `order`, slots named in `in_place` already at their offsets (their buffer not given)."""
    import torch

    from ambry_amd.messages import serialize_dev

    m = len(lat.msgs)
    order = np.arange(m) if order is None else order
    start = np.full(lat.total, P.FILL, dtype=np.uint8)
    for k, name in enumerate(P.SEGMENTS):
        if name in in_place:
            for o, lo, hi in zip(lat.out_off.tolist(), lat.lo[:, k].tolist(), lat.hi[:, k].tolist()):
                start[o + lo:o + hi] = lat.image[o + lo:o + hi]
    fwhole, fields = guarded(lat.fields)
    bwhole, blobs = guarded(lat.blobs)
    owhole, out = guarded(start, shift)
    mlen = torch.full((m,), -1, dtype=torch.int64, device="cuda")
    descs = _dev(np.frombuffer(lat.descs[order].tobytes(), dtype=np.uint8))
    prev_max = gpu.set_put_stream_max(0, stream_max)
    prev_grid = gpu.grid_size(0)
    if grid is not None:
        gpu.set_grid(0, grid)
    try:
        serialize_dev(descs, out, None if "key" in in_place else fields, None if "blob" in in_place else blobs,
                      msg_len=mlen)
        torch.cuda.synchronize()
    finally:
        gpu.set_put_stream_max(0, prev_max)
        gpu.set_grid(0, prev_grid)
    msg = P.compare_image(lat, out.cpu().numpy(), shift, form, in_place)
    assert msg is None, msg
    assert_guards(owhole, lat.total, shift)
    assert_untouched(fwhole, fields, lat.fields)
    assert_untouched(bwhole, blobs, lat.blobs)
    assert np.array_equal(mlen.cpu().numpy(), lat.length[order])
    status, end = gpu.verify_messages(out, _dev(lat.out_off))
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert not st.any(), "message %d verifies as %#x" % (int(np.nonzero(st)[0][0]), st[np.nonzero(st)[0][0]])
    assert np.array_equal(end.cpu().numpy(), lat.out_off + lat.length)
    assert prev_grid == gpu.grid_size(0)


# ---------------------------------------------------------------- the streamed form and the job path beside it
@pytest.mark.parametrize("order", ["in-order", "permuted"])
@pytest.mark.parametrize("shift", [0, 37])
@pytest.mark.parametrize("stream_max", [P.STREAM_MAX, 0])
def test_stream_lattice(gpu, stream_max, shift, order):
    """stream_lattice() streamed (the three 6,145-byte messages take the gated job path and the clear_short launch
    beside it) and, with streaming off, the same bytes through the job path's group phase (5 m >= 16,384 jobs);
    the output view at a 64-B boundary and 37 bytes past one (StreamPutArgs::oreg0 nonzero); the descriptors in
    output order and in a fixed permutation."""
    lat = P.stream_lattice()
    perm = np.random.default_rng(11).permutation(len(lat.msgs)) if order == "permuted" else None
    run_serialize(gpu, lat, "stream" if stream_max else "through", shift, perm, stream_max)


def test_stream_lattice_graph_replay(gpu):
    """One streamed run captured into a HIP graph and replayed after every blob's bytes change (same sizes): each
    replay's output is the oracle's layout of the current bytes."""
    import torch

    from ambry_amd.messages import serialize_dev

    lat = P.stream_lattice()
    m = len(lat.msgs)
    fields, blobs = _dev(lat.fields), _dev(lat.blobs)
    descs = _dev(np.frombuffer(lat.descs.tobytes(), dtype=np.uint8))
    owhole, out = guarded(np.full(lat.total, P.FILL, dtype=np.uint8), 37)
    mlen = torch.empty(m, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        serialize_dev(descs, out, fields, blobs, msg_len=mlen)  # sizes the stream's default workspace outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            serialize_dev(descs, out, fields, blobs, msg_len=mlen)
    torch.cuda.synchronize()

    def check(image):
        out.fill_(P.FILL)
        mlen.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        msg = P.compare_image(lat, out.cpu().numpy(), 37, "stream", exp=image)
        assert msg is None, msg
        assert_guards(owhole, lat.total, 37)
        assert np.array_equal(mlen.cpu().numpy(), lat.length)

    check(lat.image)
    blobs2 = lat.blobs.copy()
    image2 = lat.image.copy()
    for i, mm in enumerate(lat.msgs):
        nb = G.nonzero_bytes(900001 + i, len(mm.blob))
        src, o, n = int(lat.src[i, P.BLOB]), int(lat.out_off[i]), int(lat.length[i])
        blobs2[src:src + len(nb)] = np.frombuffer(nb, dtype=np.uint8)
        image2[o:o + n] = np.frombuffer(P.expected_bytes(dataclasses.replace(mm, blob=nb)), dtype=np.uint8)
    assert (image2 != lat.image).sum() > 10000
    blobs.copy_(_dev(blobs2))
    check(image2)


# ---------------------------------------------------------------- the copy-through sweep
@pytest.mark.parametrize("in_place", [(), ("blob",), ("key", "enckey", "props", "usermeta")],
                         ids=["both-buffers", "blob-in-place", "fields-in-place"])
@pytest.mark.parametrize("jobs", ["wave", "group"])
def test_copy_lattice(gpu, jobs, in_place):
    """copy_lattice() with streaming off: under 16,384 jobs (every job in wave mode) and above (the group phase
    takes the jobs of at most 16 KiB), both buffers given and in the two mixed forms, where the in-place slots are
    re-read where they lie; at the grid the builder computed its share cuts for."""
    lat = P.copy_lattice(jobs)
    run_serialize(gpu, lat, "through", 0, None, 0, in_place, lat.grid)


# ---------------------------------------------------------------- packed outputs of the stored lattice
def assert_packed(got, packed, offs, what, ranges=None, scratch_to=None, flag=0):
    """got (uint8 array, the whole output view) against the oracle's packed bytes, 0xA5 after them (after
    scratch_to, when the call may leave bytes of its own between the packed output's end and there)."""
    exp = np.frombuffer(packed, dtype=np.uint8)
    if not np.array_equal(got[:len(exp)], exp):
        b = int(np.nonzero(got[:len(exp)] != exp)[0][0])
        placed = np.asarray([o for o in offs if o >= 0], dtype=np.int64)
        i = int(np.searchsorted(placed, b, side="right")) - 1
        cell = ""
        if ranges is not None:
            hit = [(d, s, n, j) for d, s, n, j in ranges if d <= b < d + n]
            cell = "; no copy range (a computed byte)" if not hit else "; range %s cells %s" % (
                hit[0], vars(P.range_cells(*hit[0][:3])))
        if what != "transform-corrupt":
            cell += "; " + P.describe_packed(what, b, flag)
        raise AssertionError("%s: %d bytes differ; first byte %d (placed message %d, byte %d): %#x, expected %#x%s" % (
            what, int((got[:len(exp)] != exp).sum()), b, i, b - int(placed[i]), got[b], exp[b], cell))
    assert (got[max(len(exp), scratch_to or 0):] == 0xA5).all(), "%s: bytes written past the packed output" % what


def gather_waves():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 4


def test_rekey_over_the_stored_lattice(gpu):
    """The gather copy: stored_lattice() re-keyed with keys of 1..16 bytes, so the packed output steps through
    every destination residue; test_put_lattice.py asserts the copy_range cells its jobs hit when a wave's cost
    share is 4,096 units, which holds on this device (asserted here from its CU count)."""
    import torch

    from ambry_amd.messages import rekey_dev, rekey_out_bound

    lat = P.stored_lattice()
    descs, aux = P.rekey_inputs()
    est, eoff, eln, packed = P.rekey_expected()
    m = len(lat.offs)
    assert P.gather_cost(P.rekey_jobs()) <= P.GATHER_MIN_SHARE * gather_waves()
    whole, region = guarded(lat.region)
    awhole, auxd = guarded(aux)
    owhole, out = guarded(np.full(rekey_out_bound(len(lat.region), m, len(aux)), 0xA5, dtype=np.uint8))
    _, out_off, out_len, status = rekey_dev(region, _dev(lat.offs), _dev(np.frombuffer(descs.tobytes(), dtype=np.uint8)),
                                            auxd, out=out)
    torch.cuda.synchronize()
    assert status.cpu().numpy().view(np.uint32).tolist() == est
    assert out_off.cpu().numpy().tolist() == eoff and out_len.cpu().numpy().tolist() == eln
    assert_packed(out.cpu().numpy(), packed, eoff, "rekey", P.gather_ranges(P.rekey_jobs()))
    assert_guards(owhole, out.numel(), 0)
    assert_untouched(whole, region, lat.region)
    assert_untouched(awhole, auxd, aux)
    st, end = gpu.verify_messages(out, out_off)
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any() and end.cpu().numpy().tolist() == [o + n for o, n in zip(eoff, eln)]


@pytest.mark.parametrize("corrupt", [False, True], ids=["clean", "one-corrupt"])
def test_transform_general_path_over_the_stored_lattice(gpu, corrupt):
    """stored_lattice() to header V3. Clean, the general path's speculative pass places every record with the
    copy-through sweep at the deltas the messages' different growths give. With one flipped content bit that pass
    fails and the fallback pass rebuilds the whole output with the gather copy: every message but the corrupt one,
    byte for byte. The speculative pass placed all messages, the corrupt one included, so it wrote as far as the
    clean batch's packed length; what it left between the shorter final output and there is unspecified, and
    nothing past it may be written."""
    import torch

    from ambry_amd.messages import out_bound, transform_dev

    lat = P.stored_lattice()
    src = P.corrupted_region() if corrupt else lat.region
    est, eoff, eln, packed = P.transform_expected(corrupt)
    m = len(lat.offs)
    life = (np.arange(m) % 7).astype(np.int16)
    whole, region = guarded(src)
    owhole, out = guarded(np.full(out_bound(len(src), m), 0xA5, dtype=np.uint8))
    _, out_off, out_len, status = transform_dev(region, _dev(lat.offs), header_version=3, life_version=_dev(life), out=out)
    torch.cuda.synchronize()
    assert gpu.last_transform_path(0) == 0
    assert np.array_equal(status.cpu().numpy().view(np.uint32), est)
    assert np.array_equal(out_off.cpu().numpy(), eoff) and np.array_equal(out_len.cpu().numpy(), eln)
    assert_packed(out.cpu().numpy(), packed, eoff.tolist(), "transform-corrupt" if corrupt else "transform",
                  scratch_to=len(P.transform_expected(False)[3]))
    assert_guards(owhole, out.numel(), 0)
    assert_untouched(whole, region, src)
    placed = _dev(eoff[eoff >= 0])
    st, end = gpu.verify_messages(out, placed)
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any() and np.array_equal(end.cpu().numpy(), (eoff + eln)[eoff >= 0])


@pytest.mark.parametrize("flag", [SO.BLOB, SO.ALL, SO.BLOB_INFO], ids=["BLOB", "ALL", "BLOB_INFO"])
def test_send_over_the_stored_lattice(gpu, flag):
    """Send moves every sent record with the copy-through sweep. BLOB packs the blob records alone (every other
    record hashed and not stored, kCopySkip), so its deltas differ from the transform's; ALL and BLOB_INFO pack
    whole messages and the two middle records."""
    import torch

    from ambry_amd.messages import send_messages_dev

    lat = P.stored_lattice()
    est, einfo, packed = P.send_expected(flag)
    whole, region = guarded(lat.region)
    owhole, out = guarded(np.full(len(packed) + 64, 0xA5, dtype=np.uint8), 3)
    _, info, status = send_messages_dev(region, _dev(lat.offs), flag, out=out)
    torch.cuda.synchronize()
    assert status.cpu().numpy().view(np.uint32).tolist() == est
    got = info.cpu().numpy().view(SO.INFO)
    for name in SO.INFO.names:
        assert np.array_equal(got[name], einfo[name]), name
    assert_packed(out.cpu().numpy(), packed, einfo["out_off"].astype(np.int64).tolist(), "send", flag=flag)
    assert_guards(owhole, out.numel(), 3)
    assert_untouched(whole, region, lat.region)
