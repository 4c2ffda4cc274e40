"""The geometry lattices (geometry_lattice.py; test_geometry_lattice.py asserts what they cover) through the
kernels: every start residue and length of a CRC span on each path that assembles a record's CRC -- the run-sum
forms of region mode in two passes and in one (record_crc, record_crc_runs_wave, region_long_kernel's pieces),
the tail kernel's whole-wave forms (record_crc_direct), the transform's one-pass fast path (record_ends /
record_crc_from_ends) and the batch engine's wave mode, group phase and inline read of the stored CRC. Bit-exact
against zlib and oracle/message_format.py; a failure names the first failing span's cells()."""
import functools

import numpy as np
import pytest

import geometry_lattice as G
from gpu_buffers import GUARD, assert_guards, assert_untouched, guarded, guarded_workspace
from msgfmt import MF

pytestmark = pytest.mark.gpu


def lattice(which):
    return G.message_lattice() if which == "clean" else G.flipped()


def assert_messages(lat, shift, order, status, msg_end, what):
    """status / msg_end (device tensors, in `order`) against the oracle's; names the first failing message and
    the cells() of its probed span as the kernels see it (from the 64-aligned base below the region)."""
    st, end = G.verify_oracle(what)
    got_st, got_end = status.cpu().numpy().view(np.uint32), msg_end.cpu().numpy()
    bad = np.nonzero((got_st != st[order]) | (got_end != end[order]))[0]
    if len(bad):
        i = int(order[bad[0]])
        c = G.cells(int(lat.rec_pa[i]) + shift % 64, int(lat.rec_len[i])) if lat.probe[i] else None
        raise AssertionError("%d of %d messages differ; first message %d (%s): status %#x end %d, expected %#x %d; "
                             "probed span %s" % (len(bad), len(order), i, lat.kind[i], got_st[bad[0]], got_end[bad[0]],
                                                 st[i], end[i], c and vars(c)))


def run_verify(gpu, lat, what, mode, shift, reverse=False):
    import torch

    whole, region = guarded(lat.region, shift)
    order = np.arange(len(lat.offs))[::-1].copy() if reverse else np.arange(len(lat.offs))
    offs = torch.from_numpy(lat.offs[order].copy()).cuda()
    gpu.set_region_mode(0, mode)
    try:
        status, msg_end = gpu.verify_messages(region, offs)
        torch.cuda.synchronize()
        assert gpu.last_message_mode(0) == mode
    finally:
        gpu.set_region_mode(0, 2)
    assert_messages(lat, shift, order, status, msg_end, what)
    assert_untouched(whole, region, lat.region, shift)


# ---------------------------------------------------------------- the message verify
@pytest.mark.parametrize("shift", [0, 37])
@pytest.mark.parametrize("mode", [2, 1, 0])
@pytest.mark.parametrize("which", ["clean", "flipped"])
def test_verify_over_the_lattice(gpu, which, mode, shift):
    """All three forms: region mode in two passes (record_crc with the LDS masks, region_long_kernel's pieces),
    in one pass (the processors' record_crc and record_crc_runs_wave) and CRC jobs through the batch engine
    (5 m jobs: the group phase), the region at a run boundary and 37 bytes past one."""
    run_verify(gpu, lattice(which), which, mode, shift)


@pytest.mark.parametrize("shift", [0, 37])
@pytest.mark.parametrize("which", ["clean", "flipped"])
def test_tail_kernel_over_the_lattice(gpu, which, shift):
    """One pass with the offsets reversed: the one-pass kernel finds them unsorted and hands every message to
    region_tail_kernel, so every span goes through record_crc_direct, or record_crc_runs_wave and the long list
    past 512 runs."""
    run_verify(gpu, lattice(which), which, 1, shift, reverse=True)


@pytest.mark.parametrize("form", ["tail", "two-pass"])
@pytest.mark.parametrize("shift", G.EDGE_SHIFTS)
def test_region_edges(gpu, form, shift):
    """geometry_lattice.edge_region() at every shift: with reversed offsets in one pass (the tail kernel's
    record_crc_direct, whose lowest 16-B load for the first message's first span lies below the region's first
    block at each of these shifts and is clamped to it; test_geometry_lattice.py asserts that geometry) and in two
    passes. The clamp at the last block cannot fire for a well-formed message (see edge_region())."""
    import torch

    e = G.edge_region()
    assert G.low_load_below_region(shift, e.first_pa, e.first_len)
    whole, region = guarded(e.region, shift)
    order = np.arange(len(e.offs))[::-1].copy() if form == "tail" else np.arange(len(e.offs))
    mode = 1 if form == "tail" else 2
    gpu.set_region_mode(0, mode)
    try:
        status, msg_end = gpu.verify_messages(region, torch.from_numpy(e.offs[order].copy()).cuda())
        torch.cuda.synchronize()
        assert gpu.last_message_mode(0) == mode
    finally:
        gpu.set_region_mode(0, 2)
    assert status.cpu().numpy().view(np.uint32).tolist() == e.status[order].tolist()
    assert msg_end.cpu().numpy().tolist() == e.end[order].tolist()
    assert_untouched(whole, region, e.region, shift)


# ---------------------------------------------------------------- the transform's fast path
@functools.lru_cache(maxsize=None)
def transform_oracle():
    """(life int16[m], out_off, out_len int64[m], the packed output) of MF.transform_message over the clean
    lattice at header V3, each message with a life version of its own."""
    lat = G.message_lattice()
    life = (np.arange(len(lat.offs)) * 7 % 32749).astype(np.int16)
    out, off, ln = [], [], []
    pos = 0
    for i, o in enumerate(lat.offs.tolist()):
        st, b = MF.transform_message(lat.region, o, life=int(life[i]), version=3)
        assert st == 0
        off.append(pos)
        ln.append(len(b))
        out.append(b)
        pos += len(b)
    return life, np.asarray(off, dtype=np.int64), np.asarray(ln, dtype=np.int64), b"".join(out)


def test_transform_fast_path_over_the_lattice(gpu):
    """The clean lattice to header V3 with distinct life versions: the one-pass fast path takes the batch, the
    only form that hashes a record's head and tail runs right after the parse and the rest once the sums exist
    (record_ends / record_crc_from_ends). Every status, offset, length and output byte against the oracle."""
    import torch

    from ambry_amd.messages import out_bound, transform_dev

    lat = G.message_lattice()
    life, eoff, eln, packed = transform_oracle()
    m = len(lat.offs)
    whole, region = guarded(lat.region)
    owhole, out = guarded(np.full(out_bound(len(lat.region), m), 0xA5, dtype=np.uint8))
    _, out_off, out_len, status = transform_dev(region, torch.from_numpy(lat.offs).cuda(), header_version=3,
                                                life_version=torch.from_numpy(life).cuda(), out=out)
    torch.cuda.synchronize()
    assert gpu.last_transform_path(0) == 1
    got_st = status.cpu().numpy().view(np.uint32)
    if got_st.any():
        i = int(np.nonzero(got_st)[0][0])
        raise AssertionError("%d messages refused; first message %d (%s): status %#x; probed span %s" % (
            int((got_st != 0).sum()), i, lat.kind[i], got_st[i],
            vars(G.cells(int(lat.rec_pa[i]), int(lat.rec_len[i])))))
    assert np.array_equal(out_off.cpu().numpy(), eoff) and np.array_equal(out_len.cpu().numpy(), eln)
    got = out[:len(packed)].cpu().numpy()
    exp = np.frombuffer(packed, dtype=np.uint8)
    if not np.array_equal(got, exp):
        b = int(np.nonzero(got != exp)[0][0])
        i = int(np.searchsorted(eoff, b, side="right")) - 1
        raise AssertionError("output byte %d (message %d, byte %d): %#x, expected %#x" % (
            b, i, b - eoff[i], got[b], exp[b]))
    assert bool((out[len(packed):] == 0xA5).all()), "bytes written past the packed output"
    assert bool((owhole[:GUARD] == 0xA5).all()) and bool((owhole[GUARD + out.numel():] == 0xA5).all())
    assert_untouched(whole, region, lat.region)


# ---------------------------------------------------------------- the batch engine
@functools.lru_cache(maxsize=None)
def chunk_expect():
    return G.chunk_crcs(G.chunk_lattice())


def run_chunks(gpu, ch, lo, hi):
    import torch

    whole, mem = guarded(ch.mem)
    out = gpu.crc32_batch(mem, torch.from_numpy(ch.off[lo:hi].copy()).cuda(),
                          torch.from_numpy(ch.length[lo:hi].copy()).cuda(),
                          crc_in=torch.from_numpy(ch.crc_in[lo:hi].view(np.int32).copy()).cuda())
    torch.cuda.synchronize()
    got, exp = out.cpu().numpy().view(np.uint32), chunk_expect()[lo:hi]
    if not np.array_equal(got, exp):
        i = int(np.nonzero(got != exp)[0][0])
        raise AssertionError("%d of %d chunks differ; first chunk %d: %#x, expected %#x (crc_in %#x); %s" % (
            int((got != exp).sum()), hi - lo, lo + i, got[i], exp[i], ch.crc_in[lo + i],
            vars(G.cells(int(ch.off[lo + i]), int(ch.length[lo + i])))))
    assert_untouched(whole, mem, ch.mem)


@pytest.mark.parametrize("form", ["group-phase", "wave-mode-halves", "variant-0"])
def test_batch_over_the_chunk_lattice(gpu, oracle, form):
    """Every chunk start residue and length 0..320, and the class cuts at every residue, with crc_in: as one batch
    (at least 16,384 chunks: the group phase takes all up to 16 KiB), as two halves below that count (every
    chunk in wave mode) and through variant 0's sweep. zlib's answers, which the oracle library repeats. The
    library has no query for the form a batch took, so the forms follow from the counts alone (kGroupMinChunks)."""
    ch = G.chunk_lattice()
    n = len(ch.off)
    assert np.array_equal(chunk_expect(), oracle.batch(ch.mem, ch.off, ch.length, crc_in=ch.crc_in, threads=8))
    if form == "wave-mode-halves":
        half = (n + 1) // 2
        assert half < 16384
        run_chunks(gpu, ch, 0, half)
        run_chunks(gpu, ch, half, n)
        return
    assert n >= 16384
    default = gpu.get_variant(0)
    gpu.set_variant(0, 0 if form == "variant-0" else default)
    try:
        run_chunks(gpu, ch, 0, n)
    finally:
        gpu.set_variant(0, default)


def test_trailed_verify_over_the_chunk_lattice(gpu):
    """Every lattice chunk followed by its stored CRC, at the chunk's own residue: the group phase reads the
    8-B big-endian long itself wherever it falls (SweepArgs::exp_fill), in every size class; every seventh is
    corrupt, in its high and its low word by turns."""
    import torch

    tr = G.trailed_lattice()
    assert len(tr.off) >= 16384
    whole, mem = guarded(tr.mem)
    mism, count = gpu.verify_trailed(mem, torch.from_numpy(tr.off).cuda(), torch.from_numpy(tr.length).cuda())
    torch.cuda.synchronize()
    got = mism.cpu().numpy().astype(bool)
    if not np.array_equal(got, tr.bad):
        i = int(np.nonzero(got != tr.bad)[0][0])
        raise AssertionError("%d flags differ; first item %d: %s, expected %s; %s" % (
            int((got != tr.bad).sum()), i, got[i], tr.bad[i], vars(G.cells(int(tr.off[i]), int(tr.length[i]) - 8))))
    assert int(count.item()) == int(tr.bad.sum())
    assert_untouched(whole, mem, tr.mem)


@pytest.mark.parametrize("n", [1, 2048, 2049])
def test_trailed_verify_exact_workspace(gpu, n):
    """ambrycrc_verify_trailed_dev with a caller workspace of exactly ambrycrc_trailed_workspace_bytes(n) between
    guards: one item, and the counts on either side of one plan block (2,048 jobs). The first n lattice items,
    flags and count as the oracle's; both guards intact."""
    import ctypes

    import torch

    from ambry_amd._lib import check, lib

    tr = G.trailed_lattice()
    bad = tr.bad[:n]
    assert n == 1 or (bad.any() and not bad.all())  # corrupt and clean items both
    whole, mem = guarded(tr.mem)
    off, ln = torch.from_numpy(tr.off[:n].copy()).cuda(), torch.from_numpy(tr.length[:n].copy()).cuda()
    mism = torch.empty(n, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    wwhole, ws = guarded_workspace(lib().ambrycrc_trailed_workspace_bytes(n))
    check(lib().ambrycrc_verify_trailed_dev(mem.data_ptr(), off.data_ptr(), ln.data_ptr(), mism.data_ptr(),
                                            count.data_ptr(), n, ws.data_ptr(), ws.numel(), ctypes.c_void_p(0)),
          "ambrycrc_verify_trailed_dev")
    torch.cuda.synchronize()
    assert_guards(wwhole, ws)
    assert np.array_equal(mism.cpu().numpy().astype(bool), bad)
    assert int(count.item()) == int(bad.sum())
    assert_untouched(whole, mem, tr.mem)
