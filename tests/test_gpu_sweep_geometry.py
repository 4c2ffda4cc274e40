"""The sweep lattices (sweep_lattice.py; test_sweep_lattice.py asserts what they cover) through crc32_sweep_kernel:
every share cut, segment shape and descriptor-window case of the batch sweep, in its 64-B-run form with and
without the group phase (variant 29) and in its 16-B-piece form (variant 0), in one round and in four. Bit-exact
against zlib; a failure names the first wrong chunk and the cells of each of its segments.

Every run takes a caller `out` prefilled with 0xA5A5A5A5 (the segments XOR into it, so a chunk the plan did not
clear shows) or, in place, crc_in itself; a caller workspace of exactly ambrycrc_workspace_bytes(n) between 0xA5
guards; and leaves its input untouched. The region view starts on a 64-B boundary and 5 bytes past one: the
kernel's arithmetic is relative to the view's first byte, and so are the lattice's cells."""
import numpy as np
import pytest

import sweep_lattice as L
from gpu_buffers import assert_guards, assert_untouched, guarded, guarded_workspace

pytestmark = pytest.mark.gpu

PREFILL = 0xA5A5A5A5


def run_sweep(gpu, lat, variant, rounds=False, shift=0, in_place=False):
    """One batch call over the lattice under (variant, grid, window), all three restored afterwards."""
    import torch

    geo = lat.rounds if rounds else lat
    n = len(lat.off)
    whole, mem = guarded(lat.mem, shift)
    off, ln = torch.from_numpy(lat.off).cuda(), torch.from_numpy(lat.length).cuda()
    cin = torch.from_numpy(lat.crc_in.view(np.int32).copy()).cuda()
    out = cin if in_place else torch.from_numpy(np.full(n, PREFILL, dtype=np.uint32).view(np.int32)).cuda()
    wwhole, ws = guarded_workspace(gpu.workspace_bytes(n))
    variant_was, grid_was = gpu.get_variant(0), gpu.grid_size(0)
    try:
        gpu.set_variant(0, variant)
        gpu.set_grid(0, geo.grid)
        gpu.set_window(0, geo.window)
        gpu.crc32_batch(mem, off, ln, crc_in=cin, out=out, workspace=ws)
        torch.cuda.synchronize()
    finally:
        gpu.set_variant(0, variant_was)
        gpu.set_grid(0, grid_was)
        gpu.set_window(0, L.DEFAULT_WINDOW_BYTES)
    got = out.cpu().numpy().view(np.uint32)
    if not np.array_equal(got, lat.expect):
        bad = np.nonzero(got != lat.expect)[0]
        i = int(bad[0])
        walk = L.lattice_walk(lat.form, lat.S, rounds)
        segs = sorted(L.by_chunk(walk.segments).get(i, []), key=lambda s: (s.r0, s.share))
        raise AssertionError(
            "%d of %d chunks differ (variant %d, grid %d, window %d, shift %d%s); first chunk %d (%s): %#x, expected %#x; "
            "off %d (mod 64: %d), len %d, crc_in %#x; segments: %s" % (
                len(bad), n, variant, geo.grid, geo.window, shift, ", in place" if in_place else "", i, lat.kind[i], got[i],
                lat.expect[i], lat.off[i], lat.off[i] & 63, lat.length[i], lat.crc_in[i],
                L.describe_segments(segs) or "none (the plan's or the group phase's chunk)"))
    assert_guards(wwhole, ws)
    assert_untouched(whole, mem, lat.mem, shift)


@pytest.mark.parametrize("variant,form,S", [(29, "wave", 16384), (29, "wave", 21504), (29, "group", 16384),
                                            (0, "wave", 16384), (0, "wave", 21504), (0, "wave", 24576)])
def test_sweep_over_the_lattice(gpu, variant, form, S):
    """Variant 29 in wave form at both share sizes and in group form (at least 16,384 chunks: every chunk of at
    most 16 KiB is the group phase's and takes no share); variant 0 over the wave geometry, which holds for it at
    any chunk count (it has no group phase), and at 24 KiB too: only there does body_crc<8> roll twice. The view
    64-aligned and 5 bytes off, and once in place."""
    lat = L.sweep_lattice(form, S)
    assert lat.small_max == (L.GROUP_SMALL_MAX if len(lat.off) >= L.GROUP_MIN_CHUNKS and variant == 29 else 0)
    run_sweep(gpu, lat, variant)
    run_sweep(gpu, lat, variant, shift=5)
    run_sweep(gpu, lat, variant, in_place=True)


@pytest.mark.parametrize("variant", [29, 0])
def test_sweep_rounds_over_the_lattice(gpu, variant):
    """The 16 KiB wave lattice with a quarter of the workgroups and a window of a quarter of the stream: four
    rounds of the same 16 KiB shares, so every cut stays where it was while wave w takes shares w, w + nwaves,
    ...; a probe crosses from one round's last share into the next round's first, and the last round is part full
    (test_sweep_lattice.py test_rounds_geometry asserts all of it)."""
    lat = L.sweep_lattice("wave", 16384)
    assert L.share_size(lat.total, lat.rounds.grid, lat.rounds.window) == (lat.S, 4)
    run_sweep(gpu, lat, variant, rounds=True)
    run_sweep(gpu, lat, variant, rounds=True, shift=5, in_place=True)
