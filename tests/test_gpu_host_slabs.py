"""The host-staged GPU legs (ambrycrc_host.cpp: batch, message verify, transform) with their slab cuts
placed on purpose: every case of host_slab_model's tables, whose plans test_host_slab_model.py holds
against the model and whose inputs it ties to the reference. Here each case runs on the GPU leg --
CRCs against zlib, verify against MF.verify_message and the whole-region device call, transform
against MF.transform_message and ambrycrc_transform_messages_dev over the whole region -- and the
library's own count of committed slabs and oversize messages (ambrycrc_last_host_slabs) must be the
model's, computed from the geometry the library reports. A case first checks its stated plan under
that geometry (check_plan): were a slab constant changed, the fixed addresses would fail there
instead of quietly never crossing a slab again."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import host_slab_model as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def geo(gpu):
    info = gpu.last_host_slabs(0)
    return H.Geometry(info["slab_bytes"], info["slab_chunks"], info["slab_msgs"], info["xform_out_bytes"])


def staged(gpu):
    """(slabs, oversize) of the last host call, which took the GPU leg."""
    assert gpu.last_host_path(0) == 1
    info = gpu.last_host_slabs(0)
    return info["slabs"], info["oversize"]


def test_reported_geometry_and_arguments(gpu, geo, ambry):
    assert geo == H.HEADER_GEOMETRY
    assert ambry.lib().ambrycrc_last_host_slabs(0, None) == -1
    info = (ctypes.c_uint64 * 6)()
    assert ambry.lib().ambrycrc_last_host_slabs(63, info) == -4


def test_counts_are_zero_before_any_host_call(gpu):
    """A fresh process: the geometry is reported, both counts are 0; a CPU-leg call leaves them so."""
    code = ("import sys; sys.path.insert(0, %r); from ambry_amd import device as D; D.init(0); "
            "a = D.last_host_slabs(0); D.set_host_policy(0, D.HOST_CPU); D.crc32_batch_host([(0, 0)]); "
            "print(a['slabs'], a['oversize'], a['slab_bytes'], D.last_host_slabs(0)['slabs'])" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[-4:] == ["0", "0", str(H.S), "0"]


# ------------------------------------------------------------------ the batch leg
@pytest.fixture(scope="module")
def sources(gpu):
    """The data buffer, pageable and pinned (the same bytes), and the zlib reference over it."""
    import torch

    data = H.batch_data()
    pinned = torch.from_numpy(data).pin_memory()
    return {False: data, True: pinned.numpy(), "keep": pinned, "ref": H.CrcRef(data)}


def run_batch_case(gpu, case, sources, base, pinned, geo):
    from ambry_amd import filestore

    want_slabs, _ = H.check_plan(case, geo)
    data, ref = sources[pinned], sources["ref"]
    addr = data.ctypes.data + base
    what = (case["name"], base, pinned)
    if case["entry"] == "batch":
        cin = case["crc_in"] or [0] * len(case["chunks"])
        chunks = [(None if off is None else addr + off, n) for off, n in case["chunks"]]
        got = gpu.crc32_batch_host(chunks, device=0, pinned=pinned, crc_in=case["crc_in"])
        exp = [c if off is None else ref.crc(base + off, n, c) for (off, n), c in zip(case["chunks"], cin)]
        assert got == exp, what
    elif case["entry"] == "trailed":
        saved, bufs = [], []
        try:
            for off, n, kind in case["items"]:
                if kind != "short":
                    crc = ref.crc(base + off, n) ^ (0x100 if kind == "wrong" else 0)
                    at = base + off + n
                    saved.append((at, data[at:at + 8].copy()))
                    data[at:at + 8] = np.frombuffer(struct.pack(">Q", crc), dtype=np.uint8)
                bufs.append(data[base + off:base + off + (n if kind == "short" else n + 8)])
            got = gpu.verify_trailed_host(bufs, device=0, pinned=pinned)
        finally:
            for at, old in saved:
                data[at:at + 8] = old
        assert got == [kind != "good" for _, _, kind in case["items"]], what
    else:
        got = filestore.checksums_for_ranges(data[base:base + case["file_len"]], case["ranges"], device=0)
        assert got == [ref.crc(base + off, n) for off, n in case["chunks"]], what
    assert staged(gpu) == (want_slabs, 0), what


@pytest.mark.parametrize("family", sorted(H.BATCH_SIDES))
def test_batch_leg(gpu, geo, sources, family):
    for case in H.families(H.batch_cases())[family]:
        for base in H.ALIGNMENTS:
            run_batch_case(gpu, case, sources, base, False, geo)
            if case["pinned"] and case["entry"] != "ranges":
                run_batch_case(gpu, case, sources, base, True, geo)


# ------------------------------------------------------------------ the message legs
def device_region(region, offs):
    import torch

    return torch.from_numpy(region).cuda(), torch.tensor(offs, dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("family", sorted(H.VERIFY_SIDES))
def test_verify_leg(gpu, geo, family):
    import torch

    for case in H.families(H.verify_cases())[family]:
        want = H.check_plan(case, geo)
        with H.region_for(case) as region:
            st, end = gpu.verify_messages_host(region, case["offs"])
            counts = staged(gpu)
            assert (st.tolist(), end.tolist()) == H.oracle_verify(region, case["offs"]), case["name"]
            dev, offs = device_region(region, case["offs"])
            dst, dend = gpu.verify_messages(dev, offs)
            torch.cuda.synchronize()
        assert np.array_equal(st, dst.cpu().numpy().view(np.uint32)), case["name"]
        assert np.array_equal(end, dend.cpu().numpy().view(np.uint64)), case["name"]
        assert counts == want, case["name"]


@pytest.mark.parametrize("family", sorted(H.TRANSFORM_SIDES))
def test_transform_leg(gpu, geo, family):
    import torch

    from ambry_amd.messages import transform_dev, transform_host

    for case in H.families(H.transform_cases())[family]:
        want = H.check_plan(case, geo)
        with H.region_for(case) as region:
            cap = case["out_cap"] if case["out_cap"] is not None else H.ample_cap(case, region)
            got = transform_host(region, case["offs"], life_version=case["lives"], out_cap=cap)
            counts = staged(gpu)
            messages = H.oracle_messages(region, case["offs"], case["lives"], largest=H.SMALL_MESSAGE)
            dev, offs = device_region(region, case["offs"])
            dout, doo, dol, dst = transform_dev(dev, offs, life_version=torch.tensor(case["lives"], dtype=torch.int16,
                                                                                     device="cuda"),
                                                out=torch.empty(max(cap, 1), dtype=torch.uint8, device="cuda"))
            torch.cuda.synchronize()
            out, oo, ol, st = got
            if all(s is not None for s, _ in messages):
                H.check_transform(case, region, got, messages)
            else:  # a message left to the device call below: the small ones' bytes wherever they went
                for i, (s, body) in enumerate(messages):
                    if s is not None:
                        assert st[i] == s and (s or out[oo[i]:oo[i] + ol[i]] == body), (case["name"], i)
        assert np.array_equal(st, dst.cpu().numpy().view(np.uint32)), case["name"]
        assert np.array_equal(oo, doo.cpu().numpy()) and np.array_equal(ol, dol.cpu().numpy()), case["name"]
        assert out == dout[:len(out)].cpu().numpy().tobytes(), case["name"]
        assert counts == want, case["name"]
