"""The host-staged legs' slab cuts, without a GPU: the model's geometry is what ambrycrc_ctx.h states,
every case of host_slab_model's tables plans the cut it names on the side it names, within the
geometry, and the message cases' inputs are tied to the reference (the CPU leg, device -1, gives
MF.verify_message's and MF.transform_message's answers) before any GPU sees them."""
import ctypes
import os
import re

import numpy as np
import pytest

import host_slab_model as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEO = H.HEADER_GEOMETRY


def test_geometry_is_what_the_header_states():
    """HEADER_GEOMETRY against the constants' text in ambrycrc_ctx.h and ambrycrc.h."""
    ctx = open(os.path.join(ROOT, "ambry_amd", "csrc", "ambrycrc_ctx.h")).read()
    abi = open(os.path.join(ROOT, "include", "ambrycrc.h")).read()

    def shifted(name):
        m = re.search(r"constexpr size_t %s = (\d+)u(?:ll)? << (\d+);" % name, ctx)
        assert m, name
        return int(m.group(1)) << int(m.group(2))

    growth = int(re.search(r"#define\s+AMBRYCRC_TRANSFORM_GROWTH_MAX\s+(\d+)", abi).group(1))
    assert growth == H.GROWTH
    assert re.search(r"constexpr size_t kXformOutBytes = kSlabBytes \+ \(size_t\)AMBRYCRC_TRANSFORM_GROWTH_MAX \* "
                     r"kSlabMsgs;", ctx)
    stated = H.Geometry(shifted("kSlabBytes"), shifted("kSlabChunks"), shifted("kSlabMsgs"),
                        shifted("kSlabBytes") + growth * shifted("kSlabMsgs"))
    assert stated == GEO


def test_last_host_slabs_needs_a_context(ambry):
    info = (ctypes.c_uint64 * 6)()
    assert ambry.lib().ambrycrc_last_host_slabs(63, info) == -4  # never initialised here
    assert ambry.lib().ambrycrc_last_host_slabs(63, None) == -4


@pytest.mark.parametrize("cases,sides", [(H.batch_cases, H.BATCH_SIDES), (H.verify_cases, H.VERIFY_SIDES),
                                         (H.transform_cases, H.TRANSFORM_SIDES)], ids=["batch", "verify", "transform"])
def test_every_family_has_a_case_on_each_side(cases, sides):
    groups = H.families(cases())
    assert set(groups) == set(sides)
    for family, group in groups.items():
        assert {c["side"] for c in group} == sides[family], family
    names = [c["name"] for c in cases()]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("family", sorted(H.BATCH_SIDES))
def test_batch_plans(family):
    """Each case's plan is the one it states: piece starts multiples of 16, pieces adding up to their
    chunks, nothing past the geometry (check_plan). The chunks lie inside the data buffer."""
    for case in H.families(H.batch_cases())[family]:
        slabs, _ = H.check_plan(case, GEO)
        assert slabs == case["expect"]["slabs"]
        for off, n in case["chunks"]:
            assert n == 0 or off + n + max(H.ALIGNMENTS) <= H.DATA_BYTES + 16, case["name"]


def test_model_follows_another_geometry():
    """The model takes the geometry as arguments: under a 1 KiB slab of 4 pieces the same rules give
    other cuts (and the tables' fixed addresses no longer meet theirs)."""
    tiny = H.Geometry(1024, 4, 3, 1024 + 26 * 3)
    assert H.plan_batch([1000, 0, 50, 1, 1, 1, 1, 1], tiny) == [
        [(0, 1000, 0), (1, 0, 1008), (2, 16, 1008)], [(2, 34, 0), (3, 1, 48), (4, 1, 64), (5, 1, 80)], [(6, 1, 0), (7, 1, 16)]]
    slabs, over = H.plan_verify([5000, 0, 900, 2000, 2001, 2002, 2003], [10, 100, 124, 1025, 1, 1, 1], 6000, tiny)
    assert [(s["lo"], s["hi"], s["members"]) for s in slabs] == [(0, 1024, [1, 2]), (2001, 2004, [4, 5, 6]),
                                                                 (5000, 5010, [0])] and over == [3]
    runs, over = H.plan_transform([2000, 1000, 976, 3000, 3000, 3000, 3000], [24, 24, 24, 400, 400, 400, 400], 6000, tiny)
    assert [(r["i0"], r["n"], r["lo"], r["hi"]) for r in runs] == [(0, 2, 1000, 2024), (2, 1, 976, 1000),
                                                                  (3, 2, 3000, 3400), (5, 2, 3000, 3400)] and over == []
    with pytest.raises(AssertionError):
        H.check_plan(H.batch_cases()[0], H.Geometry(GEO.slab_bytes + 16, *GEO[1:]))


def _cpu_verify(region, offs):
    from ambry_amd import device

    st, end = device.verify_messages_host(region, offs, device=-1)
    return st.tolist(), end.tolist()


@pytest.mark.parametrize("family", sorted(H.VERIFY_SIDES))
def test_verify_cases_plan_and_reference(ambry, family):
    """The plan each case states, and the CPU leg's statuses and ends equal to MF.verify_message's."""
    for case in H.families(H.verify_cases())[family]:
        H.check_plan(case, GEO)
        with H.region_for(case) as region:
            assert _cpu_verify(region, case["offs"]) == H.oracle_verify(region, case["offs"]), case["name"]


@pytest.mark.parametrize("family", sorted(H.TRANSFORM_SIDES))
def test_transform_cases_plan_and_reference(ambry, family):
    """The plan each case states, and the CPU leg's outputs equal to MF.transform_message's bytes packed
    by the rule (every message under its own life version)."""
    from ambry_amd.messages import transform_host

    for case in H.families(H.transform_cases())[family]:
        H.check_plan(case, GEO)
        with H.region_for(case) as region:
            cap = case["out_cap"] if case["out_cap"] is not None else H.ample_cap(case, region)
            got = transform_host(region, case["offs"], life_version=case["lives"], out_cap=cap, device=-1)
            H.check_transform(case, region, got, H.oracle_messages(region, case["offs"], case["lives"]))


def test_extent_is_the_header_window_or_the_message():
    sm = H.small()
    region = np.full(400, H.JUNK, dtype=np.uint8)
    msg = sm["p2"]
    region[10:10 + len(msg)] = np.frombuffer(msg, dtype=np.uint8)
    assert H.extent(region, 10) == len(msg)
    assert H.extent(region[:10 + len(msg) - 1], 10) == 40  # the sizes no longer fit
    assert H.extent(region[:10 + 39], 10) == 39 and H.extent(region[:11], 10) == 1
    assert H.extent(region, 0) == 40 and H.extent(region, 399) == 1 and H.extent(region, 400) == 0
    assert H.extent(region, 401) == 0 and H.extent(region, 380) == 20
