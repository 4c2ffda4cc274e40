"""Two faults in one message (header_lattice.pairs() and truncated_pairs(): per base every pair of operations of
two different sites): first what the lattice covers, against the oracle alone, then every CPU entry that reads a
stored message against its oracle, as test_header_lattice.py does for one fault. Each entry assembles its answer
from pieces of its own -- the header verdict, the record checks, the CRC bits, the send's mask by flag -- so one
fault right does not make two right: a bit dropped, a bit kept that a short span should have discarded, a refused
message partly written."""
import functools
import hashlib

import numpy as np
import pytest

import hard_delete_oracle as HD
import header_lattice as HL
import recover_oracle as RO
import rekey_oracle as RK
import send_oracle as SO
from header_lattice import pair_descs, sizes_of
from msgfmt import MF

PACKED_SHA256 = "65ecbd46c26a4833c6e4a92faf4ea6a017928d75a12100bbea73abf0fd1f1fb9"


@pytest.fixture(scope="module")
def dev(ambry):
    from ambry_amd import device as D

    return D


@pytest.fixture(scope="module")
def messages(ambry):
    from ambry_amd import messages as M

    return M


def cases():
    """[(name, region, offset)]: every pair in the packed region, then the truncated regions."""
    names, region, offs = HL.pairs()
    return [(n, region, o) for n, o in zip(names, offs)] + HL.truncated_pairs()


def groups():
    """[(names, region, offsets)]: the packed pairs as one group, each truncated region on its own."""
    return [HL.pairs()] + [([n], r, [o]) for n, r, o in HL.truncated_pairs()]


@functools.lru_cache(maxsize=None)
def verdicts():
    """{case name: the verify oracle's (status, end)}."""
    return {n: MF.verify_message(r, o) for n, r, o in cases()}


@functools.lru_cache(maxsize=None)
def single_status():
    """{(base, op name): the verify oracle's status of that one fault, a clean PUT behind the message}."""
    tail = HL.bases()["v3-put-enc"].bytes()
    return {(name, op.name): MF.verify_message(HL.build(m, [op]) + tail, 0)[0]
            for name, m in HL.bases().items() for op in HL.operations(m)}


# ---------------------------------------------------------------- what the lattice covers
def test_single_fault_lattice_is_unchanged():
    names, region, offs = HL.packed()
    assert len(names) == 231 and hashlib.sha256(region).hexdigest() == PACKED_SHA256
    for name, m in HL.bases().items():  # every operation alone changes the message and keeps its length
        for op in HL.operations(m):
            b = HL.build(m, [op])
            assert b != m.bytes() and len(b) == m.end, (name, op.name)


def test_every_pair_of_sites_occurs():
    seen = {(base, a.site, b.site) for base, a, b, _ in HL.pair_cases()}
    for name, m in HL.bases().items():
        sites = sorted({op.site for op in HL.operations(m)})
        assert {"h.version", "h.crc", "h.total"} <= set(sites)
        for k in m.present():
            assert "h.rel%d" % k in sites and "r%d.field" % k in sites and "r%d.crc" % k in sites, (name, k)
        for i, a in enumerate(sites):
            for b in sites[i + 1:]:
                assert (name, a, b) in seen or (name, b, a) in seen, (name, a, b)
    names, region, offs = HL.pairs()
    assert len(names) == len(set(names)) == len(HL.pair_cases()) + 1
    assert 5000 <= len(names) <= 7000 and len(region) / len(names) < 200  # region mode applies on the device


def test_statuses_the_pairs_reach():
    """At least 25 distinct statuses; at least 500 cases whose status is the OR of two different non-zero
    single-fault statuses; at least 50 whose status is neither single status nor their OR (total+1 with blob-size+1
    cancel and leave BLOB_CRC alone); and CRC bits collected from an earlier record, then discarded by a later
    span under 8 bytes."""
    v, single = verdicts(), single_status()
    names = HL.pairs()[0]
    assert v["tail/clean"] == (0, len(HL.pairs()[1]))
    assert len({v[n][0] for n in names}) >= 25
    ored = other = discarded = 0
    for (base, a, b, _), n in zip(HL.pair_cases(), names):
        s, sa, sb = v[n][0], single[base, a.name], single[base, b.name]
        assert s or not (sa and sb), n  # only the non-ASCII owner verifies clean
        ored += bool(sa and sb) and s == sa | sb and s not in (sa, sb)
        other += s not in (sa, sb, sa | sb)
        first, second = (a, b) if a.stage == 4 else (b, a)
        if first.site.endswith(".crc") and first.site[0] == "r" and second.name.endswith("=next-7") and \
                second.site.startswith("h.rel") and int(second.site[-1]) > first.k:
            assert sa & sum(MF.RECORD_BITS) or sb & sum(MF.RECORD_BITS), n
            assert v[n] == (MF.BAD_LAYOUT, 0), n
            discarded += 1
    assert ored >= 500 and other >= 50 and discarded >= 20, (ored, other, discarded)


def test_truncated_pairs_differ_from_the_single_cuts():
    single = {(r, o) for _, r, o in HL.truncated()}
    tp = HL.truncated_pairs()
    assert 100 <= len(tp) <= 300 and len({n for n, _, _ in tp}) == len(tp)
    assert all((r, o) not in single for _, r, o in tp)
    assert {v for n, v in verdicts().items() if "/cut=" in n} >= {(MF.BAD_LAYOUT, 0), (MF.BAD_VERSION, 0)}


# ---------------------------------------------------------------- the CPU entries
def test_verify_and_transform(messages):
    for name, region, off in cases():
        buf = np.frombuffer(region, dtype=np.uint8)
        assert messages.verify_message_cpu(buf, off) == verdicts()[name], name
        for hv, life in ((3, None), (3, 5), (1, None), (1, 2)):
            st, out = messages.transform_message_cpu(buf, off, header_version=hv, life=life)
            assert (st, out) == MF.transform_message(region, off, life=life, version=hv), (name, hv)


def test_hard_delete(dev):
    for names, region, offs in groups():
        exp = HD.hard_delete(region, offs)
        for plan_only in (True, False):
            st, info, after = HD.run_cpu(dev, region, offs, plan_only=plan_only)
            assert st == exp[0] and np.array_equal(info, exp[1]), names[0]
            assert after == (region if plan_only else exp[2]), names[0]  # a refused message byte for byte as it was


def test_rekey(messages):
    for names, region, offs in groups():
        descs, aux = pair_descs(len(offs))
        buf, ax = np.frombuffer(region, dtype=np.uint8), np.frombuffer(aux, dtype=np.uint8)
        for i, off in enumerate(offs):
            for hv, life in ((3, None), (1, 4)):
                got = messages.rekey_message_cpu(buf, off, descs[i], ax, header_version=hv, life=life)
                assert got == RK.rekey_message(region, off, descs[i], aux, life=life, version=hv), (names[i], hv)


@pytest.mark.parametrize("sized", [False, True], ids=["header-size", "given-size"])
def test_send(messages, sized):
    for names, region, offs in groups():
        buf = np.frombuffer(region, dtype=np.uint8)
        sizes = sizes_of(region, offs)
        for i, name in enumerate(names):
            size = (sizes[i] or None) if sized else None  # the CPU entry's size 0 means "the header's"
            for flag in SO.FLAGS:
                st, f, b = messages.send_message_cpu(buf, offs[i], flag, size=size)
                est, ef, eb = SO.send_message(region, offs[i], size, flag)
                assert (st, {n: int(f[n]) for n in SO.INFO.names}, b) == (est, ef, eb), (name, flag)


def test_chain_and_recover(dev):
    for name, region, off in cases():
        RO.assert_call(dev.recover_messages_cpu(region, off, 3), RO.recover(region, off, 3), 3)
        assert dev.chain_messages_host(region, off, 3) == RO.chain_result(region, off, 3)[0], name
