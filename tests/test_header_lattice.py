"""Every CPU entry that reads a stored message's header, over the header lattice (tests/header_lattice.py: each
branch of the header rule placed on purpose), against its oracle: status, end or length, and the output bytes."""
import functools

import numpy as np
import pytest

import hard_delete_oracle as HD
import header_lattice as HL
import recover_oracle as RO
import rekey_oracle as RK
import send_oracle as SO
from header_lattice import rekey_desc, sizes_of
from msgfmt import MF


@pytest.fixture(scope="module")
def dev(ambry):
    from ambry_amd import device as D

    return D


@pytest.fixture(scope="module")
def messages(ambry):
    from ambry_amd import messages as M

    return M


@functools.lru_cache(maxsize=None)
def verdicts():
    """{case name: the verify oracle's (status, end)}."""
    return {n: MF.verify_message(r, o) for n, r, o in HL.cases()}


def test_lattice_places_every_verdict():
    """The lattice reaches what it is for: clean messages of every base, and each header verdict."""
    names, region, offs = HL.packed()
    assert 200 <= len(names) <= 320 and len(region) / len(names) < 200
    v = verdicts()
    assert all(v[n + "/clean"][0] == 0 for n in HL.bases())
    seen = {s for s, _ in v.values()}
    assert {0, MF.BAD_VERSION, MF.HEADER_CRC, MF.BAD_LAYOUT, MF.BAD_RECORD} <= seen
    for n, (s, e) in v.items():
        tail = n.split("/")[1]
        if tail.startswith("version="):
            assert s == MF.BAD_VERSION, n
        elif tail.startswith("crc-"):
            assert s == MF.HEADER_CRC, n
        elif tail == "enckey=-1":  # still a PUT's shape: the key and the encryption-key record read as the key
            assert s and not s & MF.BAD_LAYOUT and e != 0, n
        elif tail.startswith(("life=", "total=", "cut=", "offset-past", "total+1-at-end")) or tail.endswith(
                ("=-1", "=hs-1", "=previous", "=next-7", "slot-set")) or "<->" in tail:
            assert s == MF.BAD_LAYOUT and e == 0, n
        elif "-size" in tail or "blob-type" in tail:
            assert s == MF.BAD_RECORD and e != 0, n
        elif "version=" in tail:
            assert s == MF.BAD_VERSION and e != 0, n


def test_verify_and_transform(messages):
    for name, region, off in HL.cases():
        buf = np.frombuffer(region, dtype=np.uint8)
        assert messages.verify_message_cpu(buf, off) == verdicts()[name], name
        for hv, life in ((3, None), (3, 5), (2, None), (1, 2)):
            st, out = messages.transform_message_cpu(buf, off, header_version=hv, life=life)
            assert (st, out) == MF.transform_message(region, off, life=life, version=hv), (name, hv)


def test_hard_delete(dev):
    for name, region, off in HL.cases():
        est, einfo, erep = HD.one(region, off)
        for plan_only in (True, False):
            buf = np.frombuffer(region, dtype=np.uint8).copy()
            st, info = dev.hard_delete_message_cpu(buf, off, None, plan_only)
            assert st == est, name
            assert info == (einfo if est == 0 else np.zeros((), dtype=HD.INFO)), name
            after = bytearray(region)
            if est == 0 and not plan_only:
                after[erep[0]:erep[0] + len(erep[1])] = erep[1]
            assert buf.tobytes() == bytes(after), name
        if est == 0:  # with recovery info: the records are not read, the header still is
            buf = np.frombuffer(region, dtype=np.uint8).copy()
            assert dev.hard_delete_message_cpu(buf, off, einfo, True)[0] == HD.one(region, off, einfo)[0] == 0


def test_rekey(messages):
    d, aux = rekey_desc()
    ax = np.frombuffer(aux, dtype=np.uint8)
    for name, region, off in HL.cases():
        buf = np.frombuffer(region, dtype=np.uint8)
        for hv, life in ((3, None), (1, 4)):
            got = messages.rekey_message_cpu(buf, off, d, ax, header_version=hv, life=life)
            assert got == RK.rekey_message(region, off, d, aux, life=life, version=hv), (name, hv)


@pytest.mark.parametrize("sized", [False, True], ids=["header-size", "given-size"])
def test_send(messages, sized):
    names, region, offs = HL.packed()
    groups = [(names, region, offs)] + [([n], r, [o]) for n, r, o in HL.truncated()]
    for names, region, offs in groups:
        buf = np.frombuffer(region, dtype=np.uint8)
        sizes = sizes_of(region, offs)
        for i, name in enumerate(names):
            size = (sizes[i] or None) if sized else None  # the CPU entry's size 0 means "the header's"
            for flag in SO.FLAGS:
                st, f, b = messages.send_message_cpu(buf, offs[i], flag, size=size)
                est, ef, eb = SO.send_message(region, offs[i], size, flag)
                assert (st, {n: int(f[n]) for n in SO.INFO.names}, b) == (est, ef, eb), (name, flag)


def test_chain_and_recover(dev):
    for name, region, off in HL.cases():
        if off > len(region):
            continue  # an argument error of these entries, not a header verdict
        RO.assert_call(dev.recover_messages_cpu(region, off, 3), RO.recover(region, off, 3), 3)
        assert dev.chain_messages_host(region, off, 3) == RO.chain_result(region, off, 3)[0], name


def test_host_entries_cpu_leg(dev, messages):
    names, region, offs = HL.packed()
    groups = [(names, region, offs)] + [([n], r, [o]) for n, r, o in HL.truncated()]
    for names, region, offs in groups:
        st, end = dev.verify_messages_host(region, offs, device=-1)
        assert [(int(s), int(e)) for s, e in zip(st, end)] == [MF.verify_message(region, o) for o in offs], names[0]
        life = (np.arange(len(offs)) % 5).astype(np.int16)
        out, oo, ol, st = messages.transform_host(region, offs, life_version=life, device=-1)
        pos = 0
        for i, o in enumerate(offs):
            est, exp = MF.transform_message(region, o, life=int(life[i]), version=3)
            assert int(st[i]) == est, names[i]
            if exp is None:
                assert ol[i] == 0 and oo[i] == -1, names[i]
                continue
            assert oo[i] == pos and out[pos:pos + len(exp)] == exp, names[i]
            pos += len(exp)
