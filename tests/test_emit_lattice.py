"""Every CPU entry that writes a stored PUT message, over the writer lattice (tests/emit_lattice.py: each branch
of the writer placed on purpose), against its oracle: status for status, byte for byte."""
import numpy as np
import pytest

import emit_lattice as EL
import ingest_oracle as IO
from emit_lattice import OUT_VERSIONS, assert_packed, ingest_expected, life_of, rekey_expected, transform_expected
from msgfmt import MF


@pytest.fixture(scope="module")
def messages(ambry):
    from ambry_amd import messages as M

    return M


def test_lattice_places_every_branch():
    """From the case names and the oracles' verdicts alone: every branch of the writer occurs, and no oracle
    refuses a case (a refusal would hide the branch the case is there for)."""
    cs = EL.cases()
    region, offs, _ = EL.region()
    assert 200 <= len(cs) <= 400 and all(140 <= len(c.stored()) <= 400 for c in cs)
    names = [dict(kv.split("=") for kv in c.name.split("/")) for c in cs]
    assert all(tuple(n) == EL.KEYS for n in names)

    def seen(*keys):
        return {tuple(n[k] for k in keys) for n in names}

    assert seen("hv", "enc") == {("1", "none")} | {(h, e) for h in "23" for e in ("none", "set", "empty")}
    assert seen("hv", "bv") == {(h, b) for h in "123" for b in "123"}
    # each stored SerDe version: the stored length and the VERSION_5 length at every position of an 8-B word
    for sv in range(1, 6):
        stored = {len(c.props) % 8 for c in cs if c.sv == sv}
        out = {c.out_props_len % 8 for c in cs if c.sv == sv}
        assert stored == out == set(range(8)), sv
        # (and the appended fields both inside one word and across two)
        if EL.APPENDIX[sv]:
            assert {len(c.props) // 8 == (c.out_props_len - 1) // 8 for c in cs if c.sv == sv} >= {False}
    assert {("5", "0", "0"), ("5", "1", "1"), ("5", "2", "0"), ("5", "0", "2"), ("4", "0", "3"), ("3", "0", "3")} <= \
        seen("sv", "priv", "encb")
    assert {("1", "0"), ("2", "0"), ("3", "0"), ("3", "1"), ("3", "2")} == seen("bv", "comp")
    assert {(b, n) for b in "123" for n in "01"} <= seen("bv", "n")
    assert {"0", "1"} <= {n["um"] for n in names}
    assert {(r, b, i) for r in "01" for b in ("given", "none") for i in ("pos", "neg")} <= seen("repl", "bs", "ids")
    assert {("keep", b, i) for b in ("given", "none") for i in ("pos", "neg")} <= seen("repl", "bs", "ids")
    assert {(m, b) for m, b in (("1", "2"), ("1", "3"), ("0", "1"), ("0", "2"), ("0", "3"))} == seen("meta", "bv")
    # no oracle refuses a case, at any output header version
    assert all(MF.verify_message(region, o) == (0, o + len(c.stored())) for c, o in zip(cs, offs))
    for v in OUT_VERSIONS:
        assert all(st == 0 and b for st, b in transform_expected(v, True)), v
        assert all(st == 0 and b for st, b in rekey_expected(v, False)), v
        assert not ingest_expected(v)[0].any(), v
    # the ingest's "remaining() == 0 ? null": an empty key on the wire writes no record, a set one does
    wire, refs = EL.wire()
    st, packed, off, ln = ingest_expected(3)[:4]
    for c, o in zip(cs, off):
        assert (MF.parse_header(packed, int(o))[2][0] != MF.INVALID) == (c.enc == "set"), c.name
    # a stored empty key is a record of its own through the transform and the re-key
    for c, (_, b) in zip(cs, transform_expected(3, False)):
        assert (MF.parse_header(b, 0)[2][0] != MF.INVALID) == (c.enc != "none"), c.name
    # the fast path's run is dense and taken whole
    fr, fo, fc = EL.fast_region()
    assert len(fc) >= 24 and all(c.fast() for c in fc)
    assert {c.enc for c in fc} == {"none", "set", "empty"}


@pytest.mark.parametrize("version", OUT_VERSIONS)
def test_transform_message_cpu(messages, version):
    region, offs, cs = EL.region()
    buf = np.frombuffer(region, dtype=np.uint8)
    for use_life in (True, False):
        exp = transform_expected(version, use_life)
        for i, o in enumerate(offs):
            got = messages.transform_message_cpu(buf, o, header_version=version, life=life_of(i, version, use_life))
            assert got == exp[i], cs[i].name


@pytest.mark.parametrize("version", OUT_VERSIONS)
def test_transform_host_cpu_leg(messages, version):
    for fast_only in (False, True):
        region, offs, cs = EL.region(fast_only)
        life = (np.arange(len(offs)) % 5).astype(np.int16)
        out, oo, ol, st = messages.transform_host(region, offs, header_version=version, life_version=life, device=-1)
        assert_packed(out, oo, ol, st, transform_expected(version, True, fast_only), [c.name for c in cs])


@pytest.mark.parametrize("version", OUT_VERSIONS)
def test_rekey_message_cpu(messages, version):
    region, offs, cs = EL.region()
    descs, aux = EL.rekey_inputs()
    buf, ax = np.frombuffer(region, dtype=np.uint8), np.frombuffer(aux, dtype=np.uint8)
    for use_life in (False, True):
        exp = rekey_expected(version, use_life)
        for i, o in enumerate(offs):
            got = messages.rekey_message_cpu(buf, o, descs[i], ax, header_version=version,
                                             life=life_of(i, version, use_life))
            assert got == exp[i], cs[i].name


@pytest.mark.parametrize("version", OUT_VERSIONS)
def test_ingest_put_request_cpu(messages, version):
    wire, refs = EL.wire()
    est, packed, eoff, eln, ecrc, einfo, _ = ingest_expected(version)
    buf = np.frombuffer(wire, dtype=np.uint8)
    for i, (c, r) in enumerate(zip(EL.cases(), refs)):
        st, msg, crc, info = messages.ingest_put_request_cpu(buf, int(r["off"]), int(r["key_len"]), header_version=version)
        o, n = int(eoff[i]), int(eln[i])
        assert (st, crc, msg) == (int(est[i]), int(ecrc[i]), packed[o:o + n]), c.name
        e = einfo[i].copy()
        e["msg_off"] = 0
        assert np.frombuffer(np.asarray(info).tobytes(), dtype=IO.INFO)[0] == e, c.name


@pytest.mark.parametrize("version", OUT_VERSIONS)
def test_serialize_host(messages, version):
    msgs, exp = EL.put_messages(version, big_tail=True)
    for i, (m, e) in enumerate(zip(msgs, exp)):
        got, _ = messages.serialize_host(m)
        assert got == e, i
