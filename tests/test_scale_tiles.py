"""The tiling derivations of scale_tiles.py, each proved against the oracle itself: the oracle walks two
concatenated tiles, and must give what numpy derives from its walk over one. Plus the conditions on the tile's
mix that make a leak between successive messages of one thread visible at the strides of the capped grids."""
import numpy as np
import pytest

import rekey_oracle as RK
import scale_tiles as S
from msgfmt import MF


@pytest.fixture(scope="module")
def t():
    return S.tile()


@pytest.fixture(scope="module")
def two(t):
    """(region, offsets) of two tiles back to back."""
    return t.region * 2, S.tiled_offsets(t.offs, len(t.region), 2)


def test_tile_size(t):
    assert len(t.offs) == S.T == 1201 and all(S.T % p for p in range(2, 35))  # prime
    # about 1 KiB per message: the largest batch (304 CUs) stays under 1 GiB of region and of output
    assert len(t.region) <= 1024 * S.T
    assert S.copies_above_caps(304) * (len(t.region) + 26 * S.T + len(t.aux)) < 1 << 30
    assert S.copies_above_caps(256) * S.T == 524_837 > 2 * 4 * 256 * 256


def test_tile_mix(t):
    st, _ = S.verify_oracle(t.region, t.offs)
    ver = S.header_versions(t.region, t.offs)
    assert len(set(st.tolist())) >= 8
    assert int((st != 0).sum()) >= 80
    clean = st == 0
    assert {1, 2, 3} <= set(ver[clean].tolist())
    heads = [MF.parse_header(t.region, int(o))[2] for o in t.offs[clean]]
    assert sum(1 for r in heads if r[2] != MF.INVALID) >= 50  # update messages
    puts = [r for r in heads if r[2] == MF.INVALID]
    assert sum(1 for r in puts if r[0] != MF.INVALID) >= 100 and sum(1 for r in puts if r[0] == MF.INVALID) >= 100
    # what hard delete, transform and re-key refuse on top of the verify's failures
    rst = S.rekey_oracle(t.region, t.offs, t.descs, t.aux)[0]
    assert {MF.NOT_PUT, MF.NOT_ENCODABLE, RK.NEEDS_CONTENT, RK.BAD_DESC} <= set(rst.tolist())
    assert int((t.descs["key_len"] == 0).sum()) >= 20  # skipped by the re-key


@pytest.mark.parametrize("cus", [64, 256, 304])
@pytest.mark.parametrize("blocks_per_cu", [2, 4])
def test_tile_mix_at_the_grid_strides(t, cus, blocks_per_cu):
    """Successive messages of one thread of a capped grid (2 or 4 blocks of 256 threads per CU) differ."""
    st, _ = S.verify_oracle(t.region, t.offs)
    differ, to_refused, to_clean = S.stride_mix(st, S.header_versions(t.region, t.offs), cus, blocks_per_cu)
    assert differ >= 0.5, differ
    assert to_refused >= 1000 and to_clean >= 1000, (to_refused, to_clean)


def test_verify(t, two):
    st, end = S.verify_oracle(t.region, t.offs)
    est, eend = S.tiled_verify(st, end, len(t.region), 2)
    st2, end2 = S.verify_oracle(*two)
    assert np.array_equal(st2, est) and np.array_equal(end2, eend)
    assert (end == 0).any() and (end2[S.T:][end == 0] == 0).all()  # a refused header's end does not shift


@pytest.mark.parametrize("version", [3, 1])
def test_transform(t, two, version):
    st, off, ln, packed = S.transform_oracle(t.region, t.offs, t.life, version)
    assert (off == S.NOWHERE).sum() >= 100 and len(packed) == ln.sum()
    est, eoff, eln = S.tiled_packed(st, off, ln, len(packed), 2)
    st2, off2, ln2, packed2 = S.transform_oracle(*two, np.tile(t.life, 2), version)
    assert np.array_equal(st2, est) and np.array_equal(off2, eoff) and np.array_equal(ln2, eln)
    assert packed2 == packed * 2


@pytest.mark.parametrize("recover", [False, True])
def test_hard_delete(t, two, recover):
    st, info, out = S.hard_delete_oracle(t.region, t.offs)
    assert (st == 0).sum() >= 800 and (st != 0).sum() >= 150 and out != t.region
    rec = None
    if recover:  # the plan's info as recovery info: the same result without reading the record CRCs
        rec = info
        assert S.hard_delete_oracle(t.region, t.offs, rec)[2] == out
    st2, info2, out2 = S.hard_delete_oracle(*two, None if rec is None else np.tile(rec, 2))
    assert np.array_equal(st2, np.tile(st, 2))
    assert np.array_equal(info2, np.tile(info, 2))  # `start` is message-relative
    assert out2 == out * 2


@pytest.mark.parametrize("version,use_life", [(3, False), (1, True)])
def test_rekey(t, two, version, use_life):
    life = t.life if use_life else None
    st, off, ln, packed = S.rekey_oracle(t.region, t.offs, t.descs, t.aux, life, version)
    assert len(packed) == ln.sum()
    est, eoff, eln = S.tiled_packed(st, off, ln, len(packed), 2)
    st2, off2, ln2, packed2 = S.rekey_oracle(*two, np.tile(t.descs, 2), t.aux, None if life is None else np.tile(life, 2),
                                             version)
    assert np.array_equal(st2, est) and np.array_equal(off2, eoff) and np.array_equal(ln2, eln)
    assert packed2 == packed * 2


def test_rekey_out_cap(t, two):
    """An out_cap that ends inside the second tile: NO_ROOM from numpy's running sum, which still advances past
    a refused message; the capped derivation with room for everything is the uncapped one."""
    st, off, ln, packed = S.rekey_oracle(t.region, t.offs, t.descs, t.aux)
    p = len(packed)
    full = S.tiled_rekey_capped(st, ln, 2, 2 * p)
    for a, b in zip(full, S.tiled_packed(st, off, ln, p, 2)):
        assert np.array_equal(a, b)
    for cap in (p + p // 2, p + 1, p - 1, 0):
        est, eoff, eln = S.tiled_rekey_capped(st, ln, 2, cap)
        st2, off2, ln2, packed2 = S.rekey_oracle(*two, np.tile(t.descs, 2), t.aux, out_cap=cap)
        assert np.array_equal(st2, est) and np.array_equal(off2, eoff) and np.array_equal(ln2, eln), cap
        assert packed2 == (packed * 2)[:len(packed2)] and len(packed2) == (eoff + eln).max(initial=0)
    est = S.tiled_rekey_capped(st, ln, 2, p + p // 2)[0]
    assert (est[:S.T] != RK.NO_ROOM).all()
    refused = est[S.T:] == RK.NO_ROOM
    assert 200 <= refused.sum() and (est[S.T:][~refused] == st[~refused]).all()
    assert (st[refused] == 0).all() and (est[S.T:] == 0).sum() >= 200  # part of the second tile, not all of it


def test_serialize(ambry, t, two):
    from ambry_amd.messages import pack_batch, serialize_host

    st, _ = S.verify_oracle(t.region, t.offs)
    msgs = S.clean_puts(t.region, t.offs, st)
    assert len(msgs) >= 800 and {m.header_version for m in msgs} == {1, 2, 3}
    assert any(m.enckey is None for m in msgs) and any(m.enckey for m in msgs)
    descs, fields, blobs, total, mlen, out = S.serialize_oracle(msgs)
    descs2, fields2, blobs2, offs2, total2 = pack_batch(msgs * 2)
    assert np.array_equal(descs2, S.tiled_put_descs(descs, 2, total, len(fields), len(blobs)))
    assert (fields2, blobs2, total2) == (fields * 2, blobs * 2, 2 * total)
    assert offs2 == S.tiled_offsets(np.cumsum(mlen) - mlen, total, 2).tolist()
    assert b"".join(serialize_host(m)[0] for m in msgs) * 2 == out * 2
    # the clean PUTs the descriptors came from verify clean again once serialized
    v, end = S.verify_oracle(out, np.cumsum(mlen) - mlen)
    assert (v == 0).all() and np.array_equal(end, np.cumsum(mlen))


@pytest.mark.parametrize("flag_name", ["blob", "all"])
def test_recv_out_cap(t, flag_name):
    """The packed receive of three copies of the tile's sent body with out_cap inside the second copy: numpy's
    running sum against recv_oracle.expected over the three copies -- statuses, every info field and the end of
    the last placed slice. With room for everything it is the uncapped answer shifted copy by copy."""
    import recv_oracle as RO
    import send_oracle as SO

    flag = {"blob": RO.BLOB, "all": RO.ALL}[flag_name]
    _, sinfo, body = SO.expected(t.region, [int(o) for o in t.offs], None, flag)
    po, ps = sinfo["out_off"].astype(np.uint64), sinfo["send_len"].astype(np.uint64)
    st, info, out, _ = RO.expected(body, po, ps, flag)
    p = len(out)
    sent = np.tile(po != np.uint64(RO.NOWHERE), 3)
    po3 = np.where(sent, np.tile(po, 3) + np.repeat(np.arange(3, dtype=np.uint64) * np.uint64(len(body)), S.T),
                   np.uint64(RO.NOWHERE))
    ps3 = np.tile(ps, 3)
    for cap in (3 * p, p + p // 2, p + 1, p, p - 1, 0):
        est, einfo, eend = S.tiled_recv_capped(st, info, 3, cap)
        st3, info3, out3, _ = RO.expected(body * 3, po3, ps3, flag, out_cap=cap)
        assert np.array_equal(np.array(st3, dtype=np.uint32), est), cap
        for name in RO.INFO.names:
            assert np.array_equal(info3[name], einfo[name]), (cap, name)
        assert eend <= cap and (out3[eend:] == 0xA5).all()
    est, einfo, eend = S.tiled_recv_capped(st, info, 3, p + p // 2)
    assert p < eend <= p + p // 2
    assert (est[:S.T] != RO.NO_ROOM).all() and (est[2 * S.T:] != 0).all()
    refused = est[S.T:2 * S.T] == RO.NO_ROOM
    assert refused.sum() >= 200 and (est[S.T:2 * S.T] == 0).sum() >= 200  # part of the second copy, not all of it
