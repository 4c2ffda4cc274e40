"""Write side of the message path: PUT messages laid out and every CRC
trailer filled by libambrycrc, byte-exact against oracle/message_format.py's restatement of
PutMessageFormatInputStream (PutMessageFormatInputStream.java:76-124, header V1 :133-162) and
the record formats of MessageFormatRecord.java, with zlib CRCs. Shape of
MessageFormatInputStreamTest.java:70-243: serialize, then every record must verify."""
import itertools
import zlib

from c1_message import c1_fixture, c1_message_bytes
from datagen import stream_bytes
from msgfmt import MF
from regions import put_expected, random_messages


def test_host_serializer_matches_layout_oracle(ambry):
    from ambry_amd.messages import layout, serialize_host

    for m in random_messages(300, seed=11):
        got, crcs = serialize_host(m)
        exp = put_expected(m)
        assert got == exp
        # BlobType has two values (DataBlob, MetadataBlob): a type-2 record fails the reader's check
        assert MF.verify_message(got, 0) == (MF.BAD_RECORD if m.blob_type >= 2 else 0, len(got))
        n, offs = layout(m)
        assert n == len(got)
        assert got[offs["key"]:offs["key"] + len(m.key)] == m.key
        assert got[offs["blob"]:offs["blob"] + len(m.blob)] == m.blob
        assert got[offs["usermeta"]:offs["usermeta"] + len(m.usermeta)] == m.usermeta
        assert got[offs["props"]:offs["props"] + len(m.props)] == m.props
        if m.enckey is not None:
            assert got[offs["enckey"]:offs["enckey"] + len(m.enckey)] == m.enckey
        assert crcs[0] == zlib.crc32(got[:{1: 26, 2: 30, 3: 32}[m.header_version]])


def test_every_version_and_option(ambry):
    from ambry_amd.messages import PutMessage, serialize_host

    blob = stream_bytes(3, 0, 777).tobytes()
    for v, enc, comp, life in itertools.product((1, 2, 3), (None, b"", b"k" * 32), (False, True), (0, 7)):
        if v == 1 and enc is not None:
            continue
        m = PutMessage(key=MF.store_key("id1"), props=MF.blob_properties_bytes(777), usermeta=b"meta" * 9, blob=blob,
                       enckey=enc, header_version=v, life_version=life if v == 3 else 0, compressed=comp)
        assert serialize_host(m)[0] == put_expected(m)


def test_c1_message_serialized_by_the_product(ambry):
    """The C1 fixture's exact bytes come out of ambrycrc_serialize_put_host."""
    from ambry_amd.messages import PutMessage, serialize_host

    fx = c1_fixture()
    msg = c1_message_bytes()
    ko, kl = fx["key_offset"], fx["key_bytes"]
    (_, _), (p0, p1), (u0, u1), (b0, b1) = [tuple(r) for r in fx["record_ranges"]]
    m = PutMessage(key=msg[ko:ko + kl], props=msg[p0 + 2:p1], usermeta=msg[u0 + 6:u1], blob=msg[b0 + 13:b1])
    got, crcs = serialize_host(m)
    assert got == msg
    assert [f"0x{c:08x}" for c in (crcs[0], crcs[2], crcs[3], crcs[4])] == fx["record_crcs"]


def test_invalid_descriptors_rejected(ambry):
    import ctypes

    from ambry_amd.messages import PutMessage

    L = ambry.lib()
    for v, enc in ((0, None), (4, None), (1, b"k")):
        m = PutMessage(key=b"\x00\x01a", props=b"", usermeta=b"", blob=b"", enckey=enc, header_version=v)
        assert L.ambrycrc_put_layout(ctypes.byref(m.desc()), None) == 0
        out = ctypes.create_string_buffer(4096)
        assert L.ambrycrc_serialize_put_host(ctypes.byref(m.desc()), None, None, out, 4096, None) == -1
    m = PutMessage(key=b"\x00\x01a", props=b"", usermeta=b"", blob=b"x" * 100)
    out = ctypes.create_string_buffer(64)
    assert L.ambrycrc_serialize_put_host(ctypes.byref(m.desc()), None, None, out, 64, None) == -1  # too small
    big = PutMessage(key=b"", props=b"", usermeta=b"", blob=b"")
    d = big.desc()
    d.usermeta_len = 0x7FFFFFF0  # relative offsets past a Java int
    assert L.ambrycrc_put_layout(ctypes.byref(d), None) == 0
