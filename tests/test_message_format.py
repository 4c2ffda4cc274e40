"""§8f next #1 -- message-level verify: oracle/message_format.py (CPU restatement of the
record layouts) pinned against the reference tests' deterministic headers, and the
host-side message chain of libambrycrc checked against it."""
import struct

import numpy as np
import pytest

from datagen import stream_bytes
from msgfmt import MF
from regions import record_level_cases, verify_region


def test_oracle_headers_match_golden(vectors):
    hv = {h["name"]: h for h in vectors["message_headers"]}
    h1 = MF.header(1, 1000, -1, 10, -1, 20, 30)
    assert h1[:26].hex() == hv["MessageHeader_Format_V1 (MessageFormatRecordTest.java:70)"]["hex"]
    assert struct.unpack(">q", h1[26:])[0] == int(hv["MessageHeader_Format_V1 (MessageFormatRecordTest.java:70)"]["crc"], 16)
    h3 = MF.header(3, 1000, 5, 10, -1, 20, 30, life=2)
    assert h3[:32].hex() == hv["MessageHeader_Format_V3 (MessageFormatRecordTest.java:115)"]["hex"]
    assert struct.unpack(">q", h3[32:])[0] == 0xA4893031


def test_clean_messages_verify_and_chain(ambry):
    region, offs, expect = verify_region(n=120, corrupt_frac=0.0)
    assert all(s == 0 for s, _ in expect)
    ends = [e for _, e in expect]
    assert ends[:-1] == offs[1:] and ends[-1] == len(region)
    from ambry_amd.device import chain_messages_host

    assert chain_messages_host(region, 0) == offs


def test_oracle_detects_every_single_bit_flip():
    """MessageFormatRecordTest.deserializeTest / BlobStoreRecoveryTest.crcErrorRecoveryTest: one corrupted byte
    anywhere in a message is reported (header bit, a record bit, or a layout error) -- except inside the
    store key, which Ambry's format does not cover with any CRC (the key is validated by StoreKeyFactory)."""
    key = MF.store_key("id1")
    msg = MF.put_message(key, MF.blob_properties_bytes(4096), b"u" * 1000, stream_bytes(1, 0, 4096).tobytes(),
                         version=3, enc_key=b"k" * 100)
    assert MF.verify_message(msg, 0) == (0, len(msg))
    rng = np.random.default_rng(0)
    key_span = range(40, 40 + len(key))
    for pos in list(range(0, 200)) + list(rng.integers(200, len(msg), size=200)):
        bad = bytearray(msg)
        bad[pos] ^= 0x10
        st, _ = MF.verify_message(bytes(bad), 0)
        assert (st == 0) == (pos in key_span), pos


def test_chain_stops_at_corrupt_header(ambry):
    region, offs, _ = verify_region(n=40, corrupt_frac=0.0)
    bad = bytearray(region)
    bad[offs[25] + 3] ^= 0xFF
    from ambry_amd.device import chain_messages_host

    assert chain_messages_host(bytes(bad), 0) == offs[:25]


def test_blob_properties_versions_match_reference_test():
    """BlobPropertiesTest.basicTest (ambry-messageformat/src/test/.../BlobPropertiesTest.java:68-202)
    restated over the layouts its serializeBlobPropertiesInVersion writes (:209-275): what
    getBlobPropertiesFromStream must return at each version -- account/container UNKNOWN (-1) at
    V1, `encrypted` only from V3, contentEncoding/filename only from V4, the reserved metadata id
    only at V5, null owner/contentType read back as "" (readIntString) and null nullable strings
    as null -- and the V5 re-serialization (serializeBlobProperties, BlobPropertiesSerDe.java:83-103)."""
    acct, cont, ttl, ctime = 1234, -77, 144, 1_700_000_000_555
    for v in (1, 2, 3, 4, 5):
        for enc in (False, True):
            ce, fn = ("gzip", "filename") if v >= 4 else (None, None)
            raw = MF.blob_properties_bytes(100, service_id="ServiceId", owner_id="OwnerId", content_type="ContentType",
                                           ttl=ttl, private=True, creation_ms=ctime, account=acct, container=cont,
                                           encrypted=enc, content_encoding=ce, filename=fn, reserved="blobid",
                                           serde_version=v)
            f, end = MF.parse_blob_properties(raw, 0, len(raw))
            assert end == len(raw)
            assert (f["size"], f["service"], f["owner"], f["content_type"]) == (100, b"ServiceId", b"OwnerId",
                                                                                b"ContentType")
            assert (f["private"], f["ttl"], f["creation"]) == (True, ttl, ctime)
            assert (f["account"], f["container"]) == ((acct, cont) if v > 1 else (-1, -1))
            assert f["encrypted"] == (v >= 3 and enc)
            assert (f["content_encoding"], f["filename"]) == ((b"gzip", b"filename") if v >= 4 else (None, None))
            assert f["reserved"] == (b"blobid" if v == 5 else None)
            v5 = MF.serialize_blob_properties_v5(f)
            g, _ = MF.parse_blob_properties(v5, 0, len(v5))
            assert {k: x for k, x in g.items() if k != "version"} == {k: x for k, x in f.items() if k != "version"}
            assert v5 == MF.blob_properties_bytes(100, service_id="ServiceId", owner_id="OwnerId",
                                                  content_type="ContentType", ttl=ttl, private=True, creation_ms=ctime,
                                                  account=f["account"], container=f["container"],
                                                  encrypted=f["encrypted"], content_encoding=ce, filename=fn,
                                                  reserved="blobid" if v == 5 else None)
    # null owner / contentType serialize as int 0 and read back as "" (not null): the same bytes
    raw = MF.blob_properties_bytes(100, owner_id=None, content_type=None, serde_version=2)
    f, _ = MF.parse_blob_properties(raw, 0, len(raw))
    assert f["owner"] == b"" and f["content_type"] == b""
    assert MF.serialize_blob_properties_v5(f)[27:35] == bytes(8)


def test_props_not_encodable():
    for s in (b"\x80", b"caf\xc3\xa9", b"\xf0\x9f\x98\x80"):
        raw = MF.blob_properties_bytes(1, filename=s)
        f, _ = MF.parse_blob_properties(raw, 0, len(raw))
        with pytest.raises(MF.NotEncodable):
            MF.serialize_blob_properties_v5(f)


def test_oracle_record_level_checks():
    for i, (msg, want) in enumerate(record_level_cases()):
        assert MF.verify_message(msg, 0) == (want, len(msg)), i
