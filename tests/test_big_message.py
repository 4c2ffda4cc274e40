"""big_message.py's streamed expectations against the full oracles, on blobs small enough to materialize: with a
tile of 4,111 bytes and blobs of 70,001 and 300,007 bytes (17 and 72 whole tiles and a remainder) every entry's
streamed expectation must equal, byte for byte and field for field, what the oracle gives over the message as
bytes. This is what makes the expectations of test_gpu_big_blob.py trustworthy at 2^31 - 1 bytes, where no full
oracle can run."""
import struct
import zlib

import numpy as np
import pytest

import big_message as B
import hard_delete_oracle as HD
import ingest_oracle as IO
import recover_oracle as RC
import recv_oracle as RO
import rekey_oracle as RK
import scale_tiles as S
import send_oracle as SO
from msgfmt import MF

T = 4111
SIZES = (70001, 300007)
PAD = b"\xEE" * 37  # the message lies at an offset that is not a multiple of 64


@pytest.fixture(scope="module", params=[(n, hv) for n in SIZES for hv in (3, 1)], ids=lambda p: "%d-v%d" % p)
def case(request):
    n, hv = request.param
    b = B.big(n, T, hv, props_serde=5 if hv == 3 else 1)
    return b, b.bytes()


def test_the_stream():
    t = B.tile(T)
    whole = t * 80
    for a, b in ((0, 0), (0, 1), (5, 5), (0, T), (1, T), (T - 1, T + 1), (4000, 9000), (T, 3 * T), (7, 70001), (12345, 300007)):
        assert B.stream(T, a, b) == whole[a:b]
        assert B.stream_crc(b"head", T, a, b) == zlib.crc32(b"head" + whole[a:b])
    for n in (0, 1, B.CHUNK - 1, B.CHUNK, B.CHUNK + 1, 3 * B.CHUNK + 5):
        assert B.zeros_crc(b"head", n) == zlib.crc32(b"head" + bytes(n))
    assert B.TILE_LEN % 2 == 1 and len(B.tile()) == B.TILE_LEN
    # the largest size: 2,040 tiles and 6,247 bytes
    assert B.pieces(B.TILE_LEN, 0, 0x7FFFFFFF) == [(0, B.TILE_LEN, 2040), (0, 6247, 1)]


def test_message_and_verify(case):
    b, msg = case
    assert len(msg) == b.length and msg[b.content_rel:b.content_rel + b.size] == (B.tile(T) * 80)[:b.size]
    assert MF.verify_message(PAD + msg, len(PAD)) == B.verify_expected(b, len(PAD)) == (0, len(PAD) + len(msg))
    assert S.verify_oracle(msg, [0])[0][0] == 0


@pytest.mark.parametrize("flag", [SO.BLOB, SO.ALL])
def test_send_and_receive(case, flag):
    b, msg = case
    st, f, span = B.send_expected(b, flag)
    est, einfo, sent = SO.expected(PAD + msg, [len(PAD)], None, flag)
    assert est == [st] and B.span_bytes(span, T) == sent
    assert {k: int(einfo[0][k]) for k in SO.INFO.names} == f
    for lo, hi in ((0, None), (b.size // 3, 2 * b.size // 3), (b.size, b.size), (1, b.size)):
        rst, rf, rspan = B.recv_expected(b, flag, lo, hi)
        est, einfo, out, _ = RO.expected(sent, [0], [len(sent)], flag, ranges=[(lo, RO.TO_END if hi is None else hi)])
        assert est == [rst] and B.span_bytes(rspan, T) == out.tobytes()
        assert {k: int(einfo[0][k]) for k in RO.INFO.names} == rf


def test_hard_delete(case):
    b, msg = case
    st, info, span = B.hard_delete_expected(b)
    est, einfo, after = HD.hard_delete(PAD + msg + PAD, [len(PAD)])
    assert est == [st] and einfo[0] == info and after == PAD + B.span_bytes(span, T) + PAD
    assert MF.verify_message(B.span_bytes(span, T), 0) == (0, b.length)
    assert HD.hard_delete(PAD + msg + PAD, [len(PAD)], einfo)[2] == after  # and with the recovery info


def test_recover(case):
    b, msg = case
    st, f = B.recover_expected(b, len(PAD) + 3)
    assert (st, f) == RC.message_info(PAD + b"abc" + msg, len(PAD) + 3)
    assert RC.accept_header(PAD + msg, len(PAD)) == (0, len(PAD) + b.length)


@pytest.mark.parametrize("version,life", [(3, None), (1, None), (3, 7)])
def test_transform(case, version, life):
    b, msg = case
    st, span = B.transform_expected(b, version, life)
    est, eoff, eln, packed = S.transform_oracle(PAD + msg, [len(PAD)], None if life is None else [life], version)
    assert (int(est[0]), int(eoff[0]), int(eln[0])) == (st, 0, B.span_len(span)) and packed == B.span_bytes(span, T)


def test_rekey(case):
    b, msg = case
    aux = MF.store_key("a-new-key-of-another-length")
    d = np.zeros((), dtype=RK.DESC)
    d["key_len"], d["content_src"], d["props_blob_size"], d["account_id"], d["container_id"] = len(aux), RK.KEEP, -1, 9, 77
    st, span = B.rekey_expected(b, d, aux)
    est, eoff, eln, packed = RK.expected(PAD + msg, [len(PAD)], [d], aux)
    assert (est, eoff, eln) == ([st], [0], [B.span_len(span)]) and packed == B.span_bytes(span, T)
    # a MetadataBlob's content replaced by a stream of another length from aux
    meta = B.big(5, T, b.hv, blob_type=1)
    rule = ("stream", 3, 3 + b.size)
    d["content_src"], d["content_len"], d["props_blob_size"] = len(aux), b.size, 1 << 33
    st, span = B.rekey_expected(meta, d, aux, rule)
    est, eoff, eln, packed = RK.expected(PAD + meta.bytes(), [len(PAD)], [d], aux + B.stream(T, *rule[1:]))
    assert (est, eln) == ([st], [B.span_len(span)]) and st == 0 and packed == B.span_bytes(span, T)
    assert B.rekey_expected(b, d, aux, rule)[0] == RK.BAD_DESC  # only a MetadataBlob's content is replaced


def test_serialize(ambry, case):
    from ambry_amd.messages import serialize_host
    from regions import put_expected

    b, msg = case
    n, span = B.serialize_expected(b)
    m = B.put_message_of(b, msg[b.content_rel:b.content_rel + b.size])
    assert n == len(msg) and B.span_bytes(span, T) == put_expected(m) == msg
    assert serialize_host(m)[0] == msg


@pytest.mark.parametrize("version", [3, 4, 5])
def test_ingest(case, version):
    b, _ = case
    frame, key_len, crc = B.frame_of(b, version)
    wire = PAD + B.span_bytes(frame, T)
    refs = np.zeros(1, dtype=IO.REF)
    refs[0] = (len(PAD), key_len, 0)
    st, span, wcrc, f = B.ingest_expected(b, frame, header_version=b.hv)
    est, packed, eoff, eln, ecrc, einfo, total = IO.expected(wire, refs, header_version=b.hv)
    assert int(est[0]) == st and packed == B.span_bytes(span, T) and int(ecrc[0]) == wcrc == crc
    assert {k: int(einfo[0][k]) for k in IO.INFO.names} == f and total == int(eln[0]) == B.span_len(span)
    assert struct.unpack_from(">q", wire, len(PAD))[0] == len(wire) - len(PAD)


@pytest.mark.parametrize("um_len", [0, 5, 70001])
def test_frame_with_streamed_user_metadata(um_len):
    """The frame test_gpu_big_blob.py sends to reach the ingest's Java-int refusal, with a user metadata short
    enough for the oracle: the span is IO.frame's own bytes and the oracle accepts it, wire CRC included."""
    key, props, blob = MF.store_key("frame"), MF.blob_properties_bytes(9), b"blob bytes"
    span, crc = B.frame_with_usermeta(um_len, T, key, props, blob, enc_key=b"e" * 12)
    wire = B.span_bytes(span, T)
    assert wire == IO.frame(5, key, props, B.stream(T, 0, um_len), blob, enc_key=b"e" * 12, client_id=b"client")
    st, msg, wcrc, _ = IO.ingest_request(wire, 0, len(key), 3)
    assert (st, wcrc) == (0, crc) and msg == MF.put_message(key, props, B.stream(T, 0, um_len), blob, enc_key=b"e" * 12)


@pytest.mark.parametrize("n,hv,bv", [(300007, 3, 1), (70001, 2, 2), (70001, 1, 1)])
def test_stored_at_an_older_blob_record_version(n, hv, bv):
    """The message stored with a Blob_Format_V1 / V2 record (a 10- / 12-byte head), which the transform and the
    re-key write again as V3: the entries test_gpu_big_blob.py runs on such a message."""
    b = B.big(n, T, hv, bv=bv)
    msg = b.bytes()
    assert MF._be16(msg, b.rel[4]) == bv and b.content_rel == b.rel[4] + {1: 10, 2: 12}[bv]
    assert MF.verify_message(PAD + msg, len(PAD)) == B.verify_expected(b, len(PAD)) == (0, len(PAD) + len(msg))
    for version in (3, 1):
        st, span = B.transform_expected(b, version)
        est, eoff, eln, packed = S.transform_oracle(PAD + msg, [len(PAD)], None, version)
        assert (int(est[0]), int(eln[0])) == (st, B.span_len(span)) and packed == B.span_bytes(span, T)
        assert MF._be16(packed, MF.parse_header(packed, 0)[2][4]) == 3
    aux = MF.store_key("a-new-key-of-another-length")
    d = np.zeros((), dtype=RK.DESC)
    d["key_len"], d["content_src"], d["props_blob_size"], d["account_id"], d["container_id"] = len(aux), RK.KEEP, -1, 9, 77
    st, span = B.rekey_expected(b, d, aux)
    est, eoff, eln, packed = RK.expected(PAD + msg, [len(PAD)], [d], aux)
    assert (est, eln) == ([st], [B.span_len(span)]) and st == 0 and packed == B.span_bytes(span, T)
