// put_request.h -- a PutRequest frame as the server receives it, parsed and planned into a stored PUT
// message: PutRequest.readFrom (ambry-protocol/.../PutRequest.java:191-204, V3 :440-464, V4 :467-492,
// V5 :495-521) followed by AmbryRequests.getMessageFormatWriteSet (AmbryRequests.java:1957-1970)
// through PutMessageFormatInputStream (:60-124). Shared by the device batch (ingest_kernels.hip,
// ambrycrc_ingest.cpp) and the per-request CPU entry (ambrycrc_ingest_put_request_cpu).
//
// The frame (RequestOrResponse.writeHeader, RequestOrResponse.java:80-88; PutRequest.prepareBuffer,
// PutRequest.java:238-283), every integer big-endian:
//   long size | short type | short version | int correlationId | int clientIdLen, clientId |
//   [ blobId | BlobPropertiesSerDe bytes | int umSize, userMetadata | short blobType |
//     (V4, V5) short encKeyLen, encKey | (V5) byte isCompressed | long blobSize | blob ] | long crc
// The CRC covers the bracketed bytes. In wire order they are five segments of any length (blob id,
// properties, user metadata, encryption key, blob) with three short fixed pieces between them:
//   piece 0  umSize                                 4 B, after the properties
//   piece 1  blobType, (V4, V5) encKeyLen           2 or 4 B, after the user metadata
//   piece 2  (V5) isCompressed, blobSize            8 or 9 B, after the encryption key
// Every function reads only inside [wire, wire + wire_len), and past the frame's fixed part only
// inside the frame.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ambrycrc.h"
#include "put_layout.h"
#include "record_fields.h"

namespace ambrycrc {

constexpr uint32_t kReqFixed = 20;   // size, type, version, correlationId, clientIdLen
constexpr int32_t kReqTypePut = 0;   // RequestOrResponseType.PutRequest.ordinal() (RequestOrResponseType.java:21)
// The smallest frame readFrom accepts: a V3 request with empty client id, blob id, strings, metadata and
// blob -- the fixed part, SerDe V1 with three empty strings (27 + 12), umSize, blobType, blobSize, CRC.
constexpr uint64_t kReqMinFrame = kReqFixed + kSerdeFixed + 12 + 4 + 2 + 8 + 8;
constexpr uint32_t kIngestSegs = 5;   // CRC jobs a request: blob id, properties, user metadata, encryption key, blob
constexpr uint32_t kIngestSlots = 4;  // copy jobs a request: blob id, encryption key, user metadata, blob content

// What the parse found (56 B a request in the workspace). req_version 0: refused, nothing else is read.
struct IngestPlan {
  uint64_t body;       // wire offset of the blob id: where the CRC'd span starts
  uint64_t blob_len;
  uint32_t key_len, props_len, um_len;
  int32_t enc_len;     // -1: a V3 request, which has no such field
  uint32_t fcrc[3];    // zlib CRCs of the three fixed pieces
  uint32_t enc_pos;    // PropsFields of the wire's SerDe bytes
  uint8_t req_version; // 3..5
  uint8_t blob_type, compressed;
  uint8_t serde_version, priv_raw, enc_raw, ascii;
  uint8_t pad;
};
static_assert(sizeof(IngestPlan) == 56, "IngestPlan");

__host__ __device__ inline uint32_t ingest_piece1_len(const IngestPlan& p) { return p.req_version >= 4 ? 4u : 2u; }
__host__ __device__ inline uint32_t ingest_piece2_len(const IngestPlan& p) { return p.req_version >= 5 ? 9u : 8u; }
// Wire offsets of the segments and of the stored CRC.
__host__ __device__ inline uint64_t ingest_props_off(const IngestPlan& p) { return p.body + p.key_len; }
__host__ __device__ inline uint64_t ingest_um_off(const IngestPlan& p) { return ingest_props_off(p) + p.props_len + 4; }
__host__ __device__ inline uint64_t ingest_enc_off(const IngestPlan& p) {
  return ingest_um_off(p) + p.um_len + ingest_piece1_len(p);
}
__host__ __device__ inline uint64_t ingest_blob_off(const IngestPlan& p) {
  return ingest_enc_off(p) + (p.enc_len > 0 ? (uint32_t)p.enc_len : 0u) + ingest_piece2_len(p);
}
__host__ __device__ inline uint64_t ingest_crc_off(const IngestPlan& p) { return ingest_blob_off(p) + p.blob_len; }

// The reference and the frame up to the stored CRC: 0 and *p, or the first refusal of
//   BAD_DESC     the reference itself: off or the fixed part outside the wire buffer, size below
//                kReqMinFrame (negative included), the frame past the buffer, reserved != 0
//   NOT_PUT      type is not PutRequest's ordinal
//   BAD_VERSION  version not 3..5 (:202)
//   BAD_RECORD   a read of readFrom throws or would pass the frame's end: clientIdLen (readIntString),
//                the blob id, the properties (props_walk_b), umSize, blobType (BlobType.values()[n]),
//                encKeyLen (readShortBuffer), blobSize (negative, above Integer.MAX_VALUE), the CRC long
// Bytes after the CRC inside the frame are not looked at, as in the reference.
// crc(bytes, n): the zlib CRC of n <= 9 bytes.
template <class Crc>
__host__ __device__ inline uint32_t ingest_parse(const uint8_t* wire, uint64_t wire_len,
                                                 const ambrycrc_put_request_ref& r, Crc crc, IngestPlan* p) {
  __builtin_memset(p, 0, sizeof *p);
  if (r.reserved != 0 || r.off > wire_len || wire_len - r.off < kReqFixed) return AMBRYCRC_MSG_BAD_DESC;
  const uint8_t* f = wire + r.off;
  const int64_t size = (int64_t)ld_be64(f);
  if (size < (int64_t)kReqMinFrame || (uint64_t)size > wire_len - r.off) return AMBRYCRC_MSG_BAD_DESC;
  if ((int32_t)(int16_t)ld_be16(f + 8) != kReqTypePut) return AMBRYCRC_MSG_NOT_PUT;
  const int32_t v = (int16_t)ld_be16(f + 10);
  if (v < 3 || v > 5) return AMBRYCRC_MSG_BAD_VERSION;
  const uint64_t end = r.off + (uint64_t)size;
  uint64_t pos = r.off + kReqFixed;
  const int32_t client = (int32_t)ld_be32(f + 16);
  if (client < 0 || (uint64_t)client > end - pos) return AMBRYCRC_MSG_BAD_RECORD;
  pos += (uint64_t)client;
  if (r.key_len > end - pos) return AMBRYCRC_MSG_BAD_RECORD;
  const uint64_t body = pos;
  pos += r.key_len;
  PropsFields pf;
  uint64_t pend = 0;
  if (props_walk_b<true>(MemBytes{wire + pos}, end - pos, &pf, &pend) != 0) return AMBRYCRC_MSG_BAD_RECORD;
  const uint64_t props_len = pend;
  pos += props_len;
  uint8_t b[12];
  __builtin_memset(b, 0, sizeof b);
  if (end - pos < 4) return AMBRYCRC_MSG_BAD_RECORD;
  __builtin_memcpy(b, wire + pos, 4);
  const int32_t um = (int32_t)ld_be32(wire + pos);
  pos += 4;
  if (um < 0 || (uint64_t)um > end - pos) return AMBRYCRC_MSG_BAD_RECORD;
  const uint32_t c0 = crc(b, 4u);
  pos += (uint64_t)um;
  if (end - pos < 2) return AMBRYCRC_MSG_BAD_RECORD;
  const int32_t type = (int16_t)ld_be16(wire + pos);
  if (type < 0 || type > 1) return AMBRYCRC_MSG_BAD_RECORD;
  __builtin_memcpy(b, wire + pos, 2);
  pos += 2;
  int32_t enc = -1;
  if (v >= 4) {
    if (end - pos < 2) return AMBRYCRC_MSG_BAD_RECORD;
    enc = (int16_t)ld_be16(wire + pos);
    __builtin_memcpy(b + 2, wire + pos, 2);
    pos += 2;
    if (enc < 0 || (uint64_t)enc > end - pos) return AMBRYCRC_MSG_BAD_RECORD;
  }
  const uint32_t c1 = crc(b, v >= 4 ? 4u : 2u);
  pos += enc > 0 ? (uint64_t)enc : 0;
  uint32_t comp = 0;
  uint32_t n2 = 0;
  if (v >= 5) {
    if (end - pos < 1) return AMBRYCRC_MSG_BAD_RECORD;
    b[0] = wire[pos];
    comp = b[0] == 1 ? 1u : 0u;
    pos += 1;
    n2 = 1;
  }
  if (end - pos < 8) return AMBRYCRC_MSG_BAD_RECORD;
  const int64_t blob = (int64_t)ld_be64(wire + pos);
  __builtin_memcpy(b + n2, wire + pos, 8);
  pos += 8;
  if (blob < 0 || blob > 0x7FFFFFFFll || (uint64_t)blob > end - pos) return AMBRYCRC_MSG_BAD_RECORD;
  pos += (uint64_t)blob;
  if (end - pos < 8) return AMBRYCRC_MSG_BAD_RECORD;
  p->fcrc[0] = c0;
  p->fcrc[1] = c1;
  p->fcrc[2] = crc(b, n2 + 8);
  p->body = body;
  p->blob_len = (uint64_t)blob;
  p->key_len = r.key_len;
  p->props_len = (uint32_t)props_len;
  p->um_len = (uint32_t)um;
  p->enc_len = enc;
  p->enc_pos = pf.enc_pos;
  p->req_version = (uint8_t)v;
  p->blob_type = (uint8_t)type;
  p->compressed = (uint8_t)comp;
  p->serde_version = (uint8_t)pf.version;
  p->priv_raw = pf.priv_raw;
  p->enc_raw = pf.enc_raw;
  p->ascii = pf.ascii ? 1 : 0;
  return 0;
}

// The request's CRC jobs over the wire buffer, in job order (blob id, properties, user metadata,
// encryption key, blob). An empty segment is an empty job: it reads nothing and its CRC is 0.
__host__ __device__ inline void ingest_segments(const IngestPlan& p, uint64_t (&off)[kIngestSegs],
                                                uint64_t (&len)[kIngestSegs]) {
  off[0] = p.body;
  len[0] = p.key_len;
  off[1] = ingest_props_off(p);
  len[1] = p.props_len;
  off[2] = ingest_um_off(p);
  len[2] = p.um_len;
  off[3] = ingest_enc_off(p);
  len[3] = p.enc_len > 0 ? (uint32_t)p.enc_len : 0u;
  off[4] = ingest_blob_off(p);
  len[4] = p.blob_len;
}

// The wire CRC from the segments' zlib CRCs (job order) and the fixed pieces', by
// crc(A || B) = crc(A) x^(8|B|) + crc(B) in wire order; an empty piece is the identity.
// mul(v, n) = v x^(8n) mod P.
template <class Mul>
__host__ __device__ inline uint32_t ingest_wire_crc(const IngestPlan& p, const uint32_t (&seg)[kIngestSegs], Mul mul) {
  uint32_t c = p.key_len ? seg[0] : 0u;
  c = mul(c, (uint64_t)p.props_len) ^ seg[1];
  c = mul(c, 4ull) ^ p.fcrc[0];
  if (p.um_len) c = mul(c, (uint64_t)p.um_len) ^ seg[2];
  c = mul(c, (uint64_t)ingest_piece1_len(p)) ^ p.fcrc[1];
  if (p.enc_len > 0) c = mul(c, (uint64_t)p.enc_len) ^ seg[3];
  c = mul(c, (uint64_t)ingest_piece2_len(p)) ^ p.fcrc[2];
  if (p.blob_len) c = mul(c, p.blob_len) ^ seg[4];
  return c;
}

__host__ __device__ inline PropsFix ingest_props_fix(const IngestPlan& p) {
  PropsFields f;
  f.version = p.serde_version;
  f.enc_pos = p.enc_pos;
  f.priv_raw = p.priv_raw;
  f.enc_raw = p.enc_raw;
  f.ascii = p.ascii != 0;
  return props_fix_of(f, p.props_len);
}

// After the parse, with the computed wire CRC: 0 and the output's put descriptor (every source an
// offset in the wire buffer, out_off left 0), or the first refusal of
//   WIRE_CRC       computed CRC != the stored long, high word included (:457-460)
//   NOT_ENCODABLE  a non-ASCII string byte: the properties are written again at VERSION_5 into an
//                  exactly-sized buffer (record_fields.h)
//   BAD_INFO       creation time below -1 (MessageInfo.java:172, as recover)
//   BAD_RECORD     put_layout refuses the message (a relative offset past a Java int, as rekey_plan)
__host__ __device__ inline uint32_t ingest_verdict(const uint8_t* wire, const IngestPlan& p, uint32_t wire_crc,
                                                   int header_version, ambrycrc_put_desc* d) {
  __builtin_memset(d, 0, sizeof *d);
  if (ld_be64(wire + ingest_crc_off(p)) != (uint64_t)wire_crc) return AMBRYCRC_MSG_WIRE_CRC;
  if (!p.ascii) return AMBRYCRC_MSG_NOT_ENCODABLE;
  const uint64_t props = ingest_props_off(p);
  if ((int64_t)ld_be64(wire + props + 11) < -1) return AMBRYCRC_MSG_BAD_INFO;
  const bool keep_enc = p.enc_len > 0 && header_version >= 2;  // "blobEncryptionKey.remaining() == 0 ? null"
  d->key_src = p.body;
  d->key_len = p.key_len;
  d->enckey_src = keep_enc ? ingest_enc_off(p) : 0;
  d->enckey_len = keep_enc ? p.enc_len : -1;
  d->props_src = props;
  d->props_len = props_v5_len(ingest_props_fix(p));
  d->usermeta_src = ingest_um_off(p);
  d->usermeta_len = p.um_len;
  d->blob_src = ingest_blob_off(p);
  d->blob_len = p.blob_len;
  d->life_version = 0;
  d->blob_type = (int16_t)p.blob_type;
  d->compressed = p.compressed;
  d->header_version = (uint8_t)header_version;
  PutLayout L;
  if (!put_layout(*d, L)) {
    d->header_version = 0;
    return AMBRYCRC_MSG_BAD_RECORD;
  }
  return 0;
}

// The MessageInfo of the message written at out_off, from the wire bytes: what message_info_fields
// reads back from the stored message (record_fields.h). The creation time is >= -1 (ingest_verdict).
__host__ __device__ inline void ingest_info(const uint8_t* wire, const IngestPlan& p, const ambrycrc_put_desc& d,
                                            const PutLayout& L, uint64_t out_off, ambrycrc_message_info* o) {
  __builtin_memset(o, 0, sizeof *o);
  const uint8_t* s = wire + d.props_src;
  const int64_t ttl = (int64_t)ld_be64(s + 2), created = (int64_t)ld_be64(s + 11);
  int32_t account = -1, container = -1;  // SerDe V1: the appendix's Account / Container.UNKNOWN ids
  if (p.serde_version >= 2) {
    const uint32_t at = p.serde_version == 2 ? p.props_len - 4 : p.enc_pos - 4;
    account = (int16_t)ld_be16(s + at);
    container = (int16_t)ld_be16(s + at + 2);
  }
  o->msg_off = out_off;
  o->size = L.length;
  o->expires_at_ms = add_seconds_to_epoch(created, ttl);
  o->operation_time_ms = created;
  o->key_rel = L.hsize;
  o->key_len = d.key_len;
  o->account_id = (int16_t)account;
  o->container_id = (int16_t)container;
  o->life_version = 0;
  o->flags = 0;
  o->header_version = d.header_version;
}

}  // namespace ambrycrc
