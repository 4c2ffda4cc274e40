// rekey.h -- BlobIdTransformer's per-message decisions and its BlobProperties re-encoding
// (ambry-replication/.../BlobIdTransformer.java:72-87,159-281), shared by the device batch
// (rekey_kernels.hip, ambrycrc_rekey.cpp) and the per-message CPU entry (ambrycrc_msg_cpu.cpp).
//
// A verified PUT is re-serialized through PutMessageFormatInputStream (:259-262) with
//   the converted store key                                 (newKey, :162, :260)
//   the stored encryption key and user metadata             (:170-175)
//   BlobProperties re-encoded at VERSION_5 with the new key's accountId / containerId (:249-254) and,
//   for a metadata blob, the composite's total size (:242)
//   the stored blob content, or for a MetadataBlob the caller's rewritten content (:183-247)
// Everything here reads only inside the spans the verify established.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ambrycrc.h"
#include "msg_header.h"
#include "put_emit.h"
#include "put_layout.h"

namespace ambrycrc {

constexpr uint64_t kRekeyKeep = ~0ull;       // ambrycrc_rekey_desc::content_src: keep the stored content
constexpr uint32_t kSerdeBlobSize = 19;      // offset of blobSize in the SerDe bytes (version, ttl, private, creationTime)

// How a stored BlobPropertiesSerDe payload becomes the re-keyed VERSION_5 one -- the transform's PropsFix
// (record_fields.h) in its first 11 bytes, version 0 for a payload already canonical -- and what the write
// step needs of the stored blob record (16 B a message in the workspace).
struct RekeyFix {
  uint32_t stored_len;  // stored payload bytes
  uint32_t enc_pos;     // offset of the `encrypted` byte (stored version >= 3), else 0
  uint8_t version;      // stored SerDe version 1..5, 0 = already canonical
  uint8_t priv, enc;    // canonical bytes (`== 1`)
  uint8_t blob_head;    // stored blob record head: 10, 12 or 13 B (Blob_Format_V1 / V2 / V3)
  uint32_t acct_pos;    // offset of the accountId short in the VERSION_5 bytes (containerId follows)
  __host__ __device__ PropsFix props() const { return PropsFix{stored_len, enc_pos, version, priv, enc, {0, 0, 0, 0, 0}}; }
};
static_assert(sizeof(RekeyFix) == 16, "RekeyFix");

// The descriptor's own spans: the new key and the replacement content inside [0, aux_len), the
// content no longer than a Java array. Checked before the message is looked at.
__host__ __device__ inline bool rekey_desc_ok(const ambrycrc_rekey_desc& r, uint64_t aux_len) {
  if (r.key_src > aux_len || r.key_len > aux_len - r.key_src) return false;
  if (r.content_src == kRekeyKeep) return true;
  return r.content_len <= 0x7FFFFFFFull && r.content_src <= aux_len && r.content_len <= aux_len - r.content_src;
}

// Byte j of the re-keyed VERSION_5 payload, from the stored payload's byte j (`stored`; anything when j >=
// stored_len): the transform's re-encoding (record_fields.h props_v5_byte), then blobSize when given and the
// new accountId / containerId (over a stored V1's appended -1 ids too).
__host__ __device__ inline uint8_t rekey_props_byte(const RekeyFix& x, const ambrycrc_rekey_desc& r, uint32_t j,
                                                    uint8_t stored) {
  uint8_t b = props_v5_byte(x.props(), j, stored);
  if (r.props_blob_size >= 0 && j >= kSerdeBlobSize && j < kSerdeBlobSize + 8)
    b = (uint8_t)((uint64_t)r.props_blob_size >> (8 * (kSerdeBlobSize + 7 - j)));
  if (j >= x.acct_pos && j < x.acct_pos + 4) {
    const uint32_t ids = (uint32_t)(uint16_t)r.account_id << 16 | (uint16_t)r.container_id;
    b = (uint8_t)(ids >> (8 * (x.acct_pos + 3 - j)));
  }
  return b;
}

// BlobIdTransformer.newMessage for the message at region + off, which the verify passed clean (its
// header and every record lie inside the region, the record checks hold) and whose descriptor
// rekey_desc_ok accepted: 0 and the output's put descriptor (key_src and, with replacement content,
// blob_src are offsets in aux, the other sources offsets in the region; out_off left 0) and *x, or
// the refusal. have_life: write life_version as given, else the stored header's (0 for V1 / V2).
__host__ __device__ inline uint32_t rekey_plan(const uint8_t* region, uint64_t off, const ambrycrc_rekey_desc& r,
                                               bool have_life, int life_version, int header_version,
                                               ambrycrc_put_desc* d, RekeyFix* x) {
  const uint8_t* p = region + off;
  const MsgHeader H = msg_header_of(p);
  const int32_t bp = H.rel[1], upd = H.rel[2], um = H.rel[3], blob = H.rel[4];
  if (upd != -1 || bp == -1 || um == -1 || blob == -1) return AMBRYCRC_MSG_NOT_PUT;  // "Only 'put' records are valid"
  // the deserializers' field reads against the header's spans (msg_header.h put_fields)
  const PutFields f = put_fields(p, H);
  const int64_t props_len = f.props_len;
  const uint32_t head = f.head, type = f.type;
  PropsFields pf;
  const bool ok = f.ok && props_parse<true>(p + bp + 2, (uint64_t)props_len, &pf) == 0;
  if (!ok) return AMBRYCRC_MSG_BAD_RECORD;
  if (!pf.ascii) return AMBRYCRC_MSG_NOT_ENCODABLE;
  const bool repl = r.content_src != kRekeyKeep;
  if (repl && type == 0) return AMBRYCRC_MSG_BAD_DESC;        // content is rewritten for a MetadataBlob only (:183)
  if (!repl && type == 1) return AMBRYCRC_MSG_NEEDS_CONTENT;  // ... and always for one (:185-247)
  const PropsFix fx = props_fix_of(pf, (uint32_t)props_len);
  // accountId: V1 stores none (the appendix starts with it), V2 ends with the two shorts, from V3 on
  // they sit right before the `encrypted` byte
  const uint32_t acct = pf.version == 1 ? (uint32_t)props_len : pf.version == 2 ? (uint32_t)props_len - 4 : pf.enc_pos - 4;
  *x = RekeyFix{fx.stored_len, fx.enc_pos, fx.version, fx.priv, fx.enc, (uint8_t)head, acct};
  *d = put_desc_of_stored(off, H, f, header_version, have_life ? life_version : H.life, props_v5_len(fx));
  d->key_src = r.key_src;
  d->key_len = r.key_len;
  if (repl) {
    d->blob_src = r.content_src;
    d->blob_len = r.content_len;
  }
  PutLayout L;
  if (!put_layout(*d, L)) {  // a relative offset past a Java int
    d->header_version = 0;
    return AMBRYCRC_MSG_BAD_RECORD;
  }
  return 0;
}

}  // namespace ambrycrc
