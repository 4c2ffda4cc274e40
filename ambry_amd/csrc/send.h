// send.h -- MessageFormatSend.fetchDataFromReadSet's per-message decisions
// (ambry-messageformat/.../MessageFormatSend.java:112-242), shared by the device batch
// (send_kernels.hip, ambrycrc_send.cpp) and the per-message CPU entry (ambrycrc_msg_cpu.cpp): the
// header's fields and constraints, the record checks, and send_plan -- what is refused, what is sent,
// and what each record slot's CRC job does (copied to where, hashed only, not read). Host and device;
// everything reads only inside the spans a verified header establishes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ambrycrc.h"
#include "record_fields.h"
#include "rekey.h"  // ld_be64

namespace ambrycrc {

static_assert(sizeof(ambrycrc_send_info) == 32, "ambrycrc_send_info: 32 bytes, no padding");

constexpr uint64_t kSendNowhere = ~0ull;   // ambrycrc_send_info::out_off of a message not sent
// SendPlan::dst values besides a destination: hash the record without copying it (SweepArgs kCopySkip),
// or do not read it at all.
constexpr uint64_t kSendHash = ~0ull;
constexpr uint64_t kSendNone = ~0ull - 1;
constexpr int kSendSlots = 5;  // the verify's record slots: encryption key, properties, update, user metadata, blob

// A header whose CRC verified and whose constraints hold.
struct SendHeader {
  uint32_t hs;               // header bytes
  int32_t rel[kSendSlots];   // record offsets relative to the message, -1 absent
  uint64_t rend[kSendSlots]; // where each present record ends (its stored CRC's last byte + 1)
  uint64_t first, end;       // first record, message end
};

// The header size of the message at p (rem bytes of region from p on), or the status that ends it.
__host__ __device__ inline uint32_t send_header_size(const uint8_t* p, uint64_t rem, uint32_t* hs) {
  if (rem < 2) return AMBRYCRC_MSG_BAD_LAYOUT;
  const int v = (int16_t)ld_be16(p);
  const uint32_t h = v == 1 ? 34u : v == 2 ? 38u : v == 3 ? 40u : 0u;
  if (h == 0) return AMBRYCRC_MSG_BAD_VERSION;
  if (rem < h) return AMBRYCRC_MSG_BAD_LAYOUT;
  *hs = h;
  return 0;
}

// checkHeaderConstraints (MessageFormatRecord.java:985-1030) and the record spans of a header of hs bytes
// whose CRC verified -- the checks of msg_parse.h parse_message, in its order. 0 or AMBRYCRC_MSG_BAD_LAYOUT.
__host__ __device__ inline uint32_t send_header_fields(const uint8_t* p, uint64_t rem, uint32_t hs, SendHeader* o) {
  int64_t total;
  int32_t* rel = o->rel;
  if (hs == 40) {
    if ((int16_t)ld_be16(p + 2) < 0) return AMBRYCRC_MSG_BAD_LAYOUT;  // lifeVersion >= 0
    total = (int64_t)ld_be64(p + 4);
#pragma unroll
    for (int k = 0; k < 5; ++k) rel[k] = (int32_t)ld_be32(p + 12 + 4 * k);
  } else if (hs == 38) {
    total = (int64_t)ld_be64(p + 2);
#pragma unroll
    for (int k = 0; k < 5; ++k) rel[k] = (int32_t)ld_be32(p + 10 + 4 * k);
  } else {  // V1: no encryption-key record
    total = (int64_t)ld_be64(p + 2);
    rel[0] = -1;
#pragma unroll
    for (int k = 1; k < 5; ++k) rel[k] = (int32_t)ld_be32(p + 6 + 4 * k);
  }
  const bool is_put = rel[1] != -1 && rel[2] == -1 && rel[3] != -1 && rel[4] != -1;
  const bool is_upd = rel[2] != -1 && rel[0] == -1 && rel[1] == -1 && rel[3] == -1 && rel[4] == -1;
  if (total <= 0 || !(is_put || is_upd)) return AMBRYCRC_MSG_BAD_LAYOUT;
  int64_t prev = -1, first = -1;
  bool ordered = true;
#pragma unroll
  for (int k = 0; k < kSendSlots; ++k) {
    if (rel[k] == -1) continue;
    if (rel[k] <= prev || rel[k] < (int32_t)hs) ordered = false;
    if (first < 0) first = rel[k];
    prev = rel[k];
  }
  if (!ordered) return AMBRYCRC_MSG_BAD_LAYOUT;
  if ((uint64_t)total > rem || (uint64_t)first > rem - (uint64_t)total) return AMBRYCRC_MSG_BAD_LAYOUT;
  const uint64_t end = (uint64_t)first + (uint64_t)total;
  // a record ends where the next present one starts, the last at the message end; each holds its CRC at
  // least (backwards, constant indices: the arrays stay in registers on the device)
  uint64_t next = end;
  bool ok = true;
#pragma unroll
  for (int k = kSendSlots - 1; k >= 0; --k) {
    o->rend[k] = next;
    if (rel[k] != -1) {
      ok = ok && next >= (uint64_t)rel[k] + 8;
      next = (uint64_t)rel[k];
    }
  }
  if (!ok) return AMBRYCRC_MSG_BAD_LAYOUT;
  o->hs = hs;
  o->first = (uint64_t)first;
  o->end = end;
  return 0;
}

// What record k's deserializer reads before its CRC, for a record of `span` bytes at q (msg_parse.h
// record_check): AMBRYCRC_MSG_BAD_VERSION / _BAD_RECORD bits, 0 when the fields agree with the span.
__host__ __device__ inline uint32_t send_record_check(int k, const uint8_t* q, uint64_t span) {
  if (span < 10) return AMBRYCRC_MSG_BAD_RECORD;
  const uint32_t v = ld_be16(q);
  switch (k) {
    case 0:
    case 3: {
      if (v != 1) return AMBRYCRC_MSG_BAD_VERSION;
      if (span < 14) return AMBRYCRC_MSG_BAD_RECORD;
      const int32_t n = (int32_t)ld_be32(q + 2);
      return n >= 0 && (uint64_t)n + 14 == span ? 0u : AMBRYCRC_MSG_BAD_RECORD;
    }
    case 1:
      return props_record_check(q, span);
    case 2:
      return update_record_check(q, span);
    default: {
      if (v < 1 || v > 3) return AMBRYCRC_MSG_BAD_VERSION;
      const uint32_t head = v == 1 ? 10u : v == 2 ? 12u : 13u;
      if (span < head + 8) return AMBRYCRC_MSG_BAD_RECORD;
      const uint32_t type = v == 1 ? 0u : ld_be16(q + 2);
      const uint64_t size = ld_be64(q + (v == 1 ? 2 : v == 2 ? 4 : 5));
      return type < 2 && size <= 0x7FFFFFFFull && size + head + 8 == span ? 0u : AMBRYCRC_MSG_BAD_RECORD;
    }
  }
}

__host__ __device__ inline bool send_flag_ok(int flag) {
  return flag >= AMBRYCRC_SEND_BLOB_PROPERTIES && flag <= AMBRYCRC_SEND_BLOB_INFO;
}
// Whether the flag deserializes the encryption-key record (MessageMetadata, :150-158, :188-203).
__host__ __device__ inline bool send_reads_enckey(int flag) {
  return flag == AMBRYCRC_SEND_BLOB || flag == AMBRYCRC_SEND_BLOB_USER_METADATA || flag == AMBRYCRC_SEND_BLOB_INFO;
}
// The bits of the message verify's result that belong in `check`: everything under ALL and BLOB
// (deserializeBlobAll, :131-139), the CRC bits of the sent records under the metadata flags.
__host__ __device__ inline uint32_t send_check_mask(int flag) {
  switch (flag) {
    case AMBRYCRC_SEND_BLOB_PROPERTIES: return AMBRYCRC_MSG_PROPS_CRC;
    case AMBRYCRC_SEND_BLOB_USER_METADATA: return AMBRYCRC_MSG_USERMETA_CRC;
    case AMBRYCRC_SEND_BLOB_INFO: return AMBRYCRC_MSG_PROPS_CRC | AMBRYCRC_MSG_USERMETA_CRC;
    default: return ~0u;
  }
}

struct SendPlan {
  uint32_t status;     // what the reference throws for (AMBRYCRC_MSG_NO_ROOM comes with the placement)
  uint32_t pre;        // check bits known without the CRC pass
  uint64_t send_len;
  uint32_t rel_off, enckey_rel, enckey_len;
  bool whole;          // sent as [0, send_len) by a plain copy: no job copies, the jobs only hash
  uint64_t dst[kSendSlots];  // per record slot: offset in the sent span, kSendHash or kSendNone
};

// One message under `flag`. in_region: its offset lies inside the region, with rem bytes from it on;
// has_size / size: readSet.sizeInBytes, else the header's own length; hdr_status: the header's verdict
// (send_header_size, the CRC, send_header_fields) with H valid when it is 0; enc_crc_bad: the
// encryption-key record's CRC differs from its stored long (consulted only where the record is read).
__host__ __device__ inline void send_plan(const uint8_t* p, bool in_region, uint64_t rem, bool has_size,
                                          uint64_t size, int flag, uint32_t hdr_status, const SendHeader& H,
                                          bool enc_crc_bad, SendPlan* s) {
  s->status = s->pre = 0;
  s->send_len = 0;
  s->rel_off = s->enckey_rel = s->enckey_len = 0;
  s->whole = false;
#pragma unroll
  for (int k = 0; k < kSendSlots; ++k) s->dst[k] = kSendNone;
  if (!in_region || (has_size && (size == 0 || size > rem))) {
    s->status = AMBRYCRC_MSG_BAD_LAYOUT;
    return;
  }
  const bool all = flag == AMBRYCRC_SEND_ALL;
  if (hdr_status) {
    if (all && has_size) {  // the reference never parses the header for this send (:142)
      s->whole = true;
      s->send_len = size;
      s->pre = hdr_status;  // deserializeBlobAll's failure, counted
      return;
    }
    s->status = hdr_status;
    return;
  }
  const bool upd = H.rel[2] != -1;
  if (all) {
    const uint64_t sz = has_size ? size : H.end;
    s->send_len = sz;
    s->pre = upd ? AMBRYCRC_MSG_NOT_PUT : 0u;
    s->whole = sz != H.end;
    if (sz < H.end) s->pre |= AMBRYCRC_MSG_BAD_LAYOUT;
#pragma unroll
    for (int k = 0; k < kSendSlots; ++k)
      if (H.rel[k] != -1) s->dst[k] = s->whole ? kSendHash : (uint64_t)H.rel[k];
    return;
  }
  if (upd) {  // the reference's record offsets are -1 here: refused
    s->status = AMBRYCRC_MSG_NOT_PUT;
    return;
  }
  const uint64_t sz = has_size ? size : H.end;
  // the span: from the first sent record to the end of the last
  const bool blob = flag == AMBRYCRC_SEND_BLOB;
  const bool with_props = flag == AMBRYCRC_SEND_BLOB_PROPERTIES || flag == AMBRYCRC_SEND_BLOB_INFO;
  const bool with_um = flag == AMBRYCRC_SEND_BLOB_USER_METADATA || flag == AMBRYCRC_SEND_BLOB_INFO;
  // (every field read before the choice: loads inside its branches would merge into one load at a chosen
  // address, and the header would leave the registers for it)
  const uint64_t r1 = (uint64_t)H.rel[1], r3 = (uint64_t)H.rel[3], r4 = (uint64_t)H.rel[4];
  const uint64_t e1 = H.rend[1], e3 = H.rend[3], e4 = H.rend[4];
  const uint64_t lo = blob ? r4 : with_props ? r1 : r3;
  const uint64_t hi = blob ? e4 : with_um ? e3 : e1;
  const bool enc = send_reads_enckey(flag) && H.rel[0] != -1;
  if (hi > sz || (enc && H.rend[0] > sz)) {
    s->status = AMBRYCRC_MSG_BAD_LAYOUT;
    return;
  }
  if (enc) {  // deserializeBlobEncryptionKey (MessageFormatRecord.java:1588-1600)
    const uint32_t eb = send_record_check(0, p + H.rel[0], H.rend[0] - (uint64_t)H.rel[0]) |
                        (enc_crc_bad ? (uint32_t)AMBRYCRC_MSG_ENCKEY_CRC : 0u);
    if (eb) {
      s->status = eb;
      return;
    }
    s->enckey_rel = (uint32_t)H.rel[0] + 6;
    s->enckey_len = ld_be32(p + H.rel[0] + 2);
  }
  s->rel_off = (uint32_t)lo;
  s->send_len = hi - lo;
  if (blob) {  // deserializeBlobAll reads the other records too
    s->dst[1] = s->dst[3] = kSendHash;
    s->dst[4] = 0;
    return;
  }
  if (with_props) {
    s->dst[1] = 0;
    s->pre |= send_record_check(1, p + H.rel[1], H.rend[1] - (uint64_t)H.rel[1]);
  }
  if (with_um) {
    s->dst[3] = (uint64_t)H.rel[3] - lo;
    s->pre |= send_record_check(3, p + H.rel[3], H.rend[3] - (uint64_t)H.rel[3]);
  }
}

}  // namespace ambrycrc
