// send.h -- MessageFormatSend.fetchDataFromReadSet's per-message decisions
// (ambry-messageformat/.../MessageFormatSend.java:112-242), shared by the device batch
// (send_kernels.hip, ambrycrc_send.cpp) and the per-message CPU entry (ambrycrc_msg_cpu.cpp): the
// send_plan over a header msg_header.h decoded -- what is refused, what is sent,
// and what each record slot's CRC job does (copied to where, hashed only, not read). Host and device;
// everything reads only inside the spans a verified header establishes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ambrycrc.h"
#include "msg_header.h"

namespace ambrycrc {

static_assert(sizeof(ambrycrc_send_info) == 32, "ambrycrc_send_info: 32 bytes, no padding");

constexpr uint64_t kSendNowhere = ~0ull;   // ambrycrc_send_info::out_off of a message not sent
// SendPlan::dst values besides a destination: hash the record without copying it (SweepArgs kCopySkip),
// or do not read it at all.
constexpr uint64_t kSendHash = ~0ull;
constexpr uint64_t kSendNone = ~0ull - 1;

// A header whose CRC verified and whose constraints hold: msg_header.h's layout.
using SendHeader = MsgLayout;

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
  uint64_t dst[kMsgSlots];  // per record slot: offset in the sent span, kSendHash or kSendNone
};

// One message under `flag`. in_region: its offset lies inside the region, with rem bytes from it on;
// has_size / size: readSet.sizeInBytes, else the header's own length; hdr_status: the header's verdict
// (msg_decode, msg_layout) with H valid when it is 0; enc_crc_bad: the
// encryption-key record's CRC differs from its stored long (consulted only where the record is read).
__host__ __device__ inline void send_plan(const uint8_t* p, bool in_region, uint64_t rem, bool has_size,
                                          uint64_t size, int flag, uint32_t hdr_status, const SendHeader& H,
                                          bool enc_crc_bad, SendPlan* s) {
  s->status = s->pre = 0;
  s->send_len = 0;
  s->rel_off = s->enckey_rel = s->enckey_len = 0;
  s->whole = false;
#pragma unroll
  for (int k = 0; k < kMsgSlots; ++k) s->dst[k] = kSendNone;
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
    for (int k = 0; k < kMsgSlots; ++k)
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
    const uint32_t eb = record_check(0, p + H.rel[0], H.rend[0] - (uint64_t)H.rel[0]) |
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
    s->pre |= record_check(1, p + H.rel[1], H.rend[1] - (uint64_t)H.rel[1]);
  }
  if (with_um) {
    s->dst[3] = (uint64_t)H.rel[3] - lo;
    s->pre |= record_check(3, p + H.rel[3], H.rend[3] - (uint64_t)H.rel[3]);
  }
}

}  // namespace ambrycrc
