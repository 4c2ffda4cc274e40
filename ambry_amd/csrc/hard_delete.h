// hard_delete.h -- what the device hard delete (hard_delete_kernels.hip) and the per-message CPU entry
// (ambrycrc_hard_delete_message_cpu) share: the header's record spans, the recovery-info check and
// the record prefixes HardDeleteMessageFormatInputStream writes
// (ambry-messageformat/.../HardDeleteMessageFormatInputStream.java:58-124):
//   UserMetadata_Format_V1   short 1, int size, zeros, CRC      (MessageFormatRecord.java:1619-1635)
//   Blob_Format_V1           short 1, long size, zeros, CRC     (:1668-1680)
//   Blob_Format_V2           short 2, short type, long size, zeros, CRC   (:1717-1730)
//   Blob_Format_V3           short 3, short type, byte isCompressed = 0, long size, zeros, CRC
//                            (serializePartialBlobRecord(..., false), :1789-1795)
// Host and device; nothing here reads the region. Then the launch interface of the device pipeline.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ambrycrc.h"
#include "put_layout.h"

namespace ambrycrc {

static_assert(sizeof(ambrycrc_hard_delete_info) == 32, "ambrycrc_hard_delete_info: 32 bytes, no padding");

// The two records a hard delete rewrites, relative to the message start, from a verified header.
struct HdSpans {
  uint32_t um_rel, blob_rel;
  uint64_t um_span, blob_span;  // stored CRC included
};

// checkHeaderConstraints (MessageFormatRecord.java:985-1030) and the record spans, for a header of
// h bytes whose CRC verified (the checks of msg_parse.h parse_message, in its order): rel[] =
// encryption key, properties, update, user metadata, blob relative offsets (-1 absent), life the V3
// life version (0 for V1/V2), rem the region bytes from the message start. AMBRYCRC_MSG_BAD_LAYOUT,
// AMBRYCRC_MSG_NOT_PUT for an update message (BlobStoreHardDelete.java:129-131), or 0 with *s set.
__host__ __device__ inline uint32_t hd_header_spans(uint32_t h, int life, int64_t total, const int32_t (&rel)[5],
                                                    uint64_t rem, HdSpans* s) {
  const bool is_put = rel[1] != -1 && rel[2] == -1 && rel[3] != -1 && rel[4] != -1;
  const bool is_upd = rel[2] != -1 && rel[0] == -1 && rel[1] == -1 && rel[3] == -1 && rel[4] == -1;
  if (life < 0 || total <= 0 || !(is_put || is_upd)) return AMBRYCRC_MSG_BAD_LAYOUT;
  int64_t prev = -1, first = -1;
  for (int k = 0; k < 5; ++k) {
    if (rel[k] == -1) continue;
    if (rel[k] <= prev || rel[k] < (int32_t)h) return AMBRYCRC_MSG_BAD_LAYOUT;
    if (first < 0) first = rel[k];
    prev = rel[k];
  }
  if ((uint64_t)total > rem || (uint64_t)first > rem - (uint64_t)total) return AMBRYCRC_MSG_BAD_LAYOUT;
  const uint64_t end = (uint64_t)first + (uint64_t)total;
  for (int k = 0; k < 5; ++k) {  // every record holds its CRC at least
    if (rel[k] == -1) continue;
    uint64_t rend = end;
    for (int j = k + 1; j < 5; ++j)
      if (rel[j] != -1) {
        rend = (uint64_t)rel[j];
        break;
      }
    if (rend < (uint64_t)rel[k] + 8) return AMBRYCRC_MSG_BAD_LAYOUT;
  }
  if (is_upd) return AMBRYCRC_MSG_NOT_PUT;
  s->um_rel = (uint32_t)rel[3];
  s->blob_rel = (uint32_t)rel[4];
  s->um_span = (uint64_t)rel[4] - (uint64_t)rel[3];
  s->blob_span = end - (uint64_t)rel[4];
  return 0;
}

// Bytes of a blob record before its content (0: an unknown version).
__host__ __device__ inline uint32_t hd_blob_head(int version) {
  return version == 1 ? 10u : version == 2 ? 12u : version == 3 ? 13u : 0u;
}

// Recovery info against the header's spans: valid versions and blob type, and sizes that put the two
// records exactly on their spans -- an in-place writer never writes outside them (the reference
// trusts its own token, BlobStoreHardDelete.java:160-165).
__host__ __device__ inline bool hd_recovery_ok(const ambrycrc_hard_delete_info& r, const HdSpans& s) {
  const uint32_t head = hd_blob_head(r.blob_version);
  if (r.usermeta_version != 1 || head == 0 || r.blob_type < 0 || r.blob_type >= 2) return false;
  return (uint64_t)r.usermeta_size + 14 == s.um_span && r.blob_size <= s.blob_span &&
         r.blob_size + head + 8 == s.blob_span;
}

// The recovery info of a message (HardDeleteRecoveryMetadata's fields, HardDeleteInfo's offset and size).
__host__ __device__ inline ambrycrc_hard_delete_info hd_info(int header_version, const HdSpans& s, uint32_t um_size,
                                                             int blob_version, int blob_type, uint64_t blob_size) {
  ambrycrc_hard_delete_info o;
  o.blob_size = blob_size;
  o.size = s.um_span + s.blob_span;
  o.start = s.um_rel;
  o.usermeta_size = um_size;
  o.header_version = (int16_t)header_version;
  o.usermeta_version = 1;
  o.blob_version = (int16_t)blob_version;
  o.blob_type = (int16_t)blob_type;
  return o;
}

// The replacement records' bytes before their zero bodies; each returns its length.
constexpr uint32_t kHdUmHead = 6;
__host__ __device__ inline uint32_t hd_um_prefix(uint32_t um_size, uint8_t (&b)[16]) {
  put_be16(b, 1);
  put_be32(b + 2, um_size);
  return kHdUmHead;
}
__host__ __device__ inline uint32_t hd_blob_prefix(int version, int blob_type, uint64_t blob_size, uint8_t (&b)[16]) {
  put_be16(b, (uint32_t)version);
  if (version == 1) {
    put_be64(b + 2, blob_size);
    return 10;
  }
  put_be16(b + 2, (uint32_t)(uint16_t)blob_type);
  if (version == 2) {
    put_be64(b + 4, blob_size);
    return 12;
  }
  b[4] = 0;  // isCompressed
  put_be64(b + 5, blob_size);
  return 13;
}

// ---- launch interface between ambrycrc_hd.cpp and hard_delete_kernels.hip. CRC jobs are slot-major
// (entry i is message i's user-metadata record, entry m + i its blob record: coalesced stores, as the
// verify's jobs); fill jobs are message-major (entries 2i, 2i + 1).
struct HdArgs {
  uint8_t* region;
  uint64_t region_len;
  const uint64_t* msg_off;  // [m]
  uint64_t m;
  const ambrycrc_hard_delete_info* recovery;  // [m] or null
  int plan_only;
  const uint32_t* img;      // the table image (slice tables; the 64 words x^(8*2^k) after the LDS image)
  uint64_t* job_off;        // [2m] CRC jobs: the records less their stored CRCs (length 0: nothing to check)
  uint64_t* job_len;        // [2m]
  uint32_t* expected;       // [2m] stored CRCs
  const uint32_t* crc;      // [2m] computed by the batch engine
  uint32_t* check;          // [m] 1: compare crc with expected (no recovery info, header clean)
  ambrycrc_hard_delete_info* plan;  // [m] the parse kernel's info (valid when the final status is 0)
  uint32_t* status;         // [m] parse: provisional; seal: final
  ambrycrc_hard_delete_info* info;  // [m] or null
  uint64_t* fill_off;       // [2m] zero-fill jobs: offset in the region, length, cost (length + kCopyJobCost; 0 if empty)
  uint64_t* fill_len;
  uint64_t* fill_cost;
};
struct HdFillArgs {
  uint8_t* dst;
  const uint64_t* dst_off;  // [n]
  const uint64_t* len;      // [n]
  const uint64_t* start;    // [n + 1] exclusive scan of the costs
  uint32_t n;
};
hipError_t launch_hd_parse(const HdArgs& a, hipStream_t s);
hipError_t launch_hd_seal(const HdArgs& a, hipStream_t s);
hipError_t launch_hd_fill(const HdFillArgs& a, int grid, hipStream_t s);

}  // namespace ambrycrc
