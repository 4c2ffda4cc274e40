// hard_delete.h -- what the device hard delete (hard_delete_kernels.hip) and the per-message CPU entry
// (ambrycrc_hard_delete_message_cpu) share: the two record spans of a header, the recovery-info check and
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
#include "msg_header.h"
#include "put_layout.h"

namespace ambrycrc {

static_assert(sizeof(ambrycrc_hard_delete_info) == 32, "ambrycrc_hard_delete_info: 32 bytes, no padding");

// The two records a hard delete rewrites, relative to the message start, from a verified header.
struct HdSpans {
  uint32_t um_rel, blob_rel;
  uint64_t um_span, blob_span;  // stored CRC included
};

// The two spans of a header msg_layout accepted (msg_header.h), or AMBRYCRC_MSG_NOT_PUT for an update
// message (BlobStoreHardDelete.java:129-131). From the two offsets and the message end, which for a PUT
// are L.rend[3] and L.rend[4]: read from rend[] hd_parse_kernel needs 75 VGPRs for 69 and loses a wave.
__host__ __device__ inline uint32_t hd_header_spans(const MsgHeader& H, const MsgLayout& L, HdSpans* s) {
  s->um_rel = (uint32_t)H.rel[3];
  s->blob_rel = (uint32_t)H.rel[4];
  s->um_span = (uint64_t)H.rel[4] - (uint64_t)H.rel[3];  // a PUT: the blob record follows, then the message ends
  s->blob_span = L.end - (uint64_t)H.rel[4];
  return H.rel[2] != -1 ? (uint32_t)AMBRYCRC_MSG_NOT_PUT : 0u;  // (*s is then meaningless)
}

// Recovery info against the header's spans: valid versions and blob type, and sizes that put the two
// records exactly on their spans -- an in-place writer never writes outside them (the reference
// trusts its own token, BlobStoreHardDelete.java:160-165).
__host__ __device__ inline bool hd_recovery_ok(const ambrycrc_hard_delete_info& r, const HdSpans& s) {
  const uint32_t head = blob_head(r.blob_version);
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
