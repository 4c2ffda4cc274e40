// recv.h -- the router's GET receive, per payload (GetBlobOperation.handleBody,
// ambry-router/.../GetBlobOperation.java:1113-1141, :1615-1694): MessageFormatRecord.deserializeBlob /
// deserializeBlobAll over one payload of a GetResponse body (MessageFormatRecord.java:222-241, :257-303,
// :1668-1833), the blob content sliced to the request's range (filterChunkToRange, :1394-1412). Shared by
// the device batch (recv_kernels.hip, ambrycrc_recv.cpp) and the per-payload CPU entry
// (ambrycrc_recv_cpu.cpp): what is refused, the info fields, and the CRC jobs -- the blob record hashed as
// its head and up to three pieces of content, because only content[lo, hi) may be copied. Host and device;
// nothing past the payload's `avail` bytes is read.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/ambrycrc.h"
#include "msg_header.h"

namespace ambrycrc {

static_assert(sizeof(ambrycrc_recv_info) == 56, "ambrycrc_recv_info: 56 bytes, no padding");
static_assert(offsetof(ambrycrc_recv_info, content_rel) == 24 && offsetof(ambrycrc_recv_info, blob_type) == 52,
              "ambrycrc_recv_info: the 4-B fields from byte 24, the 1-B ones from byte 52");

constexpr uint64_t kRecvNowhere = ~0ull;  // ambrycrc_recv_info::out_off of a payload that delivers nothing
constexpr uint64_t kRecvToEnd = ~0ull;    // a range's hi: to the content's end

// CRC jobs of a payload, in this slot order (slot-major in the batch: job k*m + i). The blob record is
// head || content[0, lo) || content[lo, hi) || content[hi, size) || CRC: the head (<= 13 B) is hashed by the
// thread that combines, the three content pieces are jobs, of which only the slice is copied through.
// Under ALL the encryption-key, properties and user-metadata records follow, hashed only.
constexpr uint32_t kRecvBefore = 0, kRecvSlice = 1, kRecvAfter = 2, kRecvEnckey = 3, kRecvProps = 4, kRecvUsermeta = 5;
constexpr uint32_t kRecvSlotsBlob = 3, kRecvSlotsAll = 6;

__host__ __device__ inline bool recv_flag_ok(int flag) { return flag == AMBRYCRC_SEND_BLOB || flag == AMBRYCRC_SEND_ALL; }
__host__ __device__ inline uint32_t recv_slots(int flag) {
  return flag == AMBRYCRC_SEND_ALL ? kRecvSlotsAll : kRecvSlotsBlob;
}

// Rule 1: the payload's bytes inside the body. False (AMBRYCRC_MSG_BAD_LAYOUT): the offset at or past the
// body's end, a given size of 0, or off + size past the body.
__host__ __device__ inline bool recv_extent(uint64_t off, bool has_size, uint64_t size, uint64_t body_len,
                                            uint64_t* avail) {
  *avail = 0;
  if (off >= body_len) return false;
  const uint64_t rem = body_len - off;
  if (has_size && (size == 0 || size > rem)) return false;
  *avail = has_size ? size : rem;
  return true;
}

struct RecvRecord {  // a blob record's own fields
  uint32_t head;     // bytes before the content
  uint32_t version, type, comp;
  uint64_t size;
};

// Rule 2: Blob_Format_V1 / V2 / V3's reads before the content (MessageFormatRecord.java:1681-1833) of a
// record at q with `avail` bytes from it on -- the cases of record_check, but the record may end before
// the bytes do (the reference leaves what follows in the stream). Reads at most head bytes.
__host__ __device__ inline uint32_t recv_blob_record(const uint8_t* q, uint64_t avail, RecvRecord* r) {
  r->head = r->version = r->type = r->comp = 0;
  r->size = 0;
  if (avail < 2) return AMBRYCRC_MSG_BAD_RECORD;
  const uint32_t v = ld_be16(q);
  const uint32_t head = blob_head((int)v);
  if (head == 0) return AMBRYCRC_MSG_BAD_VERSION;
  if (avail < head + 8) return AMBRYCRC_MSG_BAD_RECORD;
  const uint32_t type = v == 1 ? 0u : ld_be16(q + 2);
  const uint32_t comp = v == 3 ? (q[4] == 1 ? 1u : 0u) : 0u;
  const uint64_t size = ld_be64(q + head - 8);
  if (type >= 2 || size > 0x7FFFFFFFull) return AMBRYCRC_MSG_BAD_RECORD;
  if ((uint64_t)head + size + 8 > avail) return AMBRYCRC_MSG_BAD_LAYOUT;
  r->head = head;
  r->version = v;
  r->type = type;
  r->comp = comp;
  r->size = size;
  return 0;
}

struct RecvPlan {
  uint32_t status;          // rules 1-4 (AMBRYCRC_MSG_NO_ROOM comes with the placement, the CRC bits with the bytes)
  ambrycrc_recv_info info;  // out_off kRecvNowhere: the placement's to set; all else zero when refused
  uint32_t rec;             // the blob record's start, relative to the payload
  // per slot, relative to the payload; length 0: nothing to hash (an absent record, an empty piece)
  uint64_t job_off[kRecvSlotsAll], job_len[kRecvSlotsAll];
};

// One payload under `flag`. in_body / avail: recv_extent's. Under ALL: hdr_status the header's verdict
// inside the payload (msg_decode and msg_layout over avail), with L and header_version valid when it is 0,
// and rec_bits the record-check bits (_BAD_VERSION / _BAD_RECORD) the verify reports for the message. lo,
// hi: the range (0, kRecvToEnd without one).
__host__ __device__ inline void recv_plan(const uint8_t* p, bool in_body, uint64_t avail, int flag,
                                          uint32_t hdr_status, const MsgLayout& L, int header_version,
                                          uint32_t rec_bits, uint64_t lo, uint64_t hi, RecvPlan* s) {
  s->status = 0;
  __builtin_memset(&s->info, 0, sizeof s->info);
  s->info.out_off = kRecvNowhere;
  s->rec = 0;
#pragma unroll
  for (uint32_t k = 0; k < kRecvSlotsAll; ++k) s->job_off[k] = s->job_len[k] = 0;
  if (!in_body) {
    s->status = AMBRYCRC_MSG_BAD_LAYOUT;
    return;
  }
  const bool all = flag == AMBRYCRC_SEND_ALL;
  uint64_t rec = 0, span = avail;
  if (all) {
    if (hdr_status) {
      s->status = hdr_status;
      return;
    }
    if (L.rel[2] != -1) {  // deserializeBlobAll: "Only 'put' records are valid"
      s->status = AMBRYCRC_MSG_NOT_PUT;
      return;
    }
    if (rec_bits) {  // a deserializer throws
      s->status = rec_bits;
      return;
    }
    rec = (uint64_t)L.rel[4];
    span = L.rend[4] - rec;
  }
  RecvRecord r;
  const uint32_t rs = recv_blob_record(p + rec, span, &r);  // (under ALL the verify's record check passed: 0)
  if (rs) {
    s->status = rs;
    return;
  }
  const uint64_t end = hi == kRecvToEnd ? r.size : hi;
  if (end > r.size || lo > end) {
    s->status = AMBRYCRC_MSG_BAD_RANGE;
    return;
  }
  const uint64_t content = rec + r.head;
  s->rec = (uint32_t)rec;
  s->info.out_len = end - lo;
  s->info.blob_size = r.size;
  s->info.content_rel = (uint32_t)content;
  s->info.blob_type = (uint8_t)r.type;
  s->info.compressed = (uint8_t)r.comp;
  s->info.blob_version = (uint8_t)r.version;
  s->job_off[kRecvBefore] = content;
  s->job_len[kRecvBefore] = lo;
  s->job_off[kRecvSlice] = content + lo;
  s->job_len[kRecvSlice] = end - lo;
  s->job_off[kRecvAfter] = content + end;
  s->job_len[kRecvAfter] = r.size - end;
  if (!all) return;
  s->info.header_version = (uint8_t)header_version;
  // (the record checks passed: each size field agrees with its span)
  if (L.rel[0] != -1) {
    s->info.enckey_rel = (uint32_t)L.rel[0] + 6;
    s->info.enckey_len = ld_be32(p + L.rel[0] + 2);
    s->job_off[kRecvEnckey] = (uint64_t)L.rel[0];
    s->job_len[kRecvEnckey] = L.rend[0] - (uint64_t)L.rel[0] - 8;
  }
  s->info.props_rel = (uint32_t)L.rel[1] + 2;
  s->info.props_len = (uint32_t)(L.rend[1] - (uint64_t)L.rel[1] - 10);
  s->job_off[kRecvProps] = (uint64_t)L.rel[1];
  s->job_len[kRecvProps] = L.rend[1] - (uint64_t)L.rel[1] - 8;
  s->info.usermeta_rel = (uint32_t)L.rel[3] + 6;
  s->info.usermeta_len = ld_be32(p + L.rel[3] + 2);
  s->job_off[kRecvUsermeta] = (uint64_t)L.rel[3];
  s->job_len[kRecvUsermeta] = L.rend[3] - (uint64_t)L.rel[3] - 8;
}

// The status bit of a hashed-only record slot (kRecvEnckey .. kRecvUsermeta).
__host__ __device__ inline uint32_t recv_record_bit(uint32_t slot) {
  return slot == kRecvEnckey ? AMBRYCRC_MSG_ENCKEY_CRC : slot == kRecvProps ? AMBRYCRC_MSG_PROPS_CRC : AMBRYCRC_MSG_USERMETA_CRC;
}

// The placement's rule 5: a slice of len bytes at `at` inside [0, out_cap).
__host__ __device__ inline bool recv_fits(uint64_t at, uint64_t len, uint64_t out_cap) {
  return at <= out_cap && len <= out_cap - at;
}

// The whole receive of one payload in host memory: ambrycrc_receive_blob_cpu with the CRC loop as a
// parameter (crc(p, n) = CRC-32 of n bytes), so a stand-alone program can run it without the library.
template <class Crc>
inline void recv_blob_host(const uint8_t* payload, uint64_t avail, int flag, uint64_t lo, uint64_t hi, uint8_t* out,
                           uint64_t out_cap, const Crc& crc, ambrycrc_recv_info* info, uint32_t* status) {
  struct HeaderCrc {
    const uint8_t* p;
    const Crc& crc;
    uint32_t operator()(uint32_t n) const { return crc(p, (uint64_t)n); }
  };
  const bool in_body = avail != 0;
  const bool all = flag == AMBRYCRC_SEND_ALL;
  MsgHeader D;
  MsgLayout L;
  memset(&D, 0, sizeof D);
  memset(&L, 0, sizeof L);
  uint32_t hdr = 0, rec_bits = 0;
  if (all && in_body) {
    hdr = msg_decode(HeaderBytes{payload}, avail, HeaderCrc{payload, crc}, &D);
    if (hdr == 0) hdr = msg_layout(D, avail, &L);
    if (hdr == 0 && L.rel[2] == -1)
      for (int k = 0; k < kMsgSlots; ++k)
        if (L.rel[k] != -1) rec_bits |= record_check(k, payload + L.rel[k], L.rend[k] - (uint64_t)L.rel[k]);
  }
  RecvPlan s;
  recv_plan(payload, in_body, avail, flag, hdr, L, D.version, rec_bits, lo, hi, &s);
  *status = s.status;
  *info = s.info;
  if (s.status) return;
  if (s.info.out_len > out_cap || (s.info.out_len && !out)) {
    *status = AMBRYCRC_MSG_NO_ROOM;
    memset(info, 0, sizeof *info);
    info->out_off = kRecvNowhere;
    return;
  }
  // the CRCs against the stored longs (a non-zero upper word never matches)
  uint32_t bits = 0;
  const uint64_t content = s.info.content_rel, size = s.info.blob_size;
  if ((uint64_t)crc(payload + s.rec, content - s.rec + size) != ld_be64(payload + content + size))
    bits |= AMBRYCRC_MSG_BLOB_CRC;
  for (uint32_t k = kRecvEnckey; k < recv_slots(flag); ++k) {
    if (s.job_len[k] == 0) continue;
    const uint8_t* q = payload + s.job_off[k];
    if ((uint64_t)crc(q, s.job_len[k]) != ld_be64(q + s.job_len[k])) bits |= recv_record_bit(k);
  }
  if (s.info.out_len) memcpy(out, payload + content + lo, s.info.out_len);
  info->out_off = 0;
  *status = bits;
}
}  // namespace ambrycrc
