// msg_header.h -- the stored message header (MessageFormatRecord.java MessageHeader_Format_V1 / V2 / V3,
// :467-486, :696-725, :951-981) and the rules every kernel and CPU entry applies to it, written once
// (DESIGN.md §18): version -> header size, where each version keeps its fields, the stored header CRC,
// checkHeaderConstraints with the record spans (msg_layout), the two laxer acceptance rules of the chain
// and of the staging extent, and what each record's deserializer reads before its CRC (record_check).
// Host and device. The decoder reads through a field source: HeaderBytes here, the header registers of
// msg_parse.h (HeaderWordSrc) in the kernels that load a header in one round trip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ambrycrc.h"
#include "record_fields.h"

namespace ambrycrc {

// Record slots of a header: encryption key, properties, update, user metadata, blob.
constexpr int kMsgSlots = 5;

__host__ __device__ inline uint32_t msg_header_size(int version) {
  return version == 1 ? 34u : version == 2 ? 38u : version == 3 ? 40u : 0u;
}
// Bytes of a blob record before its content, Blob_Format_V1 / V2 / V3 (0: an unknown version).
__host__ __device__ inline uint32_t blob_head(int version) {
  return version == 1 ? 10u : version == 2 ? 12u : version == 3 ? 13u : 0u;
}

struct MsgHeader {
  int32_t version;
  uint32_t hs;             // header bytes
  int32_t life;            // V3's life version, 0 for V1 / V2
  int64_t total;           // the records' total size
  int32_t rel[kMsgSlots];  // record offsets relative to the message, -1 absent
};

// Field source: plain bytes (host memory, or device global memory: one unaligned load a field).
struct HeaderBytes {
  const uint8_t* p;
  __host__ __device__ uint32_t u16(uint32_t at) const { return ld_be16(p + at); }
  __host__ __device__ uint32_t u32(uint32_t at) const { return ld_be32(p + at); }
  // the stored header CRC, the long at [hs - 8, hs): its upper and lower words
  __host__ __device__ void stored_crc(int, uint32_t hs, uint32_t* hi, uint32_t* lo) const {
    *hi = ld_be32(p + hs - 8);
    *lo = ld_be32(p + hs - 4);
  }
};

// The fields of a header of version v in 1..3. Every offset is a literal once the version branch is
// taken, so a register source folds each read to one expression.
template <class S>
__host__ __device__ __forceinline__ void msg_fields(const S& s, int v, MsgHeader* H) {
  H->version = v;
  H->hs = msg_header_size(v);
  if (v == 3) {
    H->life = (int16_t)s.u16(2);
    H->total = (int64_t)((uint64_t)s.u32(4) << 32 | s.u32(8));
#pragma unroll
    for (int k = 0; k < kMsgSlots; ++k) H->rel[k] = (int32_t)s.u32(12 + 4 * k);
  } else {
    H->life = 0;
    H->total = (int64_t)((uint64_t)s.u32(2) << 32 | s.u32(6));
    if (v == 1) {  // V1 has no encryption-key slot
      H->rel[0] = -1;
#pragma unroll
      for (int k = 1; k < kMsgSlots; ++k) H->rel[k] = (int32_t)s.u32(6 + 4 * k);
    } else {
#pragma unroll
      for (int k = 0; k < kMsgSlots; ++k) H->rel[k] = (int32_t)s.u32(10 + 4 * k);
    }
  }
}

// The header of a message the verify found clean.
__host__ __device__ inline MsgHeader msg_header_of(const uint8_t* p) {
  MsgHeader H;
  msg_fields(HeaderBytes{p}, (int)ld_be16(p), &H);
  return H;
}

struct NoCrc {};  // msg_decode without verifyHeader (the extent rule)
template <class Crc>
__host__ __device__ __forceinline__ bool header_crc_is(const Crc& crc, uint32_t n, uint32_t hi, uint32_t lo) {
  return hi == 0 && crc(n) == lo;
}
__host__ __device__ __forceinline__ bool header_crc_is(const NoCrc&, uint32_t, uint32_t, uint32_t) { return true; }

// The header at the source, rem bytes of region from it on: the version, the header inside the region,
// verifyHeader (:1132-1145; crc(n) = CRC-32 of the header's first n bytes, against the stored long's
// lower word, its upper word 0), then the fields. 0, or the status that ends the message; nothing past
// the header is read.
template <class S, class Crc>
__host__ __device__ __forceinline__ uint32_t msg_decode(const S& s, uint64_t rem, const Crc& crc, MsgHeader* H) {
  if (rem < 2) return AMBRYCRC_MSG_BAD_LAYOUT;
  const int v = (int16_t)s.u16(0);
  const uint32_t hs = msg_header_size(v);
  if (hs == 0) return AMBRYCRC_MSG_BAD_VERSION;
  if (rem < hs) return AMBRYCRC_MSG_BAD_LAYOUT;
  // (the fields before the CRC's verdict, which alone decides whether they count: the host's serial scan
  // then has its next offset in flight while the CRC runs)
  msg_fields(s, v, H);
  uint32_t hi, lo;
  s.stored_crc(v, hs, &hi, &lo);
  return header_crc_is(crc, hs - 8, hi, lo) ? 0u : (uint32_t)AMBRYCRC_MSG_HEADER_CRC;
}

// A decoded header's record spans.
struct MsgLayout {
  uint32_t hs;
  int32_t rel[kMsgSlots];
  uint64_t rend[kMsgSlots];  // where each present record ends (its stored CRC's last byte + 1)
  uint64_t first, end;       // first record, message end
};

// checkHeaderConstraints (MessageFormatRecord.java:985-1030) and the record spans: life version >= 0,
// total > 0, exactly a PUT's or an update's slots, the offsets ascending from the header's end on, the
// message inside rem; a record ends where the next present one starts, the last at the message end,
// and each holds its CRC at least. 0 or AMBRYCRC_MSG_BAD_LAYOUT.
__host__ __device__ __forceinline__ uint32_t msg_layout(const MsgHeader& H, uint64_t rem, MsgLayout* L) {
  const int32_t* rel = H.rel;
  const bool is_put = rel[1] != -1 && rel[2] == -1 && rel[3] != -1 && rel[4] != -1;
  const bool is_upd = rel[2] != -1 && rel[0] == -1 && rel[1] == -1 && rel[3] == -1 && rel[4] == -1;
  if (H.life < 0 || H.total <= 0 || !(is_put || is_upd)) return AMBRYCRC_MSG_BAD_LAYOUT;
  int64_t prev = -1, first = -1;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < kMsgSlots; ++k) {
    if (rel[k] == -1) continue;
    if (rel[k] <= prev || rel[k] < (int32_t)H.hs) ok = false;
    if (first < 0) first = rel[k];
    prev = rel[k];
  }
  if (!ok || (uint64_t)H.total > rem || (uint64_t)first > rem - (uint64_t)H.total) return AMBRYCRC_MSG_BAD_LAYOUT;
  const uint64_t end = (uint64_t)first + (uint64_t)H.total;
  uint64_t next = end;  // backwards, constant indices: the arrays stay in registers on the device
#pragma unroll
  for (int k = kMsgSlots - 1; k >= 0; --k) {
    L->rel[k] = rel[k];
    L->rend[k] = next;
    if (rel[k] != -1) {
      ok = ok && next >= (uint64_t)rel[k] + 8;
      next = (uint64_t)rel[k];
    }
  }
  if (!ok) return AMBRYCRC_MSG_BAD_LAYOUT;
  L->hs = H.hs;
  L->first = (uint64_t)first;
  L->end = end;
  return 0;
}

// The two laxer rules. Both take the first present offset and the total alone.
__host__ __device__ __forceinline__ bool msg_hop(const MsgHeader& H, int64_t first_min, uint64_t rem, uint64_t* next) {
  // (forwards with a break: on the host the serial scan's next offset then hangs on one predicted
  // branch, not on a chain of five selects)
  int64_t first = -1;
  for (int k = 0; k < kMsgSlots; ++k)
    if (H.rel[k] != -1) {
      first = H.rel[k];
      break;
    }
  if (H.total <= 0 || first < first_min || (uint64_t)H.total > rem || (uint64_t)first > rem - (uint64_t)H.total)
    return false;
  *next = (uint64_t)first + (uint64_t)H.total;
  return true;
}

// Chain acceptance: BlobStoreRecovery's walk (BlobStoreRecovery.java:51-71) hops over a header whose CRC
// verifies by first + total without checkHeaderConstraints -- no slot shape, no record spans -- so the
// chain accepts headers the verify then refuses. 0 and *next, or why the walk stops here.
template <class S, class Crc>
__host__ __device__ __forceinline__ uint32_t msg_chain_accept(const S& s, uint64_t rem, const Crc& crc, uint64_t* next) {
  MsgHeader H;
  const uint32_t st = msg_decode(s, rem, crc, &H);
  if (st) return st;
  return msg_hop(H, (int64_t)H.hs, rem, next) ? 0u : (uint32_t)AMBRYCRC_MSG_BAD_LAYOUT;
}

// Extent: the bytes a verify of this message may read, for staging and for the region processors' wait
// target, before anything is verified -- no CRC, any first offset >= 0. 0 when the header is
// unparseable or the message overruns rem (the verify then reads the header alone).
template <class S>
__host__ __device__ __forceinline__ uint64_t msg_extent(const S& s, uint64_t rem) {
  MsgHeader H;
  uint64_t end = 0;
  return msg_decode(s, rem, NoCrc{}, &H) == 0 && msg_hop(H, 0, rem, &end) ? end : 0;
}

// What each record's deserializer reads before its CRC (MessageFormatRecord.java), for a record
// of `span` bytes at q (its stored CRC the last 8): the record version (an unknown one throws
// UnknownFormatVersion, :147-239) and the size fields that decide where the stream looks for
// the CRC. BlobEncryptionKey_Format_V1 (:1588-1600) and UserMetadata_Format_V1 (:1637-1649): an
// int size, then that many bytes, then the CRC; Blob_Format_V1/V2/V3 (:1681-1833): blob type
// ordinal < 2, a long size <= Integer.MAX_VALUE, then the content and the CRC. A size that
// disagrees with the header's record span, or a bad type, is AMBRYCRC_MSG_BAD_RECORD (the
// reference reads the CRC at a different place, or throws). BlobProperties_Format_V1 and
// Update_Format_V1..V3: their fields, to the CRC (record_fields.h).
__host__ __device__ __forceinline__ uint32_t record_check(int k, const uint8_t* q, uint64_t span) {
  if (span < 10) return AMBRYCRC_MSG_BAD_RECORD;  // a version and a CRC at least
  const uint32_t v = ld_be16(q);
  switch (k) {
    case 0:    // encryption key
    case 3: {  // user metadata
      if (v != 1) return AMBRYCRC_MSG_BAD_VERSION;
      if (span < 14) return AMBRYCRC_MSG_BAD_RECORD;
      const int32_t n = (int32_t)ld_be32(q + 2);
      return n >= 0 && (uint64_t)n + 14 == span ? 0u : AMBRYCRC_MSG_BAD_RECORD;
    }
    case 1:  // properties (msg_parse_kernel parses them from its LDS window instead)
      return props_record_check(q, span);
    case 2:  // update
      return update_record_check(q, span);
    default: {  // blob
      const uint32_t head = blob_head((int)v);
      if (head == 0) return AMBRYCRC_MSG_BAD_VERSION;
      if (span < head + 8) return AMBRYCRC_MSG_BAD_RECORD;
      const uint32_t type = v == 1 ? 0u : ld_be16(q + 2);
      const uint64_t size = ld_be64(q + head - 8);
      return type < 2 && size <= 0x7FFFFFFFull && size + head + 8 == span ? 0u : AMBRYCRC_MSG_BAD_RECORD;
    }
  }
}

// The fields of a PUT the verify found clean (the deserializers' reads, MessageFormatRecord.java:1568-1833),
// and whether they agree with the header's spans -- after a clean verify they do.
struct PutFields {
  uint32_t enc_len;    // encryption key bytes (0 without the record)
  int64_t props_len;   // BlobPropertiesSerDe bytes
  uint32_t um_len;
  uint32_t blob_version, head, type, comp;
  uint64_t size;       // blob content bytes
  int64_t first, end;  // first record, message end
  bool ok;
};

__host__ __device__ __forceinline__ PutFields put_fields(const uint8_t* p, const MsgHeader& H) {
  const int32_t enc = H.rel[0], bp = H.rel[1], um = H.rel[3], blob = H.rel[4];
  PutFields f;
  f.first = enc != -1 ? enc : bp;
  f.end = f.first + H.total;
  f.ok = f.first >= (int64_t)H.hs;
  f.enc_len = 0;
  if (enc != -1) {
    f.enc_len = ld_be32(p + enc + 2);
    f.ok = f.ok && (int64_t)enc + 6 + f.enc_len + 8 == bp;
  }
  f.props_len = (int64_t)um - bp - 2 - 8;  // BlobProperties_Format_V1: version, SerDe bytes, CRC
  f.um_len = ld_be32(p + um + 2);           // UserMetadata_Format_V1: version, int size, ..., CRC
  f.ok = f.ok && f.props_len >= 0 && (int64_t)um + 6 + f.um_len + 8 == blob;
  f.blob_version = ld_be16(p + blob);       // Blob_Format_V1 / V2 / V3 (:1668-1833)
  f.head = blob_head((int)f.blob_version);
  f.type = f.comp = 0;
  f.size = 0;
  if (f.head) {
    f.size = ld_be64(p + blob + f.head - 8);
    if (f.blob_version >= 2) f.type = ld_be16(p + blob + 2);
    if (f.blob_version == 3) f.comp = p[blob + 4] == 1 ? 1u : 0u;
  }
  f.ok = f.ok && f.head != 0 && f.type < 2 && f.size <= 0x7FFFFFFFull &&
         (int64_t)blob + f.head + (int64_t)f.size + 8 == f.end;
  return f;
}

}  // namespace ambrycrc
