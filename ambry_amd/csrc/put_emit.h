// put_emit.h -- the write side of a stored PUT message: what every writer of one does after
// it holds an ambrycrc_put_desc and its PutLayout (put_layout.h), host and device. The serializer
// (put_kernels.hip, ambrycrc_put.cpp), the transform (message_kernels.hip, ambrycrc_msg_cpu.cpp), the re-key
// (rekey_kernels.hip, rekey.h) and the ingest (ingest_kernels.hip, ambrycrc_ingest.cpp) share
//   put_desc_of_stored   the descriptor that re-serializes a clean stored PUT
//   put_emit_header      header bytes and their CRC, from registers               (device)
//   put_emit_props       the BlobProperties record written and hashed 8 B at a time (device)
//   put_emit_record      a record's head and its trailer from its body's CRC     (device)
//   crc_head_body, blob_crc_moved   the two CRC identities behind them           (device)
//   copy_job_cost (crc32_kernels.h), store_copy_jobs   the gather copy's job lists (device)
//   put_seal_record      the CPU writers' trailers, hashed from the output
// The VERSION_5 re-encoding itself is record_fields.h props_v5_byte. The device helpers take the LDS tables
// of stage_slice_tables (crc_img.h) and the table image; they exist under hipcc only (the stand-alone test
// programs build the host side of these headers with the host compiler).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ambrycrc.h"
#include "crc32_kernels.h"
#if defined(__HIPCC__)
#include "crc_img.h"
#endif
#include "msg_header.h"
#include "put_layout.h"
#include "record_fields.h"

namespace ambrycrc {

// PutMessageFormatInputStream's arguments for the clean stored PUT at region + off (header H, fields f with
// f.ok; msg_header.h), re-serialized at header_version with `life` and a payload of props_len bytes: every
// source an offset in the region, out_off 0. A V1 output drops the encryption key. The re-key then sets its
// own key and content.
__host__ __device__ inline ambrycrc_put_desc put_desc_of_stored(uint64_t off, const MsgHeader& H, const PutFields& f,
                                                                int header_version, int life, uint32_t props_len) {
  ambrycrc_put_desc d;
  __builtin_memset(&d, 0, sizeof d);
  const int32_t enc = H.rel[0], bp = H.rel[1], um = H.rel[3], blob = H.rel[4];
  const bool keep_enc = enc != -1 && header_version >= 2;
  d.key_src = off + H.hs;
  d.key_len = (uint32_t)(f.first - H.hs);
  d.enckey_src = keep_enc ? off + enc + 6 : 0;
  d.enckey_len = keep_enc ? (int32_t)f.enc_len : -1;
  d.props_src = off + bp + 2;
  d.props_len = props_len;
  d.usermeta_src = off + um + 6;
  d.usermeta_len = f.um_len;
  d.blob_src = off + blob + f.head;
  d.blob_len = f.size;
  d.life_version = (int16_t)life;
  d.blob_type = (int16_t)f.type;
  d.compressed = (uint8_t)f.comp;
  d.header_version = (uint8_t)header_version;
  return d;
}

// ---------------------------------------------------------------- CPU writers
// CRC job k of the message at m (put_crc_job: 0 the header, then the records), hashed from the bytes in
// place, and its trailer written: the CRC, 0 for an absent record.
inline uint32_t put_seal_record(uint8_t* m, const PutLayout& L, uint32_t k) {
  uint64_t off, len;
  bool present;
  put_crc_job(L, k, &off, &len, &present);
  if (!present) return 0;
  const uint32_t c = ambrycrc_update(0, m + off, len);
  put_be64(m + off + len, (uint64_t)c);
  return c;
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------- device writers
// One CRC step over byte b through the LDS byte table (t[0..255] = T0).
__device__ __forceinline__ uint32_t crc_step_lds(const uint32_t* __restrict__ t, uint32_t c, uint32_t b) {
  return t[(c ^ b) & 0xffu] ^ (c >> 8);
}

// The header's CRC trailer, from the header bytes built in registers; BYTES: those bytes too (a caller that
// ran put_write_fixed has them in place).
template <bool BYTES>
__device__ __forceinline__ void put_emit_header(const uint32_t* __restrict__ tbl, const ambrycrc_put_desc& d,
                                                const PutLayout& L, uint8_t* msg) {
  uint8_t h[32];
  const uint32_t hn = put_header_bytes(d, L, h);
  if (BYTES) put_store_header(msg, h, hn);
  put_be64(msg + hn, (uint64_t)crc_regs_lds(tbl, 0u, h, hn));
}

// BlobProperties_Format_V1 at rec: version 1, the n payload bytes byte(j, stored byte j) made from the
// stored_len bytes at ps, and the record's CRC hashed from the bytes as they are written -- 8 B at a time,
// whole words where the load or the store has one, bytes at the two tails.
template <class ByteFn>
__device__ __forceinline__ void put_emit_props(const uint32_t* __restrict__ tbl, const uint8_t* ps, uint32_t stored_len,
                                               uint8_t* rec, uint32_t n, ByteFn byte) {
  put_be16(rec, 1u);
  uint8_t* pd = rec + 2;
  uint32_t c = crc_step_lds(tbl, crc_step_lds(tbl, 0xFFFFFFFFu, 0u), 1u);
  for (uint32_t j0 = 0; j0 < n; j0 += 8) {
    uint64_t w = 0;
    if (j0 + 8 <= stored_len) {
      __builtin_memcpy(&w, ps + j0, 8);
    } else {
#pragma unroll
      for (uint32_t b = 0; b < 8; ++b)
        if (j0 + b < stored_len) w |= (uint64_t)ps[j0 + b] << (8 * b);
    }
    uint64_t o = 0;
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
      if (j0 + b < n) {
        const uint32_t v = byte(j0 + b, (uint8_t)(w >> (8 * b)));
        o |= (uint64_t)v << (8 * b);
        c = crc_step_lds(tbl, c, v);
      }
    }
    if (j0 + 8 <= n) {
      __builtin_memcpy(pd + j0, &o, 8);
    } else {
#pragma unroll
      for (uint32_t b = 0; b < 8; ++b)
        if (j0 + b < n) pd[j0 + b] = (uint8_t)(o >> (8 * b));
    }
  }
  put_be64(pd + n, (uint64_t)~c);
}

// crc(head || body) = crc(head) x^(8|body|) + crc(body): a record's CRC from its head's hn bytes in registers
// and the CRC of its body, hashed elsewhere (an empty body: the head's alone).
template <int N>
__device__ __forceinline__ uint32_t crc_head_body(const uint32_t* __restrict__ tbl, const uint32_t* __restrict__ img,
                                                  const uint8_t (&head)[N], uint32_t hn, const uint32_t* body_crc,
                                                  uint64_t body_len) {
  uint32_t c = crc_regs_lds(tbl, 0u, head, hn);
  if (body_len) c = mul_xpow8_img(img, c, body_len) ^ *body_crc;
  return c;
}

// Record K of the message (1 encryption key, 3 user metadata, 4 blob; put_prefix_bytes): its head written at
// the record's start and its trailer after the body, from the body's CRC.
template <uint32_t K>
__device__ __forceinline__ void put_emit_record(const uint32_t* __restrict__ tbl, const uint32_t* __restrict__ img,
                                                const ambrycrc_put_desc& d, const PutLayout& L, uint8_t* msg,
                                                const uint32_t* body_crc) {
  static_assert(K == 1 || K == 3 || K == 4, "a record with a sized body");
  uint8_t b[16];
  put_prefix_bytes(d, K, b);
  uint8_t* q = msg + put_record_rel(L, K);
  if (K == 4) {
    __builtin_memcpy(q, b, 13);
    put_be64(q + 13 + d.blob_len, (uint64_t)crc_head_body(tbl, img, b, 13u, body_crc, d.blob_len));
  } else {
    const uint32_t len = K == 1 ? (uint32_t)d.enckey_len : d.usermeta_len;
    __builtin_memcpy(q, b, 6);
    put_be64(q + 6 + len, (uint64_t)crc_head_body(tbl, img, b, 6u, body_crc, len));
  }
}

// The CRC of the output's blob record when its content is a verified stored record's: stored_crc (the low
// word of that record's trailer) moved from the stored head (hn = 10, 12 or 13 bytes at sh) to the V3 head h3
// the output writes. A head that changes -- Blob_Format_V1 / V2, or a V3 isCompressed byte other than 0 / 1 --
// moves the CRC by (crc(old head) ^ crc(new head)) x^(8|content|) (zlib's crc32_combine), with no pass over
// the content. crc(b, n): the CRC of n bytes of a uint8_t[16] in registers.
template <class Crc>
__device__ __forceinline__ uint32_t blob_crc_moved(Crc crc, const uint32_t* __restrict__ img, const uint8_t* sh,
                                                   uint32_t hn, const uint8_t (&h3)[16], uint32_t stored_crc,
                                                   uint64_t size) {
  if (hn == 13 && sh[4] == h3[4]) return stored_crc;
  uint8_t oh[16];
#pragma unroll
  for (uint32_t b = 0; b < 16; ++b) oh[b] = b < hn ? sh[b] : 0;
  return stored_crc ^ mul_xpow8_img(img, crc(oh, hn) ^ crc(h3, 13u), size);
}

// Message i's SLOTS copy jobs into the gather copy's slot-major lists (job k of message i at k m + i), each
// with its cost.
template <uint32_t SLOTS>
__device__ __forceinline__ void store_copy_jobs(uint64_t* cp_src, uint64_t* cp_dst, uint64_t* cp_len, uint64_t* cp_cost,
                                                uint64_t m, uint64_t i, const uint64_t (&src)[SLOTS],
                                                const uint64_t (&dst)[SLOTS], const uint64_t (&len)[SLOTS]) {
#pragma unroll
  for (uint32_t k = 0; k < SLOTS; ++k) {
    cp_src[k * m + i] = src[k];
    cp_dst[k * m + i] = dst[k];
    cp_len[k * m + i] = len[k];
    cp_cost[k * m + i] = copy_job_cost(len[k]);
  }
}
#endif  // __HIPCC__

}  // namespace ambrycrc
