// msg_parse.h -- one stored message's header registers, properties window and CRC jobs, for the
// thread-per-message kernels of the message verify and transform (message_kernels.hip) and the
// region-mode message processors (region_kernels.hip region_fused_kernel / region_tail_kernel). The
// header rule itself is msg_header.h's; this file gives it the header as ten registers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ambrycrc.h"
#include "crc32_kernels.h"
#include "msg_header.h"

namespace ambrycrc {

// The status bit of record slot k (encryption key, properties, update, user metadata, blob).
static_assert(AMBRYCRC_MSG_ENCKEY_CRC == 2u && AMBRYCRC_MSG_PROPS_CRC == 4u && AMBRYCRC_MSG_UPDATE_CRC == 8u &&
                  AMBRYCRC_MSG_USERMETA_CRC == 16u && AMBRYCRC_MSG_BLOB_CRC == 32u,
              "record bits are consecutive");
__device__ __forceinline__ uint32_t record_bit(int k) { return AMBRYCRC_MSG_ENCKEY_CRC << k; }

// Header bytes [0, 40) of a message as ten little-endian words, one unaligned 16 + 16 + 8 B
// load when the region holds 40 bytes past `off` (the longest header, V3), else byte loads
// with zero fill. Issued before the table staging, so one memory round trip covers it.
struct HeaderWords {
  uint32_t w[10];
};

__device__ __forceinline__ HeaderWords load_header(const uint8_t* p, uint64_t rem) {
  HeaderWords h;
  if (rem >= 40) {
    __builtin_memcpy(&h.w[0], p, 16);
    __builtin_memcpy(&h.w[4], p + 16, 16);
    __builtin_memcpy(&h.w[8], p + 32, 8);
  } else {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
      uint32_t v = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if ((uint64_t)(4 * i + b) < rem) v |= (uint32_t)p[4 * i + b] << (8 * b);
      h.w[i] = v;
    }
  }
  return h;
}

// Big-endian 32-bit field at byte 4k+2 (V1/V2 layouts) and at byte 4k (V3) of the header.
__device__ __forceinline__ uint32_t be32_w2(const HeaderWords& h, int k) {
  return __builtin_bswap32(__builtin_amdgcn_alignbyte(h.w[k + 1], h.w[k], 2));
}
__device__ __forceinline__ uint32_t be32_w0(const HeaderWords& h, int k) { return __builtin_bswap32(h.w[k]); }

// CRC-32 of the first n = h - 8 header bytes (26, 30 or 32) from the words: slice-by-4 over
// whole words, then the two trailing bytes of V1/V2.
__device__ __forceinline__ uint32_t header_crc(const HeaderWords& h, uint32_t n, const uint32_t* __restrict__ t) {
  uint32_t c = 0xFFFFFFFFu;
  const uint32_t nw = n >> 2;
#pragma unroll
  for (uint32_t i = 0; i < 8; ++i) {
    if (i < nw) {
      const uint32_t x = c ^ h.w[i];
      c = t[768 + (x & 0xffu)] ^ t[512 + ((x >> 8) & 0xffu)] ^ t[256 + ((x >> 16) & 0xffu)] ^ t[x >> 24];
    }
  }
  if (n & 2u) {
    const uint32_t tw = nw == 6 ? h.w[6] : h.w[7];
    c = (c >> 8) ^ t[(c ^ tw) & 0xffu];
    c = (c >> 8) ^ t[(c ^ (tw >> 8)) & 0xffu];
  }
  return ~c;
}

// msg_header.h's field source over the header words: a field at byte 4k is a byte swap, one at 4k + 2 an
// alignbyte of two words and a swap; crc(n) hashes the words with the slice tables t.
struct HeaderWordSrc {
  const HeaderWords& h;
  __device__ __forceinline__ uint32_t u16(uint32_t at) const {
    return __builtin_bswap16((uint16_t)(h.w[at >> 2] >> (8 * (at & 3))));
  }
  __device__ __forceinline__ uint32_t u32(uint32_t at) const { return at & 2 ? be32_w2(h, at >> 2) : be32_w0(h, at >> 2); }
  // the stored header CRC, the long at [hs - 8, hs): a select among the three layouts' words
  __device__ __forceinline__ void stored_crc(int v, uint32_t, uint32_t* hi, uint32_t* lo) const {
    *hi = v == 3 ? u32(32) : v == 2 ? u32(30) : u32(26);
    *lo = v == 3 ? u32(36) : v == 2 ? u32(34) : u32(30);
  }
};
struct HeaderWordCrc {
  const HeaderWords& h;
  const uint32_t* __restrict__ t;
  __device__ __forceinline__ uint32_t operator()(uint32_t n) const { return header_crc(h, n, t); }
};

// The first bytes of a record staged in this thread's LDS slot, the rest read from global memory:
// the properties parse walks int-length strings, one dependent read per field, which from LDS
// costs an LDS round trip instead of a memory one.
constexpr uint32_t kPropsWin = AMBRY_PROPS_WIN;        // bytes staged per thread (a multiple of 16)
constexpr uint32_t kPropsSlotWords = kPropsWin / 4 + 1;  // +1 word: consecutive slots start on consecutive banks
struct WinBytes {
  const uint8_t* w;  // LDS copy of [0, n)
  const uint8_t* g;  // the same bytes in global memory
  uint32_t n;
  __device__ uint32_t u8(uint64_t i) const { return i < n ? w[i] : g[i]; }
  __device__ uint32_t be16(uint64_t i) const { return i + 2 <= n ? (uint32_t)w[i] << 8 | w[i + 1] : ld_be16(g + i); }
  __device__ uint32_t be32(uint64_t i) const {
    return i + 4 <= n ? (uint32_t)w[i] << 24 | (uint32_t)w[i + 1] << 16 | (uint32_t)w[i + 2] << 8 | w[i + 3]
                      : ld_be32(g + i);
  }
  __device__ bool ascii(uint64_t i, uint64_t len) const {
    if (i + len > n) return bytes_ascii(g + i, len);
    uint32_t acc = 0;
    for (uint64_t j = 0; j < len; ++j) acc |= w[i + j];
    return acc < 0x80u;
  }
};

// One message's header, record checks and CRC jobs (job k = [jo[k], jo[k] + jl[k]) from the
// region start, its stored CRC ex[k]; records of 1..inline_max bytes leave ex[k] to the group
// phase). slot: this thread's LDS window for the properties. DESC: the transform's ASCII scan.
struct MsgParse {
  uint64_t jo[kMsgSlots] = {0, 0, 0, 0, 0}, jl[kMsgSlots] = {0, 0, 0, 0, 0};
  uint32_t ex[kMsgSlots] = {0, 0, 0, 0, 0};
  uint32_t status = 0;
  uint64_t end = 0;
};

// WIN = false: no LDS window; the properties are parsed from memory (the region-mode processors,
// whose region bytes were just streamed past and sit in the caches).
template <bool DESC, bool WIN = true>
__device__ __forceinline__ void parse_message(uint64_t off, bool in_region, uint64_t rem, const uint8_t* p,
                                              const HeaderWords& hw, const uint32_t* __restrict__ tbl,
                                              uint32_t* __restrict__ slot, uint64_t inline_max, MsgParse& r,
                                              PropsFields& pf, bool& pf_ok) {
  do {
    // the header's verdict and record spans (msg_header.h): nothing past the header is read before them
    MsgHeader H;
    MsgLayout L;
    r.status = in_region ? msg_decode(HeaderWordSrc{hw}, rem, HeaderWordCrc{hw, tbl}, &H) : (uint32_t)AMBRYCRC_MSG_BAD_LAYOUT;
    if (r.status == 0) r.status = msg_layout(H, rem, &L);
    if (r.status) break;
    r.end = L.end;
    const int32_t(&rel)[kMsgSlots] = H.rel;
    const uint64_t(&rend)[kMsgSlots] = L.rend;  // end of record k (its stored CRC's last byte + 1)
    if (!WIN && rel[1] != -1) {  // properties parsed from memory
      const uint8_t* q = p + rel[1];
      const uint64_t span = rend[1] - (uint64_t)rel[1];
      uint32_t ps = AMBRYCRC_MSG_BAD_RECORD;
      if (span >= 10) ps = ld_be16(q) != 1 ? AMBRYCRC_MSG_BAD_VERSION : props_parse_b<DESC>(MemBytes{q + 2}, span - 10, &pf);
      pf_ok = ps == 0;
      r.status |= ps;
    }
    if (WIN && rel[1] != -1) {  // properties: staged, then parsed (the transform's ASCII scan too: DESC)
      const uint8_t* q = p + rel[1];
      const uint64_t avail = rem - (uint64_t)rel[1];
      const uint32_t w = (uint32_t)(avail < kPropsWin ? avail : kPropsWin) & ~15u;
      uint32_t v[kPropsWin / 4];
#pragma unroll
      for (uint32_t j = 0; j < kPropsWin / 16; ++j)
        if (16 * j + 16 <= w) __builtin_memcpy(&v[4 * j], q + 16 * j, 16);  // one round trip
#pragma unroll
      for (uint32_t j = 0; j < kPropsWin / 4; ++j)
        if (4 * j + 4 <= w) slot[j] = v[j];
      const uint64_t span = rend[1] - (uint64_t)rel[1];
      uint32_t ps = AMBRYCRC_MSG_BAD_RECORD;
      if (span >= 10) {
        const uint32_t ver = w >= 2 ? (uint32_t)reinterpret_cast<const uint8_t*>(slot)[0] << 8 |
                                          reinterpret_cast<const uint8_t*>(slot)[1]
                                    : ld_be16(q);
        ps = ver != 1 ? AMBRYCRC_MSG_BAD_VERSION
                      : props_parse_b<DESC>(WinBytes{reinterpret_cast<const uint8_t*>(slot) + 2, q + 2,
                                                     w >= 2 ? w - 2 : 0u},
                                            span - 10, &pf);
      }
      pf_ok = ps == 0;
      r.status |= ps;
    }
    for (int k = 0; k < kMsgSlots; ++k) {
      if (rel[k] == -1) continue;
      const uint64_t e = rend[k];
      if (k != 1) r.status |= record_check(k, p + rel[k], e - (uint64_t)rel[k]);
      r.jo[k] = off + (uint64_t)rel[k];
      r.jl[k] = e - (uint64_t)rel[k] - 8;
      // Records the group phase takes whole have their stored CRC read there, from the line
      // it is already streaming (SweepArgs::exp_fill); only the others cost a fetch here.
      if (r.jl[k] == 0 || r.jl[k] > inline_max) {
        const uint64_t stored = ld_be64(p + e - 8);
        if (stored >> 32) r.status |= record_bit(k);  // a CRC32 never has upper bits: mismatch regardless
        r.ex[k] = (uint32_t)stored;
      }
    }
  } while (false);
}

// The end of the message the header describes (first record + total size), or 0 when the header
// is unparseable or the message overruns `rem` -- what parse_message would read up to, from the
// header words alone (no CRC check): the region-mode processors' wait target.
__device__ __forceinline__ uint64_t header_end(const HeaderWords& hw, uint64_t rem) {
  return msg_extent(HeaderWordSrc{hw}, rem);
}

}  // namespace ambrycrc
