// rekey_kernels.hip -- gfx950 kernels of the batched BlobIdTransformer (ambrycrc_rekey_messages_dev):
// BlobIdTransformer.transform / newMessage (ambry-replication/.../BlobIdTransformer.java:72-87,159-281)
// for many stored messages of a log region in HBM, each re-serialized under a converted store key.
//
// Pipeline (all on the caller's stream; ambrycrc_rekey.cpp):
//   (message verify)    msg_parse_kernel, the batch CRC engine, msg_reduce_kernel: every message's
//                       verify status, as ambrycrc_verify_messages_dev
//   rekey_plan_kernel   one thread per message: skipped / bad descriptors, then for a clean message
//                       the header and properties re-parsed (rekey.h rekey_plan), the refusals, the
//                       output's put descriptor and length, and the replacement content's CRC job
//   plan (scan)         exclusive scan of the output lengths; transform_place_kernel packs the
//                       messages and refuses the ones past out_cap
//   (batch CRC engine)  the replacement contents, one job a message over aux (empty for most)
//   rekey_write_kernel  one thread per message: header with its CRC, the properties record
//                       re-encoded and hashed from the bytes it writes, the blob record's head and
//                       trailer (the stored CRC moved to the new head by linearity, or the content's
//                       CRC extended over the head), and the four copy jobs of the bodies
//   plan (scan)         exclusive scan of the copy jobs' costs
//   gather_copy_kernel  cost-balanced copy of key, encryption-key record, user-metadata record (both
//                       whole, with their verified trailers) and blob content (put_kernels.hip)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ambrycrc.h"
#include "crc32_gf2.h"
#include "crc32_kernels.h"
#include "crc32_layout.h"
#include "crc_img.h"
#include "put_layout.h"
#include "record_fields.h"
#include "rekey.h"
#include "wave_tools.h"

namespace ambrycrc {

__global__ __launch_bounds__(256) void rekey_plan_kernel(RekeyArgs a) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.m; i += (uint64_t)gridDim.x * blockDim.x) {
    const ambrycrc_rekey_desc r = a.rdesc[i];
    uint32_t st = a.status[i];
    ambrycrc_put_desc d;
    __builtin_memset(&d, 0, sizeof d);  // header_version 0: nothing to write
    RekeyFix x;
    __builtin_memset(&x, 0, sizeof x);
    uint64_t out_len = 0, cjo = 0, cjl = 0;
    if (r.key_len == 0) {
      st = 0;  // the converter had no key: TransformationOutput(null), whatever the message holds
    } else if (!rekey_desc_ok(r, a.aux_len)) {
      st = AMBRYCRC_MSG_BAD_DESC;
    } else if (st == 0) {  // verified: the header and every record lie inside the region
      st = rekey_plan(a.region, a.msg_off[i], r, a.life != nullptr, a.life ? (int)a.life[i] : 0, a.header_version, &d,
                      &x);
      PutLayout L;
      if (st == 0 && put_layout(d, L)) {
        out_len = L.length;
        if (r.content_src != kRekeyKeep) {
          cjo = r.content_src;
          cjl = r.content_len;
        }
      } else {
        d.header_version = 0;
      }
    }
    a.desc[i] = d;
    a.fix[i] = x;
    a.out_len[i] = out_len;
    a.cjob_off[i] = cjo;
    a.cjob_len[i] = cjl;
    a.status[i] = st;
  }
}

// One CRC step over byte b through the LDS byte table (t[0..255] = T0, stage_slice_tables).
__device__ __forceinline__ uint32_t crc_step(const uint32_t* __restrict__ t, uint32_t c, uint32_t b) {
  return t[(c ^ b) & 0xffu] ^ (c >> 8);
}

__global__ __launch_bounds__(256) void rekey_write_kernel(RekeyArgs a) {
  __shared__ uint32_t tbl[1024];
  stage_slice_tables(tbl, a.img);
  __syncthreads();
  const uint64_t m = a.m;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const ambrycrc_put_desc d = a.desc[i];
    uint64_t src[kRekeySlots] = {0, 0, 0, 0}, dst[kRekeySlots] = {0, 0, 0, 0}, len[kRekeySlots] = {0, 0, 0, 0};
    PutLayout L;
    if (d.header_version != 0 && put_layout(d, L)) {  // placed (transform_place_kernel zeroes the version otherwise)
      const ambrycrc_rekey_desc r = a.rdesc[i];
      const RekeyFix x = a.fix[i];
      const bool repl = r.content_src != kRekeyKeep;
      uint8_t* msg = a.out + d.out_off;
      {  // header and its CRC, from the bytes in registers
        uint8_t h[32];
        const uint32_t hn = put_header_bytes(d, L, h);
        if (hn == 32) __builtin_memcpy(msg, h, 32);
        else if (hn == 30) __builtin_memcpy(msg, h, 30);
        else __builtin_memcpy(msg, h, 26);
        put_be64(msg + hn, (uint64_t)crc_regs_lds(tbl, 0u, h, hn));
      }
      {  // BlobProperties_Format_V1: version 1, the re-keyed VERSION_5 bytes, their CRC -- 8 B at a time
        const uint8_t* ps = a.region + d.props_src;
        uint8_t* pd = msg + L.bp_rel;
        put_be16(pd, 1u);
        pd += 2;
        uint32_t c = crc_step(tbl, crc_step(tbl, 0xFFFFFFFFu, 0u), 1u);
        const uint32_t n = d.props_len;
        for (uint32_t j0 = 0; j0 < n; j0 += 8) {
          uint64_t w = 0;
          if (j0 + 8 <= x.stored_len) {
            __builtin_memcpy(&w, ps + j0, 8);
          } else {
#pragma unroll
            for (uint32_t b = 0; b < 8; ++b)
              if (j0 + b < x.stored_len) w |= (uint64_t)ps[j0 + b] << (8 * b);
          }
          uint64_t o = 0;
#pragma unroll
          for (uint32_t b = 0; b < 8; ++b) {
            if (j0 + b < n) {
              const uint32_t v = rekey_props_byte(x, r, j0 + b, (uint8_t)(w >> (8 * b)));
              o |= (uint64_t)v << (8 * b);
              c = crc_step(tbl, c, v);
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
      {  // Blob_Format_V3 head and the record's CRC
        uint8_t h3[16];
        put_prefix_bytes(d, 4, h3);
        uint8_t* bd = msg + L.blob_rel;
        __builtin_memcpy(bd, h3, 13);
        uint32_t crc;
        if (repl) {
          // crc(head || content) = crc(head) x^(8|content|) + crc(content), the content hashed from aux
          crc = mul_xpow8_img(a.img, crc_regs_lds(tbl, 0u, h3, 13u), d.blob_len) ^ a.ccrc[i];
        } else {
          // the stored record verified: its CRC is the low word of its trailer; a head that changes
          // (V1 / V2 -> V3, or a non-canonical isCompressed byte) moves it by
          // (crc(old head) ^ crc(new head)) x^(8|content|), with no pass over the content
          const uint8_t* sb = a.region + d.blob_src;
          crc = ld_be32(sb + d.blob_len + 4);
          const uint8_t* sh = sb - x.blob_head;
          if (x.blob_head != 13 || sh[4] != h3[4]) {
            uint8_t oh[16];
#pragma unroll
            for (uint32_t b = 0; b < 16; ++b) oh[b] = b < x.blob_head ? sh[b] : 0;
            const uint32_t ca = crc_regs_lds(tbl, 0u, oh, (uint32_t)x.blob_head);
            const uint32_t cb = crc_regs_lds(tbl, 0u, h3, 13u);
            crc ^= mul_xpow8_img(a.img, ca ^ cb, d.blob_len);
          }
        }
        put_be64(bd + 13 + d.blob_len, (uint64_t)crc);
      }
      // the bodies: key from aux; the encryption-key and user-metadata records whole (prefix, body
      // and verified trailer are the output's bytes); the content from the region or aux
      src[0] = (uint64_t)(uintptr_t)(a.aux + d.key_src);
      dst[0] = d.out_off + L.hsize;
      len[0] = d.key_len;
      if (L.enc_rec) {
        src[1] = (uint64_t)(uintptr_t)(a.region + d.enckey_src - 6);
        dst[1] = d.out_off + (uint64_t)L.enc_rel;
        len[1] = L.enc_rec;
      }
      src[2] = (uint64_t)(uintptr_t)(a.region + d.usermeta_src - 6);
      dst[2] = d.out_off + (uint64_t)L.um_rel;
      len[2] = L.um_rec;
      src[3] = (uint64_t)(uintptr_t)((repl ? a.aux : a.region) + d.blob_src);
      dst[3] = d.out_off + (uint64_t)L.blob_rel + 13;
      len[3] = d.blob_len;
    }
#pragma unroll
    for (uint32_t k = 0; k < kRekeySlots; ++k) {
      a.cp_src[k * m + i] = src[k];
      a.cp_dst[k * m + i] = dst[k];
      a.cp_len[k * m + i] = len[k];
      a.cp_cost[k * m + i] = len[k] ? len[k] + kCopyJobCost : 0;
    }
  }
}

// Both kernels read a message's fields in dependent steps: as msg_parse_kernel, a capped grid (4
// blocks a CU) keeps a thread's lines in L2 between them.
hipError_t launch_rekey_plan(const RekeyArgs& a, int num_cu, hipStream_t s) {
  return launch_items(rekey_plan_kernel, blocks_for(a.m, num_cu, 4), 256, s, a);
}

hipError_t launch_rekey_write(const RekeyArgs& a, int num_cu, hipStream_t s) {
  return launch_items(rekey_write_kernel, blocks_for(a.m, num_cu, 4), 256, s, a);
}

}  // namespace ambrycrc
