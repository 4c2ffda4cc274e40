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
#include "put_emit.h"
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

// Five waves a SIMD, as before the writers were shared (put_emit.h): left to itself the allocator takes two or
// three VGPRs past the 96 that allow them.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void rekey_write_kernel(RekeyArgs a) {
  __shared__ uint32_t tbl[1024];
  stage_slice_tables(tbl, a.img);
  __syncthreads();
  const uint64_t m = a.m;
  const auto crc16 = [&](const uint8_t(&b)[16], uint32_t n) { return crc_regs_lds(tbl, 0u, b, n); };
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const ambrycrc_put_desc d = a.desc[i];
    uint64_t src[kRekeySlots] = {0, 0, 0, 0}, dst[kRekeySlots] = {0, 0, 0, 0}, len[kRekeySlots] = {0, 0, 0, 0};
    PutLayout L;
    if (d.header_version != 0 && put_layout(d, L)) {  // placed (transform_place_kernel zeroes the version otherwise)
      const ambrycrc_rekey_desc r = a.rdesc[i];
      const RekeyFix x = a.fix[i];
      const bool repl = r.content_src != kRekeyKeep;
      uint8_t* msg = a.out + d.out_off;
      put_emit_header<true>(tbl, d, L, msg);
      // BlobProperties_Format_V1: the re-keyed VERSION_5 bytes
      put_emit_props(tbl, a.region + d.props_src, x.stored_len, msg + L.bp_rel, d.props_len,
                     [&](uint32_t j, uint8_t stored) { return rekey_props_byte(x, r, j, stored); });
      if (repl) {  // Blob_Format_V3 over the content hashed from aux
        put_emit_record<4>(tbl, a.img, d, L, msg, &a.ccrc[i]);
      } else {  // ... or over the stored record's content, whose record verified: its CRC moved to the new head
        uint8_t h3[16];
        put_prefix_bytes(d, 4, h3);
        uint8_t* bd = msg + L.blob_rel;
        __builtin_memcpy(bd, h3, 13);
        const uint8_t* sb = a.region + d.blob_src;
        put_be64(bd + 13 + d.blob_len, (uint64_t)blob_crc_moved(crc16, a.img, sb - x.blob_head, x.blob_head, h3,
                                                                ld_be32(sb + d.blob_len + 4), d.blob_len));
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
    store_copy_jobs(a.cp_src, a.cp_dst, a.cp_len, a.cp_cost, m, i, src, dst, len);
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
