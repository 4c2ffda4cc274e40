// ingest_kernels.hip -- gfx950 kernels of the batched PutRequest ingest (ambrycrc_ingest_put_requests_dev):
// PutRequest.readFrom (ambry-protocol/.../PutRequest.java:191-204, :440-521) and
// AmbryRequests.getMessageFormatWriteSet (AmbryRequests.java:1957-1970) for many frames of a wire
// buffer in HBM, each checked against the CRC it carries and written as a stored PUT message.
//
// Pipeline (all on the caller's stream; ambrycrc_ingest.cpp):
//   ingest_plan_kernel     one thread per request: the reference and the frame parsed (put_request.h
//                          ingest_parse), the three fixed pieces of the CRC'd span hashed from
//                          registers, the request's five CRC jobs over the wire buffer
//   (batch CRC engine)     the 5m jobs: every wire byte hashed once
//   ingest_verdict_kernel  one thread per request: the wire CRC combined from the jobs' CRCs and the
//                          fixed pieces' (no second read), compared with the stored long; the other
//                          refusals; the output's put descriptor and length
//   plan (scan)            exclusive scan of the output lengths; transform_place_kernel packs the
//                          messages and refuses the ones past out_cap
//   ingest_write_kernel    one thread per placed request: header with its CRC, the record heads, the
//                          properties record re-encoded and hashed from the bytes it writes, the other
//                          trailers from the jobs' CRCs extended over the record heads, the
//                          MessageInfo, and the four copy jobs of the bodies
//   plan (scan)            exclusive scan of the copy jobs' costs
//   gather_copy_kernel     cost-balanced copy of blob id, encryption key, user metadata and blob content
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ambrycrc.h"
#include "crc32_gf2.h"
#include "crc32_kernels.h"
#include "crc32_layout.h"
#include "crc_img.h"
#include "put_emit.h"
#include "put_layout.h"
#include "put_request.h"
#include "record_fields.h"
#include "wave_tools.h"

namespace ambrycrc {

__global__ __launch_bounds__(256) void ingest_plan_kernel(IngestArgs a) {
  __shared__ uint32_t tbl[1024];
  stage_slice_tables(tbl, a.img);
  __syncthreads();
  const uint64_t m = a.m;
  const auto crc = [&](const uint8_t(&b)[12], uint32_t n) { return crc_regs_lds(tbl, 0u, b, n); };
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    IngestPlan p;
    const uint32_t st = ingest_parse(a.wire, a.wire_len, a.req[i], crc, &p);
    uint64_t off[kIngestSegs] = {0, 0, 0, 0, 0}, len[kIngestSegs] = {0, 0, 0, 0, 0};
    if (st == 0) ingest_segments(p, off, len);
    else p.req_version = 0;
    a.plan[i] = p;
    a.status[i] = st;
#pragma unroll
    for (uint32_t k = 0; k < kIngestSegs; ++k) {
      a.job_off[k * m + i] = off[k];
      a.job_len[k * m + i] = len[k];
    }
  }
}

__global__ __launch_bounds__(256) void ingest_verdict_kernel(IngestArgs a) {
  const uint64_t m = a.m;
  const uint32_t* img = a.img;
  const auto mul = [&](uint32_t v, uint64_t n) { return mul_xpow8_img(img, v, n); };
  // the packed length starts at 0 for ingest_write_kernel, two launches on: a store here, not a
  // memset between the kernels, so that a captured call holds kernel nodes only
  if (a.total && blockIdx.x == 0 && threadIdx.x == 0) *a.total = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t st = a.status[i];
    ambrycrc_put_desc d;
    __builtin_memset(&d, 0, sizeof d);  // header_version 0: nothing to write
    uint64_t out_len = 0;
    uint32_t wcrc = 0;
    if (st == 0) {
      const IngestPlan p = a.plan[i];
      uint32_t seg[kIngestSegs];
#pragma unroll
      for (uint32_t k = 0; k < kIngestSegs; ++k) seg[k] = a.seg[k * m + i];
      wcrc = ingest_wire_crc(p, seg, mul);
      st = ingest_verdict(a.wire, p, wcrc, a.header_version, &d);
      PutLayout L;
      if (st == 0 && put_layout(d, L)) out_len = L.length;
      else d.header_version = 0;
    }
    a.desc[i] = d;
    a.out_len[i] = out_len;
    a.status[i] = st;
    if (a.wire_crc) a.wire_crc[i] = wcrc;
  }
}

// Five waves a SIMD, as before the writers were shared (put_emit.h): left to itself the allocator takes two or
// three VGPRs past the 96 that allow them.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void ingest_write_kernel(IngestArgs a) {
  __shared__ uint32_t tbl[1024];
  stage_slice_tables(tbl, a.img);
  __syncthreads();
  const uint64_t m = a.m;
  uint64_t top = 0;  // the end of the last message this thread placed
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const ambrycrc_put_desc d = a.desc[i];
    uint64_t src[kIngestSlots] = {0, 0, 0, 0}, dst[kIngestSlots] = {0, 0, 0, 0}, len[kIngestSlots] = {0, 0, 0, 0};
    ambrycrc_message_info info;
    __builtin_memset(&info, 0, sizeof info);
    PutLayout L;
    if (d.header_version != 0 && put_layout(d, L)) {  // placed (transform_place_kernel zeroes the version otherwise)
      const IngestPlan p = a.plan[i];
      uint8_t* msg = a.out + d.out_off;
      top = d.out_off + L.length;
      put_emit_header<true>(tbl, d, L, msg);
      // each record of head || body from its head and the body's CRC, hashed on the wire; the properties
      // written again at VERSION_5 and hashed from the bytes written
      if (L.enc_rec) put_emit_record<1>(tbl, a.img, d, L, msg, &a.seg[3 * m + i]);
      const PropsFix x = ingest_props_fix(p);
      put_emit_props(tbl, a.wire + d.props_src, x.stored_len, msg + L.bp_rel, d.props_len,
                     [&](uint32_t j, uint8_t stored) { return props_v5_byte(x, j, stored); });
      put_emit_record<3>(tbl, a.img, d, L, msg, &a.seg[2 * m + i]);
      put_emit_record<4>(tbl, a.img, d, L, msg, &a.seg[4 * m + i]);
      ingest_info(a.wire, p, d, L, d.out_off, &info);
      src[0] = (uint64_t)(uintptr_t)(a.wire + d.key_src);
      dst[0] = d.out_off + L.hsize;
      len[0] = d.key_len;
      if (L.enc_rec) {
        src[1] = (uint64_t)(uintptr_t)(a.wire + d.enckey_src);
        dst[1] = d.out_off + (uint64_t)L.enc_rel + 6;
        len[1] = (uint64_t)d.enckey_len;
      }
      src[2] = (uint64_t)(uintptr_t)(a.wire + d.usermeta_src);
      dst[2] = d.out_off + (uint64_t)L.um_rel + 6;
      len[2] = d.usermeta_len;
      src[3] = (uint64_t)(uintptr_t)(a.wire + d.blob_src);
      dst[3] = d.out_off + (uint64_t)L.blob_rel + 13;
      len[3] = d.blob_len;
    }
    if (a.info) a.info[i] = info;
    store_copy_jobs(a.cp_src, a.cp_dst, a.cp_len, a.cp_cost, m, i, src, dst, len);
  }
  if (a.total) {  // every lane is back from its loop: one atomic a wave that placed something
    const uint64_t w = wave_max_u64(top);
    if (w && (threadIdx.x & 63u) == 0) atomicMax(a.total, (unsigned long long)w);
  }
}

// The three kernels read a request's fields in dependent steps: as rekey's, a capped grid (4 blocks a
// CU) keeps a thread's lines in L2 between them.
constexpr uint32_t kIngestBlocksPerCu = 4;

hipError_t launch_ingest_plan(const IngestArgs& a, int num_cu, hipStream_t s) {
  return launch_items(ingest_plan_kernel, blocks_for(a.m, num_cu, kIngestBlocksPerCu), 256, s, a);
}

// (with a packed length to zero, at least one block even for no request)
hipError_t launch_ingest_verdict(const IngestArgs& a, int num_cu, hipStream_t s) {
  const uint32_t blocks = blocks_for(a.m, num_cu, kIngestBlocksPerCu);
  return launch_items(ingest_verdict_kernel, blocks == 0 && a.total ? 1u : blocks, 256, s, a);
}

hipError_t launch_ingest_write(const IngestArgs& a, int num_cu, hipStream_t s) {
  return launch_items(ingest_write_kernel, blocks_for(a.m, num_cu, kIngestBlocksPerCu), 256, s, a);
}

}  // namespace ambrycrc
