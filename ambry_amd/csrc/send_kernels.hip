// send_kernels.hip -- gfx950 kernels of the batched MessageFormatSend (ambrycrc_send_messages_dev):
// MessageFormatSend.fetchDataFromReadSet (ambry-messageformat/.../MessageFormatSend.java:112-242) for
// many stored messages of a log region in HBM under one MessageFormatFlags value.
//
// Pipeline (all on the caller's stream; ambrycrc_send.cpp):
//   msg_parse_kernel     the verify's parse: header verdicts, message ends, five CRC jobs a message
//   (batch CRC engine)   the slot-0 jobs alone -- the encryption-key records, ~100 B each -- so that
//                        deserializeBlobEncryptionKey's verdict is known before anything is placed
//                        (not under ALL and BLOB_PROPERTIES, which never read that record)
//   send_plan_kernel     one thread per message: send.h send_plan -- the refusals, the span, the info
//                        fields, and for each job: copied to where in the span, hashed only, or emptied
//                        (a record the flag does not send and the reference does not read)
//   plan (scan)          exclusive scan of the span lengths
//   send_jobs_kernel     one thread per message: the packed placement (AMBRYCRC_MSG_NO_ROOM past
//                        out_cap, the running offset still advancing), every job's destination in the
//                        output, and the plain copy of a message that goes whole
//   (batch CRC engine)   the copy-through sweep over the 5m jobs: each sent record read once, hashed
//                        and written; msg_reduce_kernel turns the CRCs into the verify's bits
//   plan + gather_copy   only with a size given under ALL: the messages that go whole without jobs
//   send_finish_kernel   one thread per message: the final check bits, and the bytes no job covers --
//                        each sent record's 8-B trailer, under ALL the header and the store key
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ambrycrc.h"
#include "crc32_kernels.h"
#include "send.h"
#include "wave_tools.h"

namespace ambrycrc {

static_assert(kSendHash == kCopySkip, "a hashed-only slot is the sweep's kCopySkip");

__global__ __launch_bounds__(256) void send_plan_kernel(SendArgs a) {
  const uint64_t m = a.m;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t off = a.msg_off[i];
    const bool in_region = off <= a.region_len;  // an offset past the region is refused, never dereferenced
    const uint64_t rem = in_region ? a.region_len - off : 0;
    const uint8_t* p = a.region + (in_region ? off : 0);
    const bool has_size = a.msg_size != nullptr;
    const uint64_t size = has_size ? a.msg_size[i] : 0;
    // the parse's verdict on the header: a message end of 0 is a header that did not parse, its status
    // then the header's bit alone; otherwise the fields are re-read from the lines the parse left in L2
    SendHeader H;
    __builtin_memset(&H, 0, sizeof H);
    uint32_t hdr = 0;
    if (a.msg_end[i] == 0) {
      hdr = a.vstatus[i];
      if (hdr == 0) hdr = AMBRYCRC_MSG_BAD_LAYOUT;
    } else {
      MsgHeader D;  // (its CRC verified by the parse)
      hdr = msg_decode(HeaderBytes{p}, rem, NoCrc{}, &D);
      if (hdr == 0) hdr = msg_layout(D, rem, &H);
    }
    bool enc_bad = false;
    if (a.enc_crc && hdr == 0 && H.rel[0] != -1)  // the stored long against the CRC of [rel, rend - 8)
      enc_bad = ld_be64(p + H.rend[0] - 8) != (uint64_t)a.enc_crc[i];
    SendPlan s;
    send_plan(p, in_region, rem, has_size, size, a.flag, hdr, H, enc_bad, &s);
    ambrycrc_send_info o;
    o.out_off = kSendNowhere;
    o.send_len = s.status ? 0 : s.send_len;
    o.rel_off = s.status ? 0u : s.rel_off;
    o.enckey_rel = s.status ? 0u : s.enckey_rel;
    o.enckey_len = s.status ? 0u : s.enckey_len;
    o.check = s.status ? 0u : s.pre;
    a.info[i] = o;
    a.status[i] = s.status;
    a.len[i] = o.send_len;
#pragma unroll
    for (int k = 0; k < kMsgSlots; ++k) {
      const uint64_t j = (uint64_t)k * m + i;
      const uint64_t d = s.status ? kSendNone : s.dst[k];
      if (d == kSendNone) {  // not read: an empty job, whose CRC (0) equals its expected value
        a.job_off[j] = 0;
        a.job_len[j] = 0;
        a.expected[j] = 0;
        a.copy_off[j] = kCopySkip;
      } else {
        a.copy_off[j] = d;
      }
    }
    if (a.g_src) {
      a.g_src[i] = (uint64_t)(uintptr_t)p;
      a.g_len[i] = !s.status && s.whole ? s.send_len : 0;
    }
  }
}

__global__ __launch_bounds__(256) void send_jobs_kernel(SendArgs a) {
  const uint64_t m = a.m;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t len = a.len[i];
    uint64_t at = kSendNowhere;
    if (len) {
      const uint64_t st = a.start[i];
      if (st <= a.out_cap && len <= a.out_cap - st) {
        at = st;
      } else {
        a.status[i] |= AMBRYCRC_MSG_NO_ROOM;
        a.info[i].send_len = 0;
      }
    }
    a.info[i].out_off = at;
#pragma unroll
    for (int k = 0; k < kMsgSlots; ++k) {
      const uint64_t j = (uint64_t)k * m + i;
      const uint64_t c = a.copy_off[j];
      if (c != kCopySkip) a.copy_off[j] = at != kSendNowhere ? at + c : kCopySkip;
    }
    if (a.g_src) {
      const uint64_t gl = at != kSendNowhere ? a.g_len[i] : 0;
      a.g_dst[i] = gl ? at : 0;
      a.g_len[i] = gl;
      a.g_cost[i] = copy_job_cost(gl);
    }
  }
}

// n >= 8 bytes by 8-B moves at any alignment, four loads in flight before their stores; the last
// piece is [n - 8, n), overlapping the one before (transform_finish_kernel's key copy).
__device__ __forceinline__ void move8(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint64_t n) {
  for (uint64_t b0 = 0; b0 < n; b0 += 32) {
    uint64_t v[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) __builtin_memcpy(&v[u], src + min(b0 + 8 * u, n - 8), 8);
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) __builtin_memcpy(dst + min(b0 + 8 * u, n - 8), &v[u], 8);
  }
}

__global__ __launch_bounds__(256) void send_finish_kernel(SendArgs a) {
  const uint64_t m = a.m;
  const uint32_t mask = send_check_mask(a.flag);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t st = a.status[i];
    const uint64_t at = a.info[i].out_off;
    a.info[i].check = (st & ~(uint32_t)AMBRYCRC_MSG_NO_ROOM) ? 0u : ((a.vstatus[i] & mask) | a.info[i].check);
    if (at == kSendNowhere) continue;
    // the trailers of the records the sweep copied (a job ends where its stored CRC starts)
    uint64_t lowest = kCopySkip;
#pragma unroll
    for (int k = 0; k < kMsgSlots; ++k) {
      const uint64_t j = (uint64_t)k * m + i;
      const uint64_t c = a.copy_off[j];
      if (c == kCopySkip) continue;
      const uint64_t jl = a.job_len[j];
      uint64_t t;
      __builtin_memcpy(&t, a.region + a.job_off[j] + jl, 8);
      __builtin_memcpy(a.out + c + jl, &t, 8);
      lowest = c < lowest ? c : lowest;
    }
    // ALL: header and store key, the bytes ahead of the first record (34 B at least)
    if (a.flag == AMBRYCRC_SEND_ALL && lowest != kCopySkip) move8(a.out + at, a.region + a.msg_off[i], lowest - at);
  }
}

// As the re-key's thread-per-message kernels: a capped grid (4 blocks a CU) that loops keeps a
// thread's lines in L2 between its dependent reads.
hipError_t launch_send_plan(const SendArgs& a, int num_cu, hipStream_t s) {
  return launch_items(send_plan_kernel, blocks_for(a.m, num_cu, 4), 256, s, a);
}

hipError_t launch_send_jobs(const SendArgs& a, int num_cu, hipStream_t s) {
  return launch_items(send_jobs_kernel, blocks_for(a.m, num_cu, 4), 256, s, a);
}

hipError_t launch_send_finish(const SendArgs& a, int num_cu, hipStream_t s) {
  return launch_items(send_finish_kernel, blocks_for(a.m, num_cu, 4), 256, s, a);
}

}  // namespace ambrycrc
