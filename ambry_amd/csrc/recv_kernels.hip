// recv_kernels.hip -- gfx950 kernels of the batched GET receive (ambrycrc_receive_blobs_dev):
// GetBlobOperation.handleBody (ambry-router/.../GetBlobOperation.java:1113-1141, :1615-1694) for many
// payloads of a GetResponse body in HBM -- deserializeBlob / deserializeBlobAll, the content sliced to the
// request's range and filed where the caller wants it.
//
// Pipeline (all on the caller's stream; ambrycrc_recv.cpp):
//   msg_parse_kernel     ALL only, the verify's parse: header verdicts, record checks, message ends
//   recv_plan_kernel     one thread per payload: recv.h recv_plan -- the refusals, the info fields, the
//                        slice length, and the CRC jobs: the blob record's content before the slice, the
//                        slice, the content after it; under ALL the three other records, hashed only.
//                        Under BLOB it reads the record's head itself (<= 13 B: no parse kernel ahead)
//   plan (scan)          packed only: exclusive scan of the slice lengths
//   recv_place_kernel    one thread per payload: the slice's place (AMBRYCRC_MSG_NO_ROOM past out_cap, a
//                        packed offset still advancing) and the slice job's copy destination
//   (batch CRC engine)   the copy-through sweep over the jobs: every byte read once, hashed, and the
//                        slices written
//   recv_finish_kernel   one thread per payload: the blob record's CRC from its head (hashed here) and
//                        the pieces' CRCs, crc(A || B) = crc(A) x^(8|B|) + crc(B), against the stored long;
//                        under ALL the other records' CRCs against theirs
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ambrycrc.h"
#include "crc32_kernels.h"
#include "crc_img.h"
#include "recv.h"
#include "wave_tools.h"

namespace ambrycrc {

__global__ __launch_bounds__(256) void recv_plan_kernel(RecvArgs a) {
  const uint64_t m = a.m;
  const bool all = a.flag == AMBRYCRC_SEND_ALL;
  const uint32_t slots = recv_slots(a.flag);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t off = a.pay_off[i];
    const bool has_size = a.pay_size != nullptr;
    const uint64_t size = has_size ? a.pay_size[i] : 0;
    const uint64_t lo = a.range ? a.range[2 * i] : 0;
    const uint64_t hi = a.range ? a.range[2 * i + 1] : kRecvToEnd;
    uint64_t avail;
    const bool in_body = recv_extent(off, has_size, size, a.body_len, &avail);  // a payload outside is never dereferenced
    const uint8_t* p = a.body + (in_body ? off : 0);
    MsgHeader D;
    MsgLayout L;
    __builtin_memset(&D, 0, sizeof D);
    __builtin_memset(&L, 0, sizeof L);
    uint32_t hdr = 0, rec_bits = 0;
    if (all && in_body) {
      // the header inside the payload's own bytes: what precedes the CRC in msg_decode first, then the
      // parse's verdict on the CRC (it judged the header against the body's end, which lies no nearer),
      // then the constraints over avail
      const uint32_t vs = a.vstatus[i];
      hdr = msg_decode(HeaderBytes{p}, avail, NoCrc{}, &D);
      if (hdr == 0) {
        if (a.msg_end[i] == 0) hdr = vs ? vs : (uint32_t)AMBRYCRC_MSG_BAD_LAYOUT;
        else hdr = msg_layout(D, avail, &L);
      }
      rec_bits = vs & (AMBRYCRC_MSG_BAD_VERSION | AMBRYCRC_MSG_BAD_RECORD);
    }
    RecvPlan s;
    recv_plan(p, in_body, avail, a.flag, hdr, L, D.version, rec_bits, lo, hi, &s);
    a.info[i] = s.info;
    a.status[i] = s.status;
    a.len[i] = s.info.out_len;  // (0 when refused)
#pragma unroll
    for (uint32_t k = 0; k < kRecvSlotsAll; ++k) {
      if (k >= slots) break;
      const uint64_t j = (uint64_t)k * m + i;
      a.job_off[j] = s.status ? 0 : off + s.job_off[k];
      a.job_len[j] = s.job_len[k];
      a.copy_off[j] = kCopySkip;
    }
  }
}

__global__ __launch_bounds__(256) void recv_place_kernel(RecvArgs a) {
  const uint64_t m = a.m;
  const uint32_t slots = recv_slots(a.flag);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    if (a.status[i]) continue;
    const uint64_t len = a.len[i];
    const uint64_t at = a.dst_off ? a.dst_off[i] : a.start[i];
    if (recv_fits(at, len, a.out_cap)) {
      a.info[i].out_off = at;
      if (len) a.copy_off[(uint64_t)kRecvSlice * m + i] = at;
      continue;
    }
    ambrycrc_recv_info o;
    __builtin_memset(&o, 0, sizeof o);
    o.out_off = kRecvNowhere;
    a.info[i] = o;
    a.status[i] = AMBRYCRC_MSG_NO_ROOM;
#pragma unroll
    for (uint32_t k = 0; k < kRecvSlotsAll; ++k) {  // nothing of it is read
      if (k >= slots) break;
      a.job_off[(uint64_t)k * m + i] = 0;
      a.job_len[(uint64_t)k * m + i] = 0;
    }
  }
}

__global__ __launch_bounds__(256) void recv_finish_kernel(RecvArgs a) {
  const uint64_t m = a.m;
  const uint32_t* img = a.img;
  const bool all = a.flag == AMBRYCRC_SEND_ALL;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    if (a.status[i]) continue;
    // the blob record: head, then the three content pieces in order
    const uint64_t content = a.job_off[(uint64_t)kRecvBefore * m + i];
    const uint32_t head = blob_head((int)a.info[i].blob_version);
    uint64_t jl[3];
    uint32_t jc[3];
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
      jl[k] = a.job_len[(uint64_t)k * m + i];
      jc[k] = a.crc[(uint64_t)k * m + i];
    }
    uint32_t c = crc_bytes_img(img, 0u, a.body + content - head, head);
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k)
      if (jl[k]) c = mul_xpow8_img(img, c, jl[k]) ^ jc[k];
    // the stored long: a non-zero upper word never matches
    uint32_t bits = ld_be64(a.body + content + jl[0] + jl[1] + jl[2]) != (uint64_t)c ? (uint32_t)AMBRYCRC_MSG_BLOB_CRC : 0u;
    if (all) {
#pragma unroll
      for (uint32_t k = kRecvEnckey; k < kRecvSlotsAll; ++k) {
        const uint64_t j = (uint64_t)k * m + i;
        const uint64_t n = a.job_len[j];
        if (n && ld_be64(a.body + a.job_off[j] + n) != (uint64_t)a.crc[j]) bits |= recv_record_bit(k);
      }
    }
    a.status[i] = bits;
  }
}

// As send's thread-per-message kernels: a capped grid (4 blocks a CU) that loops.
hipError_t launch_recv_plan(const RecvArgs& a, int num_cu, hipStream_t s) {
  return launch_items(recv_plan_kernel, blocks_for(a.m, num_cu, 4), 256, s, a);
}

hipError_t launch_recv_place(const RecvArgs& a, int num_cu, hipStream_t s) {
  return launch_items(recv_place_kernel, blocks_for(a.m, num_cu, 4), 256, s, a);
}

hipError_t launch_recv_finish(const RecvArgs& a, int num_cu, hipStream_t s) {
  return launch_items(recv_finish_kernel, blocks_for(a.m, num_cu, 4), 256, s, a);
}

}  // namespace ambrycrc
