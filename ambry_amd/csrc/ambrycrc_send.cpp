// ambrycrc_send.cpp -- batched MessageFormatSend over a device-resident log region
// (ambrycrc_send_messages_dev): MessageFormatSend.fetchDataFromReadSet
// (ambry-messageformat/.../MessageFormatSend.java:112-242). Kernels: send_kernels.hip; the shared
// per-message rules: send.h; the per-message CPU entry: ambrycrc_msg_cpu.cpp. A plain pipeline on the
// caller's stream, in job mode: parse, the encryption-key CRCs, plan, place, the copy-through CRC pass,
// finish.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "../../include/ambrycrc.h"
#include "ambrycrc_ctx.h"
#include "crc32_kernels.h"
#include "send.h"

using namespace ambrycrc;
using namespace ambrycrc::detail;

namespace {

// Workspace of m messages, 8-B arrays first: span lengths, message ends, the 5m copy destinations, the
// plain-copy jobs (src, dst, len, cost); then the 4-B ones: the verify's status, the encryption-key CRCs,
// the two scans' per-entry outputs. After it the verify's workspace: its job arrays, then the batch
// area, which the slot-0 batch, the two scans and the CRC pass use in turn (one stream, one after another).
size_t send_own_bytes(size_t m) {
  return (m * ((2 + (size_t)kSendSlots + 4) * sizeof(uint64_t) + 4 * sizeof(uint32_t)) + 255) & ~size_t(255);
}

// The plan kernel's exclusive scan of len[0..n) into byte_start (no small-chunk classes).
PlanArgs scan_args(const uint64_t* off, const uint64_t* len, size_t n, void* ws, uint32_t* out) {
  PlanArgs p;
  p.gate = nullptr;
  p.off = off;
  p.len = len;
  p.crc_in = nullptr;
  p.n = (uint32_t)n;
  p.byte_start = static_cast<uint64_t*>(ws);
  const size_t blocks = (n + kPlanPerBlock - 1) / kPlanPerBlock;
  p.block_sum = p.byte_start + n + 1;
  p.block_small = p.block_sum + blocks;
  p.small_total = p.block_small + blocks;
  p.small_idx = reinterpret_cast<uint32_t*>(p.small_total + 5);
  p.crc_stage = nullptr;
  p.out = out;
  p.small_max = 0;
  return p;
}

}  // namespace

extern "C" {

size_t ambrycrc_send_workspace_bytes(size_t m) { return send_own_bytes(m) + ambrycrc_messages_workspace_bytes(m); }

int ambrycrc_send_messages_dev(const uint8_t* d_region, uint64_t region_len, const uint64_t* d_msg_off,
                               const uint64_t* d_msg_size, size_t m, int flag, uint8_t* d_out, uint64_t out_cap,
                               ambrycrc_send_info* d_info, uint32_t* d_status, void* d_ws, size_t ws_bytes,
                               hipStream_t stream) {
  if (m == 0) return AMBRYCRC_OK;
  if (!d_region || !d_msg_off || !d_out || !d_info || !d_status || !send_flag_ok(flag) ||
      (size_t)kMsgSlots * m >= (1ull << 31))
    return AMBRYCRC_EINVAL;
  DevCtx* c = ctx_current();
  if (!c) return AMBRYCRC_ENOINIT;
  WsLease lease;
  int rc = lease.acquire(c, stream, &d_ws, ws_bytes, ambrycrc_send_workspace_bytes(m));
  if (rc) return rc;
  uint8_t* w = static_cast<uint8_t*>(d_ws);
  uint64_t* len = reinterpret_cast<uint64_t*>(w);
  uint64_t* msg_end = len + m;
  uint64_t* copy_off = msg_end + m;
  uint64_t* g = copy_off + (size_t)kSendSlots * m;
  uint32_t* vstatus = reinterpret_cast<uint32_t*>(g + 4 * m);
  uint32_t* enc_crc = vstatus + m;
  uint32_t* scan_out = enc_crc + m;
  uint32_t* gscan_out = scan_out + m;
  void* shared = w + send_own_bytes(m);
  const bool whole_copies = flag == AMBRYCRC_SEND_ALL && d_msg_size != nullptr;
  const bool enc_first = send_reads_enckey(flag);

  // 1. the verify's parse (job mode): header verdicts, message ends, the five jobs a message
  MsgStage ms;
  rc = enqueue_messages_parse(c, d_region, region_len, d_msg_off, m, vstatus, msg_end, shared, stream, &ms);
  if (rc) return rc;
  // 2. the encryption-key records' CRCs, ahead of the placement: a bad one refuses its message
  if (enc_first) {
    rc = enqueue_batch(c, d_region, ms.a.job_off, ms.a.job_len, nullptr, enc_crc, m, ms.batch_ws, stream);
    if (rc) return rc;
  }
  // 3. the rules of send.h: status, info, span lengths, each job copied / hashed / emptied
  SendArgs a;
  a.region = d_region;
  a.region_len = region_len;
  a.msg_off = d_msg_off;
  a.msg_size = d_msg_size;
  a.m = m;
  a.flag = flag;
  a.out = d_out;
  a.out_cap = out_cap;
  a.info = d_info;
  a.status = d_status;
  a.vstatus = vstatus;
  a.msg_end = msg_end;
  a.job_off = ms.a.job_off;
  a.job_len = ms.a.job_len;
  a.expected = ms.a.expected;
  a.enc_crc = enc_first ? enc_crc : nullptr;
  a.len = len;
  a.copy_off = copy_off;
  a.g_src = whole_copies ? g : nullptr;
  a.g_dst = g + m;
  a.g_len = g + 2 * m;
  a.g_cost = g + 3 * m;
  const PlanArgs p = scan_args(d_msg_off, len, m, ms.batch_ws, scan_out);
  a.start = p.byte_start;
  if (launch_send_plan(a, stream) != hipSuccess) return AMBRYCRC_EHIP;
  // 4. packed placement: exclusive scan of the span lengths, then every job's destination
  if (launch_plan(p, stream) != hipSuccess) return AMBRYCRC_EHIP;
  if (launch_send_jobs(a, stream) != hipSuccess) return AMBRYCRC_EHIP;
  // 5. the verify's CRC pass as a copy-through: every sent record read once, hashed and written
  rc = enqueue_messages_check(c, ms, stream, d_out, copy_off);
  if (rc) return rc;
  // 6. a size given under ALL: the messages that go whole without jobs (none, for nearly every batch)
  if (whole_copies) {
    const PlanArgs q = scan_args(a.g_dst, a.g_cost, m, ms.batch_ws, gscan_out);
    if (launch_plan(q, stream) != hipSuccess) return AMBRYCRC_EHIP;
    CopyArgs ca;
    ca.src = a.g_src;
    ca.dst_off = a.g_dst;
    ca.len = a.g_len;
    ca.start = q.byte_start;
    ca.n = (uint32_t)m;
    ca.dst = d_out;
    ca.gate = nullptr;
    if (launch_gather_copy(ca, c->num_cu * 8, stream) != hipSuccess) return AMBRYCRC_EHIP;
  }
  // 7. the final check bits, the trailers, and under ALL the headers and store keys
  return hip_err(launch_send_finish(a, stream));
}

}  // extern "C"
