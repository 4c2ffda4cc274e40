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
  // the own area, then the verify's workspace: its job arrays, then the batch area, which the slot-0 batch,
  // the two scans and the CRC pass use in turn (one stream, one after another)
  Carver k(d_ws);
  SendArgs a;
  const SendOwn w = send_own(k, m, a);
  void* shared = k.here();
  const bool whole_copies = flag == AMBRYCRC_SEND_ALL && d_msg_size != nullptr;
  const bool enc_first = send_reads_enckey(flag);

  // 1. the verify's parse (job mode): header verdicts, message ends, the five jobs a message
  MsgStage ms;
  rc = enqueue_messages_parse(c, d_region, region_len, d_msg_off, m, w.vstatus, w.msg_end, shared, stream, &ms);
  if (rc) return rc;
  // 2. the encryption-key records' CRCs, ahead of the placement: a bad one refuses its message
  if (enc_first) {
    rc = enqueue_batch(c, d_region, ms.a.job_off, ms.a.job_len, nullptr, w.enc_crc, m, ms.batch_ws, stream);
    if (rc) return rc;
  }
  // 3. the rules of send.h: status, info, span lengths, each job copied / hashed / emptied
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
  a.job_off = ms.a.job_off;
  a.job_len = ms.a.job_len;
  a.expected = ms.a.expected;
  if (!enc_first) a.enc_crc = nullptr;
  if (!whole_copies) a.g_src = nullptr;
  const PlanArgs p = plan_scan_args(d_msg_off, a.len, m, ms.batch_ws, w.scan_out);
  a.start = p.byte_start;
  if (launch_send_plan(a, c->num_cu, stream) != hipSuccess) return AMBRYCRC_EHIP;
  // 4. packed placement: exclusive scan of the span lengths, then every job's destination
  if (launch_plan(p, stream) != hipSuccess) return AMBRYCRC_EHIP;
  if (launch_send_jobs(a, c->num_cu, stream) != hipSuccess) return AMBRYCRC_EHIP;
  // 5. the verify's CRC pass as a copy-through: every sent record read once, hashed and written
  rc = enqueue_messages_check(c, ms, stream, d_out, a.copy_off);
  if (rc) return rc;
  // 6. a size given under ALL: the messages that go whole without jobs (none, for nearly every batch)
  if (whole_copies) {
    rc = enqueue_scan_copy(c, a.g_src, a.g_dst, a.g_len, a.g_cost, m, d_out, ms.batch_ws, w.gscan_out, nullptr, stream);
    if (rc) return rc;
  }
  // 7. the final check bits, the trailers, and under ALL the headers and store keys
  return hip_err(launch_send_finish(a, c->num_cu, stream));
}

}  // extern "C"
