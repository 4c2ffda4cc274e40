// ambrycrc_recv.cpp -- batched GET receive over a device-resident GetResponse body
// (ambrycrc_receive_blobs_dev): GetBlobOperation.handleBody (ambry-router/.../GetBlobOperation.java
// :1113-1141, :1615-1694). Kernels: recv_kernels.hip; the shared per-payload rules: recv.h; the per-payload
// CPU entry: ambrycrc_recv_cpu.cpp. A plain pipeline on the caller's stream: (ALL: the verify's parse,)
// plan, place, one copy-through CRC pass, finish.
#include <hip/hip_runtime.h>

#include "../../include/ambrycrc.h"
#include "ambrycrc_ctx.h"
#include "crc32_kernels.h"
#include "recv.h"

using namespace ambrycrc;
using namespace ambrycrc::detail;

extern "C" {

size_t ambrycrc_receive_workspace_size(size_t m) { return recv_ws_bytes(m); }

int ambrycrc_receive_blobs_dev(const uint8_t* d_body, uint64_t body_len, const uint64_t* d_pay_off,
                               const uint64_t* d_pay_size, size_t m, int flag, const uint64_t* d_range,
                               const uint64_t* d_dst_off, uint8_t* d_out, uint64_t out_cap, ambrycrc_recv_info* d_info,
                               uint32_t* d_status, void* d_ws, size_t ws_bytes, hipStream_t stream) {
  if (m == 0) return AMBRYCRC_OK;
  if (!d_body || !d_pay_off || !d_out || !d_info || !d_status || !recv_flag_ok(flag) ||
      (size_t)kRecvSlotsAll * m >= (1ull << 31))
    return AMBRYCRC_EINVAL;
  DevCtx* c = ctx_current();
  if (!c) return AMBRYCRC_ENOINIT;
  WsLease lease;
  int rc = lease.acquire(c, stream, &d_ws, ws_bytes, ambrycrc_receive_workspace_size(m));
  if (rc) return rc;
  // the own area; then, under ALL, the verify's job arrays (its parse fills them; the receive cuts its
  // own jobs); then the batch area, which the placement scan and the CRC pass use in turn
  Carver k(d_ws);
  RecvArgs a;
  const RecvOwn w = recv_own(k, m, a);
  void* batch_ws = k.here();
  const bool all = flag == AMBRYCRC_SEND_ALL;
  // 1. ALL: the verify's parse -- header verdicts, record checks, message ends
  if (all) {
    MsgStage ms;
    rc = enqueue_messages_parse(c, d_body, body_len, d_pay_off, m, w.vstatus, w.msg_end, batch_ws, stream, &ms);
    if (rc) return rc;
    batch_ws = ms.batch_ws;
  }
  // 2. the rules of recv.h: status, info, slice lengths, the CRC jobs
  a.body = d_body;
  a.body_len = body_len;
  a.pay_off = d_pay_off;
  a.pay_size = d_pay_size;
  a.m = m;
  a.flag = flag;
  a.range = d_range;
  a.dst_off = d_dst_off;
  a.out = d_out;
  a.out_cap = out_cap;
  a.info = d_info;
  a.status = d_status;
  a.img = c->d_img;
  const PlanArgs p = plan_scan_args(d_pay_off, a.len, m, batch_ws, w.scan_out);
  a.start = p.byte_start;
  if (launch_recv_plan(a, c->num_cu, stream) != hipSuccess) return AMBRYCRC_EHIP;
  // 3. placement: packed by an exclusive scan of the slice lengths, or where the caller says
  if (!d_dst_off && launch_plan(p, stream) != hipSuccess) return AMBRYCRC_EHIP;
  if (launch_recv_place(a, c->num_cu, stream) != hipSuccess) return AMBRYCRC_EHIP;
  // 4. one CRC pass over every job, the slices copied through
  rc = enqueue_batch(c, d_body, a.job_off, a.job_len, nullptr, w.crc, (size_t)recv_slots(flag) * m, batch_ws, stream,
                     nullptr, d_out, a.copy_off);
  if (rc) return rc;
  // 5. the pieces combined, every CRC against its stored long
  return hip_err(launch_recv_finish(a, c->num_cu, stream));
}

}  // extern "C"
