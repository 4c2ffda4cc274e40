// ambrycrc_hd.cpp -- batched hard delete of stored PUT messages in a device-resident log region
// (ambrycrc_hard_delete_messages_dev): BlobStoreHardDelete.getHardDeleteInfo
// (ambry-messageformat/.../BlobStoreHardDelete.java:97-179) and the records of
// HardDeleteMessageFormatInputStream (:58-124), written in place. Kernels: hard_delete_kernels.hip;
// the per-message CPU entry is in ambrycrc_msg_cpu.cpp; the shared layout logic in hard_delete.h.
#include <hip/hip_runtime.h>

#include "../../include/ambrycrc.h"
#include "ambrycrc_ctx.h"
#include "crc32_kernels.h"
#include "hard_delete.h"

using namespace ambrycrc;
using namespace ambrycrc::detail;

extern "C" {

size_t ambrycrc_hard_delete_workspace_bytes(size_t m) { return hd_own_bytes(m) + ws_need(2 * m); }

int ambrycrc_hard_delete_messages_dev(uint8_t* d_region, uint64_t region_len, const uint64_t* d_msg_off, size_t m,
                                      const ambrycrc_hard_delete_info* d_recovery, int plan_only, uint32_t* d_status,
                                      ambrycrc_hard_delete_info* d_info, void* d_ws, size_t ws_bytes,
                                      hipStream_t stream) {
  if (m == 0) return AMBRYCRC_OK;
  if (!d_region || !d_msg_off || !d_status || 2 * (uint64_t)m >= (1ull << 31)) return AMBRYCRC_EINVAL;
  DevCtx* c = ctx_current();
  if (!c) return AMBRYCRC_ENOINIT;
  WsLease lease;
  int rc = lease.acquire(c, stream, &d_ws, ws_bytes, ambrycrc_hard_delete_workspace_bytes(m));
  if (rc) return rc;
  const size_t j = 2 * m;
  Carver k(d_ws);
  HdArgs a;
  a.region = d_region;
  a.region_len = region_len;
  a.msg_off = d_msg_off;
  a.m = m;
  a.recovery = d_recovery;
  a.plan_only = plan_only;
  a.img = c->d_img;
  const HdOwn w = hd_own(k, m, a);
  a.status = d_status;
  a.info = d_info;
  // after the own area one batch workspace, used by the CRC batch and after it by the scan of the fill
  // costs (same stream, one after the other)
  void* batch_ws = k.here();
  if (launch_hd_parse(a, stream) != hipSuccess) return AMBRYCRC_EHIP;
  // The two records of every message without recovery info; a message with it, or refused by the
  // parse, has empty jobs, which the engine passes over. Whether any message needs a check is known
  // only on the device, so the batch is always enqueued (an all-empty one reads nothing).
  rc = enqueue_batch(c, d_region, a.job_off, a.job_len, nullptr, w.crc, j, batch_ws, stream);
  if (rc) return rc;
  if (launch_hd_seal(a, stream) != hipSuccess) return AMBRYCRC_EHIP;
  if (plan_only) return AMBRYCRC_OK;
  // cost offsets of the fill jobs: the plan kernel's exclusive scan (no small-chunk classes)
  const PlanArgs p = plan_scan_args(a.fill_off, a.fill_cost, j, batch_ws, w.scan_out);
  if (launch_plan(p, stream) != hipSuccess) return AMBRYCRC_EHIP;
  HdFillArgs f;
  f.dst = d_region;
  f.dst_off = a.fill_off;
  f.len = a.fill_len;
  f.start = p.byte_start;
  f.n = (uint32_t)j;
  return hip_err(launch_hd_fill(f, c->grid, stream));
}

}  // extern "C"
