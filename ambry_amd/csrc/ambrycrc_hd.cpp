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

namespace {

// Workspace of m messages, 2m jobs: CRC jobs (off, len) and fill jobs (off, len, cost) of 8 B, the
// parse kernel's info (32 B a message), then expected / crc / the scan's per-job output (4 B a job)
// and the check flags (4 B a message); then one batch workspace, used by the CRC batch and after it
// by the scan of the fill costs (same stream, one after the other).
size_t hd_own_bytes(size_t m) {
  const size_t j = 2 * m;
  return (j * 5 * sizeof(uint64_t) + m * sizeof(ambrycrc_hard_delete_info) + j * 3 * sizeof(uint32_t) +
          m * sizeof(uint32_t) + 255) &
         ~size_t(255);
}

}  // namespace

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
  uint8_t* w = static_cast<uint8_t*>(d_ws);
  HdArgs a;
  a.region = d_region;
  a.region_len = region_len;
  a.msg_off = d_msg_off;
  a.m = m;
  a.recovery = d_recovery;
  a.plan_only = plan_only;
  a.img = c->d_img;
  a.job_off = reinterpret_cast<uint64_t*>(w);
  a.job_len = a.job_off + j;
  a.fill_off = a.job_len + j;
  a.fill_len = a.fill_off + j;
  a.fill_cost = a.fill_len + j;
  a.plan = reinterpret_cast<ambrycrc_hard_delete_info*>(a.fill_cost + j);
  a.expected = reinterpret_cast<uint32_t*>(a.plan + m);
  uint32_t* crc = a.expected + j;
  a.crc = crc;
  uint32_t* scan_out = crc + j;
  a.check = scan_out + j;
  a.status = d_status;
  a.info = d_info;
  void* batch_ws = w + hd_own_bytes(m);
  if (launch_hd_parse(a, stream) != hipSuccess) return AMBRYCRC_EHIP;
  // The two records of every message without recovery info; a message with it, or refused by the
  // parse, has empty jobs, which the engine passes over. Whether any message needs a check is known
  // only on the device, so the batch is always enqueued (an all-empty one reads nothing).
  rc = enqueue_batch(c, d_region, a.job_off, a.job_len, nullptr, crc, j, batch_ws, stream);
  if (rc) return rc;
  if (launch_hd_seal(a, stream) != hipSuccess) return AMBRYCRC_EHIP;
  if (plan_only) return AMBRYCRC_OK;
  // cost offsets of the fill jobs: the plan kernel's exclusive scan (no small-chunk classes)
  PlanArgs p;
  p.gate = nullptr;
  p.off = a.fill_off;
  p.len = a.fill_cost;
  p.crc_in = nullptr;
  p.n = (uint32_t)j;
  p.byte_start = static_cast<uint64_t*>(batch_ws);
  const size_t blocks = (j + kPlanPerBlock - 1) / kPlanPerBlock;
  p.block_sum = p.byte_start + j + 1;
  p.block_small = p.block_sum + blocks;
  p.small_total = p.block_small + blocks;
  p.small_idx = reinterpret_cast<uint32_t*>(p.small_total + 5);
  p.crc_stage = nullptr;
  p.out = scan_out;
  p.small_max = 0;
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
