// ambrycrc_recover.cpp -- the message chain and BlobStoreRecovery.recover over a device-resident log
// region (ambrycrc_chain_messages_dev, ambrycrc_recover_messages_dev; BlobStoreRecovery.java:43-139).
// Kernels: recover_kernels.hip; the acceptance test and the scan geometry: recover.h; the field reader:
// record_fields.h; the CPU entry: ambrycrc_msg_cpu.cpp. Both entries only enqueue: the launch count is a
// function of max_m alone.
#include <hip/hip_runtime.h>

#include "../../include/ambrycrc.h"
#include "ambrycrc_ctx.h"
#include "crc32_kernels.h"
#include "recover.h"

using namespace ambrycrc;
using namespace ambrycrc::detail;

namespace {

bool args_ok(const uint8_t* d_region, uint64_t region_len, uint64_t start, size_t max_m) {
  return (d_region || region_len == 0) && start <= region_len && max_m != 0 && max_m < (1ull << 31);
}

int enqueue_chain(DevCtx* c, const uint8_t* d_region, uint64_t region_len, uint64_t start, size_t max_m,
                  uint64_t* d_msg_off, ambrycrc_recover_result* d_result, void* d_ws, hipStream_t stream,
                  ChainArgs* out, void** rest) {
  Carver ws(d_ws);
  ChainArgs a;
  a.region = d_region;
  a.region_len = region_len;
  a.start = start;
  a.max_m = max_m;
  a.img = c->d_img;
  const uint64_t lead = reinterpret_cast<uintptr_t>(d_region + start) & 15u;
  a.nblocks = (lead + (region_len - start) + kScanBlock - 1) / kScanBlock;
  a.ntiles = chain_tiles(a.nblocks);
  chain_ws(ws, region_len, max_m, a);
  *rest = ws.here();  // recover: the verify's workspace
  a.msg_off = d_msg_off;
  a.result = d_result;
  a.info = nullptr;
  a.status = nullptr;
  *out = a;
  if (launch_chain_scan(a, c->num_cu, stream) != hipSuccess) return AMBRYCRC_EHIP;
  if (launch_chain_tile_sums(a, stream) != hipSuccess) return AMBRYCRC_EHIP;
  if (launch_chain_prefix(a, stream) != hipSuccess) return AMBRYCRC_EHIP;
  if (launch_chain_compact(a, stream) != hipSuccess) return AMBRYCRC_EHIP;
  if (launch_chain_rescan(a, c->num_cu, stream) != hipSuccess) return AMBRYCRC_EHIP;
  if (launch_chain_link(a, c->num_cu, stream) != hipSuccess) return AMBRYCRC_EHIP;
  const uint32_t rounds = chain_rounds(max_m);
  for (uint32_t k = 0; k < rounds; ++k)
    if (launch_chain_round(a, k, c->num_cu, stream) != hipSuccess) return AMBRYCRC_EHIP;
  return hip_err(launch_chain_emit(a, c->num_cu, stream));
}

}  // namespace

extern "C" {

size_t ambrycrc_chain_workspace_bytes(uint64_t region_len, size_t max_m) { return chain_bytes(region_len, max_m); }

int ambrycrc_chain_messages_dev(const uint8_t* d_region, uint64_t region_len, uint64_t start, size_t max_m,
                                uint64_t* d_msg_off, ambrycrc_recover_result* d_result, void* d_ws, size_t ws_bytes,
                                hipStream_t stream) {
  if (!args_ok(d_region, region_len, start, max_m) || !d_msg_off || !d_result) return AMBRYCRC_EINVAL;
  DevCtx* c = ctx_current();
  if (!c) return AMBRYCRC_ENOINIT;
  WsLease lease;
  const int rc = lease.acquire(c, stream, &d_ws, ws_bytes, chain_bytes(region_len, max_m));
  if (rc) return rc;
  ChainArgs a;
  void* rest;
  return enqueue_chain(c, d_region, region_len, start, max_m, d_msg_off, d_result, d_ws, stream, &a, &rest);
}

size_t ambrycrc_recover_workspace_bytes(uint64_t region_len, size_t max_m) {
  return chain_bytes(region_len, max_m) + ambrycrc_messages_workspace_bytes(max_m);
}

int ambrycrc_recover_messages_dev(const uint8_t* d_region, uint64_t region_len, uint64_t start, size_t max_m,
                                  uint64_t* d_msg_off, ambrycrc_message_info* d_info, uint32_t* d_status,
                                  ambrycrc_recover_result* d_result, void* d_ws, size_t ws_bytes, hipStream_t stream) {
  if (!args_ok(d_region, region_len, start, max_m) || !d_msg_off || !d_info || !d_status || !d_result ||
      (size_t)kMsgSlots * max_m >= (1ull << 31))
    return AMBRYCRC_EINVAL;
  DevCtx* c = ctx_current();
  if (!c) return AMBRYCRC_ENOINIT;
  WsLease lease;
  int rc = lease.acquire(c, stream, &d_ws, ws_bytes, ambrycrc_recover_workspace_bytes(region_len, max_m));
  if (rc) return rc;
  ChainArgs a;
  void* verify_ws;
  rc = enqueue_chain(c, d_region, region_len, start, max_m, d_msg_off, d_result, d_ws, stream, &a, &verify_ws);
  if (rc) return rc;
  // the verify over all max_m slots: the unused ones hold UINT64_MAX, an offset past the region, which
  // every verify form answers with AMBRYCRC_MSG_BAD_LAYOUT without reading anything
  if (region_len) {
    rc = enqueue_messages(c, d_region, region_len, d_msg_off, max_m, d_status, nullptr, verify_ws,
                          ambrycrc_messages_workspace_bytes(max_m), stream);
    if (rc) return rc;
  }
  a.info = d_info;
  a.status = d_status;
  if (launch_recover_info(a, c->num_cu, stream) != hipSuccess) return AMBRYCRC_EHIP;
  return hip_err(launch_recover_finish(a, stream));
}

}  // extern "C"
