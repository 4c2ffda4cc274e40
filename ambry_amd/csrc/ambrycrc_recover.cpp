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

// Scan blocks of any [start, region_len) of a region at any address: the span plus a leading granule.
uint64_t max_scan_blocks(uint64_t region_len) { return (region_len + 15) / kScanBlock + 1; }

size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

uint64_t tiles_of(uint64_t blocks) { return (blocks + kSumTile - 1) / kSumTile; }

// Workspace: the head, the 8-B arrays (pos, next, the tile sums), the 4-B ones (jump x 2, ord, the block
// counts and first indices), then the staged 2-B offsets.
size_t chain_bytes(uint64_t region_len, size_t max_m) {
  const uint64_t nb = max_scan_blocks(region_len);
  return align256(sizeof(ChainHead) + max_m * (2 * sizeof(uint64_t) + 3 * sizeof(uint32_t)) +
                  tiles_of(nb) * sizeof(uint64_t) + nb * (2 * sizeof(uint32_t) + kStageMax * sizeof(uint16_t)));
}

bool args_ok(const uint8_t* d_region, uint64_t region_len, uint64_t start, size_t max_m) {
  return (d_region || region_len == 0) && start <= region_len && max_m != 0 && max_m < (1ull << 31);
}

int enqueue_chain(DevCtx* c, const uint8_t* d_region, uint64_t region_len, uint64_t start, size_t max_m,
                  uint64_t* d_msg_off, ambrycrc_recover_result* d_result, void* d_ws, hipStream_t stream,
                  ChainArgs* out) {
  uint8_t* w = static_cast<uint8_t*>(d_ws);
  ChainArgs a;
  a.region = d_region;
  a.region_len = region_len;
  a.start = start;
  a.max_m = max_m;
  a.img = c->d_img;
  const uint64_t lead = reinterpret_cast<uintptr_t>(d_region + start) & 15u;
  a.nblocks = (lead + (region_len - start) + kScanBlock - 1) / kScanBlock;
  a.head = reinterpret_cast<ChainHead*>(w);
  a.pos = reinterpret_cast<uint64_t*>(w + sizeof(ChainHead));
  a.next = a.pos + max_m;
  a.ntiles = tiles_of(a.nblocks);
  const uint64_t nb = max_scan_blocks(region_len);
  a.part = a.next + max_m;
  a.jump[0] = reinterpret_cast<uint32_t*>(a.part + tiles_of(nb));
  a.jump[1] = a.jump[0] + max_m;
  a.ord = a.jump[1] + max_m;
  a.cnt = a.ord + max_m;
  a.blk = a.cnt + nb;
  a.stage = reinterpret_cast<uint16_t*>(a.blk + nb);
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
  return enqueue_chain(c, d_region, region_len, start, max_m, d_msg_off, d_result, d_ws, stream, &a);
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
  rc = enqueue_chain(c, d_region, region_len, start, max_m, d_msg_off, d_result, d_ws, stream, &a);
  if (rc) return rc;
  // the verify over all max_m slots: the unused ones hold UINT64_MAX, an offset past the region, which
  // every verify form answers with AMBRYCRC_MSG_BAD_LAYOUT without reading anything
  if (region_len) {
    rc = enqueue_messages(c, d_region, region_len, d_msg_off, max_m, d_status, nullptr,
                          static_cast<uint8_t*>(d_ws) + chain_bytes(region_len, max_m),
                          ambrycrc_messages_workspace_bytes(max_m), stream);
    if (rc) return rc;
  }
  a.info = d_info;
  a.status = d_status;
  if (launch_recover_info(a, c->num_cu, stream) != hipSuccess) return AMBRYCRC_EHIP;
  return hip_err(launch_recover_finish(a, stream));
}

}  // extern "C"
