// ambrycrc_rekey.cpp -- batched BlobIdTransformer over a device-resident log region
// (ambrycrc_rekey_messages_dev): BlobIdTransformer.transform / newMessage
// (ambry-replication/.../BlobIdTransformer.java:72-87,159-281). Kernels: rekey_kernels.hip; the shared
// per-message logic: rekey.h; the per-message CPU entry: ambrycrc_msg_cpu.cpp. A plain pipeline on the
// caller's stream -- no speculation, no side stream: verify, plan, place, write, copy.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "../../include/ambrycrc.h"
#include "ambrycrc_ctx.h"
#include "crc32_kernels.h"
#include "rekey.h"

using namespace ambrycrc;
using namespace ambrycrc::detail;

extern "C" {

size_t ambrycrc_rekey_workspace_bytes(size_t m) {
  return rekey_own_bytes(m) + std::max(ambrycrc_messages_workspace_bytes(m), ws_need((size_t)kRekeySlots * m));
}

uint64_t ambrycrc_rekey_out_bound(uint64_t region_len, size_t m, uint64_t aux_len) {
  const uint64_t b = ambrycrc_transform_out_bound(region_len, m);
  return aux_len > UINT64_MAX - b ? UINT64_MAX : b + aux_len;
}

int ambrycrc_rekey_messages_dev(const uint8_t* d_region, uint64_t region_len, const uint64_t* d_msg_off, size_t m,
                                const ambrycrc_rekey_desc* d_desc, const uint8_t* d_aux, uint64_t aux_len,
                                const int16_t* d_life_version, int header_version, uint8_t* d_out, uint64_t out_cap,
                                uint64_t* d_out_off, uint64_t* d_out_len, uint32_t* d_status, void* d_ws,
                                size_t ws_bytes, hipStream_t stream) {
  static_assert(sizeof(ambrycrc_rekey_desc) == 40, "ambrycrc_rekey_desc");
  if (m == 0) return AMBRYCRC_OK;
  if (!d_region || !d_msg_off || !d_desc || !d_out || !d_out_len || !d_status || (!d_aux && aux_len) ||
      header_version < 1 || header_version > 3 || (size_t)kMsgSlots * m >= (1ull << 31))
    return AMBRYCRC_EINVAL;
  DevCtx* c = ctx_current();
  if (!c) return AMBRYCRC_ENOINIT;
  WsLease lease;
  int rc = lease.acquire(c, stream, &d_ws, ws_bytes, ambrycrc_rekey_workspace_bytes(m));
  if (rc) return rc;
  const size_t j = (size_t)kRekeySlots * m;
  Carver k(d_ws);
  RekeyArgs a;
  a.region = d_region;
  a.region_len = region_len;
  a.msg_off = d_msg_off;
  a.m = m;
  a.rdesc = d_desc;
  a.aux = d_aux ? d_aux : d_region;  // aux_len 0: every span is refused or empty; never dereferenced
  a.aux_len = aux_len;
  a.life = d_life_version;
  a.header_version = header_version;
  const RekeyOwn w = rekey_own(k, m, a);
  a.out_len = d_out_len;
  a.status = d_status;
  a.out = d_out;
  a.img = c->d_img;
  // after the own area one shared area, used in turn by the verify, the placement scan, the content CRC
  // batch and the copy scan (same stream, one after the other)
  void* shared = k.here();

  // 1. the message verify (job mode), into d_status
  MsgStage ms;
  rc = enqueue_messages_parse(c, d_region, region_len, d_msg_off, m, d_status, nullptr, shared, stream, &ms);
  if (rc) return rc;
  rc = enqueue_messages_check(c, ms, stream);
  if (rc) return rc;
  // 2. refusals, output descriptors and lengths
  if (launch_rekey_plan(a, c->num_cu, stream) != hipSuccess) return AMBRYCRC_EHIP;
  // 3. packed placement: exclusive scan of the lengths, then the transform's place step (NO_ROOM
  //    for a message past out_cap, which still advances the running offset)
  rc = enqueue_place(d_msg_off, a.desc, d_out_len, d_out_off, d_status, m, out_cap, shared, w.scan_out, stream);
  if (rc) return rc;
  // 4. the replacement contents' CRCs (one job a message over aux; most are empty and read nothing),
  //    then header, record heads, properties and every trailer
  rc = enqueue_batch(c, a.aux, a.cjob_off, a.cjob_len, nullptr, w.ccrc, m, shared, stream);
  if (rc) return rc;
  if (launch_rekey_write(a, c->num_cu, stream) != hipSuccess) return AMBRYCRC_EHIP;
  // 5. the bodies, balanced by cost over the whole grid
  return enqueue_scan_copy(c, a.cp_src, a.cp_dst, a.cp_len, a.cp_cost, j, d_out, shared, w.cp_scan_out, nullptr, stream);
}

}  // extern "C"
