// ambrycrc_ingest.cpp -- batched PutRequest ingest over a device-resident wire buffer
// (ambrycrc_ingest_put_requests_dev) and its per-request CPU form: PutRequest.readFrom
// (ambry-protocol/.../PutRequest.java:191-204, :440-521), then AmbryRequests.getMessageFormatWriteSet
// (AmbryRequests.java:1957-1970). Kernels: ingest_kernels.hip; the shared per-request logic:
// put_request.h. A plain pipeline on the caller's stream -- no speculation, no side stream: plan, hash,
// verdict, place, write, copy.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "../../include/ambrycrc.h"
#include "ambrycrc_ctx.h"
#include "crc32_gf2.h"
#include "crc32_kernels.h"
#include "put_emit.h"
#include "put_request.h"

using namespace ambrycrc;
using namespace ambrycrc::detail;

extern "C" {

size_t ambrycrc_ingest_puts_workspace_size(size_t m) {
  return ingest_own_bytes(m) + ws_need((size_t)kIngestSegs * m);
}

uint64_t ambrycrc_ingest_out_bound(uint64_t wire_len, size_t m) {
  const uint64_t k = AMBRYCRC_INGEST_GROWTH_MAX;
  if ((uint64_t)m > (UINT64_MAX - wire_len) / k) return UINT64_MAX;
  return wire_len + (uint64_t)m * k;
}

int ambrycrc_ingest_put_requests_dev(const uint8_t* d_wire, uint64_t wire_len, const ambrycrc_put_request_ref* d_req,
                                     size_t m, int header_version, uint8_t* d_out, uint64_t out_cap,
                                     uint64_t* d_out_off, uint64_t* d_out_len, ambrycrc_message_info* d_info,
                                     uint32_t* d_wire_crc, uint64_t* d_total, uint32_t* d_status, void* d_ws,
                                     size_t ws_bytes, hipStream_t stream) {
  static_assert(sizeof(ambrycrc_put_request_ref) == 16, "ambrycrc_put_request_ref");
  if (header_version < 1 || header_version > 3 || (size_t)kIngestSegs * m >= (1ull << 31)) return AMBRYCRC_EINVAL;
  if (m == 0) {  // nothing but the packed length, 0: the verdict kernel's store (one block, no request)
    if (!d_total) return AMBRYCRC_OK;
    IngestArgs z;
    memset(&z, 0, sizeof z);
    z.total = reinterpret_cast<unsigned long long*>(d_total);
    return launch_ingest_verdict(z, 1, stream) == hipSuccess ? AMBRYCRC_OK : AMBRYCRC_EHIP;
  }
  if (!d_wire || !d_req || !d_out || !d_out_off || !d_out_len || !d_status) return AMBRYCRC_EINVAL;
  DevCtx* c = ctx_current();
  if (!c) return AMBRYCRC_ENOINIT;
  WsLease lease;
  int rc = lease.acquire(c, stream, &d_ws, ws_bytes, ambrycrc_ingest_puts_workspace_size(m));
  if (rc) return rc;
  Carver k(d_ws);
  IngestArgs a;
  memset(&a, 0, sizeof a);
  a.wire = d_wire;
  a.wire_len = wire_len;
  a.req = d_req;
  a.m = m;
  a.header_version = header_version;
  const IngestOwn w = ingest_own(k, m, a);
  a.out_len = d_out_len;
  a.out_off = d_out_off;
  a.status = d_status;
  a.wire_crc = d_wire_crc;
  a.info = d_info;
  a.total = reinterpret_cast<unsigned long long*>(d_total);
  a.out = d_out;
  a.img = c->d_img;
  // after the own area one shared area, used in turn by the CRC batch, the placement scan and the copy
  // scan (same stream, one after the other); the batch's 5m jobs are the most
  void* shared = k.here();

  // 1. the parse, steps 1-4 of the refusals, and the five CRC jobs a request
  if (launch_ingest_plan(a, c->num_cu, stream) != hipSuccess) return AMBRYCRC_EHIP;
  // 2. every wire byte hashed once (a refused request's jobs are empty and read nothing)
  rc = enqueue_batch(c, d_wire, a.job_off, a.job_len, nullptr, w.seg, (size_t)kIngestSegs * m, shared, stream);
  if (rc) return rc;
  // 3. the wire CRC from the segments', the verdict, descriptors and lengths
  if (launch_ingest_verdict(a, c->num_cu, stream) != hipSuccess) return AMBRYCRC_EHIP;
  // 4. packed placement: exclusive scan of the lengths, then the transform's place step (NO_ROOM for
  //    a message past out_cap, which still advances the running offset)
  rc = enqueue_place(a.job_off, a.desc, d_out_len, d_out_off, d_status, m, out_cap, shared, w.scan_out, stream);
  if (rc) return rc;
  // 5. header, record heads, properties, every trailer, the MessageInfo, the packed length (zeroed
  //    by the verdict kernel)
  if (launch_ingest_write(a, c->num_cu, stream) != hipSuccess) return AMBRYCRC_EHIP;
  // 6. the bodies, balanced by cost over the whole grid
  return enqueue_scan_copy(c, a.cp_src, a.cp_dst, a.cp_len, a.cp_cost, (size_t)kIngestSlots * m, d_out, shared,
                           w.cp_scan_out, nullptr, stream);
}

int ambrycrc_ingest_put_request_cpu(const uint8_t* wire, uint64_t wire_len, const ambrycrc_put_request_ref* req,
                                    int header_version, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                                    ambrycrc_message_info* info, uint32_t* wire_crc, uint32_t* status) {
  if ((!wire && wire_len) || !req || !out_len || !status || header_version < 1 || header_version > 3)
    return AMBRYCRC_EINVAL;
  *out_len = 0;
  if (info) memset(info, 0, sizeof *info);
  if (wire_crc) *wire_crc = 0;
  const auto crc = [](const uint8_t* b, uint32_t n) { return ambrycrc_update(0, b, n); };
  IngestPlan p;
  *status = ingest_parse(wire, wire_len, *req, crc, &p);
  if (*status) return AMBRYCRC_OK;
  // the CRC'd span in one pass of the CLMUL loop (the device combines it from the segments' CRCs)
  const uint32_t wcrc = ambrycrc_update(0, wire + p.body, ingest_crc_off(p) - p.body);
  if (wire_crc) *wire_crc = wcrc;
  ambrycrc_put_desc d;
  *status = ingest_verdict(wire, p, wcrc, header_version, &d);
  if (*status) return AMBRYCRC_OK;
  PutLayout L;
  if (!put_layout(d, L)) return AMBRYCRC_EINVAL;  // (ingest_verdict checked it)
  if (!out || L.length > out_cap) {
    *status = AMBRYCRC_MSG_NO_ROOM;
    return AMBRYCRC_OK;
  }
  // bodies in place, then every trailer hashed from the output
  put_write_fixed(d, L, out);
  if (d.key_len) memcpy(out + L.hsize, wire + d.key_src, d.key_len);
  if (L.enc_rec) memcpy(out + L.enc_rel + 6, wire + d.enckey_src, (size_t)d.enckey_len);
  const PropsFix x = ingest_props_fix(p);
  uint8_t* ps = out + L.bp_rel + 2;
  for (uint32_t j = 0; j < d.props_len; ++j) ps[j] = props_v5_byte(x, j, j < x.stored_len ? wire[d.props_src + j] : 0);
  if (d.usermeta_len) memcpy(out + L.um_rel + 6, wire + d.usermeta_src, d.usermeta_len);
  if (d.blob_len) memcpy(out + L.blob_rel + 13, wire + d.blob_src, d.blob_len);
  for (uint32_t k = 0; k < kPutSlots; ++k) put_seal_record(out, L, k);
  if (info) ingest_info(wire, p, d, L, 0, info);
  *out_len = L.length;
  return AMBRYCRC_OK;
}

}  // extern "C"
