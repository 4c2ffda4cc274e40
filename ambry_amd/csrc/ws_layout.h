// ws_layout.h -- every device workspace of libambrycrc, described once. A description is a function
// that names a workspace's arrays through a Carver, in order, and stores them in the kernel arguments
// that use them; run over a base pointer it hands out the arrays, run over null it only measures, so a
// workspace's size and its pointers cannot disagree. The *_bytes helpers below and the public
// ambrycrc_*_workspace_bytes functions are descriptions run over null. Host code only;
// tests/native/ws_layout_asan.cpp walks every description under ASan + UBSan.
//
// Rules of a description: 8-B arrays first, then 4-B, then smaller; take() never pads, so anything that
// must start on a boundary follows an explicit align(); an area that another one follows ends with
// align(256). Areas used in turn on one stream share their bytes: the std::max over them stays with
// the entry that owns that policy, not here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "crc32_kernels.h"
#include "hard_delete.h"
#include "put_layout.h"
#include "put_request.h"
#include "record_fields.h"
#include "recover.h"
#include "recv.h"
#include "rekey.h"
#include "send.h"

namespace ambrycrc {
namespace detail {

struct Take {  // one array handed out: offset from the base, bytes, alignment of its type
  size_t off, bytes, align;
};

class Carver {
 public:
  // base null: measure only (every take() returns null). log (the layout test's): every take, in order.
  explicit Carver(void* base, std::vector<Take>* log = nullptr) : base_(static_cast<uint8_t*>(base)), log_(log) {}
  template <class T>
  T* take(size_t n) {
    if (log_) log_->push_back({at_, n * sizeof(T), alignof(T)});
    T* p = static_cast<T*>(here());
    at_ += n * sizeof(T);
    return p;
  }
  // n elements for each of the arrays named, in the order named
  template <class T, class... Ts>
  void take_each(size_t n, T*& first, Ts*&... rest) {
    first = take<T>(n);
    if constexpr (sizeof...(rest) > 0) take_each(n, rest...);
  }
  void align(size_t a) { at_ = (at_ + a - 1) & ~(a - 1); }  // a: a power of two
  size_t bytes() const { return at_; }
  void* here() const { return base_ ? base_ + at_ : nullptr; }  // where the next take() starts

 private:
  uint8_t* base_;
  std::vector<Take>* log_;
  size_t at_ = 0;
};

// Bytes of a description of m items that fills an Args: the description run over null.
template <class R, class Args>
size_t measure(R (*describe)(Carver&, size_t, Args&), size_t m) {
  Carver c(nullptr);
  Args a;
  describe(c, m, a);
  return c.bytes();
}

// ------------------------------------------------------------ plan scratch
// The plan kernel's scratch for n chunks: small_total is total, start of size classes 1..3 in
// small_idx, spare; crc_stage is crc_in as read by the plan; B = ceil(n / kPlanPerBlock).
inline void plan_scratch(Carver& c, size_t n, PlanArgs& p) {
  const size_t blocks = (n + kPlanPerBlock - 1) / kPlanPerBlock;
  p.byte_start = c.take<uint64_t>(n + 1);
  c.take_each(blocks, p.block_sum, p.block_small);
  p.small_total = c.take<uint64_t>(5);
  c.take_each(n, p.small_idx, p.crc_stage);
  c.align(256);
}
// Bytes of batch workspace for n chunks (ambrycrc_workspace_bytes).
inline size_t ws_need(size_t n) { return measure(plan_scratch, n); }

// ambrycrc_verify_dev: the batch's scratch, then (own_out: no caller d_out) the CRCs. Returns them.
inline uint32_t* verify_scratch(Carver& c, size_t n, bool own_out) {
  PlanArgs p;
  plan_scratch(c, n, p);
  uint32_t* out = own_out ? c.take<uint32_t>(n) : nullptr;
  c.align(256);
  return out;
}

// ------------------------------------------------------------ message jobs
// The job arrays at the start of a message-verify workspace (the rest: the batch's scratch in job mode,
// the run sums in region mode). Returns a.crc, writable: the batch's output.
inline uint32_t* msg_jobs(Carver& c, size_t m, MsgArgs& a) {
  const size_t j = (size_t)kMsgSlots * m;
  c.take_each(j, a.job_off, a.job_len);
  a.expected = c.take<uint32_t>(j);
  uint32_t* crc = c.take<uint32_t>(j);
  a.crc = crc;
  c.take<uint8_t>(j);  // one byte a job that no kernel uses: the public size has always counted it
  c.align(256);
  return crc;
}
inline size_t msg_jobs_bytes(size_t m) { return measure(msg_jobs, m); }

// Region mode keeps its long-record list (LongList) in the job arrays' space, `bytes` long, which it does
// not use otherwise: the counters, records from byte 64 (at most 4,096), then the piece slots.
inline void long_list(Carver& c, size_t bytes, LongList& l) {
  l.ctr = c.take<unsigned long long>(1);
  l.claim = c.take<uint32_t>(1);
  c.align(64);
  l.cap = (uint32_t)std::min<size_t>(4096, (bytes - 64) / 2 / sizeof(LongRec));
  l.rec = c.take<LongRec>(l.cap);
  c.align(256);
  l.pcap = (uint32_t)std::min<size_t>(1u << 30, (bytes - c.bytes()) / sizeof(uint32_t));
  l.slot = c.take<uint32_t>(l.pcap);
}

// Region mode's sums (region_ws_bytes, crc32_kernels.h): the run sums, the one-pass kernels' control
// words and their deferred list for m messages.
inline void region_sums(Carver& c, const uint8_t* region, uint64_t len, size_t m, FusedArgs& f) {
  f.g.rk = c.take<uint32_t>(region_rk_bytes(region, len) / sizeof(uint32_t));
  f.ctl = c.take<uint32_t>(64);
  f.defer = c.take<uint32_t>(m);
  c.align(256);
}

// ------------------------------------------------------------ put jobs
// The serializer's job path for m messages: copy jobs (src, dst, len, cost) and CRC jobs (off, len, crc,
// crc_in) of kPutSlots per message; one batch scratch shared by the copy plan and the CRC batch (same
// stream, one after the other); the streamed form's `big` word. The transform, which never streams,
// uses this much; ambrycrc_serialize_puts_workspace_bytes adds the streamed form's run slots after it.
struct PutCore {
  uint32_t* crc;  // a.crc, writable
  void* batch_ws;
  uint32_t* big;
};
inline PutCore put_core(Carver& c, size_t m, PutArgs& a) {
  const size_t j = (size_t)kPutSlots * m;
  PutCore w;
  c.take_each(j, a.cp_src, a.cp_dst, a.cp_len, a.cp_cost, a.crc_off, a.crc_len);
  a.crc = w.crc = c.take<uint32_t>(j);
  a.crc_in = c.take<uint32_t>(j);
  c.align(256);
  w.batch_ws = c.here();
  PlanArgs p;
  plan_scratch(c, j, p);
  w.big = c.take<uint32_t>(1);
  c.align(256);
  return w;
}
inline size_t put_core_bytes(size_t m) { return measure(put_core, m); }

// ------------------------------------------------------------ the transform's own area
// Descriptors, the placement scan's per-message output, in_crc (4 per message), the speculative pass's
// xstatus, its two gate words (fail, xfail); from a 16-B boundary the verify jobs' copy destinations
// (kPutSlots per message) and the properties re-encodings.
struct TransformOwn {
  uint32_t *scan_out, *xstatus, *fail;
  uint64_t* copy_off;
};
inline TransformOwn transform_own(Carver& c, size_t m, TransformArgs& t) {
  TransformOwn w;
  t.desc = c.take<ambrycrc_put_desc>(m);
  w.scan_out = c.take<uint32_t>(m);
  t.in_crc = c.take<uint32_t>(4 * m);
  w.xstatus = c.take<uint32_t>(m);
  w.fail = c.take<uint32_t>(2);
  c.align(16);
  w.copy_off = c.take<uint64_t>((size_t)kPutSlots * m);
  t.pfix = c.take<PropsFix>(m);
  c.align(256);
  return w;
}
inline size_t transform_own_bytes(size_t m) { return measure(transform_own, m); }

// ------------------------------------------------------------ hard delete
// m messages, 2m jobs: CRC jobs (off, len) and fill jobs (off, len, cost), the parse kernel's info, then
// expected / crc / the fill scan's per-job output and the check flags.
struct HdOwn {
  uint32_t *crc, *scan_out;  // a.crc, writable; the scan's output
};
inline HdOwn hd_own(Carver& c, size_t m, HdArgs& a) {
  HdOwn w;
  c.take_each(2 * m, a.job_off, a.job_len, a.fill_off, a.fill_len, a.fill_cost);
  a.plan = c.take<ambrycrc_hard_delete_info>(m);
  c.take_each(2 * m, a.expected, w.crc, w.scan_out);
  a.crc = w.crc;
  a.check = c.take<uint32_t>(m);
  c.align(256);
  return w;
}
inline size_t hd_own_bytes(size_t m) { return measure(hd_own, m); }

// ------------------------------------------------------------ rekey
// Put descriptors, RekeyFix, the content CRC jobs (off, len) and the kRekeySlots copy jobs a message
// (src, dst, len, cost), then the placement scan's per-message output, the content CRCs and the copy
// scan's per-job output.
struct RekeyOwn {
  uint32_t *scan_out, *ccrc, *cp_scan_out;  // ccrc: a.ccrc, writable
};
inline RekeyOwn rekey_own(Carver& c, size_t m, RekeyArgs& a) {
  RekeyOwn w;
  a.desc = c.take<ambrycrc_put_desc>(m);
  a.fix = c.take<RekeyFix>(m);
  c.take_each(m, a.cjob_off, a.cjob_len);
  c.take_each((size_t)kRekeySlots * m, a.cp_src, a.cp_dst, a.cp_len, a.cp_cost);
  c.take_each(m, w.scan_out, w.ccrc);
  a.ccrc = w.ccrc;
  w.cp_scan_out = c.take<uint32_t>((size_t)kRekeySlots * m);
  c.align(256);
  return w;
}
inline size_t rekey_own_bytes(size_t m) { return measure(rekey_own, m); }

// ------------------------------------------------------------ ingest
// Put descriptors, the parse's plans, the kIngestSegs CRC jobs a request (off, len) and the kIngestSlots
// copy jobs (src, dst, len, cost), then the jobs' CRCs, the placement scan's per-request output and the
// copy scan's per-job output. Walked under ASan + UBSan by tests/native/ingest_ws_asan.cpp.
struct IngestOwn {
  uint32_t *seg, *scan_out, *cp_scan_out;  // seg: a.seg, writable
};
inline IngestOwn ingest_own(Carver& c, size_t m, IngestArgs& a) {
  IngestOwn w;
  a.desc = c.take<ambrycrc_put_desc>(m);
  a.plan = c.take<IngestPlan>(m);
  c.take_each((size_t)kIngestSegs * m, a.job_off, a.job_len);
  c.take_each((size_t)kIngestSlots * m, a.cp_src, a.cp_dst, a.cp_len, a.cp_cost);
  w.seg = c.take<uint32_t>((size_t)kIngestSegs * m);
  a.seg = w.seg;
  w.scan_out = c.take<uint32_t>(m);
  w.cp_scan_out = c.take<uint32_t>((size_t)kIngestSlots * m);
  c.align(256);
  return w;
}
inline size_t ingest_own_bytes(size_t m) { return measure(ingest_own, m); }

// ------------------------------------------------------------ send
// Span lengths, message ends, the kMsgSlots copy destinations a message, the plain-copy jobs (src, dst,
// len, cost); then the verify's status, the encryption-key CRCs and the two scans' per-entry outputs.
struct SendOwn {
  uint64_t* msg_end;                                   // a.msg_end, a.vstatus, a.enc_crc, writable
  uint32_t *vstatus, *enc_crc, *scan_out, *gscan_out;  // ... and the scans' outputs
};
inline SendOwn send_own(Carver& c, size_t m, SendArgs& a) {
  SendOwn w;
  c.take_each(m, a.len, w.msg_end);
  a.copy_off = c.take<uint64_t>((size_t)kMsgSlots * m);
  c.take_each(m, a.g_src, a.g_dst, a.g_len, a.g_cost);
  c.take_each(m, w.vstatus, w.enc_crc, w.scan_out, w.gscan_out);
  a.msg_end = w.msg_end;
  a.vstatus = w.vstatus;
  a.enc_crc = w.enc_crc;
  c.align(256);
  return w;
}
inline size_t send_own_bytes(size_t m) { return measure(send_own, m); }

// ------------------------------------------------------------ receive
// Slice lengths, message ends, the kRecvSlotsAll jobs a payload (off, len, copy destination); then the
// verify's status, the placement scan's per-payload output and the jobs' CRCs. Sized for ALL under either
// flag. Walked under ASan + UBSan by tests/native/recv_asan.cpp.
struct RecvOwn {
  uint64_t* msg_end;                  // a.msg_end, a.vstatus, a.crc, writable
  uint32_t *vstatus, *scan_out, *crc;
};
inline RecvOwn recv_own(Carver& c, size_t m, RecvArgs& a) {
  RecvOwn w;
  c.take_each(m, a.len, w.msg_end);
  c.take_each((size_t)kRecvSlotsAll * m, a.job_off, a.job_len, a.copy_off);
  c.take_each(m, w.vstatus, w.scan_out);
  w.crc = c.take<uint32_t>((size_t)kRecvSlotsAll * m);
  a.msg_end = w.msg_end;
  a.vstatus = w.vstatus;
  a.crc = w.crc;
  c.align(256);
  return w;
}
inline size_t recv_own_bytes(size_t m) { return measure(recv_own, m); }
// The whole receive workspace: the own area, the verify's job arrays (ALL's parse), one batch scratch for
// the placement scan and the CRC pass in turn.
inline size_t recv_ws_bytes(size_t m) { return recv_own_bytes(m) + msg_jobs_bytes(m) + ws_need((size_t)kRecvSlotsAll * m); }

// ------------------------------------------------------------ chain
// Scan blocks of any [start, region_len) of a region at any address: the span plus a leading granule.
inline uint64_t max_scan_blocks(uint64_t region_len) { return (region_len + 15) / kScanBlock + 1; }
inline uint64_t chain_tiles(uint64_t blocks) { return (blocks + kSumTile - 1) / kSumTile; }
// The head, the 8-B arrays (pos, next, the tile sums), the 4-B ones (jump x 2, ord, the block counts and
// first indices), then the staged 2-B offsets; each sized for the most blocks the region can take.
inline void chain_ws(Carver& c, uint64_t region_len, size_t max_m, ChainArgs& a) {
  const uint64_t nb = max_scan_blocks(region_len);
  a.head = c.take<ChainHead>(1);
  c.take_each(max_m, a.pos, a.next);
  a.part = c.take<uint64_t>(chain_tiles(nb));
  c.take_each(max_m, a.jump[0], a.jump[1], a.ord);
  c.take_each(nb, a.cnt, a.blk);
  a.stage = c.take<uint16_t>(nb * kStageMax);
  c.align(256);
}
inline size_t chain_bytes(uint64_t region_len, size_t max_m) {
  Carver c(nullptr);
  ChainArgs a;
  chain_ws(c, region_len, max_m, a);
  return c.bytes();
}

// ------------------------------------------------------------ trailed
// CRC-trailered records: job lengths, stored and computed CRCs, the forced-mismatch flags (the batch's
// scratch follows). Returns a.crc, writable: the batch's output.
inline uint32_t* trailed_own(Carver& c, size_t n, TrailerArgs& a) {
  a.job_len = c.take<uint64_t>(n);
  uint32_t* crc;
  c.take_each(n, a.expected, crc);
  a.crc = crc;
  a.force = c.take<uint8_t>(n);
  c.align(256);
  return crc;
}
inline size_t trailed_own_bytes(size_t n) { return measure(trailed_own, n); }

}  // namespace detail
}  // namespace ambrycrc
