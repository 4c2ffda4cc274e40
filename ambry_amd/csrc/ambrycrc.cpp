// ambrycrc.cpp -- host side of libambrycrc: the table image, per-device contexts and default
// workspaces, the batch and message engines' front end (kernel launches), the C ABI
// (include/ambrycrc.h) of the device-resident entries, the host streaming primitives and the
// diagnostic knobs. The host-resident entries are in ambrycrc_host.cpp.
#include "../../include/ambrycrc.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "crc32_gf2.h"
#include "crc32_kernels.h"
#include "crc32_layout.h"
#include "ambrycrc_ctx.h"
#include "host_crc.h"

using namespace ambrycrc;
using namespace ambrycrc::detail;

namespace {

// ------------------------------------------------------------ host tables
struct HostTables {
  uint32_t t[8][256];
  uint32_t xpow2[64];
  HostTables() {
    slice_tables(t, 8);
    xpow8_pow2_table(xpow2);
  }
};

const HostTables& host_tables() {
  static const HostTables tables;  // C++11 thread-safe static init
  return tables;
}

uint32_t host_xpow8(uint64_t n) {
  const HostTables& h = host_tables();
  uint32_t r = kOne;
  for (int k = 0; n; ++k, n >>= 1)
    if (n & 1) r = gf2_mul(r, h.xpow2[k]);
  return r;
}

// ------------------------------------------------------------ LDS image
std::vector<uint32_t> build_table_image() {
  const uint32_t words = kImgBytes / 4;
  std::vector<uint32_t> img(words, 0u);
  uint32_t t[4][256];
  slice_tables(t, 4);
  for (uint32_t j = 0; j < 4; ++j)
    for (uint32_t b = 0; b < 256; ++b)
      for (uint32_t l = 0; l < 32; ++l) {
        const uint32_t addr = ((j >> 1) << 16) | (b << 8) | ((j & 1) << 7) | (l << 2);
        img[addr / 4] = t[j][b];
      }
  auto put_nib = [&](uint32_t off, uint32_t c) {
    uint32_t nt[8][16];
    nibble_tables(c, nt);
    for (int n = 0; n < 8; ++n)
      for (int x = 0; x < 16; ++x) img[(kNibBase + off + 64u * n + 4u * x) / 4] = nt[n][x];
  };
  put_nib(kFoldOff, host_xpow8(kBlockBytes));
  for (uint32_t l = 0; l < kTreeLevels; ++l) put_nib(kTreeOff + kNibSetBytes * l, host_xpow8(16ull << l));
  for (uint32_t k = 0; k < kPowTables; ++k) put_nib(kPowOff + kNibSetBytes * k, host_xpow8(1ull << k));
  const HostTables& h = host_tables();
  for (int k = 0; k < 64; ++k) img[kLdsBytes / 4 + k] = h.xpow2[k];
  // x^-1 in the reflected order: u * x = v  <=>  u = v << 1 (bit 31 of v clear), or
  // ((v ^ P) << 1) | 1 (set), since u * x = (u >> 1) ^ (P if bit 0 of u).
  uint32_t inv = kOne;
  for (int i = 0; i < 8; ++i) inv = (inv & 0x80000000u) ? (((inv ^ kPoly) << 1) | 1u) : (inv << 1);  // x^-8
  for (uint32_t k = 0; k < kInvPowSets; ++k) {
    uint32_t nt[8][16];
    nibble_tables(inv, nt);
    for (int n = 0; n < 8; ++n)
      for (int x = 0; x < 16; ++x) img[(kImgInvOff + kNibSetBytes * k + 64u * n + 4u * x) / 4] = nt[n][x];
    inv = gf2_mul(inv, inv);
  }
  // region pass 2's words (crc32_layout.h kImgRegOff)
  uint32_t* reg = img.data() + kImgRegOff / 4;
  for (uint32_t lo = 0; lo < 64; ++lo) {
    const uint32_t ni = 64 - lo < 4 ? 64 - lo : 4;
    uint32_t r = 0;
    for (uint32_t i = 0; i < 64; ++i) r = t[0][(r ^ (i >= lo && i < lo + ni ? 0xFFu : 0u)) & 0xFFu] ^ (r >> 8);
    reg[kRegH0 + lo] = r;
  }
  for (uint32_t a = 0; a <= 4; ++a) {
    reg[kRegGe + a] = a < 4 ? 0xFFFFFFFFu << (8 * a) : 0u;
    reg[kRegLt + a] = a < 4 ? (1u << (8 * a)) - 1u : 0xFFFFFFFFu;
  }
  {
    uint32_t nt[8][16];
    nibble_tables(host_xpow8(256), nt);
    for (uint32_t j = 0; j < 4; ++j)
      for (uint32_t b = 0; b < 256; ++b)
        reg[kRegAuxWords + 256 * j + b] = nt[2 * j][b & 15] ^ nt[2 * j + 1][b >> 4];
  }
  {
    uint32_t inv8 = kOne;  // x^-8
    for (int i = 0; i < 8; ++i) inv8 = (inv8 & 0x80000000u) ? (((inv8 ^ kPoly) << 1) | 1u) : (inv8 << 1);
    uint32_t inv64 = kOne;
    for (int i = 0; i < 8; ++i) inv64 = gf2_mul(inv64, inv8);
    uint32_t u0 = kOne, u1 = kOne;  // x^(-8 d0), x^(-64 d1)
    for (uint32_t d = 0; d < 8; ++d) {
      uint32_t nt[8][16];
      nibble_tables(u0, nt);
      for (int n = 0; n < 8; ++n)
        for (int x = 0; x < 16; ++x) reg[kRegAuxWords + kRegByteWords + 128u * d + 16u * n + x] = nt[n][x];
      nibble_tables(u1, nt);
      for (int n = 0; n < 8; ++n)
        for (int x = 0; x < 16; ++x) reg[kRegAuxWords + kRegByteWords + 128u * (8 + d) + 16u * n + x] = nt[n][x];
      u0 = gf2_mul(u0, inv8);
      u1 = gf2_mul(u1, inv64);
    }
  }
  return img;
}

// Device pointers a and b of n uint32 each either coincide or do not overlap (in-place
// continuation d_out == d_crc_in is supported; a shifted overlap is not).
bool same_or_disjoint(const uint32_t* a, const uint32_t* b, size_t n) {
  if (!a || !b || a == b) return true;
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x + 4 * n <= y || y + 4 * n <= x;
}

}  // namespace

namespace ambrycrc {
namespace detail {

std::mutex g_mu;
DevCtx* g_ctx[kMaxDevices] = {nullptr};

int hip_err(hipError_t e) { return e == hipSuccess ? AMBRYCRC_OK : AMBRYCRC_EHIP; }

DevCtx* ctx_for(int device) {
  if (device < 0 || device >= kMaxDevices) return nullptr;
  std::lock_guard<std::mutex> g(g_mu);
  return g_ctx[device];
}

DevCtx* ctx_current() {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  return ctx_for(dev);
}

PlanArgs plan_scan_args(const uint64_t* off, const uint64_t* len, size_t n, void* scratch, uint32_t* out,
                        const uint32_t* gate, const uint32_t* crc_in) {
  Carver k(scratch);
  PlanArgs p;
  plan_scratch(k, n, p);
  p.gate = gate;
  p.off = off;
  p.len = len;
  p.crc_in = crc_in;
  p.n = (uint32_t)n;
  if (!crc_in) p.crc_stage = nullptr;
  p.out = out;
  p.small_max = 0;
  return p;
}

int enqueue_scan_copy(DevCtx* c, const uint64_t* src, const uint64_t* dst_off, const uint64_t* len,
                      const uint64_t* cost, size_t n, uint8_t* dst, void* scratch, uint32_t* out,
                      const uint32_t* gate, hipStream_t s) {
  const PlanArgs p = plan_scan_args(dst_off, cost, n, scratch, out, gate);
  if (launch_plan(p, s) != hipSuccess) return AMBRYCRC_EHIP;
  CopyArgs ca;
  ca.src = src;
  ca.dst_off = dst_off;
  ca.len = len;
  ca.start = p.byte_start;
  ca.n = (uint32_t)n;
  ca.dst = dst;
  ca.gate = gate;
  return hip_err(launch_gather_copy(ca, c->num_cu * 8, s));
}

void region_args(const DevCtx* c, const uint8_t* d_region, uint64_t region_len, size_t m, void* sums, FusedArgs* f) {
  RegionArgs& r = f->g;
  const uintptr_t rp = reinterpret_cast<uintptr_t>(d_region);
  r.base = d_region - (rp & 63u);
  r.reg0 = rp & 63u;
  r.reg_end = r.reg0 + region_len;
  r.lo16 = r.reg0 & ~uint64_t(15);
  r.hi16 = (r.reg_end - 1) & ~uint64_t(15);
  r.nsb = region_nsb(d_region, region_len);
  r.img = c->d_img;
  Carver k(sums);
  region_sums(k, d_region, region_len, m, *f);
  f->ngroups = (r.nsb + 3) / 4;
}

// Frees retired default workspaces whose last user has completed. Caller holds c->ws_mu.
void reap_retired_ws(DevCtx* c) {
  auto& r = c->ws_retired;
  for (size_t i = 0; i < r.size();) {
    if (hipEventQuery(r[i].done) == hipSuccess) {
      (void)hipFree(r[i].ptr);
      (void)hipEventDestroy(r[i].done);
      r[i] = r.back();
      r.pop_back();
    } else {
      ++i;
    }
  }
}

// The default workspace of `stream` with at least `need` bytes. Caller holds c->ws_mu until the
// work that uses it is enqueued on `stream`. A buffer that is too small is retired behind an
// event on the stream (work already queued there may still read it), never freed in place.
// (A destroyed stream's handle may be reused by a new stream; hipStreamDestroy drains the old
// stream's work first, so the buffer is idle by then.)
//
// Under stream capture (a HIP graph) nothing here may query events, synchronize or allocate: a
// capture uses the stream's buffer as an earlier uncaptured call sized it, or gets EINVAL. The graph
// then holds that buffer's address, so the entry is marked captured: when a later call grows it, or
// the entry is evicted, the buffer is kept (c->ws_kept) until shutdown instead of being freed, and
// replays stay valid. Replays share it with later calls on the stream, so they must be ordered with
// them (launched on that stream), as any two calls on one stream are.
int stream_ws(DevCtx* c, hipStream_t s, size_t need, void** out, size_t* entry, bool* capturing_out) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess) return AMBRYCRC_EHIP;
  const bool capturing = cap != hipStreamCaptureStatusNone;
  if (capturing_out) *capturing_out = capturing;
  if (!capturing) reap_retired_ws(c);
  DevCtx::StreamWs* w = nullptr;
  for (auto& e : c->ws_list)
    if (e.stream == s) w = &e;
  if (capturing && (!w || w->bytes < need)) return AMBRYCRC_EINVAL;
  if (capturing) {
    w->captured = true;
    *entry = (size_t)(w - c->ws_list.data());
    *out = w->ptr;
    return AMBRYCRC_OK;
  }
  if (!w && c->ws_list.size() >= kMaxStreamWs) {
    // evict the least recently used stream's buffer: retired behind its last call's event
    // (the entry's event moves with it), the entry reused for s
    w = &c->ws_list[0];
    for (auto& e : c->ws_list)
      if (e.tick < w->tick) w = &e;
    if (w->ptr && w->captured) {
      c->ws_kept.push_back(w->ptr);
      if (w->last) (void)hipEventDestroy(w->last);
    } else if (w->ptr) {
      if (w->last) {
        c->ws_retired.push_back({w->ptr, w->last});
      } else {
        (void)hipDeviceSynchronize();  // no event to wait on (its creation failed): drain, then free
        (void)hipFree(w->ptr);
      }
    } else if (w->last) {
      (void)hipEventDestroy(w->last);
    }
    *w = {s, nullptr, 0, nullptr, 0, false};
  }
  if (!w) {
    c->ws_list.push_back({s, nullptr, 0, nullptr, 0, false});
    w = &c->ws_list.back();
  }
  w->tick = ++c->ws_tick;
  *entry = (size_t)(w - c->ws_list.data());
  if (w->bytes >= need) {
    *out = w->ptr;
    return AMBRYCRC_OK;
  }
  if (w->ptr && w->captured) {
    c->ws_kept.push_back(w->ptr);
    w->ptr = nullptr;
    w->captured = false;
  } else if (w->ptr) {
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return AMBRYCRC_EHIP;
    if (hipEventRecord(ev, s) != hipSuccess) {
      (void)hipEventDestroy(ev);
      return AMBRYCRC_EHIP;
    }
    c->ws_retired.push_back({w->ptr, ev});
    w->ptr = nullptr;
  }
  const size_t sz = std::max(need, w->bytes * 2);
  w->bytes = 0;
  if (hipMalloc(&w->ptr, sz) != hipSuccess) {
    w->ptr = nullptr;
    return AMBRYCRC_ENOMEM;
  }
  w->bytes = sz;
  *out = w->ptr;
  return AMBRYCRC_OK;
}

// Largest chunk the group phase takes whole for a batch of n chunks on c's variant (0: none).
uint64_t batch_small_max(const DevCtx* c, size_t n) {
  if (n < kGroupMinChunks || !variant_groups(c->variant)) return 0;
  return kGroupSmallMax;
}

// exp_fill: SweepArgs::exp_fill (message verify; honoured by the group phase of variant 29).
// crc_in may equal out (an in-place continuation): the plan copies crc_in into the workspace
// before it initialises out, and the CRC kernels read the copy.
int enqueue_batch(DevCtx* c, const uint8_t* base, const uint64_t* off, const uint64_t* len, const uint32_t* crc_in,
                  uint32_t* out, size_t n, void* ws, hipStream_t s, uint32_t* exp_fill, uint8_t* copy_dst,
                  const uint64_t* copy_off, const uint32_t* gate) {
  if (n == 0) return AMBRYCRC_OK;
  PlanArgs p = plan_scan_args(off, len, n, ws, out, gate, crc_in);
  p.small_max = copy_dst ? (n >= kGroupMinChunks ? kGroupSmallMax : 0) : batch_small_max(c, n);
  hipError_t e = launch_plan(p, s);
  if (e != hipSuccess) return AMBRYCRC_EHIP;
  SweepArgs t;
  t.base = base;
  t.off = off;
  t.len = len;
  t.crc_in = p.crc_stage;
  t.n = (uint32_t)n;
  t.byte_start = p.byte_start;
  t.img = c->d_img;
  t.out = out;
  t.small_max = p.small_max;
  t.small_total = p.small_total;
  t.small_idx = p.small_idx;
  t.exp_fill = exp_fill;
  t.window = c->window;
  t.copy_dst = copy_dst;
  t.copy_off = copy_off;
  t.gate = gate;
  if (gate && !copy_dst) return AMBRYCRC_EINVAL;  // only the copy-through sweep checks the gate
  EventPair ev{nullptr, nullptr};
  if (c->timing) {
    std::lock_guard<std::mutex> g(c->ev_mu);
    if (!c->free_events.empty()) {
      ev = c->free_events.back();
      c->free_events.pop_back();
    } else if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess) {
      return AMBRYCRC_EHIP;
    }
    if (hipEventRecord(ev.a, s) != hipSuccess) return AMBRYCRC_EHIP;
  }
  e = copy_dst ? launch_sweep_copy(t, c->grid, c->num_cu, c->variant == kVariantSplit ? kVariantSplit : kVariantDefault, s)
               : launch_sweep(t, c->grid, c->num_cu, c->variant, s);
  if (e != hipSuccess) return AMBRYCRC_EHIP;
  if (c->timing) {
    if (hipEventRecord(ev.b, s) != hipSuccess) return AMBRYCRC_EHIP;
    std::lock_guard<std::mutex> g(c->ev_mu);
    c->pending.push_back(ev);
  }
  return AMBRYCRC_OK;
}

void free_ctx(DevCtx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  if (c->d_img) (void)hipFree(c->d_img);
  if (c->h_words) (void)hipHostFree(c->h_words);
  for (auto& w : c->ws_list) {
    if (w.ptr) (void)hipFree(w.ptr);
    if (w.last) (void)hipEventDestroy(w.last);
  }
  for (auto& r : c->ws_retired) {
    (void)hipFree(r.ptr);
    (void)hipEventDestroy(r.done);
  }
  for (void* p : c->ws_kept) (void)hipFree(p);
  for (DevCtx::XformSide* x : c->xs_list) {
    if (x->side) (void)hipStreamDestroy(x->side);
    if (x->d_gates) (void)hipFree(x->d_gates);
    if (x->d_done) (void)hipFree(x->d_done);
    if (x->fork) (void)hipEventDestroy(x->fork);
    for (hipEvent_t e : x->ev)
      if (e) (void)hipEventDestroy(e);
    delete x;
  }
  for (auto& e : c->pending) {
    (void)hipEventDestroy(e.a);
    (void)hipEventDestroy(e.b);
  }
  for (auto& e : c->free_events) {
    (void)hipEventDestroy(e.a);
    (void)hipEventDestroy(e.b);
  }
  release_slabs(c);  // whatever the host legs' first uses got to, even if one failed part way
  delete c;
}

// A processor wave finishes a 64-message batch in ~20-40 us (a chain of dependent reads under the
// streamers' load), so the processors a CU needs grow with its messages; the rest of its waves
// stream, and too few streamers starve them (a cliff: 3 of 12 at 1 KiB blobs, 0.367 -> 0.438 ms).
// Measured per messages per CU (r04am-ao, r04au; ms per call): verify form (12 waves) 4 KiB blobs
// (1,024 per CU) best at 5 (0.377; 8: 0.410), 3 KiB (1,280) at 6 (0.408; 5: 0.418), 2 KiB (1,536)
// at 6 (0.374; 5: 0.397, 8: 0.387), 1 KiB (2,048) at 8 (0.367), 100 B (4,096) at 9 (0.532; 8:
// 0.575); copy form (8 waves) at 4 from 128 to 1,024 per CU (4 KiB PUTs 0.663; 3: 0.69, 5: 0.78;
// 16 KiB PUTs 0.549, 2: 0.562; 32 KiB 0.563, 2: 0.570; r04ba). Verify below 512 per CU (not swept):
// one processor per 128 messages, at least 2.
uint32_t fused_proc_waves(const DevCtx* c, size_t m, bool copy) {
  const int waves = copy ? kFusedWavesCopy : kFusedWavesVerify;
  const int most = std::min(kFusedProcMax, waves - 2);  // at least two streamers
  if (c->fused_proc > 0) return (uint32_t)std::min(c->fused_proc, most);
  const size_t per_cu = m / (size_t)std::max(1, c->num_cu);
  int p;
  if (copy) p = 4;
  else if (per_cu <= 512) p = (int)std::max<size_t>(2, (per_cu + 127) / 128);
  else p = per_cu <= 1024 ? 5 : per_cu <= 1536 ? 6 : per_cu <= 3072 ? 8 : 9;
  return (uint32_t)std::min(p, most);
}

int enqueue_messages(DevCtx* c, const uint8_t* d_region, uint64_t region_len, const uint64_t* d_msg_off, size_t m,
                     uint32_t* d_status, uint64_t* d_msg_end, void* d_ws, size_t ws_bytes, hipStream_t stream) {
  const bool region = c->region_mode && region_len > 0 && region_len <= c->region_max * (uint64_t)m &&
                      msg_jobs_bytes(m) + region_ws_bytes(d_region, region_len, m) <= ws_bytes;
  MsgStage st;
  c->last_msg_mode.store(region ? c->region_mode : 0);
  if (!region) {
    const int rc = enqueue_messages_parse(c, d_region, region_len, d_msg_off, m, d_status, d_msg_end, d_ws, stream, &st);
    return rc ? rc : enqueue_messages_check(c, st, stream);
  }
  // Region mode: pass 1 sweeps the region into 64-B run sums (kept where job mode keeps its batch
  // workspace), pass 2 parses every message and assembles its record CRCs from them.
  st.a.region = d_region;
  st.a.region_len = region_len;
  st.a.msg_off = d_msg_off;
  st.a.m = m;
  st.a.img = c->d_img;
  st.a.status = d_status;
  st.a.msg_end = d_msg_end;
  st.a.inline_max = 0;
  Carver jobs(d_ws);
  msg_jobs(jobs, m, st.a);
  FusedArgs f;
  region_args(c, d_region, region_len, m, jobs.here(), &f);
  // long records (more than region::kLongRuns runs) listed in the job arrays' space, which region
  // mode does not use
  Carver k(d_ws);
  long_list(k, jobs.bytes(), f.g.lng);
  if (c->region_mode == 2) {  // the two-pass form: runs kernel, then one thread per message
    const RegionArgs& r = f.g;  // the whole grid takes the long records after pass 2
    if (launch_region_runs(r, c->grid, stream) != hipSuccess ||
        launch_region_msg(st.a, r, c->num_cu, stream) != hipSuccess)
      return AMBRYCRC_EHIP;
    return hip_err(launch_region_long(st.a, r, c->num_cu, stream));
  }
  f.a = st.a;
  f.nproc = fused_proc_waves(c, m, false);
  // long records: listed by the processors (the counters in ctl instead, zeroed with it), taken by
  // region_long_kernel after the tail
  f.g.lng.ctr = reinterpret_cast<unsigned long long*>(f.ctl + 4);
  f.g.lng.claim = f.ctl + 6;
  if (hipMemsetAsync(f.ctl, 0, 32, stream) != hipSuccess) return AMBRYCRC_EHIP;
  return hip_err(launch_region_fused(f, c->num_cu, stream));
}

int enqueue_messages_parse(DevCtx* c, const uint8_t* d_region, uint64_t region_len, const uint64_t* d_msg_off,
                           size_t m, uint32_t* d_status, uint64_t* d_msg_end, void* d_ws, hipStream_t stream,
                           MsgStage* st, const TransformArgs* desc, const uint32_t* gate) {
  const size_t j = (size_t)kMsgSlots * m;
  Carver k(d_ws);
  MsgArgs& a = st->a;
  a.gate = gate;
  a.region = d_region;
  a.region_len = region_len;
  a.msg_off = d_msg_off;
  a.m = m;
  a.img = c->d_img;
  st->crc = msg_jobs(k, m, a);
  a.status = d_status;
  a.msg_end = d_msg_end;
  // The class-sized group phase (variant 29) reads the stored CRCs of the records it
  // takes whole; the parse kernel reads the rest.
  const bool inline_exp = variant_groups(c->variant);
  a.inline_max = inline_exp ? batch_small_max(c, j) : 0;
  st->batch_ws = k.here();
  st->j = j;
  return hip_err(desc ? launch_msg_parse_desc(a, *desc, c->num_cu, stream) : launch_msg_parse(a, c->num_cu, stream));
}

int enqueue_messages_check(DevCtx* c, const MsgStage& st, hipStream_t stream, uint8_t* copy_dst,
                           const uint64_t* copy_off) {
  const MsgArgs& a = st.a;
  // copy-through runs the group-phase kernel whatever c's variant, so the stored CRCs of the records
  // it takes are read there exactly when the parse kernel left them to it (inline_max)
  const int rc = enqueue_batch(c, a.region, a.job_off, a.job_len, nullptr, st.crc, st.j, st.batch_ws, stream,
                               a.inline_max ? a.expected : nullptr, copy_dst, copy_off, copy_dst ? a.gate : nullptr);
  if (rc) return rc;
  return hip_err(launch_msg_reduce(a, stream));
}

}  // namespace detail
}  // namespace ambrycrc

// ================================================================= C ABI
extern "C" {

const char* ambrycrc_strerror(int code) {
  switch (code) {
    case AMBRYCRC_OK: return "ok";
    case AMBRYCRC_EINVAL: return "invalid argument";
    case AMBRYCRC_EHIP: return "HIP runtime error";
    case AMBRYCRC_ENOMEM: return "out of memory";
    case AMBRYCRC_ENOINIT: return "ambrycrc_init() not called for the current device";
    case AMBRYCRC_ENODEV: return "no usable gfx950 device";
    case AMBRYCRC_ECOMM: return "RCCL unavailable or a collective call failed";
    case AMBRYCRC_EPROBE: return "A/B probe build (wrong CRCs) refused: set AMBRYCRC_ALLOW_PROBE=1 to time it";
    default: return "unknown error";
  }
}

const char* ambrycrc_version(void) {
  // "ambrycrc <semver> gfx950", then " ab-probe-build" and " AMBRY_X=v" for every compile-time
  // knob that differs from its product default (build_knobs.h): the product build has neither.
  static const std::string v = [] {
    std::string s = "ambrycrc 0.4.0 gfx950";
    if (AMBRY_IS_PROBE_BUILD) s += " ab-probe-build";
#define AMBRY_KNOB_REPORT(name, def) \
  if ((long)(name) != (long)(def)) s += " " #name "=" + std::to_string((long)(name));
    AMBRY_KNOB_LIST(AMBRY_KNOB_REPORT)
#undef AMBRY_KNOB_REPORT
    return s;
  }();
  return v.c_str();
}

uint32_t ambrycrc_update(uint32_t crc, const void* p, size_t n) {
  if (!p || n == 0) return crc;
  return ~host_update_reg(~crc, static_cast<const uint8_t*>(p), n);
}

const char* ambrycrc_host_impl(void) { return host_impl_name(host_impl()); }

uint32_t ambrycrc_update_iov(uint32_t crc, const void* const* ptrs, const size_t* lens, size_t n) {
  if (!ptrs || !lens) return crc;
  uint32_t reg = ~crc;
  for (size_t i = 0; i < n; ++i)
    if (ptrs[i] && lens[i]) reg = host_update_reg(reg, static_cast<const uint8_t*>(ptrs[i]), lens[i]);
  return ~reg;
}

int ambrycrc_batch_cpu(const void* const* ptrs, const uint64_t* lens, const uint32_t* crc_in, uint32_t* out, size_t n,
                       int threads) {
  if (n == 0) return AMBRYCRC_OK;
  if (!ptrs || !lens || !out || threads < 0) return AMBRYCRC_EINVAL;
  for (size_t i = 0; i < n; ++i)
    if (lens[i] && !ptrs[i]) return AMBRYCRC_EINVAL;
  if (threads == 0) {
    cpu_set_t set;
    threads = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set) : 1;
  }
  threads = (int)std::min<size_t>((size_t)std::max(threads, 1), n);
  auto run = [&](size_t a, size_t b) {
    for (size_t i = a; i < b; ++i) {
      const uint32_t c = crc_in ? crc_in[i] : 0u;
      out[i] = lens[i] ? ~host_update_reg(~c, static_cast<const uint8_t*>(ptrs[i]), lens[i]) : c;
    }
  };
  if (threads == 1) {
    run(0, n);
    return AMBRYCRC_OK;
  }
  std::vector<size_t> cut(threads + 1, n);
  const int rc = ambrycrc_shard_by_bytes(lens, n, threads, cut.data());
  if (rc) return rc;
  std::vector<std::thread> th;
  th.reserve(threads - 1);
  for (int t = 1; t < threads; ++t) {
    if (cut[t] >= cut[t + 1]) continue;
    try {
      th.emplace_back(run, cut[t], cut[t + 1]);
    } catch (...) {  // no thread (the C ABI does not throw): the part runs here
      run(cut[t], cut[t + 1]);
    }
  }
  run(cut[0], cut[1]);
  for (auto& t : th) t.join();
  return AMBRYCRC_OK;
}

uint32_t ambrycrc_update_byte(uint32_t crc, int b) {
  const HostTables& h = host_tables();
  uint32_t c = ~crc;
  c = (c >> 8) ^ h.t[0][(c ^ (uint32_t)b) & 0xff];
  return ~c;
}

uint32_t ambrycrc_combine(uint32_t crc1, uint32_t crc2, uint64_t len2) {
  return gf2_mul(crc1, host_xpow8(len2)) ^ crc2;
}

uint32_t ambrycrc_zeros(uint32_t crc, uint64_t n) {
  // register' = register * x^(8n); value = ~register.
  return ~gf2_mul(~crc, host_xpow8(n));
}

int ambrycrc_init(int device) {
  if (device < 0 || device >= kMaxDevices) return AMBRYCRC_EINVAL;
  if (AMBRY_IS_PROBE_BUILD) {  // a timing build: its CRCs are wrong by construction
    const char* allow = getenv("AMBRYCRC_ALLOW_PROBE");
    if (!allow || strcmp(allow, "1") != 0) return AMBRYCRC_EPROBE;
  }
  std::lock_guard<std::mutex> g(g_mu);
  if (g_ctx[device]) return AMBRYCRC_OK;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device >= count) return AMBRYCRC_ENODEV;
  int prev = 0;
  (void)hipGetDevice(&prev);
  if (hipSetDevice(device) != hipSuccess) return AMBRYCRC_EHIP;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return AMBRYCRC_EHIP;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    (void)hipSetDevice(prev);
    return AMBRYCRC_ENODEV;
  }
  DevCtx* c = new DevCtx();
  c->device = device;
  c->num_cu = prop.multiProcessorCount;
  c->grid = c->num_cu;
  // AMBRYCRC_VARIANT selects a built-in shape for A/B runs; anything else is ignored (a
  // stray value must never change the checksums).
  if (const char* v = getenv("AMBRYCRC_VARIANT")) {
    char* end = nullptr;
    const long x = strtol(v, &end, 10);
    if (end != v && *end == '\0' && x >= 0 && x < 1000 && variant_supported((int)x)) c->variant = (int)x;
  }
  if (const char* v = getenv("AMBRYCRC_REGION")) c->region_mode = strcmp(v, "0") == 0 ? 0 : strcmp(v, "1") == 0 ? 1 : 2;
  if (const char* v = getenv("AMBRYCRC_STREAM_PUT_MAX")) {  // A/B: serialize copy mode's streamed form (0: off)
    char* end = nullptr;
    const unsigned long x = strtoul(v, &end, 10);
    if (end != v && *end == '\0') c->stream_put_max = x < kStreamPutMax ? x : kStreamPutMax;
  }
  if (const char* v = getenv("AMBRYCRC_XFORM_SIDE")) c->xform_side = strcmp(v, "0") == 0 ? 0 : 1;  // A/B: §12.9
  {  // the side-stream verdict needs hipStreamWaitValue32
    int can = 0;
    if (hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, device) != hipSuccess || !can)
      c->xform_side = 0;
  }
  if (const char* v = getenv("AMBRYCRC_XFORM_FAST_MAX")) {  // A/B: the transform fast path's cut-off
    char* end = nullptr;
    const unsigned long long x = strtoull(v, &end, 10);
    if (end != v && *end == '\0' && x <= (1ull << 30)) c->xform_fast_max = x;
  }
  if (const char* v = getenv("AMBRYCRC_FUSED_PROC")) {  // A/B: processor waves of the one-pass kernels
    char* end = nullptr;
    const long x = strtol(v, &end, 10);
    if (end != v && *end == '\0' && x >= 0 && x <= kFusedProcMax) c->fused_proc = (int)x;
  }
  if (const char* v = getenv("AMBRYCRC_REGION_MAX_PER_MESSAGE")) {  // A/B: the region-mode cut-off
    char* end = nullptr;
    const unsigned long long x = strtoull(v, &end, 10);
    if (end != v && *end == '\0' && x > 0 && x <= (1ull << 30)) c->region_max = x;
  }
  if (const char* v = getenv("AMBRYCRC_XFORM_HOST_VERDICT")) c->xform_host_verdict = strcmp(v, "1") == 0;
  std::vector<uint32_t> img = build_table_image();
  // the table image, then one 256-B line of device words (d_path)
  const size_t img_bytes = (img.size() * 4 + 255) & ~size_t(255);
  if (hipMalloc(reinterpret_cast<void**>(&c->d_img), img_bytes + 256) != hipSuccess) {
    delete c;
    return AMBRYCRC_ENOMEM;
  }
  c->d_path = c->d_img + img_bytes / 4;
  if (hipMemcpy(c->d_img, img.data(), img.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(c->d_path, 0xFF, 256) != hipSuccess) {
    free_ctx(c);
    return AMBRYCRC_EHIP;
  }
  if (hipHostMalloc(reinterpret_cast<void**>(&c->h_words), DevCtx::kHostWords * sizeof(uint32_t),
                    hipHostMallocDefault) != hipSuccess) {
    c->h_words = nullptr;
    free_ctx(c);
    return AMBRYCRC_ENOMEM;
  }
  g_ctx[device] = c;
  (void)hipSetDevice(prev);
  return AMBRYCRC_OK;
}

int ambrycrc_shutdown(void) {
  std::lock_guard<std::mutex> g(g_mu);
  int prev = 0;
  (void)hipGetDevice(&prev);
  for (int d = 0; d < kMaxDevices; ++d) {
    free_ctx(g_ctx[d]);
    g_ctx[d] = nullptr;
  }
  (void)hipSetDevice(prev);
  return AMBRYCRC_OK;
}

size_t ambrycrc_workspace_bytes(size_t n) { return ws_need(n); }

int ambrycrc_batch_dev(const uint8_t* d_base, const uint64_t* d_off, const uint64_t* d_len, const uint32_t* d_crc_in,
                       uint32_t* d_out, size_t n, void* d_ws, size_t ws_bytes, hipStream_t stream) {
  if (n == 0) return AMBRYCRC_OK;
  if (!d_base || !d_off || !d_len || !d_out || n >= (1ull << 31)) return AMBRYCRC_EINVAL;
  if (!same_or_disjoint(d_crc_in, d_out, n)) return AMBRYCRC_EINVAL;
  DevCtx* c = ctx_current();
  if (!c) return AMBRYCRC_ENOINIT;
  WsLease lease;
  const int rc = lease.acquire(c, stream, &d_ws, ws_bytes, ws_need(n));
  if (rc) return rc;
  return enqueue_batch(c, d_base, d_off, d_len, d_crc_in, d_out, n, d_ws, stream);
}

int ambrycrc_verify_dev(const uint8_t* d_base, const uint64_t* d_off, const uint64_t* d_len, const uint32_t* d_crc_in,
                        const uint32_t* d_expected, uint32_t* d_out, uint8_t* d_mismatch, uint32_t* d_mismatch_count,
                        size_t n, void* d_ws, size_t ws_bytes, hipStream_t stream) {
  if (n == 0) return AMBRYCRC_OK;
  if (!d_base || !d_off || !d_len || !d_expected || n >= (1ull << 31)) return AMBRYCRC_EINVAL;
  if (!same_or_disjoint(d_crc_in, d_out, n)) return AMBRYCRC_EINVAL;
  DevCtx* c = ctx_current();
  if (!c) return AMBRYCRC_ENOINIT;
  // Without a caller d_out, the CRCs live in the workspace after the batch's own part.
  Carver need(nullptr);
  verify_scratch(need, n, !d_out);
  WsLease lease;
  int rc = lease.acquire(c, stream, &d_ws, ws_bytes, need.bytes());
  if (rc) return rc;
  Carver k(d_ws);
  if (!d_out) d_out = verify_scratch(k, n, true);
  rc = enqueue_batch(c, d_base, d_off, d_len, d_crc_in, d_out, n, d_ws, stream);
  if (rc) return rc;
  return hip_err(launch_verify(d_out, d_expected, d_mismatch, d_mismatch_count, (uint32_t)n, stream));
}

int ambrycrc_put_crcs(const uint8_t* const* fields, const uint64_t* field_len, const uint8_t* const* prefix,
                      const uint64_t* prefix_len, const uint32_t* blob_crc, const uint64_t* blob_len, size_t n,
                      uint32_t* wire_out, uint32_t* record_out) {
  if (n == 0) return AMBRYCRC_OK;
  if (!blob_crc || !blob_len) return AMBRYCRC_EINVAL;
  if (wire_out && (!fields || !field_len)) return AMBRYCRC_EINVAL;
  if (record_out && (!prefix || !prefix_len)) return AMBRYCRC_EINVAL;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t xb = host_xpow8(blob_len[i]);  // shared by both combines
    if (wire_out) wire_out[i] = gf2_mul(ambrycrc_update(0, fields[i], field_len[i]), xb) ^ blob_crc[i];
    if (record_out) record_out[i] = gf2_mul(ambrycrc_update(0, prefix[i], prefix_len[i]), xb) ^ blob_crc[i];
  }
  return AMBRYCRC_OK;
}

int ambrycrc_set_variant(int device, int variant) {
  DevCtx* c = ctx_for(device);
  if (!c) return AMBRYCRC_ENOINIT;
  if (!variant_supported(variant)) return AMBRYCRC_EINVAL;
  c->variant = variant;
  return AMBRYCRC_OK;
}

long ambrycrc_set_put_stream_max(int device, long bytes) {
  DevCtx* c = ctx_for(device);
  if (!c) return AMBRYCRC_ENOINIT;
  if (bytes < 0 || (uint64_t)bytes > kStreamPutMax) return AMBRYCRC_EINVAL;
  const long prev = (long)c->stream_put_max;
  c->stream_put_max = (uint64_t)bytes;
  return prev;
}

int ambrycrc_set_region_mode(int device, int enable) {
  DevCtx* c = ctx_for(device);
  if (!c) return AMBRYCRC_ENOINIT;
  if (enable < 0 || enable > 2) return AMBRYCRC_EINVAL;
  c->region_mode = enable;
  return AMBRYCRC_OK;
}


int ambrycrc_get_region_mode(int device) {
  DevCtx* c = ctx_for(device);
  return c ? c->region_mode : AMBRYCRC_ENOINIT;
}

int ambrycrc_last_message_mode(int device) {
  DevCtx* c = ctx_for(device);
  return c ? c->last_msg_mode.load() : AMBRYCRC_ENOINIT;
}

int ambrycrc_last_transform_path(int device) {
  DevCtx* c = ctx_for(device);
  if (!c) return AMBRYCRC_ENOINIT;
  const int p = c->last_xform_path.load();
  if (p != 2) return p;
  // decided on the device: region_patch_kernel's word, once the device has finished the call
  uint32_t w = ~0u;
  int prev = 0;
  (void)hipGetDevice(&prev);
  if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(&w, c->d_path, sizeof w, hipMemcpyDeviceToHost) != hipSuccess) {
    (void)hipSetDevice(prev);
    return AMBRYCRC_EHIP;
  }
  (void)hipSetDevice(prev);
  return w <= 1 ? (int)w : -1;
}

int ambrycrc_set_transform_verdict(int device, int host) {
  DevCtx* c = ctx_for(device);
  if (!c) return AMBRYCRC_ENOINIT;
  if (host != 0 && host != 1) return AMBRYCRC_EINVAL;
  const int prev = c->xform_host_verdict.exchange(host);
  return prev;
}

int ambrycrc_get_variant(int device) {
  DevCtx* c = ctx_for(device);
  return c ? c->variant : AMBRYCRC_ENOINIT;
}

int ambrycrc_set_grid(int device, int workgroups) {
  DevCtx* c = ctx_for(device);
  if (!c) return AMBRYCRC_ENOINIT;
  if (workgroups < 0) return AMBRYCRC_EINVAL;
  c->grid = workgroups ? workgroups : c->num_cu;
  return AMBRYCRC_OK;
}

int ambrycrc_grid_size(int device) {
  DevCtx* c = ctx_for(device);
  return c ? c->grid : 0;
}

int ambrycrc_set_window(int device, uint64_t bytes) {
  DevCtx* c = ctx_for(device);
  if (!c) return AMBRYCRC_ENOINIT;
  if (bytes != 0 && bytes < (1u << 20)) return AMBRYCRC_EINVAL;
  c->window = bytes;
  return AMBRYCRC_OK;
}

int ambrycrc_timing_enable(int device, int enable) {
  DevCtx* c = ctx_for(device);
  if (!c) return AMBRYCRC_ENOINIT;
  c->timing = enable != 0;
  return AMBRYCRC_OK;
}

int ambrycrc_timing_collect_each(int device, float* ms_out, int cap, int* launches) {
  DevCtx* c = ctx_for(device);
  if (!c) return AMBRYCRC_ENOINIT;
  if (cap < 0 || (cap > 0 && !ms_out)) return AMBRYCRC_EINVAL;
  std::lock_guard<std::mutex> g(c->ev_mu);
  int cnt = 0;
  for (auto& e : c->pending) {
    if (hipEventSynchronize(e.b) != hipSuccess) return AMBRYCRC_EHIP;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e.a, e.b) != hipSuccess) return AMBRYCRC_EHIP;
    if (cnt < cap) ms_out[cnt] = ms;
    ++cnt;
    c->free_events.push_back(e);
  }
  c->pending.clear();
  if (launches) *launches = cnt;
  return AMBRYCRC_OK;
}

int ambrycrc_timing_collect(int device, double* total_ms, int* launches) {
  DevCtx* c = ctx_for(device);
  if (!c) return AMBRYCRC_ENOINIT;
  std::vector<float> ms;
  {
    std::lock_guard<std::mutex> g(c->ev_mu);
    ms.resize(c->pending.size() + 4096);  // room for launches recorded meanwhile
  }
  int cnt = 0;
  const int rc = ambrycrc_timing_collect_each(device, ms.data(), (int)ms.size(), &cnt);
  if (rc != AMBRYCRC_OK) return rc;
  double sum = 0;
  cnt = std::min(cnt, (int)ms.size());
  for (int i = 0; i < cnt; ++i) sum += ms[i];
  if (total_ms) *total_ms = sum;
  if (launches) *launches = cnt;
  return AMBRYCRC_OK;
}

int ambrycrc_fill_random_dev(uint8_t* d_dst, uint64_t nbytes, uint64_t seed, uint64_t stream_off,
                             hipStream_t stream) {
  if (nbytes == 0) return AMBRYCRC_OK;
  if (!d_dst || (reinterpret_cast<uintptr_t>(d_dst) & 15) || (stream_off & 15)) return AMBRYCRC_EINVAL;
  return hip_err(launch_fill(d_dst, nbytes, seed, stream_off, stream));
}

int ambrycrc_debug_readbw_dev(const uint8_t* d_base, uint64_t nbytes, uint32_t* d_out, int variant,
                              hipStream_t stream) {
  DevCtx* c = ctx_current();
  if (!c) return AMBRYCRC_ENOINIT;
  if (!d_base || !d_out) return AMBRYCRC_EINVAL;
  return hip_err(launch_readbw(d_base, nbytes, d_out, c->grid, variant, stream));
}

size_t ambrycrc_messages_workspace_bytes(size_t m) {
  // job arrays, then the batch workspace of job mode or the run sums of region mode (a region of
  // up to kRegionMaxPerMessage bytes per message: region / 16 bytes + two super-blocks' slack)
  const size_t region = m * (kRegionMaxPerMessage / 16) + 2048 + 512 + 4 * m;
  return msg_jobs_bytes(m) + std::max(ws_need((size_t)kMsgSlots * m), region);
}

int ambrycrc_verify_messages_dev(const uint8_t* d_region, uint64_t region_len, const uint64_t* d_msg_off, size_t m,
                                 uint32_t* d_status, uint64_t* d_msg_end, void* d_ws, size_t ws_bytes,
                                 hipStream_t stream) {
  if (m == 0) return AMBRYCRC_OK;
  if (!d_region || !d_msg_off || !d_status || (size_t)kMsgSlots * m >= (1ull << 31)) return AMBRYCRC_EINVAL;
  DevCtx* c = ctx_current();
  if (!c) return AMBRYCRC_ENOINIT;
  WsLease lease;
  size_t need = ambrycrc_messages_workspace_bytes(m);
  // The library's own workspace also covers region mode past the default per-message size
  // (AMBRYCRC_REGION_MAX_PER_MESSAGE, for A/B runs); a caller's is used as sized.
  if (!d_ws && c->region_mode && region_len <= c->region_max * (uint64_t)m)
    need = std::max(need, msg_jobs_bytes(m) + region_ws_bytes(d_region, region_len, m));
  const int rc = lease.acquire(c, stream, &d_ws, ws_bytes, need);
  if (rc) return rc;
  return enqueue_messages(c, d_region, region_len, d_msg_off, m, d_status, d_msg_end, d_ws,
                          ws_bytes ? ws_bytes : need, stream);
}

size_t ambrycrc_trailed_workspace_bytes(size_t n) { return trailed_own_bytes(n) + ws_need(n); }

int ambrycrc_verify_trailed_dev(const uint8_t* d_base, const uint64_t* d_off, const uint64_t* d_len,
                                uint8_t* d_mismatch, uint32_t* d_mismatch_count, size_t n, void* d_ws,
                                size_t ws_bytes, hipStream_t stream) {
  if (n == 0) return AMBRYCRC_OK;
  if (!d_base || !d_off || !d_len || n >= (1ull << 31)) return AMBRYCRC_EINVAL;
  DevCtx* c = ctx_current();
  if (!c) return AMBRYCRC_ENOINIT;
  WsLease lease;
  int rc = lease.acquire(c, stream, &d_ws, ws_bytes, ambrycrc_trailed_workspace_bytes(n));
  if (rc) return rc;
  Carver k(d_ws);
  TrailerArgs a;
  a.base = d_base;
  a.off = d_off;
  a.len = d_len;
  a.n = n;
  uint32_t* crc = trailed_own(k, n, a);
  a.mismatch = d_mismatch;
  a.count = d_mismatch_count;
  const bool inline_exp = variant_groups(c->variant);
  a.inline_max = inline_exp ? batch_small_max(c, n) : 0;
  if (launch_trailer_parse(a, stream) != hipSuccess) return AMBRYCRC_EHIP;
  rc = enqueue_batch(c, d_base, d_off, a.job_len, nullptr, crc, n, k.here(), stream,
                         a.inline_max ? a.expected : nullptr);
  if (rc) return rc;
  return hip_err(launch_trailer_verify(a, stream));
}

long ambrycrc_debug_table_image(uint32_t* out, size_t max_words) {
  std::vector<uint32_t> img = build_table_image();
  if (!out || max_words < img.size()) return AMBRYCRC_EINVAL;
  memcpy(out, img.data(), img.size() * 4);
  return (long)(img.size() * 4);
}

}  // extern "C"
