// ambrycrc_host.cpp -- the host-resident path of libambrycrc: the entries whose bytes live in host
// memory (ambrycrc_*_host, ambrycrc_batch_multi). Each call takes the CPU leg or a GPU leg (the leg
// policy and its rate tracking are here); the three GPU legs -- batch, message verify, transform --
// stage their bytes through one ring of pinned slabs per device (HostCall, SlabRing, stage_span).
#include "../../include/ambrycrc.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sched.h>
#if defined(__x86_64__)
#include <emmintrin.h>
#endif

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "ambrycrc_ctx.h"

using namespace ambrycrc;
using namespace ambrycrc::detail;

namespace {

// ------------------------------------------------------------ staging copy pool
// Pageable host chunks (a Netty direct ByteBuf, a FileChannel read buffer) must be
// memcpy'd into a pinned slab before the DMA engine can move them. One core copies
// ~25 GB/s, half of PCIe Gen5 x16, so the slab fill is split over a few worker
// threads (AMBRYCRC_COPY_THREADS, default 8; 1 disables the pool). Process-wide,
// started on first use; jobs from concurrent callers interleave safely.
class CopyPool {
 public:
  static CopyPool& get() {
    static CopyPool pool;
    return pool;
  }
  int threads() const { return nthreads_; }
  // Runs fn(0..parts-1) across the workers and the calling thread; returns when all are done.
  void run(int parts, const std::function<void(int)>& fn) {
    if (parts <= 1 || workers_.empty()) {
      for (int i = 0; i < parts; ++i) fn(i);
      return;
    }
    Batch b{&fn, parts};
    {
      std::lock_guard<std::mutex> g(mu_);
      for (int i = 1; i < parts; ++i) queue_.push_back({&b, i});
    }
    cv_.notify_all();
    fn(0);
    finish_one(b);
    // help with this batch's remaining parts instead of idling
    for (;;) {
      Job j{nullptr, 0};
      {
        std::lock_guard<std::mutex> g(mu_);
        for (size_t q = 0; q < queue_.size(); ++q)
          if (queue_[q].batch == &b) {
            j = queue_[q];
            queue_.erase(queue_.begin() + q);
            break;
          }
      }
      if (!j.batch) break;
      (*j.batch->fn)(j.part);
      finish_one(b);
    }
    std::unique_lock<std::mutex> lk(b.mu);
    b.cv.wait(lk, [&] { return b.left == 0; });
  }
  ~CopyPool() {
    {
      std::lock_guard<std::mutex> g(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : workers_) t.join();
  }

 private:
  struct Batch {
    const std::function<void(int)>* fn;
    int left;
    std::mutex mu;
    std::condition_variable cv;
  };
  struct Job {
    Batch* batch;
    int part;
  };
  CopyPool() {
    int t = 8;
    if (const char* e = getenv("AMBRYCRC_COPY_THREADS")) t = atoi(e);
    nthreads_ = std::max(1, std::min(t, 64));
    try {
      for (int i = 1; i < nthreads_; ++i) workers_.emplace_back([this] { loop(); });
    } catch (...) {  // fewer workers than asked (the C ABI does not throw): the parts queue on those started
    }
    nthreads_ = (int)workers_.size() + 1;
  }
  static void finish_one(Batch& b) {
    std::lock_guard<std::mutex> g(b.mu);
    if (--b.left == 0) b.cv.notify_all();
  }
  void loop() {
    for (;;) {
      Job j;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || !queue_.empty(); });
        if (stop_ && queue_.empty()) return;
        j = queue_.front();
        queue_.erase(queue_.begin());
      }
      (*j.batch->fn)(j.part);
      finish_one(*j.batch);
    }
  }
  int nthreads_ = 1;
  std::vector<std::thread> workers_;
  std::vector<Job> queue_;
  std::mutex mu_;
  std::condition_variable cv_;
  bool stop_ = false;
};

struct CopyJob {
  uint8_t* dst;
  const uint8_t* src;
  uint64_t n;
};

// Copies the jobs (disjoint destinations) with the pool: the slab's bytes are split into
// `parts` equal ranges, each thread copying its range of every job it overlaps.
void parallel_copy(const std::vector<CopyJob>& jobs, uint64_t total) {
  if (jobs.empty()) return;
  CopyPool& pool = CopyPool::get();
  const int parts = (int)std::min<uint64_t>((uint64_t)pool.threads(), std::max<uint64_t>(1, total >> 20));
  if (parts <= 1) {
    for (const CopyJob& j : jobs) memcpy(j.dst, j.src, j.n);
    return;
  }
  std::vector<uint64_t> start(jobs.size() + 1, 0);
  for (size_t i = 0; i < jobs.size(); ++i) start[i + 1] = start[i] + jobs[i].n;
  pool.run(parts, [&](int p) {
    const uint64_t lo = total * (uint64_t)p / (uint64_t)parts, hi = total * (uint64_t)(p + 1) / (uint64_t)parts;
    size_t i = std::upper_bound(start.begin(), start.end(), lo) - start.begin() - 1;
    for (; i < jobs.size() && start[i] < hi; ++i) {
      const uint64_t a = std::max(lo, start[i]), b = std::min(hi, start[i + 1]);
      if (b > a) memcpy(jobs[i].dst + (a - start[i]), jobs[i].src + (a - start[i]), b - a);
    }
  });
}

// ------------------------------------------------------------ leg policy: the CPU leg's rate
std::atomic<int> g_cpu_threads{0};  // the process's CPU-leg budget (ambrycrc_set_host_cpu_threads(-1, n)); 0: default

// The calibration for `t` threads: each thread hashes its own slice (16 MiB, 256 MiB in all at most,
// 1 MiB at least) of a buffer the calling thread wrote with nontemporal stores -- so the timed pass
// reads DRAM, not the L3, from the pages one writer placed, as a caller's buffer is. Slices each
// thread wrote itself read 440-679 GiB/s against 172-246 measured on a 2 GiB sample the main thread
// wrote (r05ao, r05aq: 16 threads, their own slices near them and in their CCDs' L3); a single
// thread times threads (round 5's first form): 662 against 262.
double calibrate_cpu(int t) {
  const size_t slice = std::max<size_t>(1u << 20, std::min<size_t>(16u << 20, ((size_t)256 << 20) / (size_t)t)) &
                       ~size_t(4095);
  const size_t total = slice * (size_t)t;
  std::unique_ptr<uint8_t[]> buf(new (std::nothrow) uint8_t[total]);  // not zero-filled: first touch below
  if (!buf) return 1.0;
  // The threads hash their slices once from a common start (all spawned and waiting: spawning
  // inside the timed span read ~half the rate on a 16-CPU box), timed from the start to the last
  // thread's end. (A second pass would read the L3.)
  std::atomic<int> ready{0};
  std::atomic<int> go{0};
  std::atomic<int64_t> last_end{0};
  std::atomic<uint32_t> sink{0};
  std::vector<std::thread> th;
  th.reserve(t);
  {
    uint8_t* p = buf.get();
#if defined(__x86_64__)
    for (size_t i = 0; i < total; i += 16) {  // 16-B aligned (new[] of >= 1 MiB, 4 KiB slices)
      const __m128i v = _mm_set_epi32((int)(i * 131u), (int)(i * 7u), (int)(i ^ 0x5bd1e995u), (int)i);
      _mm_stream_si128(reinterpret_cast<__m128i*>(p + i), v);
    }
    _mm_sfence();
#else
    for (size_t i = 0; i < total; ++i) p[i] = (uint8_t)(i * 131u + 7u);
#endif
  }
  auto body = [&](int k) {
    const uint8_t* p = buf.get() + slice * (size_t)k;
    ready.fetch_add(1);
    while (go.load(std::memory_order_acquire) == 0) std::this_thread::yield();
    sink ^= ambrycrc_update(0, p, slice);
    const int64_t e = std::chrono::steady_clock::now().time_since_epoch().count();
    int64_t cur = last_end.load();
    while (e > cur && !last_end.compare_exchange_weak(cur, e)) {
    }
  };
  try {
    for (int k = 0; k < t; ++k) th.emplace_back(body, k);
  } catch (...) {  // no thread for every slice (the C ABI must not throw): release them, no estimate
    go.store(1, std::memory_order_release);
    for (auto& x : th) x.join();
    return 1.0;
  }
  // (the main thread sleeps while it waits: spinning would take a CPU from the hashing threads)
  while (ready.load() < t) std::this_thread::sleep_for(std::chrono::microseconds(20));
  const int64_t t0 = std::chrono::steady_clock::now().time_since_epoch().count();
  go.store(1, std::memory_order_release);
  for (auto& x : th) x.join();
  const double best = std::chrono::duration<double>(std::chrono::steady_clock::duration(last_end.load() - t0)).count();
  if (!(best > 0)) return 1.0;
  return (double)total / best / (double)(1ull << 30);
}

// The CPU leg's CRC rate on c: as its large calls measured it, else the calibration at c's budget.
double host_batch_cpu_gibps(const DevCtx* c) {
  const int t = host_cpu_threads(c);
  const double r = c ? c->cpu_batch_gibps[std::min(t, DevCtx::kMaxCpuThreads)].load() : -1.0;
  return r >= 0 ? r : host_cpu_gibps(t);
}

// A leg's rate from a call of >= 64 MiB folded into `a` (EWMA; a negative rate: not measured yet).
void note_rate(std::atomic<double>& a, uint64_t bytes, double seconds) {
  if (bytes < (64ull << 20) || seconds <= 0) return;
  const double r = (double)bytes / seconds / (double)(1ull << 30);
  const double old = a.load();
  a.store(old < 0 ? r : 0.5 * old + 0.5 * r);
}

double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// The context of a host call (device < 0: none, the CPU leg) and its status.
int host_ctx(int device, DevCtx** c) {
  *c = device >= 0 ? ctx_for(device) : nullptr;
  return device >= 0 && !*c ? AMBRYCRC_ENOINIT : AMBRYCRC_OK;
}

// The sizes a message header (versions 1-3) at p gives, unchecked: the header's own length h, the
// records' total size and the first record's offset from p (-1: the header names no record). False for
// another version or fewer than h bytes in `rem`. msg_header.h's decoder, kept written out for the two
// serial scans below: they walk hundreds of thousands of headers, a cache miss each, and the misses of
// successive messages overlap only as far as the core's reorder window reaches. Through the shared
// decoder (its struct, its CRC verdict before the fields) ambrycrc_chain_messages_host ran a tenth
// slower; the header lattice tests hold this copy to the shared rule.
struct HeaderSizes {
  uint32_t h;
  int64_t total, first;
};
__attribute__((always_inline)) inline bool header_sizes(const uint8_t* p, uint64_t rem, HeaderSizes* s) {
  const int v = (int16_t)ld_be16(p);
  s->h = msg_header_size(v);
  if (s->h == 0 || rem < s->h) return false;
  int32_t rel[kMsgSlots];
  if (v == 1) {
    s->total = (int64_t)ld_be64(p + 2);
    rel[0] = -1;
    for (int k = 0; k < 4; ++k) rel[k + 1] = (int32_t)ld_be32(p + 10 + 4 * k);
  } else if (v == 2) {
    s->total = (int64_t)ld_be64(p + 2);
    for (int k = 0; k < kMsgSlots; ++k) rel[k] = (int32_t)ld_be32(p + 10 + 4 * k);
  } else {
    s->total = (int64_t)ld_be64(p + 4);
    for (int k = 0; k < kMsgSlots; ++k) rel[k] = (int32_t)ld_be32(p + 12 + 4 * k);
  }
  s->first = -1;
  for (int k = 0; k < kMsgSlots; ++k)
    if (rel[k] != -1) {
      s->first = rel[k];
      break;
    }
  return true;
}

// ------------------------------------------------------------ slab ownership
// Every member is allocated on its own, skipping what an earlier (failed) attempt already got, and
// released on its own: a first use that ran out of memory half way is resumed by the next call, and
// ambrycrc_shutdown frees whatever exists.
template <class T>
bool host_alloc(T** p, size_t bytes) {
  return *p || hipHostMalloc(reinterpret_cast<void**>(p), bytes, hipHostMallocDefault) == hipSuccess;
}
template <class T>
bool dev_alloc(T** p, size_t bytes) {
  return *p || hipMalloc(reinterpret_cast<void**>(p), bytes) == hipSuccess;
}
template <class... T>
void host_free(T*&... p) {  // each of them that exists
  ((p ? (void)hipHostFree(p) : (void)0, p = nullptr), ...);
}
template <class... T>
void dev_free(T*&... p) {
  ((p ? (void)hipFree(p) : (void)0, p = nullptr), ...);
}

int alloc_slab(HostSlab& s) {
  if (!host_alloc(&s.h_data, kSlabBytes) || !host_alloc(&s.h_meta, 2 * kSlabChunks * sizeof(uint64_t)) ||
      !host_alloc(&s.h_out, kSlabChunks * sizeof(uint32_t)) || !dev_alloc(&s.d_data, kSlabBytes) ||
      !dev_alloc(&s.d_meta, 2 * kSlabChunks * sizeof(uint64_t)) || !dev_alloc(&s.d_out, kSlabChunks * sizeof(uint32_t)) ||
      !dev_alloc(&s.d_ws, ws_need(kSlabChunks)))
    return AMBRYCRC_ENOMEM;
  if (!s.stream && hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess) return AMBRYCRC_EHIP;
  if (!s.done && hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess) return AMBRYCRC_EHIP;
  return AMBRYCRC_OK;
}
void release_slab(HostSlab& s) {
  host_free(s.h_data, s.h_meta, s.h_out);
  dev_free(s.d_data, s.d_meta, s.d_out, s.d_ws);
  if (s.stream) (void)hipStreamDestroy(s.stream);
  if (s.done) (void)hipEventDestroy(s.done);
  s.stream = nullptr;
  s.done = nullptr;
}

int alloc_slab(MsgSlab& ms) {
  return host_alloc(&ms.h_off, kSlabMsgs * sizeof(uint64_t)) && host_alloc(&ms.h_status, kSlabMsgs * sizeof(uint32_t)) &&
                 host_alloc(&ms.h_end, kSlabMsgs * sizeof(uint64_t)) && dev_alloc(&ms.d_off, kSlabMsgs * sizeof(uint64_t)) &&
                 dev_alloc(&ms.d_status, kSlabMsgs * sizeof(uint32_t)) && dev_alloc(&ms.d_end, kSlabMsgs * sizeof(uint64_t)) &&
                 dev_alloc(&ms.d_ws, ambrycrc_messages_workspace_bytes(kSlabMsgs))
             ? AMBRYCRC_OK
             : AMBRYCRC_ENOMEM;
}
void release_slab(MsgSlab& ms) {
  host_free(ms.h_off, ms.h_status, ms.h_end);
  dev_free(ms.d_off, ms.d_status, ms.d_end, ms.d_ws);
}

int alloc_slab(XformSlab& x) {
  return host_alloc(&x.h_life, kSlabMsgs * sizeof(int16_t)) && dev_alloc(&x.d_life, kSlabMsgs * sizeof(int16_t)) &&
                 host_alloc(&x.h_out, kXformOutBytes) && dev_alloc(&x.d_out, kXformOutBytes) &&
                 host_alloc(&x.h_olen, kSlabMsgs * sizeof(uint64_t)) && dev_alloc(&x.d_olen, kSlabMsgs * sizeof(uint64_t)) &&
                 dev_alloc(&x.d_ooff, kSlabMsgs * sizeof(uint64_t)) &&
                 dev_alloc(&x.d_ws, ambrycrc_transform_workspace_bytes(kSlabMsgs))
             ? AMBRYCRC_OK
             : AMBRYCRC_ENOMEM;
}
void release_slab(XformSlab& x) {
  host_free(x.h_life, x.h_out, x.h_olen);
  dev_free(x.d_life, x.d_out, x.d_olen, x.d_ooff, x.d_ws);
}

template <class Slab>
int setup_slabs(Slab (&slabs)[kSlabs], bool& ready) {
  for (int w = 0; w < kSlabs && !ready; ++w)
    if (const int rc = alloc_slab(slabs[w])) return rc;
  ready = true;
  return AMBRYCRC_OK;
}

// What a leg stages through: the batch leg the slabs alone, message verify its members on top of
// them, the transform its own on top of both.
enum Staging { kStageBatch, kStageMessages, kStageTransform };

// ------------------------------------------------------------ one GPU-leg call
// Holds the device's slabs (c->mu) for the whole call with the call's device current and the
// slabs the leg needs set up; the caller's current device is restored on every way out. What the
// call staged -- slabs committed, messages sent down the oversize path -- is stored in the context
// as the call ends, still under c->mu (ambrycrc_last_host_slabs).
struct HostCall {
  std::lock_guard<std::mutex> lock;
  DevCtx* ctx;
  int prev = 0;
  int rc = AMBRYCRC_OK;
  uint64_t slabs = 0, oversize = 0;
  HostCall(DevCtx* c, int device, Staging need) : lock(c->mu), ctx(c) {
    (void)hipGetDevice(&prev);
    rc = hip_err(hipSetDevice(device));
    if (!rc) rc = setup_slabs(c->slab, c->slabs_ready);
    if (!rc && need >= kStageMessages) rc = setup_slabs(c->msg_slab, c->msg_slabs_ready);
    if (!rc && need >= kStageTransform) rc = setup_slabs(c->xform_slab, c->xform_slabs_ready);
  }
  ~HostCall() {
    ctx->last_host_slabs = slabs;
    ctx->last_host_oversize = oversize;
    (void)hipSetDevice(prev);
  }
};

// The ring of c's kSlabs staging slabs over one call. A leg fills the slab acquire() gives it,
// issues the slab's copies and kernels on the slab's stream and ends with commit(); up to
// kSlabs - 1 slabs are then in flight while the host fills the next. Rec is what the leg must
// remember of a slab in flight; consume(w, rec) runs once slab w's results are on the host, slabs
// in the order they were committed.
//
// A slab whose issue failed is never in flight and nothing of it is consumed; what was issued
// before it is still waited for (and consumed), and what the failed slab itself got as far as
// queueing is waited for too, so no DMA targets a slab the next call refills. The first error is
// the call's status.
template <class Rec>
class SlabRing {
 public:
  SlabRing(DevCtx* c, HostCall& call, std::function<void(int, Rec&)> consume)
      : c_(c), call_(call), consume_(std::move(consume)) {}
  bool ok() const { return rc_ == AMBRYCRC_OK; }
  void fail(int rc) {
    if (ok()) rc_ = rc;
  }
  int slot() const { return k_ % kSlabs; }
  HostSlab& slab() const { return c_->slab[slot()]; }
  // The record of the slab to fill next, its last use drained (the oldest in flight); null when
  // that failed.
  Rec* acquire() {
    fail(drain(slot()));
    return ok() ? &rec_[slot()] : nullptr;
  }
  // Ends the acquired slab's issue, which gave issue_rc: in flight behind its event, or failed.
  bool commit(int issue_rc) {
    HostSlab& s = slab();
    if (!issue_rc) issue_rc = hip_err(hipEventRecord(s.done, s.stream));
    if (issue_rc) {
      (void)hipStreamSynchronize(s.stream);
      fail(issue_rc);
      return false;
    }
    busy_[slot()] = true;
    ++k_;
    ++call_.slabs;
    return true;
  }
  // Waits for and consumes everything in flight, oldest first; the call's status.
  int drain_all() {
    for (int d = 0; d < kSlabs; ++d) fail(drain((k_ + d) % kSlabs));
    return rc_;
  }

 private:
  int drain(int w) {
    if (!busy_[w]) return AMBRYCRC_OK;
    busy_[w] = false;
    if (hipEventSynchronize(c_->slab[w].done) != hipSuccess) return AMBRYCRC_EHIP;
    consume_(w, rec_[w]);
    return AMBRYCRC_OK;
  }
  DevCtx* c_;
  HostCall& call_;
  std::function<void(int, Rec&)> consume_;
  Rec rec_[kSlabs];
  bool busy_[kSlabs] = {};
  int k_ = 0;  // slabs committed; the next uses ring entry k_ % kSlabs
  int rc_ = AMBRYCRC_OK;
};

template <class T>
bool h2d(T* dst, const T* src, size_t count, hipStream_t s) {
  return hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, s) == hipSuccess;
}
template <class T>
bool d2h(T* dst, const T* src, size_t count, hipStream_t s) {
  return hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, s) == hipSuccess;
}

// Pageable bytes into the slab: the jobs (destinations in s.h_data, `bytes` in all) through the copy
// pool -- which overlaps the DMA and kernels of the slabs already issued -- then one H2D of the
// slab's first `used` bytes.
int stage_jobs(HostSlab& s, const std::vector<CopyJob>& jobs, uint64_t bytes, uint64_t used) {
  parallel_copy(jobs, bytes);
  return h2d(s.d_data, s.h_data, used, s.stream) ? AMBRYCRC_OK : AMBRYCRC_EHIP;
}

// The n bytes at src as the slab's data: pinned bytes by one H2D straight from the caller's.
int stage_span(HostSlab& s, const uint8_t* src, uint64_t n, int pinned) {
  if (!n) return AMBRYCRC_OK;
  if (pinned) return h2d(s.d_data, src, n, s.stream) ? AMBRYCRC_OK : AMBRYCRC_EHIP;
  return stage_jobs(s, {{s.h_data, src, n}}, n, n);
}

// ------------------------------------------------------------ the batch leg
int batch_host_gpu(DevCtx* c, const void* const* ptrs, const uint64_t* lens, const uint32_t* crc_in, uint32_t* out,
                   size_t n, int device, int pinned) {
  HostCall call(c, device, kStageBatch);
  if (call.rc) return call.rc;

  // Pieces: chunks are cut at slab boundaries; pieces of one chunk are combined on the host, in
  // order (the ring consumes oldest first).
  struct Piece {
    size_t chunk;
    uint64_t len;
  };
  std::vector<uint32_t> acc(n, 0u);
  for (size_t i = 0; i < n; ++i) acc[i] = crc_in ? crc_in[i] : 0u;
  SlabRing<std::vector<Piece>> ring(c, call, [&](int w, std::vector<Piece>& pieces) {
    const uint32_t* h_out = c->slab[w].h_out;
    for (size_t j = 0; j < pieces.size(); ++j)
      acc[pieces[j].chunk] = ambrycrc_combine(acc[pieces[j].chunk], h_out[j], pieces[j].len);
  });

  size_t ci = 0;
  uint64_t cpos = 0;
  std::vector<CopyJob> copies;
  while (ci < n) {
    std::vector<Piece>* pieces = ring.acquire();
    if (!pieces) break;
    HostSlab& s = ring.slab();
    pieces->clear();
    copies.clear();
    uint64_t used = 0, copy_bytes = 0;
    int rc = AMBRYCRC_OK;
    while (ci < n && pieces->size() < kSlabChunks) {
      const uint64_t rem = lens[ci] - cpos;
      const uint64_t room = kSlabBytes - used;
      if (rem > 0 && room < 16) break;
      const uint64_t take = std::min(rem, room);
      if (take > 0 && !ptrs[ci]) {
        rc = AMBRYCRC_EINVAL;
        break;
      }
      const uint8_t* src = static_cast<const uint8_t*>(ptrs[ci]) + cpos;
      if (pinned) {
        if (take && !h2d(s.d_data + used, src, take, s.stream)) {
          rc = AMBRYCRC_EHIP;
          break;
        }
      } else if (take) {
        copies.push_back({s.h_data + used, src, take});
        copy_bytes += take;
      }
      s.h_meta[pieces->size()] = used;
      s.h_meta[kSlabChunks + pieces->size()] = take;
      pieces->push_back({ci, take});
      used = (used + take + 15) & ~uint64_t(15);
      cpos += take;
      if (cpos >= lens[ci]) {
        ++ci;
        cpos = 0;
      }
      if (used >= kSlabBytes) break;
    }
    const size_t np = pieces->size();
    if (!rc && !pinned && used) rc = stage_jobs(s, copies, copy_bytes, std::min<uint64_t>(used, kSlabBytes));
    if (!rc && (!h2d(s.d_meta, s.h_meta, np, s.stream) ||
                !h2d(s.d_meta + kSlabChunks, s.h_meta + kSlabChunks, np, s.stream)))
      rc = AMBRYCRC_EHIP;
    if (!rc) rc = enqueue_batch(c, s.d_data, s.d_meta, s.d_meta + kSlabChunks, nullptr, s.d_out, np, s.d_ws, s.stream);
    if (!rc && !d2h(s.h_out, s.d_out, np, s.stream)) rc = AMBRYCRC_EHIP;
    if (!ring.commit(rc)) break;
  }
  if (const int rc = ring.drain_all()) return rc;
  for (size_t i = 0; i < n; ++i) out[i] = acc[i];
  return AMBRYCRC_OK;
}

// ------------------------------------------------------------ the message legs
// Bytes of each message that its verify or transform may read (message_extent_of; 0 for an offset
// past the region's end): one header read each, scattered over the region (a cache and TLB miss
// apiece), so they are read by the copy pool's threads in parallel.
std::vector<uint64_t> message_extents(const uint8_t* region, uint64_t region_len, const uint64_t* msg_off, size_t m) {
  std::vector<uint64_t> ext(m);
  CopyPool& pool = CopyPool::get();
  const int parts = (int)std::min<size_t>((size_t)pool.threads(), std::max<size_t>(1, m / 4096));
  pool.run(parts, [&](int p) {
    for (size_t i = m * (size_t)p / (size_t)parts; i < m * (size_t)(p + 1) / (size_t)parts; ++i)
      ext[i] = msg_off[i] > region_len ? 0 : message_extent_of(region + msg_off[i], region_len - msg_off[i]);
  });
  return ext;
}

// One message too large for a slab: whole in device buffers of its own, which the scope owns and
// frees when it ends, and run synchronously on the null stream. The two message legs add their
// outputs and workspace with alloc(), then upload() the message.
struct OversizeMsg {
  std::vector<void*> held;
  bool ok = true;  // every alloc() so far succeeded
  uint8_t* d_buf;
  uint64_t* d_off;
  uint32_t* d_status;
  explicit OversizeMsg(uint64_t n) : d_buf(alloc<uint8_t>(n)), d_off(alloc<uint64_t>(8)), d_status(alloc<uint32_t>(4)) {}
  ~OversizeMsg() {
    for (void* p : held) (void)hipFree(p);
  }
  template <class T>
  T* alloc(size_t bytes) {
    void* p = nullptr;
    if (ok && hipMalloc(&p, bytes) == hipSuccess) held.push_back(p);
    else ok = false;
    return ok ? static_cast<T*>(p) : nullptr;
  }
  int upload(const uint8_t* msg, uint64_t n) {
    const uint64_t zero = 0;
    if (!ok) return AMBRYCRC_ENOMEM;
    const int rc = hip_err(hipMemcpy(d_buf, msg, n, hipMemcpyHostToDevice));
    return rc ? rc : hip_err(hipMemcpy(d_off, &zero, 8, hipMemcpyHostToDevice));
  }
  // The status word and one more 8-byte word of the outputs, back on the host.
  int fetch(uint32_t* status, uint64_t* word, const uint64_t* d_word) {
    const int rc = hip_err(hipMemcpy(status, d_status, 4, hipMemcpyDeviceToHost));
    return rc ? rc : hip_err(hipMemcpy(word, d_word, 8, hipMemcpyDeviceToHost));
  }
};

int verify_oversize(DevCtx* c, const uint8_t* msg, uint64_t n, uint32_t* status, uint64_t* end) {
  OversizeMsg o(n);
  const size_t ws_bytes = ambrycrc_messages_workspace_bytes(1);
  uint64_t* d_end = o.alloc<uint64_t>(8);
  void* d_ws = o.alloc<void>(ws_bytes);
  int rc = o.upload(msg, n);
  if (!rc) rc = enqueue_messages(c, o.d_buf, n, o.d_off, 1, o.d_status, d_end, d_ws, ws_bytes, nullptr);
  return rc ? rc : o.fetch(status, end, d_end);
}

// *bytes: the transformed message when *status == 0, *len long.
int transform_oversize(const uint8_t* msg, uint64_t n, const int16_t* life, int header_version, uint32_t* status,
                       uint64_t* len, std::vector<uint8_t>* bytes) {
  OversizeMsg o(n);
  const uint64_t cap = ambrycrc_transform_out_bound(n, 1);
  const size_t ws_bytes = ambrycrc_transform_workspace_bytes(1);
  uint8_t* d_out = o.alloc<uint8_t>(cap);
  uint64_t* d_ooff = o.alloc<uint64_t>(8);
  uint64_t* d_olen = o.alloc<uint64_t>(8);
  int16_t* d_life = o.alloc<int16_t>(2);
  void* d_ws = o.alloc<void>(ws_bytes);
  int rc = o.upload(msg, n);
  if (!rc && life) rc = hip_err(hipMemcpy(d_life, life, 2, hipMemcpyHostToDevice));
  if (!rc)
    rc = ambrycrc_transform_messages_dev(o.d_buf, n, o.d_off, 1, life ? d_life : nullptr, header_version, d_out, cap,
                                         d_ooff, d_olen, o.d_status, d_ws, ws_bytes, nullptr);
  if (!rc) rc = o.fetch(status, len, d_olen);
  if (!rc && *status == 0) {
    bytes->resize(*len);
    if (*len && hipMemcpy(bytes->data(), d_out, *len, hipMemcpyDeviceToHost) != hipSuccess) rc = AMBRYCRC_EHIP;
  }
  return rc;
}

int verify_messages_host_gpu(DevCtx* c, const uint8_t* region, uint64_t region_len, const uint64_t* msg_off, size_t m,
                             uint32_t* status, uint64_t* msg_end, int device, int pinned) {
  HostCall call(c, device, kStageMessages);
  if (call.rc) return call.rc;

  // Messages in offset order; each slab stages one contiguous span [lo, hi) of the region
  // that covers every packed message's extent. A message whose extent exceeds a slab gets
  // a staging buffer of its own.
  std::vector<size_t> order(m);
  for (size_t i = 0; i < m; ++i) order[i] = i;
  if (!std::is_sorted(msg_off, msg_off + m))  // a recovery scan's offsets already are
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return msg_off[x] < msg_off[y]; });
  const std::vector<uint64_t> ext = message_extents(region, region_len, msg_off, m);

  struct Span {
    uint64_t lo = 0;
    std::vector<size_t> msgs;
  };
  SlabRing<Span> ring(c, call, [&](int w, Span& sp) {
    const MsgSlab& ms = c->msg_slab[w];
    for (size_t q = 0; q < sp.msgs.size(); ++q) {
      status[sp.msgs[q]] = ms.h_status[q];
      if (msg_end) msg_end[sp.msgs[q]] = ms.h_end[q] ? sp.lo + ms.h_end[q] : 0;
    }
  });
  size_t oi = 0;
  while (oi < m && ring.ok()) {
    const size_t first = order[oi];
    const uint64_t lo = std::min(msg_off[first], region_len);
    if (ext[first] > kSlabBytes) {  // (its results do not wait for the slabs in flight: they go by index)
      uint32_t st = 0;
      uint64_t en = 0;
      ++call.oversize;
      ring.fail(verify_oversize(c, region + lo, ext[first], &st, &en));
      status[first] = st;
      if (msg_end) msg_end[first] = en ? lo + en : 0;
      ++oi;
      continue;
    }
    Span* sp = ring.acquire();
    if (!sp) break;
    HostSlab& s = ring.slab();
    MsgSlab& ms = c->msg_slab[ring.slot()];
    sp->lo = lo;
    sp->msgs.clear();
    uint64_t hi = lo;
    while (oi < m && sp->msgs.size() < kSlabMsgs) {
      const size_t i = order[oi];
      const uint64_t o = std::min(msg_off[i], region_len);
      const uint64_t e = o + ext[i];
      if (ext[i] > kSlabBytes || std::max(hi, e) - lo > kSlabBytes) break;
      hi = std::max(hi, e);
      ms.h_off[sp->msgs.size()] = o - lo;
      sp->msgs.push_back(i);
      ++oi;
    }
    const uint64_t span = hi - lo;
    const size_t nm = sp->msgs.size();
    // an offset past the region end must stay past the slab end (BAD_LAYOUT either way)
    for (size_t q = 0; q < nm; ++q)
      if (msg_off[sp->msgs[q]] > region_len) ms.h_off[q] = span + 1;
    int rc = stage_span(s, region + lo, span, pinned);
    if (!rc && !h2d(ms.d_off, ms.h_off, nm, s.stream)) rc = AMBRYCRC_EHIP;
    if (!rc)
      rc = enqueue_messages(c, s.d_data, span, ms.d_off, nm, ms.d_status, ms.d_end, ms.d_ws,
                            ambrycrc_messages_workspace_bytes(kSlabMsgs), s.stream);
    if (!rc && (!d2h(ms.h_status, ms.d_status, nm, s.stream) || !d2h(ms.h_end, ms.d_end, nm, s.stream)))
      rc = AMBRYCRC_EHIP;
    ring.commit(rc);
  }
  return ring.drain_all();
}

int transform_messages_host_gpu(DevCtx* c, const uint8_t* region, uint64_t region_len, const uint64_t* msg_off, size_t m,
                                const int16_t* life_version, int header_version, uint8_t* out, uint64_t out_cap,
                                uint64_t* out_off, uint64_t* out_len, uint32_t* status, int device, int pinned) {
  HostCall call(c, device, kStageTransform);
  if (call.rc) return call.rc;
  // Extents as the verify's (a transform reads nothing outside them either).
  const std::vector<uint64_t> ext = message_extents(region, region_len, msg_off, m);
  // Packing follows ambrycrc_transform_messages_dev over the whole batch: message i's bytes go at
  // the sum of the transformed lengths of the messages before it, or it gets AMBRYCRC_MSG_NO_ROOM
  // when they would pass out_cap (that sum still grows by its length, as the device's exclusive
  // scan of the lengths does). Slabs hold runs of consecutive messages in index order, each run's
  // span [lo, hi) staged once; the slab's transform packs its messages from 0 in the same order.
  uint64_t vpos = 0;  // the device scan's running start
  auto place = [&](size_t i, uint32_t st, uint64_t len, const uint8_t* bytes, std::vector<CopyJob>* jobs) {
    if (st == 0 && len) {
      if (vpos + len <= out_cap) {
        if (out_off) out_off[i] = vpos;
        out_len[i] = len;
        status[i] = 0;
        if (jobs) jobs->push_back({out + vpos, bytes, len});
        else memcpy(out + vpos, bytes, len);
      } else {
        if (out_off) out_off[i] = ~0ull;
        out_len[i] = 0;
        status[i] = AMBRYCRC_MSG_NO_ROOM;
      }
      vpos += len;
      return;
    }
    if (out_off) out_off[i] = ~0ull;
    out_len[i] = 0;
    status[i] = st;
  };
  struct Run {
    size_t i0 = 0, n = 0;
  };
  std::vector<CopyJob> jobs;
  SlabRing<Run> ring(c, call, [&](int w, Run& r) {
    const MsgSlab& ms = c->msg_slab[w];
    const XformSlab& x = c->xform_slab[w];
    jobs.clear();
    uint64_t at = 0, bytes = 0;  // the slab's packed output
    for (size_t q = 0; q < r.n; ++q) {
      const uint64_t len = ms.h_status[q] == 0 ? x.h_olen[q] : 0;
      const size_t before = jobs.size();
      place(r.i0 + q, ms.h_status[q], len, x.h_out + at, &jobs);
      if (jobs.size() > before) bytes += len;
      at += len;
    }
    parallel_copy(jobs, bytes);
  });
  size_t i = 0;
  while (i < m && ring.ok()) {
    if (ext[i] > kSlabBytes) {
      uint32_t st = 0;
      uint64_t len = 0;
      std::vector<uint8_t> bytes;
      ++call.oversize;
      int rc = ring.drain_all();  // the output is packed in message order
      if (!rc)
        rc = transform_oversize(region + std::min(msg_off[i], region_len), ext[i], life_version ? life_version + i : nullptr,
                                header_version, &st, &len, &bytes);
      if (!rc) place(i, st, st == 0 ? len : 0, bytes.data(), nullptr);
      ring.fail(rc);
      ++i;
      continue;
    }
    Run* r = ring.acquire();
    if (!r) break;
    HostSlab& s = ring.slab();
    MsgSlab& ms = c->msg_slab[ring.slot()];
    XformSlab& x = c->xform_slab[ring.slot()];
    uint64_t lo = std::min(msg_off[i], region_len), hi = lo + ext[i];
    size_t n = 0;
    // A run ends where its span would pass a slab, or where the summed extents of its messages
    // (each output at most its extent + the growth bound) would pass the slab's output buffer:
    // messages that share bytes (duplicate offsets) never meet a cap one call over the whole region
    // would not have.
    uint64_t outs = 0;
    while (i + n < m && n < kSlabMsgs && ext[i + n] <= kSlabBytes) {
      const uint64_t o = std::min(msg_off[i + n], region_len), e = o + ext[i + n];
      const uint64_t nlo = std::min(lo, o), nhi = std::max(hi, e);
      const uint64_t nouts = outs + ext[i + n] + AMBRYCRC_TRANSFORM_GROWTH_MAX;
      if (nhi - nlo > kSlabBytes || (n && nouts > kXformOutBytes)) break;
      lo = nlo;
      hi = nhi;
      outs = nouts;
      ++n;
    }
    const uint64_t span = hi - lo;
    for (size_t q = 0; q < n; ++q) {
      ms.h_off[q] = msg_off[i + q] > region_len ? span + 1 : msg_off[i + q] - lo;
      if (life_version) x.h_life[q] = life_version[i + q];
    }
    const uint64_t cap = std::min<uint64_t>(kXformOutBytes, std::max(outs, ambrycrc_transform_out_bound(span, n)));
    int rc = stage_span(s, region + lo, span, pinned);
    if (!rc && (!h2d(ms.d_off, ms.h_off, n, s.stream) || (life_version && !h2d(x.d_life, x.h_life, n, s.stream))))
      rc = AMBRYCRC_EHIP;
    if (!rc)
      rc = ambrycrc_transform_messages_dev(s.d_data, span, ms.d_off, n, life_version ? x.d_life : nullptr, header_version,
                                           x.d_out, cap, x.d_ooff, x.d_olen, ms.d_status, x.d_ws,
                                           ambrycrc_transform_workspace_bytes(kSlabMsgs), s.stream);
    if (!rc && (!d2h(ms.h_status, ms.d_status, n, s.stream) || !d2h(x.h_olen, x.d_olen, n, s.stream) ||
                !d2h(x.h_out, x.d_out, cap, s.stream)))
      rc = AMBRYCRC_EHIP;
    *r = {i, n};
    if (ring.commit(rc)) i += n;
  }
  return ring.drain_all();
}

}  // namespace

namespace ambrycrc {
namespace detail {

int host_cpu_share() {
  static const int share = [] {
    int n = 1;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) n = std::max(1, CPU_COUNT(&set));
    // a cgroup v2 CPU quota ("max 100000" when unlimited): a container's share of a larger machine
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
      char q[32] = {0};
      long long period = 0;
      if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
        const long long quota = atoll(q);
        if (quota > 0) n = std::min<long long>(n, std::max<long long>(1, (quota + period - 1) / period));
      }
      fclose(f);
    }
    if (const char* v = getenv("OMP_NUM_THREADS")) {
      const int t = atoi(v);
      if (t > 0) n = std::min(n, t);
    }
    return std::min(n, 256);
  }();
  return share;
}

int host_cpu_threads(const DevCtx* c) {
  int t = c ? c->cpu_threads.load(std::memory_order_relaxed) : 0;
  if (t <= 0) t = g_cpu_threads.load(std::memory_order_relaxed);
  if (t > 0) return t;
  if (const char* v = getenv("AMBRYCRC_CPU_THREADS")) {
    const int e = atoi(v);
    if (e > 0) return std::min(e, 256);
  }
  return std::max(1, host_cpu_share() / 2);
}

double host_cpu_gibps(int threads) {
  static std::mutex mu;
  static std::vector<std::pair<int, double>> cache;  // (threads, GiB/s), one calibration per budget
  threads = std::max(1, std::min(threads, 256));
  std::lock_guard<std::mutex> g(mu);  // one calibration at a time: concurrent ones would share the CPUs
  for (const auto& e : cache)
    if (e.first == threads) return e.second;
  const double r = calibrate_cpu(threads);
  cache.emplace_back(threads, r);
  return r;
}

bool host_take_cpu(DevCtx* c, int device, int pinned, uint64_t bytes) {
  if (device < 0) return true;
  if (!c || c->host_policy == 1) return false;
  if (c->host_policy == 2) return true;
  if (pinned) return false;
  const bool cpu = host_batch_cpu_gibps(c) > c->gpu_host_gibps.load();
  if (bytes >= (64ull << 20) && c->batch_calls.fetch_add(1) % 16 == 15) return !cpu;  // the other leg's rate
  return cpu;
}

void host_note_cpu(DevCtx* c, uint64_t bytes, double seconds) {
  if (c) note_rate(c->cpu_batch_gibps[std::min(host_cpu_threads(c), DevCtx::kMaxCpuThreads)], bytes, seconds);
}

void host_note_gpu(DevCtx* c, uint64_t bytes, double seconds) {
  if (c) note_rate(c->gpu_host_gibps, bytes, seconds);
}

// The CPU leg of a message entry before it has been measured: verify parses and CRCs each
// message, the transform also copies it out (measured on 16 CPUs, r05ag: verify 86 / 142 GiB/s and
// transform 40 / 60 GiB/s for 4 KiB / 64 KiB PUTs, against a CRC rate of 146-262: ~50 % and ~25 %).
double host_msg_cpu_gibps(const DevCtx* c, int op) {
  const double r = c->msg_cpu_gibps[op].load();
  return r >= 0 ? r
                : host_cpu_gibps(host_cpu_threads(c)) * 0.01 *
                      (op == kMsgVerify ? AMBRY_HOST_VERIFY_CPU_PCT : AMBRY_HOST_XFORM_CPU_PCT);
}

bool host_take_cpu_msg(DevCtx* c, int device, int pinned, int op, uint64_t bytes) {
  if (device < 0) return true;
  if (!c || c->host_policy == 1) return false;
  if (c->host_policy == 2) return true;
  if (pinned) return false;
  const bool cpu = host_msg_cpu_gibps(c, op) > c->msg_gpu_gibps[op].load();
  if (bytes >= (64ull << 20) && c->msg_calls[op].fetch_add(1) % 16 == 15) return !cpu;  // the other leg's rate
  return cpu;
}

void host_note_msg(DevCtx* c, int op, bool cpu, uint64_t bytes, double seconds) {
  if (c) note_rate(cpu ? c->msg_cpu_gibps[op] : c->msg_gpu_gibps[op], bytes, seconds);
}

void release_slabs(DevCtx* c) {
  for (int w = 0; w < kSlabs; ++w) {
    release_slab(c->xform_slab[w]);
    release_slab(c->msg_slab[w]);
    release_slab(c->slab[w]);
  }
  c->slabs_ready = c->msg_slabs_ready = c->xform_slabs_ready = false;
}

// The 40-B header window, and, when the header's sizes fit `rem`, the whole message [0, first
// record + total). Every early exit of msg_parse_kernel reads the header alone, so a staging copy
// of this extent gives the same status bits as the whole region would.
uint64_t message_extent_of(const uint8_t* p, uint64_t rem) {
  const uint64_t hdr = std::min<uint64_t>(rem, 40);
  if (rem < 2) return rem;
  HeaderSizes s;  // msg_header.h's extent rule: no CRC, any first offset >= 0
  if (!header_sizes(p, rem, &s) || s.total <= 0 || s.first < 0 || (uint64_t)s.total > rem ||
      (uint64_t)s.first > rem - (uint64_t)s.total)
    return hdr;
  return std::max<uint64_t>(hdr, (uint64_t)s.first + (uint64_t)s.total);
}

}  // namespace detail
}  // namespace ambrycrc

// ================================================================= C ABI: the host-memory entries
// Host-resident dispatch: the CPU leg or the GPU leg per call.
extern "C" {

int ambrycrc_batch_host(const void* const* ptrs, const uint64_t* lens, const uint32_t* crc_in, uint32_t* out, size_t n,
                        int device, int pinned) {
  if (n == 0) return AMBRYCRC_OK;
  if (!ptrs || !lens || !out) return AMBRYCRC_EINVAL;
  DevCtx* c;
  if (const int rc = host_ctx(device, &c)) return rc;
  uint64_t bytes = 0;
  for (size_t i = 0; i < n; ++i) bytes += lens[i];
  const auto t0 = std::chrono::steady_clock::now();
  if (host_take_cpu(c, device, pinned, bytes)) {
    if (c) c->last_host_path.store(0);
    const int rc = ambrycrc_batch_cpu(ptrs, lens, crc_in, out, n, host_cpu_threads(c));
    if (rc == AMBRYCRC_OK && device >= 0) host_note_cpu(c, bytes, seconds_since(t0));
    return rc;
  }
  c->last_host_path.store(1);
  const int rc = batch_host_gpu(c, ptrs, lens, crc_in, out, n, device, pinned);
  if (rc == AMBRYCRC_OK && !pinned) host_note_gpu(c, bytes, seconds_since(t0));
  return rc;
}

int ambrycrc_batch_multi(const void* const* ptrs, const uint64_t* lens, const uint32_t* crc_in, uint32_t* out,
                         size_t n, const int* devices, int ndev, int pinned) {
  if (ndev <= 0 || ndev > kMaxDevices * 8) return AMBRYCRC_EINVAL;
  if (n == 0) return AMBRYCRC_OK;
  if (!ptrs || !lens || !out) return AMBRYCRC_EINVAL;
  std::vector<int> dev(ndev);
  for (int g = 0; g < ndev; ++g) {
    dev[g] = devices ? devices[g] : g;
    if (!ctx_for(dev[g])) return AMBRYCRC_ENOINIT;
  }
  // host-resident dispatch once for the whole batch: the CPU leg when the CPU threads beat every
  // listed GPU's host path together (auto, pageable), else each range on its GPU
  {
    DevCtx* c0 = ctx_for(dev[0]);
    double gpus = 0;
    for (int g = 0; g < ndev; ++g) gpus += ctx_for(dev[g])->gpu_host_gibps.load();
    const int policy = c0->host_policy.load();
    const bool cpu = policy == 2 || (policy == 0 && !pinned && host_batch_cpu_gibps(c0) > gpus);
    c0->last_host_path.store(cpu ? 0 : 1);
    if (cpu) return ambrycrc_batch_cpu(ptrs, lens, crc_in, out, n, host_cpu_threads(c0));
  }
  std::vector<size_t> cut(ndev + 1, n);
  const int src = ambrycrc_shard_by_bytes(lens, n, ndev, cut.data());
  if (src) return src;
  std::vector<int> rc(ndev, AMBRYCRC_OK);
  std::vector<std::thread> th;
  th.reserve(ndev);
  for (int r = 0; r < ndev; ++r) {
    const size_t a = cut[r], b = cut[r + 1];
    if (a >= b) continue;
    auto part = [&, r, a, b] {
      rc[r] = batch_host_gpu(ctx_for(dev[r]), ptrs + a, lens + a, crc_in ? crc_in + a : nullptr, out + a, b - a, dev[r],
                             pinned);
    };
    try {
      th.emplace_back(part);
    } catch (...) {  // no thread (the C ABI does not throw): this device's share runs here
      part();
    }
  }
  for (auto& t : th) t.join();
  for (int r = 0; r < ndev; ++r)
    if (rc[r]) return rc[r];
  return AMBRYCRC_OK;
}

int ambrycrc_range_checksums_host(const uint8_t* file, uint64_t file_len, const int64_t* first, const int64_t* second,
                                  size_t n, uint32_t* out, int device) {
  if (n == 0) return AMBRYCRC_OK;
  if (!first || !second || !out || (!file && file_len)) return AMBRYCRC_EINVAL;
  for (size_t i = 0; i < n; ++i)
    if (first[i] < 0 || second[i] < 0 || first[i] > second[i]) return AMBRYCRC_EINVAL;
  std::vector<const void*> ptrs(n);
  std::vector<uint64_t> lens(n);
  for (size_t i = 0; i < n; ++i) {
    const uint64_t a = std::min<uint64_t>((uint64_t)first[i], file_len);
    const uint64_t b = std::min<uint64_t>((uint64_t)second[i], file_len);
    ptrs[i] = file ? file + a : nullptr;
    lens[i] = b - a;
  }
  return ambrycrc_batch_host(ptrs.data(), lens.data(), nullptr, out, n, device, 0);
}

int ambrycrc_verify_trailed_host(const void* const* ptrs, const uint64_t* lens, uint8_t* mismatch, size_t n,
                                 int device, int pinned) {
  if (n == 0) return AMBRYCRC_OK;
  if (!ptrs || !lens || !mismatch) return AMBRYCRC_EINVAL;
  std::vector<uint64_t> body(n);
  for (size_t i = 0; i < n; ++i) body[i] = lens[i] >= 8 ? lens[i] - 8 : 0;
  std::vector<uint32_t> crc(n);
  const int rc = ambrycrc_batch_host(ptrs, body.data(), nullptr, crc.data(), n, device, pinned);
  if (rc) return rc;
  for (size_t i = 0; i < n; ++i)
    mismatch[i] = lens[i] < 8 || ambrycrc::ld_be64(static_cast<const uint8_t*>(ptrs[i]) + body[i]) != (uint64_t)crc[i];
  return AMBRYCRC_OK;
}

int ambrycrc_verify_messages_host(const uint8_t* region, uint64_t region_len, const uint64_t* msg_off, size_t m,
                                  uint32_t* status, uint64_t* msg_end, int device, int pinned) {
  if (m == 0) return AMBRYCRC_OK;
  if (!msg_off || !status || (!region && region_len)) return AMBRYCRC_EINVAL;
  DevCtx* c;
  if (const int rc = host_ctx(device, &c)) return rc;
  const bool cpu = host_take_cpu_msg(c, device, pinned, kMsgVerify, region_len);
  if (c) c->last_host_path.store(cpu ? 0 : 1);
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = cpu ? verify_messages_cpu(region, region_len, msg_off, m, status, msg_end, host_cpu_threads(c))
                     : verify_messages_host_gpu(c, region, region_len, msg_off, m, status, msg_end, device, pinned);
  if (rc == AMBRYCRC_OK && !pinned && device >= 0) host_note_msg(c, kMsgVerify, cpu, region_len, seconds_since(t0));
  return rc;
}

int ambrycrc_transform_messages_host(const uint8_t* region, uint64_t region_len, const uint64_t* msg_off, size_t m,
                                     const int16_t* life_version, int header_version, uint8_t* out, uint64_t out_cap,
                                     uint64_t* out_off, uint64_t* out_len, uint32_t* status, int device, int pinned) {
  if (m == 0) return AMBRYCRC_OK;
  if (!msg_off || !out_len || !status || (!region && region_len) || (!out && out_cap) || header_version < 1 ||
      header_version > 3)
    return AMBRYCRC_EINVAL;
  DevCtx* c;
  if (const int rc = host_ctx(device, &c)) return rc;
  const bool cpu = host_take_cpu_msg(c, device, pinned, kMsgTransform, region_len);
  if (c) c->last_host_path.store(cpu ? 0 : 1);
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = cpu ? transform_messages_cpu(region, region_len, msg_off, m, life_version, header_version, out, out_cap,
                                              out_off, out_len, status, host_cpu_threads(c))
                     : transform_messages_host_gpu(c, region, region_len, msg_off, m, life_version, header_version, out,
                                                   out_cap, out_off, out_len, status, device, pinned);
  if (rc == AMBRYCRC_OK && !pinned && device >= 0) host_note_msg(c, kMsgTransform, cpu, region_len, seconds_since(t0));
  return rc;
}

size_t ambrycrc_chain_messages_host(const uint8_t* region, uint64_t region_len, uint64_t start, uint64_t* offs,
                                    size_t max) {
  if (!region || !offs) return 0;
  size_t cnt = 0;
  uint64_t off = start;
  while (cnt < max && off < region_len && region_len - off >= 2) {  // msg_header.h's chain acceptance
    const uint8_t* p = region + off;
    const uint64_t rem = region_len - off;
    HeaderSizes s;
    if (!header_sizes(p, rem, &s)) break;
    if ((uint64_t)ambrycrc_update(0, p, s.h - 8) != ld_be64(p + s.h - 8)) break;
    if (s.total <= 0 || s.first < (int64_t)s.h || (uint64_t)s.total > rem || (uint64_t)s.first > rem - (uint64_t)s.total)
      break;
    offs[cnt++] = off;
    off += (uint64_t)s.first + (uint64_t)s.total;
  }
  return cnt;
}

int ambrycrc_set_host_policy(int device, int policy) {
  DevCtx* c = ctx_for(device);
  if (!c) return AMBRYCRC_ENOINIT;
  if (policy < 0 || policy > 2) return AMBRYCRC_EINVAL;
  return c->host_policy.exchange(policy);
}

int ambrycrc_host_rates(int device, double* cpu_gibps, double* gpu_gibps, int* cpu_threads) {
  DevCtx* c = device < 0 ? nullptr : ctx_for(device);
  if (!c && device >= 0) return AMBRYCRC_ENOINIT;
  const double cpu = host_batch_cpu_gibps(c), gpu = c ? c->gpu_host_gibps.load() : 0.0;
  if (cpu_gibps) *cpu_gibps = cpu;
  if (gpu_gibps) *gpu_gibps = gpu;
  if (cpu_threads) *cpu_threads = host_cpu_threads(c);
  return cpu > gpu ? 0 : 1;  // auto's leg for pageable bytes, whatever the policy
}

int ambrycrc_set_host_cpu_threads(int device, int threads) {
  if (threads < 0 || threads > 256) return AMBRYCRC_EINVAL;
  if (device < 0) return g_cpu_threads.exchange(threads);
  DevCtx* c = ctx_for(device);
  if (!c) return AMBRYCRC_ENOINIT;
  const int prev = c->cpu_threads.exchange(threads);
  if (prev != threads)  // the message legs' measured rates were at the old budget (the batch's are kept per budget)
    for (auto& r : c->msg_cpu_gibps) r.store(-1.0);
  return prev;
}

int ambrycrc_host_calibrate(int device, double* cpu_gibps) {
  DevCtx* c = device < 0 ? nullptr : ctx_for(device);
  if (!c && device >= 0) return AMBRYCRC_ENOINIT;
  const double r = host_cpu_gibps(host_cpu_threads(c));
  if (cpu_gibps) *cpu_gibps = r;
  return AMBRYCRC_OK;
}

int ambrycrc_host_msg_rates(int device, int op, double* cpu_gibps, double* gpu_gibps) {
  DevCtx* c = ctx_for(device);
  if (!c) return AMBRYCRC_ENOINIT;
  if (op != kMsgVerify && op != kMsgTransform) return AMBRYCRC_EINVAL;
  const double cpu = host_msg_cpu_gibps(c, op), gpu = c->msg_gpu_gibps[op].load();
  if (cpu_gibps) *cpu_gibps = cpu;
  if (gpu_gibps) *gpu_gibps = gpu;
  return cpu > gpu ? 0 : 1;
}

int ambrycrc_last_host_path(int device) {
  DevCtx* c = ctx_for(device);
  return c ? c->last_host_path.load() : AMBRYCRC_ENOINIT;
}

int ambrycrc_last_host_slabs(int device, uint64_t info[6]) {
  DevCtx* c = ctx_for(device);
  if (!c) return AMBRYCRC_ENOINIT;
  if (!info) return AMBRYCRC_EINVAL;
  info[0] = kSlabBytes;
  info[1] = kSlabChunks;
  info[2] = kSlabMsgs;
  info[3] = kXformOutBytes;
  std::lock_guard<std::mutex> g(c->mu);
  info[4] = c->last_host_slabs;
  info[5] = c->last_host_oversize;
  return AMBRYCRC_OK;
}

}  // extern "C"
