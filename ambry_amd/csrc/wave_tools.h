// wave_tools.h -- the wave-level device helpers and the launch helper that the kernel files share:
// one definition each, so a fix to the search or to the cost-share walk is made once. Included by
// the .hip files only (host code never sees it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ambrycrc {

// ---------------------------------------------------------------- wave helpers
__device__ __forceinline__ uint64_t readlane64(uint64_t v, uint32_t lane) {
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, lane);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), lane);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t w = __shfl_xor(v, o);
    v = w > v ? w : v;
  }
  return v;
}

// Largest c in [0, n) with start[c] <= g (start nondecreasing, start[0] = 0): the job or chunk that
// holds position g of an exclusive scan. 64-ary search: one coalesced probe per lane per round,
// log64(n) rounds. Every lane gets the answer (wave-uniform arguments but `lane`).
__device__ __forceinline__ uint32_t find_start(const uint64_t* __restrict__ start, uint32_t n, uint64_t g,
                                               uint32_t lane) {
  uint32_t lo = 0, hi = n;  // invariant: start[lo] <= g, answer in [lo, hi)
  while (hi - lo > 1) {
    const uint32_t step = (hi - lo + 63) / 64;
    const uint32_t idx = lo + lane * step;
    const bool ok = idx < hi && start[idx] <= g;
    const uint64_t m = __ballot(ok);
    const uint32_t last = 63u - (uint32_t)__builtin_clzll(m);
    const uint32_t nhi = lo + (last + 1) * step;
    lo = lo + last * step;
    hi = nhi < hi ? nhi : hi;
  }
  return lo;
}

// The persistent, cost-balanced walk of gather_copy_kernel and hd_fill_kernel: wave `wave` of
// `nwaves` takes [wave * S, (wave + 1) * S) of the jobs' concatenated costs (start = exclusive scan
// of the costs, len[j] + a fixed cost per job, 0 for an empty job; start[n] = their total). Job j's
// bytes are the first len[j] units of its cost range, so every byte is handled by exactly one wave.
// Descriptors 64 at a time (lane l <- job c + l), broadcast by readlane; control flow is
// wave-uniform; no atomics, no hand-off.
//   fetch(i):      lane's load of job i's further words into the caller's lane registers (called by
//                  the lanes that hold a job of the window only)
//   body(j, r0, n): bytes [r0, r0 + n) of the job in lane j's registers (n > 0, all wave-uniform)
// The caller computes wave and nwaves: read from blockDim / gridDim here, the kernel's launch bounds
// are no longer folded into them (a dependent load of the group size in the prologue).
template <class Fetch, class Body>
__device__ __forceinline__ void cost_share_walk(const uint64_t* start, const uint64_t* len, uint32_t n, uint32_t wave,
                                                uint64_t nwaves, uint32_t lane, Fetch fetch, Body body) {
  const uint64_t total = start[n];
  uint64_t S = (total + nwaves - 1) / nwaves;
  S = (S + 255) & ~uint64_t(255);
  S = S < 4096 ? 4096 : S;
  const uint64_t g0 = (uint64_t)wave * S;
  if (g0 >= total) return;
  const uint64_t g1 = g0 + S < total ? g0 + S : total;
  uint32_t c = __builtin_amdgcn_readfirstlane(find_start(start, n, g0, lane));
  while (c < n) {
    const uint32_t cnt = n - c < 64u ? n - c : 64u;
    uint64_t w_st = ~0ull, w_len = 0;
    if (lane < cnt) {
      w_st = start[c + lane];
      w_len = len[c + lane];
      fetch(c + lane);
    }
    bool work = false;
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint64_t st = readlane64(w_st, j);
      if (st >= g1) return;
      const uint64_t ln = readlane64(w_len, j);
      if (ln == 0) continue;
      work = true;
      const uint64_t r0 = g0 > st ? g0 - st : 0;
      const uint64_t r1 = g1 - st < ln ? g1 - st : ln;
      if (r0 < r1) body(j, r0, r1 - r0);
    }
    // A window of empty jobs (refused messages; the encryption-key slot of messages without one:
    // cost 0, all at one start) may be the head of a long run; jump to its end instead of walking it
    // 64 at a time.
    uint32_t next = c + cnt;
    if (!work && next < n) {
      const uint32_t far = __builtin_amdgcn_readfirstlane(find_start(start, n, readlane64(w_st, cnt - 1), lane));
      next = far > next ? far : next;
    }
    c = next;
  }
}

// ---------------------------------------------------------------- launch helpers
// Blocks of `threads` for `items` one-per-thread items, at most num_cu * per_cu of them (per_cu 0:
// uncapped; the kernels behind a cap loop over their items). 0 items give 0 blocks.
inline uint32_t blocks_for(uint64_t items, int num_cu = 0, uint32_t per_cu = 0, uint32_t threads = 256) {
  uint64_t blocks = (items + threads - 1) / threads;
  const uint64_t cap = (uint64_t)(num_cu > 0 ? num_cu : 1) * per_cu;
  if (cap && blocks > cap) blocks = cap;
  return (uint32_t)blocks;
}

// Launches `kernel` on `blocks` x `threads`; 0 blocks (nothing to do) is no launch and no error.
template <class... P, class... A>
inline hipError_t launch_items(void (*kernel)(P...), uint32_t blocks, uint32_t threads, hipStream_t s, const A&... args) {
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, s, args...);
  return hipGetLastError();
}

}  // namespace ambrycrc
