// region_kernels.hip -- gfx950 kernels of the message verify's and transform's region mode
// (DESIGN.md §8.1): the 64-B run sums of a log region and the one-pass form that verifies or
// re-encodes the region's messages beside them.
//
//   region_runs_kernel    pass 1 of the two-pass form: the raw CRC of every 64-B run of the region
//                         (pass 2, region_msg_kernel, is message_kernels.hip's)
//   region_fused_kernel   one pass: streaming waves hash the runs as pass 1 does, processor waves
//                         (region_proc.h) take their CU's messages as its run sums complete
//   region_tail_kernel    the messages the fused kernel deferred, once every run sum exists
//   region_patch_kernel   the transform fast path's last step: life versions and header CRCs
//
// The wave primitives (LDS staging, quad transpose, run_crc) are crc_wave.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crc32_kernels.h"
#include "crc32_layout.h"
#include "crc_wave.h"
#include "region_proc.h"
#include "wave_tools.h"

namespace ambrycrc {

// ---- region mode, pass 1 (RegionArgs): the raw CRC of every 64-B run of a log region ----
// The wave body of C3 without its fold and tree: each wave streams a contiguous share of 4 KiB
// super-blocks (four coalesced 1 KiB loads per lane, nontemporal, s_setprio 3 while issuing
// them, the next super-block in flight), the quad transpose leaves lane 4m + j the run
// [64m, 64m + 64) of block j, one 16-step slice-by-4 chain from a zero register gives its raw
// CRC, stored at run index 16j + m of the super-block. Loads are unconditional: a piece outside
// the region reads the nearest piece that holds region bytes, zeroed after (the run sums of
// runs that straddle the region's ends are never used; region_msg_kernel (region_crc.h) recomputes those
// runs from the bytes). Runs have no loop-carried state, so consecutive super-blocks' chains
// are independent.
template <bool NT = true>
__device__ __forceinline__ void region_sb_load(const RegionArgs& a, uint64_t s, uint32_t lane, u32x4 (&x)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint64_t p = s * kSuperBlock + (uint64_t)kBlockBytes * i + 16u * lane;
    const uint64_t q = p < a.lo16 ? a.lo16 : (p > a.hi16 ? a.hi16 : p);
    x[i] = ld16<NT>(reinterpret_cast<const u32x4*>(a.base + q));
  }
}

__device__ __forceinline__ void region_sb_zero(const RegionArgs& a, uint64_t s, uint32_t lane, u32x4 (&x)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint64_t p = s * kSuperBlock + (uint64_t)kBlockBytes * i + 16u * lane;
    if (p < a.lo16 || p > a.hi16) x[i] = u32x4{0u, 0u, 0u, 0u};
  }
}

// A/B knobs: AMBRY_RUNS_PROBE 1 = no run sums into LDS, 5 = no global stores,
// 6 = every wave's stores to one 1 KiB line set (timing only, wrong sums); AMBRY_RUNS_STORE_NT 0 =
// plain stores.
__global__ __launch_bounds__(1024) void region_runs_kernel(RegionArgs a) {
  if (a.lng.ctr && blockIdx.x == 0 && threadIdx.x == 0) {  // pass 2's long-record list starts empty
    *a.lng.ctr = 0;
    *a.lng.claim = 0;
  }
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  // Shares wave-major over workgroups, as the sweep kernel's (CU-major shares measured the same).
  const uint32_t wave = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) * gridDim.x + blockIdx.x);
  fill_lds_slices(a.img);
  const uint32_t lane = threadIdx.x & 63u;
  const LaneConst k = make_lane_const(lane);
  // Groups of four super-blocks: contiguous shares (wave w: [s0, s1) in steps of 4), or with
  // AMBRY_RUNS_GIL interleaved over the waves (wave w: groups w, w + nwaves, ...), which keeps all
  // waves' concurrent reads inside a 64 MiB window and their stores inside 4 MiB.
#if AMBRY_RUNS_GIL
  const uint64_t first = 4 * (uint64_t)wave, step = 4 * nwaves, end = a.nsb;
#else
  const uint64_t first = a.nsb * wave / nwaves, step = 4, end = a.nsb * (wave + 1) / nwaves;
#endif
  if (first >= end) return;
  // Four super-block buffers: while one is hashed the next three are in flight. Each buffer is
  // hashed in place and only then reloaded (no register copies of loads still in flight), and every
  // load and store is issued on every path (indices past the end re-read the last super-block;
  // lanes with nothing to store write the workspace's spill line), so each wait is for the oldest
  // buffer only. A group's four super-blocks' sums gather in the wave's LDS buffer (word 64u + run
  // index) and go out as one 16-B store per lane: 1 KiB contiguous per wave, 8 whole 128-B lines.
  uint32_t* buf = g_lds_runs + kSliceBytes / 4 + (threadIdx.x >> 6) * (kRunsBufBytes / 4);
  const uint32_t slot = 16u * (lane & 3u) + (lane >> 2);
  const uint64_t slast = end - 1;
  auto at = [&](uint64_t s) { return s < end ? s : slast; };
  auto hash = [&](uint64_t s, uint32_t u, u32x4 (&cur)[4]) {
    region_sb_zero(a, s, lane, cur);
    quad_transpose_asm(cur);
    const uint32_t r = run_crc<4, 1>(cur, k, 0u);
    if (AMBRY_RUNS_PROBE == 0 || r == 0x9E3779B9u) buf[64u * u + slot] = r;
  };
  u32x4 b0[4], b1[4], b2[4], b3[4];
  region_sb_load<AMBRY_RUNS_NT != 0>(a, first, lane, b0);
  region_sb_load<AMBRY_RUNS_NT != 0>(a, at(first + 1), lane, b1);
  region_sb_load<AMBRY_RUNS_NT != 0>(a, at(first + 2), lane, b2);
  region_sb_load<AMBRY_RUNS_NT != 0>(a, at(first + 3), lane, b3);
  u32x4* spill = reinterpret_cast<u32x4*>(a.rk + kRunPad + a.nsb * 64) + lane;
  for (uint64_t g = first; g < end; g += step) {
    const uint64_t nx = g + step;
    hash(g, 0, b0);
    __builtin_amdgcn_s_setprio(3);
    region_sb_load<AMBRY_RUNS_NT != 0>(a, at(nx), lane, b0);
    __builtin_amdgcn_s_setprio(0);
    if (g + 1 < end) hash(g + 1, 1, b1);
    __builtin_amdgcn_s_setprio(3);
    region_sb_load<AMBRY_RUNS_NT != 0>(a, at(nx + 1), lane, b1);
    __builtin_amdgcn_s_setprio(0);
    if (g + 2 < end) hash(g + 2, 2, b2);
    __builtin_amdgcn_s_setprio(3);
    region_sb_load<AMBRY_RUNS_NT != 0>(a, at(nx + 2), lane, b2);
    __builtin_amdgcn_s_setprio(0);
    if (g + 3 < end) hash(g + 3, 3, b3);
    __builtin_amdgcn_s_setprio(3);
    region_sb_load<AMBRY_RUNS_NT != 0>(a, at(nx + 3), lane, b3);
    __builtin_amdgcn_s_setprio(0);
    const u32x4 v = *reinterpret_cast<const u32x4*>(buf + 4u * lane);
    u32x4* dst = 4u * lane < 64u * (end - g) ? reinterpret_cast<u32x4*>(a.rk + kRunPad + g * 64) + lane : spill;
    if constexpr (AMBRY_RUNS_PROBE == 6) dst = reinterpret_cast<u32x4*>(a.rk + kRunPad) + lane;
    if constexpr (AMBRY_RUNS_PROBE == 5) {
      if (v.x == 0x9E3779B9u) *dst = v;
    } else if constexpr (AMBRY_RUNS_STORE_NT) {
      __builtin_nontemporal_store(v, dst);
    } else {
      *dst = v;
    }
  }
}

hipError_t launch_region_runs(const RegionArgs& a, int grid, hipStream_t s) {
  return launch_items(region_runs_kernel, a.nsb ? (uint32_t)grid : 0u, 1024, s, a);
}

// ---- region mode in one pass: region_fused_kernel (FusedArgs, crc32_kernels.h) ----
// Workgroup b (one per CU) owns groups [G0, G1) of 16 KiB (4 super-blocks). Streaming wave v <
// S = 16 - f.nproc takes groups G0 + v, G0 + v + S, ...: the CU's frontier
// advances S groups at a time, each wave's 4 super-blocks hashed as region_runs_kernel does them,
// the next 4 in flight, the 256 run sums stored as one 1 KiB wave store. At the top of each group
// the wave waits for all its memory operations (the previous group's store included) and publishes
// how many of its groups are complete in LDS (done[v]).
// Processor wave p takes 64-message batches p, p + f.nproc, ... of the CU's messages -- those
// whose offsets lie in the share, found by a 64-way search of the sorted offsets -- waiting on the
// frontier (the longest complete prefix of the share's groups) first until the batch's headers are
// streamed, then until its messages' ends are; then region::process_message. A message that
// starts before the share or ends past it goes to the deferred list for region_tail_kernel.
// Offsets out of order anywhere set ctl[0], and the tail kernel then redoes every message.
// Base-relative position of message i's start (past the region: its end).
__device__ __forceinline__ uint64_t msg_pos(const FusedArgs& f, uint64_t i) {
  const uint64_t o = f.a.msg_off[i];
  return f.g.reg0 + (o < f.a.region_len ? o : f.a.region_len);
}

// Smallest i in [0, m] with msg_pos(i) >= key (sorted offsets), by 64-way probes; every lane
// gets it. Unsorted offsets give some index in [0, m] (the tail kernel redoes them all).
__device__ __forceinline__ uint64_t lower_bound_wave(const FusedArgs& f, uint64_t key, uint32_t lane) {
  uint64_t lo = 0, hi = f.a.m;  // answer in [lo, hi]
  while (hi - lo > 64) {
    const uint64_t n = hi - lo;
    const uint64_t q = lo + n * (lane + 1) / 65;  // lo <= q < hi, increasing with lane
    const uint64_t ball = __ballot(msg_pos(f, q) >= key);
    if (ball == 0) {
      lo = lo + n * 64 / 65 + 1;
    } else {
      const uint32_t L = (uint32_t)__builtin_ctzll(ball);
      const uint64_t qL = lo + n * (L + 1) / 65;
      const uint64_t qP = L ? lo + n * L / 65 : lo;
      hi = qL;
      lo = L ? qP + 1 : lo;
    }
  }
  const uint64_t i = lo + lane;
  const uint64_t ball = __ballot(i < hi && msg_pos(f, i) < key);
  return lo + (uint64_t)__popcll(ball);
}

template <bool COPY, int W>
__global__ __launch_bounds__(64 * W) void region_fused_kernel(FusedArgs f) {
  __shared__ uint32_t tbl[1024];
  __shared__ uint32_t nib[region::kNibTotal];
  __shared__ uint32_t dn[region::kDirSets * region::kNibWords];
  __shared__ uint32_t done[16];
  {  // LDS-DMA of the slice tables (the streamers'), then the processors' compact tables and nibble sets
    issue_lds_slices(f.g.img);
    for (uint32_t i = threadIdx.x; i < 1024; i += blockDim.x) {
      const uint32_t j = i >> 8, b = i & 255u;
      tbl[i] = f.g.img[(((j >> 1) << 16) | (b << 8) | ((j & 1) << 7)) >> 2];
    }
    region::stage_nib(nib, f.g.img);
    region::stage_direct_nib(dn, f.g.img);
    if (threadIdx.x < 16) done[threadIdx.x] = 0;
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t v = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t G0 = f.ngroups * blockIdx.x / gridDim.x, G1 = f.ngroups * (blockIdx.x + 1) / gridDim.x;
  const RegionArgs a = f.g;
  const uint32_t nstream = W - f.nproc;
  if (v < nstream) {
    // ---- streaming wave
    const LaneConst k = make_lane_const(lane);
    uint32_t* buf = g_lds_runs + kSliceBytes / 4 + v * (kRunsBufBytes / 4);
    const uint32_t slot = 16u * (lane & 3u) + (lane >> 2);
    const uint64_t mine = G1 - G0 > v ? (G1 - G0 - v + nstream - 1) / nstream : 0;
    // COPY: out[0] is region byte msg_off[0] (base-relative `shift`); every piece holding region
    // bytes is stored at its place, cut to [shift, shift + out_cap)
    const uint64_t shift = COPY ? a.reg0 + f.a.msg_off[0] : 0;
    auto copy = [&](uint64_t sb, const u32x4 (&cur)[4]) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint64_t p = sb * kSuperBlock + (uint64_t)kBlockBytes * q + 16u * lane;
        if (p < a.lo16 || p > a.hi16 || p + 16 <= shift) continue;  // no region byte at or after out[0]
        const uint64_t d0 = p >= shift ? p - shift : 0;               // its first output byte
        if (d0 >= f.out_cap) continue;
        if (p >= shift && d0 + 16 <= f.out_cap) {
          st16u_nt(f.out + (p - shift), cur[q]);  // streamed once: nontemporal
        } else {  // the piece holding out[0] or out[out_cap - 1]: byte by byte (rare)
          const u32x4 v = cur[q];
#pragma unroll 1
          for (uint32_t b = 0; b < 16; ++b) {
            const uint32_t w = b < 4 ? v.x : b < 8 ? v.y : b < 12 ? v.z : v.w;
            if (p + b >= shift && p + b - shift < f.out_cap) st8g(f.out + (p + b - shift), w >> (8 * (b & 3)));
          }
        }
      }
    };
    auto hash = [&](uint64_t sb, uint32_t u, u32x4 (&cur)[4]) -> uint32_t {
      if constexpr (COPY) copy(sb, cur);
      region_sb_zero(a, sb, lane, cur);
      quad_transpose_asm(cur);
      const uint32_t r = run_crc<4, 1>(cur, k, 0u);
      buf[64u * u + slot] = r;
      return r;
    };
    const uint64_t gfirst = G0 + v, gstep = nstream, mine_n = mine;
    if (mine_n) {
      u32x4 b0[4], b1[4], b2[4], b3[4];
      uint64_t g = gfirst;
      region_sb_load<AMBRY_FUSED_NT != 0>(a, 4 * g, lane, b0);
      region_sb_load<AMBRY_FUSED_NT != 0>(a, 4 * g + 1, lane, b1);
      region_sb_load<AMBRY_FUSED_NT != 0>(a, 4 * g + 2, lane, b2);
      region_sb_load<AMBRY_FUSED_NT != 0>(a, 4 * g + 3, lane, b3);
      for (uint64_t j = 0; j < mine_n; ++j, g += gstep) {
        const uint64_t nx = j + 1 < mine_n ? g + gstep : g;  // the last group re-reads itself
        // COPY: a message that cannot take the fast path anywhere ends the pass (the general path
        // redoes the batch); every 8th group, one L2 read
        if (COPY && (j & 7) == 7 && __hip_atomic_load(f.xfail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        const uint32_t r0 = hash(4 * g, 0, b0);
        if (j >= 2) {
          // Publication of groups 0 .. j - 2 (their run-sum stores were issued before group j's
          // loads): a workgroup-scope release fence, then the relaxed LDS store of done[v], paired
          // with the acquire fence after the processors' poll (wait_for) -- release/acquire in the
          // HIP memory model, the readers being waves of this workgroup. For gfx950 without
          // threadgroup split the compiler implements it with s_waitcnt lgkmcnt(0) alone: a CU's
          // vector memory operations go through its L1 in order, so a processor's later load of a
          // published sum sees the store (ISA diff against the unfenced form: one s_nop became that
          // wait). No s_waitcnt vmcnt(0), which would also drain the loads in flight.
          // z = 0, computed from r0, keeps the store after group j's loads have landed.
          uint32_t z;
          asm volatile("v_mov_b32 %0, 0" : "=v"(z) : "v"(r0));
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          __hip_atomic_store(&done[v], (uint32_t)j - 1u + __builtin_amdgcn_readfirstlane(z), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __builtin_amdgcn_s_setprio(3);
        region_sb_load<AMBRY_FUSED_NT != 0>(a, 4 * nx, lane, b0);
        __builtin_amdgcn_s_setprio(0);
        hash(4 * g + 1, 1, b1);
        __builtin_amdgcn_s_setprio(3);
        region_sb_load<AMBRY_FUSED_NT != 0>(a, 4 * nx + 1, lane, b1);
        __builtin_amdgcn_s_setprio(0);
        hash(4 * g + 2, 2, b2);
        __builtin_amdgcn_s_setprio(3);
        region_sb_load<AMBRY_FUSED_NT != 0>(a, 4 * nx + 2, lane, b2);
        __builtin_amdgcn_s_setprio(0);
        hash(4 * g + 3, 3, b3);
        __builtin_amdgcn_s_setprio(3);
        region_sb_load<AMBRY_FUSED_NT != 0>(a, 4 * nx + 3, lane, b3);
        __builtin_amdgcn_s_setprio(0);
        const u32x4 sums = *reinterpret_cast<const u32x4*>(buf + 4u * lane);
        *(reinterpret_cast<u32x4*>(a.rk + kRunPad + g * 256) + lane) = sums;
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __hip_atomic_store(&done[v], (uint32_t)mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return;
  }
  // ---- processor wave
  const uint32_t p = v - nstream;
  const uint64_t s_lo = G0 * kGroupBytes, s_hi = G1 * kGroupBytes;  // the share, base-relative
  {  // this wave's slice of the global sortedness check
    const uint64_t waves = (uint64_t)gridDim.x * f.nproc, w = (uint64_t)blockIdx.x * f.nproc + p;
    const uint64_t c0 = f.a.m * w / waves, c1 = f.a.m * (w + 1) / waves;
    bool bad = false;
    for (uint64_t i = c0 + lane; i < c1; i += 64)
      if (i + 1 < f.a.m && f.a.msg_off[i] > f.a.msg_off[i + 1]) bad = true;
    if (__ballot(bad) && lane == 0) atomicOr(f.ctl, 1u);
  }
  const uint64_t M0 = blockIdx.x == 0 ? 0 : lower_bound_wave(f, s_lo, lane);
  const uint64_t M1 = blockIdx.x + 1 == gridDim.x ? f.a.m : lower_bound_wave(f, s_hi, lane);
  // frontier: base-relative end of the longest complete prefix of the share's groups
  auto frontier = [&]() -> uint64_t {
    uint64_t q = ~0ull;
    if (lane < nstream)
      q = lane + (uint64_t)nstream *
                     __hip_atomic_load(&done[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint64_t w = __shfl_xor(q, o);
      q = w < q ? w : q;
    }
    return G0 * kGroupBytes + (q < G1 - G0 ? q : G1 - G0) * kGroupBytes;
  };
  auto wait_for = [&](uint64_t target) {
    if (target > s_hi) target = s_hi;
    while (frontier() < target) __builtin_amdgcn_s_sleep(8);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  };
  for (uint64_t b = M0 + 64 * (uint64_t)p; b < M1; b += 64 * (uint64_t)f.nproc) {
    if (COPY && __hip_atomic_load(f.xfail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;  // as the streamers
    const uint64_t i = b + lane;
    const bool have = i < M1;
    // The batch is parsed at once (headers, properties, record heads, stored CRCs: region bytes,
    // there whether streamed or not), then the processor waits until the frontier passes its
    // messages' ends and assembles their record CRCs: after the last group of a share, only that
    // last step is left.
    uint32_t st;
    uint64_t mend;
    const region::TabR tr{reinterpret_cast<const uint8_t*>(g_lds_runs), (lane & 31u) << 2};
    constexpr bool kEnds = COPY ? AMBRY_FUSED_ENDS >= 1 : AMBRY_FUSED_ENDS >= 2;
    region::FastPre pre{false, 0};  // COPY: the fast path's shape checks, right after the parse
    region::process_message<kEnds>(f.a, f.g, tbl, tr, nib, have, i, lane, st, mend, [&](uint64_t pos, uint64_t end) -> bool {
      // the lane's message ends at pos + end (base-relative): before the share, or past it (the
      // copy form: more than kDirectSpan past it; its records past the share are hashed from the
      // bytes) -> the tail's. (Measured: the copy form 0.713 -> 0.695 ms per 262,144 4 KiB PUTs;
      // the verify form 0.385 -> 0.399 ms, so it keeps deferring them.)
      if (pos < s_lo || pos + end > s_hi + (COPY ? kDirectSpan : 0)) {
        const uint32_t at = atomicAdd(f.ctl + 1, 1u);
        if (at < f.a.m) f.defer[at] = (uint32_t)i;  // (unsorted offsets may defer more: ctl[0] covers them)
        return false;
      }
      if constexpr (COPY) pre = region::transform_fast_pre(f, tbl, i, end);
      return true;
    }, [&](uint64_t need) { wait_for(need); }, dn, COPY ? s_hi : ~0ull);
    if constexpr (COPY) region::transform_fast_post(f, st != ~0u, i, st, mend, pre);  // `out` untouched
  }
}

// The deferred messages (or, with ctl[0] set, every message) once all run sums exist: one lane
// per message, 64 per wave, grid-stride over the list.
template <bool COPY>
__global__ __launch_bounds__(256) void region_tail_kernel(FusedArgs f) {
  const bool all = *f.ctl != 0;
  const uint64_t n = all ? f.a.m : f.ctl[1];
  if (n == 0) return;
  if (COPY && all) {  // offsets out of order: not the fast path's layout
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(f.xfail, 1u);
    return;
  }
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  if (n <= waves && (uint64_t)blockIdx.x * (blockDim.x >> 6) >= n) return;  // no message for this block
  __shared__ uint32_t tbl[1024];
  __shared__ uint32_t nib[region::kNibTotal];
  __shared__ uint32_t dn[region::kDirSets * region::kNibWords];
  stage_slice_tables(tbl, f.g.img);
  region::stage_nib(nib, f.g.img);
  region::stage_direct_nib(dn, f.g.img);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t w0 = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (n <= waves) {
    // Few messages (the share boundaries' deferrals): a wave per message, each short record hashed
    // by the wave straight from the region (record_crc_direct), a long one (more than 512 runs)
    // from the run sums (record_crc_runs_wave). Lane 0 alone walking the run sums took 69 us per
    // 262,144-message transform; a run-sum tree per record with gf2 multiplies, 60 us; a lane per
    // 4 MiB message, 12 ms for 4,096 of them.
    for (uint64_t w = w0; w < n; w += waves) {
      const uint64_t i = all ? w : f.defer[w];
      uint32_t st;
      uint64_t mend;
      region::process_message_direct(f.a, f.g, tbl, nib, dn, i, lane, st, mend, COPY ? nullptr : &f.g.lng);
      if constexpr (COPY) region::transform_fast(f, tbl, lane == 0, i, st, mend);
    }
    return;
  }
  for (uint64_t w = w0; 64 * w < n; w += waves) {
    const uint64_t j = 64 * w + lane;
    const bool have = j < n;
    const uint64_t i = have ? (all ? j : f.defer[j]) : 0;
    uint32_t st;
    uint64_t mend;
    region::process_message(f.a, f.g, tbl, region::TabC{tbl}, nib, have, i, lane, st, mend,
                            [](uint64_t, uint64_t) -> bool { return true; }, [](uint64_t) {}, dn);
    if constexpr (COPY) region::transform_fast(f, tbl, have, i, st, mend);
  }
}

// The transform fast path's last step: with *xfail clear (every message qualified, in the fused
// and the tail kernel), each message's life version (bytes 2-3) and header CRC (bytes 36-39; 32-35
// are the stored CRC's zero high word) go into `out` -- after both kernels that wrote `out`'s
// bytes have completed, so no store of theirs can land after these. One lane per message. Also
// the device-side verdict for ambrycrc_last_transform_path (path_out).
__global__ __launch_bounds__(256) void region_patch_kernel(FusedArgs f) {
  const bool fail = __hip_atomic_load(f.xfail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
  if (f.path_out && blockIdx.x == 0 && threadIdx.x == 0) *f.path_out = fail ? 0u : 1u;
  if (fail || !f.life) return;
  const uint64_t off0 = f.a.msg_off[0];
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < f.a.m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t pt = f.patch[i];
    uint8_t* o = f.out + (f.a.msg_off[i] - off0);
    const uint32_t lv = (uint32_t)pt, c = (uint32_t)(pt >> 32);
    o[2] = (uint8_t)(lv >> 8);
    o[3] = (uint8_t)lv;
    o[36] = (uint8_t)(c >> 24);
    o[37] = (uint8_t)(c >> 16);
    o[38] = (uint8_t)(c >> 8);
    o[39] = (uint8_t)c;
  }
}


hipError_t launch_region_fused(const FusedArgs& f, int num_cu, hipStream_t s) {

  if (f.a.m == 0) return hipSuccess;
  const bool copy = f.out != nullptr;
  if (f.ngroups) {
    if (copy)
      hipLaunchKernelGGL((region_fused_kernel<true, kFusedWavesCopy>), dim3((uint32_t)num_cu), dim3(64 * kFusedWavesCopy), 0, s, f);
    else
      hipLaunchKernelGGL((region_fused_kernel<false, kFusedWavesVerify>), dim3((uint32_t)num_cu), dim3(64 * kFusedWavesVerify),
                         0, s, f);
  } else if (hipMemsetAsync(f.ctl, 0xFF, 4, s) != hipSuccess) {  // empty region: all to the tail
    return hipGetLastError();
  }
  // A wave per deferred message whenever there are at most 4 per CU (~1 per share boundary, each
  // maybe a 4 MiB message whose records a lane alone would walk for milliseconds): blocks without a
  // message return before staging their tables.
  const uint32_t blocks = blocks_for(f.a.m, num_cu, 4, 4);
  if (copy) hipLaunchKernelGGL(region_tail_kernel<true>, dim3(blocks), dim3(256), 0, s, f);
  else hipLaunchKernelGGL(region_tail_kernel<false>, dim3(blocks), dim3(256), 0, s, f);
  if (!copy && f.g.lng.ctr) {  // the long records the tail listed, over the whole grid
    const hipError_t e = launch_region_long(f.a, f.g, num_cu, s);
    if (e != hipSuccess) return e;
  }
  if (copy && (f.life || f.path_out)) {
    hipLaunchKernelGGL(region_patch_kernel, dim3(f.life ? blocks_for(f.a.m, num_cu, 8) : 1u), dim3(256), 0, s, f);
  }
  return hipGetLastError();
}

}  // namespace ambrycrc
