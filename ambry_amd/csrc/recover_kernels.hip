// recover_kernels.hip -- gfx950 kernels of the device message chain and of recovery's MessageInfo
// (ambrycrc_chain_messages_dev, ambrycrc_recover_messages_dev).
//
// Every accepted header in [start, region_len) is a node (pos, next = pos + first + total) of a graph
// whose edges all point forward; the chain is the path from `start`. Pipeline, all on the caller's
// stream, no launch waiting on another workgroup:
//   chain_scan          the region streamed once in 16-B nontemporal loads; every byte position tested
//                       for a big-endian short in 1..3 (SWAR), each candidate validated with the chain's
//                       acceptance test (msg_header.h msg_chain_accept); per kScanBlock bytes the node count
//                       and the in-block offsets of the first kStageMax nodes
//   chain_tile_sums     the counts summed per tile of kSumTile blocks
//   chain_prefix        one workgroup: exclusive prefix of the tile sums, the node total
//   chain_compact       one thread a block: its first node's index, its staged nodes written in
//                       position order (the first max_m kept, the position of node max_m the cutoff)
//   chain_rescan        only the blocks with more than kStageMax nodes, read again
//   chain_link          next -> node index by binary search (kNoNode when it is no kept node); the
//                       node at `start` gets ordinal 0; the offsets' UINT64_MAX fill
//   chain_round x R     pointer doubling, one launch a round: a marked node with ordinal r marks
//                       jump_k[i] with r + 2^k; jump_{k+1}[i] = jump_k[jump_k[i]]. A mark is the node's
//                       distance from `start`, so every writer of a slot writes the same value
//   chain_emit          d_msg_off[ordinal] = pos; the path's last node writes the result
//   recover_info        after the verify: one thread per chained message, the MessageInfo fields
//   recover_finish      one thread: the clean prefix's length, where and why recovery stopped
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ambrycrc.h"
#include "crc32_kernels.h"
#include "crc_img.h"
#include "msg_parse.h"
#include "recover.h"
#include "wave_tools.h"

namespace ambrycrc {

namespace {

typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));

// The chain's acceptance test (msg_header.h msg_chain_accept) on the device: the header's 40 bytes in one
// round trip (msg_parse.h load_header), every field and the CRC from those registers, as msg_parse_kernel
// hashes a header. t: the LDS tables of stage_slice_tables. Written out here, not through msg_chain_accept:
// the walk needs the first present offset alone, so V1's four offsets are read where V2 keeps its first four,
// without the shift into the five slots -- through the shared decoder chain_rescan_kernel takes 7 more
// SGPRs and loses a wave of occupancy. The header lattice tests hold it to the shared rule.
struct LdsCrc {
  const uint32_t* t;
};

__device__ __forceinline__ uint32_t chain_header(const uint8_t* p, uint64_t rem, const LdsCrc& crc, uint64_t* next) {
  if (rem < 2) return AMBRYCRC_MSG_BAD_LAYOUT;
  const HeaderWords hw = load_header(p, rem);
  const int v = (int16_t)__builtin_bswap16((uint16_t)hw.w[0]);
  const uint32_t h = msg_header_size(v);
  if (h == 0) return AMBRYCRC_MSG_BAD_VERSION;
  if (rem < h) return AMBRYCRC_MSG_BAD_LAYOUT;
  const uint32_t st_hi = v == 3 ? be32_w0(hw, 8) : v == 2 ? be32_w2(hw, 7) : be32_w2(hw, 6);
  const uint32_t st_lo = v == 3 ? be32_w0(hw, 9) : v == 2 ? be32_w2(hw, 8) : be32_w2(hw, 7);
  if (st_hi != 0 || header_crc(hw, h - 8, crc.t) != st_lo) return AMBRYCRC_MSG_HEADER_CRC;
  int64_t total;
  int32_t rel[kMsgSlots];
  if (v == 3) {
    total = (int64_t)(((uint64_t)be32_w0(hw, 1) << 32) | be32_w0(hw, 2));
#pragma unroll
    for (int k = 0; k < kMsgSlots; ++k) rel[k] = (int32_t)be32_w0(hw, 3 + k);
  } else {
    total = (int64_t)(((uint64_t)be32_w2(hw, 0) << 32) | be32_w2(hw, 1));
    rel[4] = -1;  // V1 has four slots
#pragma unroll
    for (int k = 0; k < kMsgSlots; ++k)
      if (k < (v == 1 ? 4 : 5)) rel[k] = (int32_t)be32_w2(hw, 2 + k);
  }
  int64_t first = -1;
#pragma unroll
  for (int k = kMsgSlots - 1; k >= 0; --k)
    if (rel[k] != -1) first = rel[k];
  if (total <= 0 || first < (int64_t)h || (uint64_t)total > rem || (uint64_t)first > rem - (uint64_t)total)
    return AMBRYCRC_MSG_BAD_LAYOUT;
  *next = (uint64_t)first + (uint64_t)total;
  return 0;
}

// 0x80 in every byte of v that is zero (exact: no borrow between bytes).
__device__ __forceinline__ uint64_t zero_bytes(uint64_t v) {
  const uint64_t m = 0x7F7F7F7F7F7F7F7Full;
  return ~(((v & m) + m) | v | m);
}

// Index of `key` among the sorted pos[0 .. n), or kNoNode.
__device__ __forceinline__ uint32_t find_node(const uint64_t* __restrict__ pos, uint32_t n, uint64_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (pos[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && pos[lo] == key ? lo : kNoNode;
}

// The thread-per-message kernels' grid: capped, and one block for an empty chain (they still run).
uint32_t msg_blocks(const ChainArgs& a, int num_cu, uint32_t per_cu) {
  return blocks_for(a.max_m ? a.max_m : 1, num_cu, per_cu);
}

}  // namespace

// Scan block b = bytes [b * kScanBlock, (b + 1) * kScanBlock) from `base`, the 16-B-aligned address at or
// below region + start; byte x of it is region position start + x - lead. A position belongs to the
// thread whose load holds its first byte; the second byte of a load's last position comes from the
// next lane's load (the same wave) or, for a wave's last lane, from one byte load -- so the pairs that
// straddle two lanes, two waves' loads and two blocks are each seen once, by the lane holding byte 0.
struct ScanGeom {
  const uint8_t* base;
  uint64_t lead, span;  // bytes of the first granule before `start`; base-relative end of the region
};

__device__ __forceinline__ ScanGeom scan_geom(const ChainArgs& a) {
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(a.region + a.start);
  ScanGeom g;
  g.lead = p0 & 15u;
  g.base = reinterpret_cast<const uint8_t*>(p0 - g.lead);
  g.span = g.lead + (a.region_len - a.start);
  return g;
}

// This thread's 16 bytes of block b, and for a wave's last lane the byte after them.
__device__ __forceinline__ void scan_load(const ScanGeom& g, uint64_t b, uint32_t lane, u32x4v& w, uint32_t& tail) {
  const uint64_t x = b * kScanBlock + 16ull * threadIdx.x;
  w = u32x4v{0u, 0u, 0u, 0u};
  tail = 0;
  if (x < g.span) w = __builtin_nontemporal_load(reinterpret_cast<const u32x4v*>(g.base + x));
  if (lane == 63 && x + 16 < g.span) tail = g.base[x + 16];
}

// The nodes among this thread's 16 positions of block b, a bit per byte of its load. Every lane of the
// wave calls this (the shuffle).
__device__ __forceinline__ uint32_t scan_nodes(const ChainArgs& a, const ScanGeom& g, const LdsCrc& crc, uint64_t b,
                                               uint32_t lane, const u32x4v& w, uint32_t tail) {
  const uint64_t x = b * kScanBlock + 16ull * threadIdx.x;
  uint32_t nb = (uint32_t)__shfl((int)w.x, (int)((lane + 1) & 63u)) & 0xffu;
  if (lane == 63) nb = tail;
  const uint64_t lo = (uint64_t)w.x | (uint64_t)w.y << 32, hi = (uint64_t)w.z | (uint64_t)w.w << 32;
  const uint64_t z_lo = zero_bytes(lo), z_hi = zero_bytes(hi);
  const uint64_t v_lo = zero_bytes(lo & 0xFCFCFCFCFCFCFCFCull) & ~z_lo;  // 0x80 in every byte in 1..3
  const uint64_t v_hi = zero_bytes(hi & 0xFCFCFCFCFCFCFCFCull) & ~z_hi;
  const uint64_t v_n = nb >= 1 && nb <= 3 ? 0x80ull : 0ull;
  const uint64_t cand[2] = {z_lo & ((v_lo >> 8) | (v_hi << 56)), z_hi & ((v_hi >> 8) | (v_n << 56))};
  uint32_t nodes = 0;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    uint64_t c = cand[half];
    while (c) {
      const uint32_t i = (uint32_t)(__builtin_ctzll(c) >> 3) + 8u * half;
      c &= c - 1;
      const uint64_t xr = x + i;
      if (xr < g.lead || xr + 2 > g.span) continue;
      const uint64_t pos = a.start + (xr - g.lead);
      uint64_t nx;
      if (chain_header(a.region + pos, a.region_len - pos, crc, &nx) == 0) nodes |= 1u << i;
    }
  }
  return nodes;
}

// Exclusive prefix of v over the 256 threads of the workgroup (*total: their sum). Two barriers.
template <class T>
__device__ __forceinline__ T block_exclusive(T v, T* wsum, uint32_t lane, uint32_t wv, T* total) {
  T inc = v;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const T up = __shfl_up(inc, d);
    if (lane >= d) inc += up;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  T before = 0, sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    if (k < wv) before += wsum[k];
    sum += wsum[k];
  }
  __syncthreads();  // wsum is reused
  *total = sum;
  return before + inc - v;
}

// Node index idx (the idx-th accepted header by position) at region position pos: kept below max_m, the
// cutoff at max_m, dropped above.
__device__ __forceinline__ void put_node(const ChainArgs& a, const LdsCrc& crc, uint64_t idx, uint64_t pos) {
  if (idx < a.max_m) {
    uint64_t nx = 0;
    (void)chain_header(a.region + pos, a.region_len - pos, crc, &nx);
    a.pos[idx] = pos;
    a.next[idx] = pos + nx;
  } else if (idx == a.max_m) {
    a.head->cutoff = pos;
  }
}

// Pass 1: every block's node count, and the in-block offsets of its first kStageMax nodes in position
// order. The next block's load is issued before this block's bytes are looked at.
__global__ __launch_bounds__(256) void chain_scan_kernel(ChainArgs a) {
  __shared__ uint32_t tbl[1024];
  __shared__ uint32_t wsum[4];
  stage_slice_tables(tbl, a.img);
  __syncthreads();
  const LdsCrc crc{tbl};
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const ScanGeom g = scan_geom(a);
  u32x4v w, w_next;
  uint32_t tail, tail_next;
  if (blockIdx.x < a.nblocks) scan_load(g, blockIdx.x, lane, w, tail);
  for (uint64_t b = blockIdx.x; b < a.nblocks; b += gridDim.x) {  // (uniform in the workgroup)
    const uint64_t bn = b + gridDim.x;
    if (bn < a.nblocks) scan_load(g, bn, lane, w_next, tail_next);
    uint32_t nodes = scan_nodes(a, g, crc, b, lane, w, tail);
    const uint32_t cnt = (uint32_t)__builtin_popcount(nodes);
    uint32_t total;
    uint32_t j = block_exclusive(cnt, wsum, lane, wv, &total);
    while (nodes && j < kStageMax) {
      const uint32_t i = (uint32_t)__builtin_ctz(nodes);
      nodes &= nodes - 1;
      a.stage[b * kStageMax + j++] = (uint16_t)(16u * threadIdx.x + i);
    }
    if (threadIdx.x == 0) a.cnt[b] = total;
    w = w_next;
    tail = tail_next;
  }
}

// part[t] = the nodes of tile t (kSumTile blocks).
__global__ __launch_bounds__(256) void chain_tile_sums_kernel(ChainArgs a) {
  __shared__ uint32_t wsum[4];
  static_assert(kSumTile == 256, "one block a thread");
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t b = (uint64_t)blockIdx.x * kSumTile + threadIdx.x;
  uint32_t total;
  (void)block_exclusive(b < a.nblocks ? a.cnt[b] : 0u, wsum, lane, wv, &total);
  if (threadIdx.x == 0) a.part[blockIdx.x] = total;
}

// One workgroup: part[0 .. ntiles) -> its exclusive prefix in place; the head's fields for this call.
__global__ __launch_bounds__(1024) void chain_prefix_kernel(ChainArgs a) {
  __shared__ uint64_t part[1024];
  const uint32_t t = threadIdx.x;
  const uint64_t chunk = (a.ntiles + 1023) / 1024;
  const uint64_t i0 = (uint64_t)t * chunk < a.ntiles ? (uint64_t)t * chunk : a.ntiles;
  const uint64_t i1 = i0 + chunk < a.ntiles ? i0 + chunk : a.ntiles;
  uint64_t sum = 0;
  for (uint64_t i = i0; i < i1; ++i) sum += a.part[i];
  part[t] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {  // inclusive scan of the partial sums
    const uint64_t v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint64_t run = part[t] - sum;
  for (uint64_t i = i0; i < i1; ++i) {
    const uint64_t v = a.part[i];
    a.part[i] = run;
    run += v;
  }
  if (t == 1023) {
    const uint64_t total = part[1023];
    a.head->n = (uint32_t)(total < a.max_m ? total : a.max_m);
    a.head->cutoff = a.region_len;
    a.head->first_bad = kNoNode;
  }
}

// Pass 2, one thread a block: the index of the block's first node, and the staged nodes written in
// position order -- only their headers are read again. A block with more than kStageMax nodes is left to
// chain_rescan_kernel.
__global__ __launch_bounds__(256) void chain_compact_kernel(ChainArgs a) {
  __shared__ uint32_t tbl[1024];
  __shared__ uint64_t wsum[4];
  stage_slice_tables(tbl, a.img);
  __syncthreads();
  const LdsCrc crc{tbl};
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const ScanGeom g = scan_geom(a);
  const uint64_t b = (uint64_t)blockIdx.x * kSumTile + threadIdx.x;
  const uint32_t cnt = b < a.nblocks ? a.cnt[b] : 0u;
  uint64_t total;
  uint64_t idx = a.part[blockIdx.x] + block_exclusive((uint64_t)cnt, wsum, lane, wv, &total);
  if (b >= a.nblocks) return;
  a.blk[b] = idx > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)idx;
  if (cnt == 0 || cnt > kStageMax || idx > a.max_m) return;
  for (uint32_t q = 0; q < cnt; ++q, ++idx)
    put_node(a, crc, idx, a.start + (b * kScanBlock + a.stage[b * kStageMax + q] - g.lead));
}

// The blocks with more than kStageMax nodes again, as pass 1 read them: all their nodes written. A
// workgroup looks at a tile's counts at once and moves on when none is that large.
__global__ __launch_bounds__(256) void chain_rescan_kernel(ChainArgs a) {
  __shared__ uint32_t tbl[1024];
  __shared__ uint32_t wsum[4];
  stage_slice_tables(tbl, a.img);
  __syncthreads();
  const LdsCrc crc{tbl};
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const ScanGeom g = scan_geom(a);
  for (uint64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {  // (uniform in the workgroup)
    const uint64_t mine = t * kSumTile + threadIdx.x;
    if (!__syncthreads_or(mine < a.nblocks && a.cnt[mine] > kStageMax)) continue;
    for (uint64_t b = t * kSumTile; b < (t + 1) * kSumTile && b < a.nblocks; ++b) {
      const uint32_t first_idx = a.blk[b];
      if (a.cnt[b] <= kStageMax || (uint64_t)first_idx > a.max_m) continue;  // (uniform)
      u32x4v w;
      uint32_t tail;
      scan_load(g, b, lane, w, tail);
      uint32_t nodes = scan_nodes(a, g, crc, b, lane, w, tail);
      uint32_t total;
      uint64_t idx = (uint64_t)first_idx + block_exclusive((uint32_t)__builtin_popcount(nodes), wsum, lane, wv, &total);
      while (nodes) {
        const uint32_t i = (uint32_t)__builtin_ctz(nodes);
        nodes &= nodes - 1;
        put_node(a, crc, idx++, a.start + (b * kScanBlock + 16ull * threadIdx.x + i - g.lead));
      }
    }
  }
}

__global__ __launch_bounds__(256) void chain_link_kernel(ChainArgs a) {
  const uint32_t n = a.head->n;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.max_m; i += (uint64_t)gridDim.x * blockDim.x) {
    a.msg_off[i] = ~0ull;
    if (i >= n) continue;
    a.jump[0][i] = find_node(a.pos, n, a.next[i]);
    a.ord[i] = a.pos[i] == a.start ? 0u : kNoNode;
  }
}

// Round k: in = jump[k & 1] holds the node 2^k hops on. A mark read while another thread of this launch
// writes it is either absent (the writer's round marks that slot's successors in a later round, as
// planned) or the node's true distance, whose successor's distance is that plus 2^k: harmless.
__global__ __launch_bounds__(256) void chain_round_kernel(ChainArgs a, uint32_t k) {
  const uint32_t n = a.head->n;
  const uint32_t* __restrict__ in = a.jump[k & 1u];
  uint32_t* __restrict__ out = a.jump[(k & 1u) ^ 1u];
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t j = in[i];
    const uint32_t o = __hip_atomic_load(&a.ord[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (j == kNoNode) {
      out[i] = kNoNode;
      continue;
    }
    if (o != kNoNode) __hip_atomic_store(&a.ord[j], o + (1u << k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    out[i] = in[j];
  }
}

// Where and why the walk stopped at position e after `chained` messages.
__device__ __forceinline__ void chain_result(const ChainArgs& a, const uint32_t* tbl, uint64_t chained, uint64_t e) {
  ambrycrc_recover_result r;
  r.chained = chained;
  r.recovered = chained;
  r.end_off = e;
  r.end_status = 0;
  r.more = 0;
  if (e != a.region_len) {
    if (e >= a.head->cutoff || chained == a.max_m) {
      r.more = 1;
    } else {
      uint64_t nx;
      r.end_status = chain_header(a.region + e, a.region_len - e, LdsCrc{tbl}, &nx);
    }
  }
  *a.result = r;
}

__global__ __launch_bounds__(256) void chain_emit_kernel(ChainArgs a) {
  __shared__ uint32_t tbl[1024];
  stage_slice_tables(tbl, a.img);
  __syncthreads();
  const uint32_t n = a.head->n;
  if (blockIdx.x == 0 && threadIdx.x == 0 && (n == 0 || a.pos[0] != a.start))  // `start` is no node
    chain_result(a, tbl, 0, a.start);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t o = a.ord[i];
    if (o == kNoNode) continue;
    a.msg_off[o] = a.pos[i];
    const uint64_t e = a.next[i];
    if (find_node(a.pos, n, e) == kNoNode) chain_result(a, tbl, (uint64_t)o + 1, e);  // the path's last node
  }
}

__global__ __launch_bounds__(256) void recover_info_kernel(ChainArgs a) {
  const uint64_t chained = a.result->chained;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.max_m; i += (uint64_t)gridDim.x * blockDim.x) {
    ambrycrc_message_info o;
    __builtin_memset(&o, 0, sizeof o);
    if (i < chained) {
      uint32_t st = a.status[i];
      if (st == 0) {
        const uint64_t off = a.msg_off[i];
        st = message_info_fields(a.region + off, off, &o);
        if (st) a.status[i] = st;
      }
      if (st) atomicMin(&a.head->first_bad, (uint32_t)i);
    } else {
      a.status[i] = AMBRYCRC_MSG_BAD_LAYOUT;  // an unused slot: what the verify says of its UINT64_MAX
    }
    a.info[i] = o;
  }
}

__global__ void recover_finish_kernel(ChainArgs a) {
  const uint32_t fb = a.head->first_bad;
  if (fb == kNoNode || (uint64_t)fb >= a.result->chained) return;
  a.result->recovered = fb;
  a.result->end_off = a.msg_off[fb];
  a.result->end_status = a.status[fb];
  a.result->more = 0;
}

hipError_t launch_chain_scan(const ChainArgs& a, int num_cu, hipStream_t s) {
  return launch_items(chain_scan_kernel, blocks_for(a.nblocks, num_cu, 8, 1), 256, s, a);
}

hipError_t launch_chain_tile_sums(const ChainArgs& a, hipStream_t s) {
  return launch_items(chain_tile_sums_kernel, (uint32_t)a.ntiles, 256, s, a);
}

hipError_t launch_chain_prefix(const ChainArgs& a, hipStream_t s) {
  return launch_items(chain_prefix_kernel, 1, 1024, s, a);
}

hipError_t launch_chain_compact(const ChainArgs& a, hipStream_t s) {
  return launch_items(chain_compact_kernel, (uint32_t)a.ntiles, 256, s, a);
}

hipError_t launch_chain_rescan(const ChainArgs& a, int num_cu, hipStream_t s) {
  return launch_items(chain_rescan_kernel, blocks_for(a.ntiles, num_cu, 8, 1), 256, s, a);
}

hipError_t launch_chain_link(const ChainArgs& a, int num_cu, hipStream_t s) {
  return launch_items(chain_link_kernel, msg_blocks(a, num_cu, 8), 256, s, a);
}

hipError_t launch_chain_round(const ChainArgs& a, uint32_t k, int num_cu, hipStream_t s) {
  return launch_items(chain_round_kernel, msg_blocks(a, num_cu, 8), 256, s, a, k);
}

hipError_t launch_chain_emit(const ChainArgs& a, int num_cu, hipStream_t s) {
  return launch_items(chain_emit_kernel, msg_blocks(a, num_cu, 8), 256, s, a);
}

// As msg_parse_kernel's grid: 2 blocks of 256 a CU, looping past it.
hipError_t launch_recover_info(const ChainArgs& a, int num_cu, hipStream_t s) {
  return launch_items(recover_info_kernel, msg_blocks(a, num_cu, 2), 256, s, a);
}

hipError_t launch_recover_finish(const ChainArgs& a, hipStream_t s) {
  return launch_items(recover_finish_kernel, 1, 1, s, a);
}

}  // namespace ambrycrc
