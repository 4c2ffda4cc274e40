// recover.h -- the device message chain and the MessageInfo extraction of a log region
// (ambrycrc_chain_messages_dev, ambrycrc_recover_messages_dev / _cpu): the header
// acceptance test as the CPU entry runs it (recover_kernels.hip restates it over msg_parse.h's header
// words, one memory round trip a header), the scan geometry the tests build their lattices from, and
// the kernels' arguments (recover_kernels.hip, ambrycrc_recover.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ambrycrc.h"
#include "record_fields.h"

namespace ambrycrc {

// The candidate scan reads the region in blocks of kScanBlock bytes, counted from the 16-B-aligned
// address at or below region + start: one workgroup of 256 threads a block, one 16-B load a thread, so
// a wave's load covers kScanWave bytes. Nodes are counted and compacted per block.
constexpr uint32_t kScanBlock = 4096;
constexpr uint32_t kScanWave = 1024;
static_assert(kScanBlock == 256 * 16 && kScanWave == 64 * 16, "one 16-B load a thread");

// The scan stages the in-block offsets of a block's first kStageMax nodes (a V3 update message with a
// 7-byte key is 73 bytes: 56 a block), so that compaction re-reads only the nodes' headers; a block with
// more (shorter messages still, or valid headers packed inside blob content) is scanned again. Block counts are summed in tiles of kSumTile.
constexpr uint32_t kStageMax = 64;
constexpr uint32_t kSumTile = 256;

constexpr uint32_t kNoNode = 0xFFFFFFFFu;  // a jump that leaves the nodes; an ordinal not (yet) marked

// Doubling rounds for max_m nodes: ceil(log2 max_m) + 1, a function of max_m alone.
inline uint32_t chain_rounds(uint64_t max_m) {
  uint32_t r = 0;
  while ((1ull << r) < max_m) ++r;
  return r + 1;
}

// ambrycrc_chain_messages_host's acceptance test for the header at p with rem bytes to the region's
// end, in the reference's order (BlobStoreRecovery.java:51-71): 0 and *next = first record offset +
// message size, or why the walk stops here. crc(p, n): CRC-32 of n bytes at p.
template <class Crc>
__host__ __device__ inline uint32_t chain_header(const uint8_t* p, uint64_t rem, Crc crc, uint64_t* next) {
  if (rem < 2) return AMBRYCRC_MSG_BAD_LAYOUT;
  const int32_t v = (int16_t)ld_be16(p);
  const uint32_t h = v == 1 ? 34u : v == 2 ? 38u : v == 3 ? 40u : 0u;
  if (h == 0) return AMBRYCRC_MSG_BAD_VERSION;
  if (rem < h) return AMBRYCRC_MSG_BAD_LAYOUT;
  if (ld_be32(p + h - 8) != 0 || ld_be32(p + h - 4) != crc(p, h - 8)) return AMBRYCRC_MSG_HEADER_CRC;
  const int64_t total = (int64_t)ld_be64(p + (v == 3 ? 4 : 2));
  const uint8_t* r = p + (v == 3 ? 12 : 10);
  int64_t first = -1;
  for (int k = (v == 1 ? 4 : 5) - 1; k >= 0; --k)
    if ((int32_t)ld_be32(r + 4 * k) != -1) first = (int32_t)ld_be32(r + 4 * k);
  if (total <= 0 || first < (int64_t)h || (uint64_t)total > rem || (uint64_t)first > rem - (uint64_t)total)
    return AMBRYCRC_MSG_BAD_LAYOUT;
  *next = (uint64_t)first + (uint64_t)total;
  return 0;
}

// The chain's state in the workspace, written by the kernels only.
struct ChainHead {
  uint64_t cutoff;     // position of node max_m, or region_len: the nodes kept are those below it
  uint32_t n;          // nodes kept (<= max_m)
  uint32_t first_bad;  // recover: lowest chained index with a non-zero status (kNoNode: none)
  uint64_t pad[6];
};
static_assert(sizeof(ChainHead) == 64, "ChainHead");

struct ChainArgs {
  const uint8_t* region;
  uint64_t region_len, start;
  uint64_t max_m;
  const uint32_t* img;   // the CRC table image
  uint64_t nblocks;      // scan blocks
  uint64_t ntiles;       // tiles of kSumTile scan blocks
  ChainHead* head;
  uint32_t* cnt;         // [nblocks] nodes per scan block
  uint32_t* blk;         // [nblocks] index of a block's first node (saturating at 2^32 - 1, above any max_m)
  uint64_t* part;        // [ntiles] nodes per tile, then their exclusive prefix
  uint16_t* stage;       // [nblocks * kStageMax] in-block offsets of a block's first nodes
  uint64_t *pos, *next;  // [max_m] the nodes in position order: start, and start + first + total
  uint32_t *jump[2];     // [max_m] ping-pong: the node 2^k hops on, or kNoNode
  uint32_t* ord;         // [max_m] distance from `start` along the chain, or kNoNode
  uint64_t* msg_off;     // out
  ambrycrc_recover_result* result;
  // recover
  ambrycrc_message_info* info;
  uint32_t* status;
};

hipError_t launch_chain_scan(const ChainArgs& a, int num_cu, hipStream_t s);
hipError_t launch_chain_tile_sums(const ChainArgs& a, hipStream_t s);
hipError_t launch_chain_prefix(const ChainArgs& a, hipStream_t s);
hipError_t launch_chain_compact(const ChainArgs& a, hipStream_t s);
hipError_t launch_chain_rescan(const ChainArgs& a, int num_cu, hipStream_t s);
hipError_t launch_chain_link(const ChainArgs& a, int num_cu, hipStream_t s);
hipError_t launch_chain_round(const ChainArgs& a, uint32_t k, int num_cu, hipStream_t s);
hipError_t launch_chain_emit(const ChainArgs& a, int num_cu, hipStream_t s);
hipError_t launch_recover_info(const ChainArgs& a, int num_cu, hipStream_t s);
hipError_t launch_recover_finish(const ChainArgs& a, hipStream_t s);

}  // namespace ambrycrc
