// recover.h -- the device message chain and the MessageInfo extraction of a log region
// (ambrycrc_chain_messages_dev, ambrycrc_recover_messages_dev / _cpu): the scan geometry the
// tests build their lattices from, the MessageInfo fields of a clean message, and the kernels' arguments
// (recover_kernels.hip, ambrycrc_recover.cpp). The chain's acceptance test is msg_header.h msg_chain_accept.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ambrycrc.h"
#include "msg_header.h"

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

// ---- the MessageInfo fields of recovery (BlobStoreRecovery.java:75-116), read from a message the
// verify found clean (status 0: the header's constraints hold and every record parses, so each read
// below lies inside its record).

// Fills *o for the clean message at p, `off` bytes into its region. 0, or AMBRYCRC_MSG_BAD_INFO when
// the operation time is below -1 (MessageInfo.java:172 throws); *o is then left zero.
__host__ __device__ inline uint32_t message_info_fields(const uint8_t* p, uint64_t off, ambrycrc_message_info* o) {
  __builtin_memset(o, 0, sizeof *o);
  const MsgHeader H = msg_header_of(p);
  const uint32_t v = (uint32_t)H.version, h = H.hs;
  const int32_t enc = H.rel[0], props = H.rel[1], upd = H.rel[2];
  const int32_t first = enc != -1 ? enc : props != -1 ? props : upd;
  int64_t op_time, expires = -1;
  int32_t account = -1, container = -1;
  uint32_t flags = 0;
  if (props != -1) {  // BlobProperties_Format_V1: record version, then the SerDe bytes
    const uint8_t* s = p + props + 2;
    const uint32_t sv = ld_be16(s);
    const int64_t ttl = (int64_t)ld_be64(s + 2);
    op_time = (int64_t)ld_be64(s + 11);
    if (sv > 1) {  // the two shorts follow the three int-strings
      uint64_t pos = kSerdeFixed;
      for (int k = 0; k < 3; ++k) pos += 4 + (uint64_t)ld_be32(s + pos);
      account = (int16_t)ld_be16(s + pos);
      container = (int16_t)ld_be16(s + pos + 2);
    }
    expires = add_seconds_to_epoch(op_time, ttl);
  } else {  // Update_Format_V1 (a delete, no fields: MessageFormatRecord.java:1242), V2 (a delete), V3
    const uint8_t* q = p + upd;
    const uint32_t uv = ld_be16(q);
    op_time = -1;
    uint32_t type = 0;
    if (uv >= 2) {
      account = (int16_t)ld_be16(q + 2);
      container = (int16_t)ld_be16(q + 4);
      op_time = (int64_t)ld_be64(q + 6);
      if (uv == 3) type = ld_be16(q + 14);
    }
    flags = 1u << type;
  }
  if (op_time < -1) return AMBRYCRC_MSG_BAD_INFO;
  o->msg_off = off;
  o->size = (uint64_t)first + (uint64_t)H.total;
  o->expires_at_ms = expires;
  o->operation_time_ms = op_time;
  o->key_rel = h;
  o->key_len = (uint32_t)first - h;
  o->account_id = (int16_t)account;
  o->container_id = (int16_t)container;
  o->life_version = (int16_t)H.life;
  o->flags = (uint8_t)flags;
  o->header_version = (uint8_t)v;
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
