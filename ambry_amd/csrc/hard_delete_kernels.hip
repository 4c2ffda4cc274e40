// hard_delete_kernels.hip -- gfx950 kernels of the batched hard delete (ambrycrc_hard_delete_messages_dev):
// BlobStoreHardDelete.getHardDeleteInfo (ambry-messageformat/.../BlobStoreHardDelete.java:97-179) for
// many stored PUT messages of a log region in HBM, in place.
//
// Pipeline (all on the caller's stream; ambrycrc_hd.cpp):
//   hd_parse_kernel  one thread per message: the header's verdict and spans (msg_header.h, from the
//                    header words of msg_parse.h), update messages refused, then either
//                    the recovery info checked against the header's spans, or the user-metadata and
//                    blob records' field checks and two CRC jobs (the records less their stored CRCs)
//   plan + sweep     the batch CRC engine over the 2m jobs (crc32_kernels.hip; empty jobs cost nothing)
//   hd_seal_kernel   one thread per message: final status; for a clean message the two record
//                    prefixes and CRC trailers -- crc(prefix || 0^n) = the prefix CRC shifted by
//                    x^(8n), no pass over the zeros -- and two zero-fill jobs
//   plan             exclusive scan of the fill jobs' costs
//   hd_fill_kernel   persistent, cost-balanced zero fill of the record bodies (store-only)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ambrycrc.h"
#include "crc32_gf2.h"
#include "crc32_kernels.h"
#include "crc32_layout.h"
#include "crc_img.h"
#include "hard_delete.h"
#include "msg_parse.h"
#include "wave_tools.h"

namespace ambrycrc {

typedef uint32_t u32x4p __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void hd_parse_kernel(HdArgs a) {
  __shared__ uint32_t tbl[1024];
  stage_slice_tables(tbl, a.img);
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t off = a.msg_off[i];
    const bool in_region = off <= a.region_len;  // an offset past the region is refused, never dereferenced
    const uint64_t rem = in_region ? a.region_len - off : 0;
    const uint8_t* p = a.region + (in_region ? off : 0);
    const HeaderWords hw = load_header(p, rem);
    uint32_t status;
    HdSpans s{0, 0, 0, 0};
    // the header's verdict and record spans (msg_header.h), then the two spans (hard_delete.h)
    MsgHeader H;
    MsgLayout L;
    status = in_region ? msg_decode(HeaderWordSrc{hw}, rem, HeaderWordCrc{hw, tbl}, &H) : (uint32_t)AMBRYCRC_MSG_BAD_LAYOUT;
    if (status == 0) status = msg_layout(H, rem, &L);
    if (status == 0) status = hd_header_spans(H, L, &s);
    const int v = H.version;  // read only where the status is 0
    uint64_t jo[2] = {0, 0}, jl[2] = {0, 0};
    uint32_t ex[2] = {0, 0}, check = 0;
    ambrycrc_hard_delete_info o;
    __builtin_memset(&o, 0, sizeof o);
    if (status == 0) {
      ambrycrc_hard_delete_info r;
      r.header_version = 0;
      if (a.recovery) r = a.recovery[i];
      if (r.header_version != 0) {  // "Skipping crc check": the records are not read
        if (hd_recovery_ok(r, s)) o = hd_info(v, s, r.usermeta_size, r.blob_version, r.blob_type, r.blob_size);
        else status = AMBRYCRC_MSG_BAD_RECORD;
      } else {
        const uint8_t* um = p + s.um_rel;
        const uint8_t* bl = p + s.blob_rel;
        status = record_check(3, um, s.um_span) | record_check(4, bl, s.blob_span);
        const uint64_t um_crc = ld_be64(um + s.um_span - 8), bl_crc = ld_be64(bl + s.blob_span - 8);
        if (um_crc >> 32) status |= AMBRYCRC_MSG_USERMETA_CRC;  // a CRC32 never has upper bits
        if (bl_crc >> 32) status |= AMBRYCRC_MSG_BLOB_CRC;
        jo[0] = off + s.um_rel;
        jl[0] = s.um_span - 8;
        ex[0] = (uint32_t)um_crc;
        jo[1] = off + s.blob_rel;
        jl[1] = s.blob_span - 8;
        ex[1] = (uint32_t)bl_crc;
        check = 1;
        if (status == 0) {  // the fields record_check just validated
          const int bv = (int)ld_be16(bl);
          o = hd_info(v, s, ld_be32(um + 2), bv, bv == 1 ? 0 : (int)ld_be16(bl + 2), ld_be64(bl + blob_head(bv) - 8));
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      a.job_off[(uint64_t)k * a.m + i] = jo[k];
      a.job_len[(uint64_t)k * a.m + i] = jl[k];
      a.expected[(uint64_t)k * a.m + i] = ex[k];
    }
    a.check[i] = check;
    a.plan[i] = o;
    a.status[i] = status;
  }
}

// v * x^(8n) mod P from the 64 words x^(8*2^k) staged in LDS (crc32_gf2.h).
__device__ __forceinline__ uint32_t mul_xpow8_lds(const uint32_t* __restrict__ xp, uint32_t v, uint64_t n) {
  for (uint32_t k = 0; n; ++k, n >>= 1)
    if (n & 1u) v = gf2_mul(v, xp[k]);
  return v;
}

// One replacement record at q: prefix bytes, then (left to hd_fill_kernel) n zeros, then the CRC of
// prefix || 0^n as a big-endian long -- ambrycrc_zeros(crc(prefix), n).
__device__ __forceinline__ void hd_write_record(uint8_t* q, const uint8_t (&b)[16], uint32_t pn, uint64_t n,
                                                const uint32_t* __restrict__ tbl, const uint32_t* __restrict__ xp) {
#pragma unroll
  for (uint32_t j = 0; j < 13; ++j)
    if (j < pn) q[j] = b[j];
  const uint32_t c = ~mul_xpow8_lds(xp, ~crc_regs_lds(tbl, 0u, b, pn), n);
  put_be64(q + pn + n, (uint64_t)c);
}

__global__ __launch_bounds__(256) void hd_seal_kernel(HdArgs a) {
  __shared__ uint32_t tbl[1024];
  __shared__ uint32_t xp[64];
  stage_slice_tables(tbl, a.img);
  if (threadIdx.x < 64) xp[threadIdx.x] = a.img[kLdsBytes / 4 + threadIdx.x];
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.m) return;
  uint32_t st = a.status[i];
  if (a.check[i]) {
    if (a.crc[i] != a.expected[i]) st |= AMBRYCRC_MSG_USERMETA_CRC;
    if (a.crc[a.m + i] != a.expected[a.m + i]) st |= AMBRYCRC_MSG_BLOB_CRC;
  }
  ambrycrc_hard_delete_info o = a.plan[i];
  uint64_t fo[2] = {0, 0}, fl[2] = {0, 0};
  if (st != 0) {
    __builtin_memset(&o, 0, sizeof o);
  } else if (!a.plan_only) {
    const uint64_t at = a.msg_off[i] + o.start;
    uint8_t b[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t pn = hd_um_prefix(o.usermeta_size, b);
    hd_write_record(a.region + at, b, pn, o.usermeta_size, tbl, xp);
    fo[0] = at + pn;
    fl[0] = o.usermeta_size;
    const uint64_t bat = at + pn + o.usermeta_size + 8;
    pn = hd_blob_prefix(o.blob_version, o.blob_type, o.blob_size, b);
    hd_write_record(a.region + bat, b, pn, o.blob_size, tbl, xp);
    fo[1] = bat + pn;
    fl[1] = o.blob_size;
  }
  a.status[i] = st;
  if (a.info) a.info[i] = o;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    // message-major, so that the short user-metadata jobs are spread over the waves' shares between
    // the blobs (slot-major put 65,536 1000-B jobs on 47 waves: 1.33 ms against 1.06 for 64 KiB blobs)
    a.fill_off[2 * i + k] = fo[k];
    a.fill_len[2 * i + k] = fl[k];
    a.fill_cost[2 * i + k] = copy_job_cost(fl[k]);
  }
}

// ---------------------------------------------------------------- zero fill
// One wave zeroes [dst, dst + n) (wave-uniform arguments): single bytes up to 16-B alignment, the body
// as 16-B stores, lane-strided (1 KiB per wave store), four per lane in flight, then the tail bytes.
// Nothing is read. Plain stores: nontemporal ones measured slower here (1,024 x 4 MiB blobs 1.005 ms a
// fill call against 0.823, 65,536 x 64 KiB 1.058 against 0.971).
__device__ __forceinline__ void fill_range(uint8_t* __restrict__ dst, uint64_t n, uint32_t lane) {
  const uint64_t head0 = (16 - ((uintptr_t)dst & 15)) & 15;
  const uint64_t head = head0 < n ? head0 : n;
  if (lane < head) dst[lane] = 0;
  const uint64_t body = n - head;
  const uint64_t n16 = body >> 4;
  uint8_t* d1 = dst + head;
  u32x4p* d0 = reinterpret_cast<u32x4p*>(d1);
  const u32x4p z = {0u, 0u, 0u, 0u};
  constexpr int U = 4;
  uint64_t p = lane;
  for (; p + 64 * (U - 1) < n16; p += 64 * U) {
#pragma unroll
    for (int u = 0; u < U; ++u) d0[p + 64 * u] = z;
  }
  for (; p < n16; p += 64) d0[p] = z;
  const uint64_t t = body & 15;
  if (lane < t) d1[16 * n16 + lane] = 0;
}

// Persistent, cost-balanced zero fill of the jobs' bytes (cost_share_walk, wave_tools.h).
__global__ __launch_bounds__(256) void hd_fill_kernel(HdFillArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint32_t wave = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) * gridDim.x + blockIdx.x);
  uint64_t w_dst = 0;
  cost_share_walk(
      a.start, a.len, a.n, wave, nwaves, lane, [&](uint32_t i) { w_dst = a.dst_off[i]; },
      [&](uint32_t j, uint64_t r0, uint64_t n) { fill_range(a.dst + readlane64(w_dst, j) + r0, n, lane); });
}

hipError_t launch_hd_parse(const HdArgs& a, hipStream_t s) {
  return launch_items(hd_parse_kernel, blocks_for(a.m), 256, s, a);
}

hipError_t launch_hd_seal(const HdArgs& a, hipStream_t s) {
  return launch_items(hd_seal_kernel, blocks_for(a.m), 256, s, a);
}

hipError_t launch_hd_fill(const HdFillArgs& a, int grid, hipStream_t s) {
  return launch_items(hd_fill_kernel, a.n ? (uint32_t)grid : 0u, 256, s, a);
}

}  // namespace ambrycrc
