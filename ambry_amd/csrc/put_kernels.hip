// put_kernels.hip -- gfx950 kernels of the PUT-message write path (ambrycrc_serialize_puts_dev):
// the batch form of PutMessageFormatInputStream (PutMessageFormatInputStream.java:76-124) +
// MessageFormatInputStream.read* (MessageFormatInputStream.java:40-96), which Ambry's server runs
// per PUT, computing every record CRC while it streams the message out.
//
//   put_layout_kernel   one thread per message: header fields and record prefixes (byte stores,
//                       ~70 B per message), the copy jobs of the variable fields and the CRC jobs
//   gather_copy_kernel  byte-balanced copy of every job (HBM read + write bound): each wave owns
//                       an equal share of the concatenated job bytes; 16-B destination pieces are
//                       built from two aligned source loads and v_alignbyte_b32, so loads and
//                       stores stay coalesced whatever the source/destination misalignment
//   (plan + sweep)      the batch CRC kernels over the CRC jobs, in the output buffer
//   put_seal_kernel     one thread per CRC job: the big-endian 8-B trailer
// Copy mode's messages of at most kStreamPutMax bytes take the streamed form instead of jobs:
//   put_stream_kernel       a wave per message: its bytes, and the raw CRC of every 64-B output run
//                           (the wave primitives of crc_wave.h, as region_runs_kernel hashes them)
//   put_stream_seal_kernel  one thread per message: every record's CRC from the run sums, the trailers
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crc32_kernels.h"
#include "crc32_layout.h"
#include "crc_img.h"
#include "crc_wave.h"
#include "put_emit.h"
#include "put_layout.h"
#include "record_fields.h"
#include "region_crc.h"
#include "wave_tools.h"

namespace ambrycrc {

typedef uint32_t u32x4p __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void put_layout_kernel(PutArgs a) {
  // The CRCs this kernel takes itself (the header's; copy-through's record-prefix seeds) run over
  // bytes it builds in registers, through LDS tables: not over bytes it just stored, read back
  // one dependent global load per byte.
  __shared__ uint32_t tbl[1024];
  if (a.gate && *a.gate == 0) return;  // grid-uniform
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t m = a.m;
  const bool live = i < m;
  ambrycrc_put_desc d;
  PutLayout L;
  const bool ok = live && put_layout(d = a.desc[i], L);
  // copy mode: a message this short is the streamed kernels' (put_stream_kernel) and gets no jobs
  const bool streamed = a.stream_max && ok && L.length <= a.stream_max;
  if (a.clear_short) {  // the job path runs (a long message is present): the streamed ones' entries are empty
    if (streamed) {
      for (uint32_t k = 0; k < kPutSlots; ++k) {
        a.cp_len[k * m + i] = 0;
        a.cp_cost[k * m + i] = 0;
        a.crc_len[k * m + i] = 0;
        a.crc_off[k * m + i] = 0;
        a.crc_in[k * m + i] = 0;
      }
    }
    return;
  }
  bool hashes = a.copy_through || a.in_crc;  // kernel-uniform
  // with streaming, only a block holding a message for the job path hashes (every thread reaches the barrier)
  if (hashes && a.stream_max) hashes = __syncthreads_or(live && !streamed);
  if (hashes) {
    stage_slice_tables(tbl, a.img);
    __syncthreads();
  }
  if (!live) return;
  if (!ok) {  // the host checks descriptors it can see; a bad one here writes nothing
    for (uint32_t k = 0; k < kPutSlots; ++k) {
      a.cp_len[k * m + i] = 0;
      a.cp_cost[k * m + i] = 0;
      a.crc_len[k * m + i] = 0;
      a.crc_off[k * m + i] = 0;
      if (a.copy_through) a.crc_in[k * m + i] = 0;
    }
    if (a.msg_len) a.msg_len[i] = 0;
    return;
  }
  if (a.stream_max) {
    if (streamed) {  // its job entries: zeroed by the clear_short launch only if the job path runs
      if (a.msg_len) a.msg_len[i] = L.length;
      put_write_fixed(d, L, a.out + d.out_off);  // the gaps' bytes, which put_stream_kernel's edge pieces read
      return;
    }
    *a.big = 1u;  // a longer one: the job path runs (every writer stores the same word)
  }
  uint8_t* msg = a.out + d.out_off;
  put_write_fixed(d, L, msg);
  if (hashes) put_emit_header<false>(tbl, d, L, msg);  // (the header's trailer: in both modes that hash)
  uint64_t fo[5];
  put_field_offsets(d, L, fo);
  const uint64_t src[5] = {d.key_src, d.enckey_src, d.props_src, d.usermeta_src, d.blob_src};
  // a transform's V5 re-encoding copies the stored payload; props_fix_kernel completes it
  const uint64_t props_copy = a.pfix && a.pfix[i].version ? a.pfix[i].stored_len : d.props_len;
  const uint64_t len[5] = {d.key_len, L.enc_rec ? (uint64_t)d.enckey_len : 0, props_copy, d.usermeta_len,
                           d.blob_len};
#pragma unroll
  for (uint32_t k = 0; k < kPutSlots; ++k) {
    const uint8_t* base = k == 4 ? a.blobs : a.fields;
    a.cp_src[k * m + i] = base ? (uint64_t)(uintptr_t)(base + src[k]) - a.src_base
                               : (a.copy_through ? (uint64_t)(uintptr_t)(msg + fo[k]) - a.src_base : 0);
    a.cp_dst[k * m + i] = d.out_off + fo[k];
    a.cp_len[k * m + i] = base || a.copy_through ? len[k] : 0;
    a.cp_cost[k * m + i] = base ? copy_job_cost(len[k]) : 0;
    uint64_t off, ln;
    bool present;
    put_crc_job(L, k, &off, &ln, &present);
    a.crc_off[k * m + i] = d.out_off + off;
    a.crc_len[k * m + i] = present ? ln : 0;
    // transform: every record's CRC known
    if (a.in_crc && present && k) put_be64(msg + off + ln, (uint64_t)a.in_crc[4 * i + k - 1]);
    if (a.copy_through) {  // the batch's seeds: each record's prefix CRC (the header is hashed whole, above)
      uint32_t seed = 0;
      if (k && present) {
        uint8_t b[16];
        const uint32_t pl = put_prefix_bytes(d, k, b);
        seed = crc_regs_lds(tbl, 0u, b, pl);
      }
      a.crc_in[k * m + i] = seed;
    }
  }
  if (a.msg_len) a.msg_len[i] = L.length;
}

__global__ __launch_bounds__(256) void put_seal_kernel(PutArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= kPutSlots * a.m || (a.gate && *a.gate == 0)) return;
  if (a.copy_through && j < a.m) return;  // slot 0's job is the key; the layout kernel sealed the header
  const uint64_t len = a.crc_len[j];
  if (len == 0) return;  // absent encryption-key record (every present record has >= 6 bytes)
  put_be64(a.out + a.crc_off[j] + len, (uint64_t)a.crc[j]);
}

// ---- copy-mode serialization of small messages (put_stream_kernel; StreamPutArgs, crc32_kernels.h) ----
// The uniform layout of one message (PutMessageFormatInputStream.java:76-124 through put_layout.h):
// five data segments copied from their sources and six gaps between them -- the header, the record
// prefixes and trailers -- whose bytes are computed (every CRC field zero here: put_stream_seal_kernel
// writes them). Segments and gaps alternate: gap g = [hi[g-1], lo[g]) (hi[-1] = 0, lo[5] = len), an
// absent encryption key an empty segment at the key's end.
struct StreamMsg {
  int32_t len;                    // message bytes (<= kStreamPutMax)
  int32_t lo[5], hi[5];           // data segment k at [lo, hi) of the message (key, enc key, props, um, blob)
  const uint8_t* src[5];          // its source
};

__device__ __forceinline__ bool stream_msg(const ambrycrc_put_desc& d, const uint8_t* fields, const uint8_t* blobs,
                                           StreamMsg& M) {
  PutLayout L;
  if (!put_layout(d, L) || L.length > kStreamPutMax) return false;
  M.len = (int32_t)L.length;
  uint64_t fo[5];
  put_field_offsets(d, L, fo);
  const uint64_t ln[5] = {d.key_len, L.enc_rec ? (uint64_t)d.enckey_len : 0, d.props_len, d.usermeta_len, d.blob_len};
  const uint64_t so[5] = {d.key_src, d.enckey_src, d.props_src, d.usermeta_src, d.blob_src};
  if (!L.enc_rec) fo[1] = fo[0] + ln[0];  // the empty segment at the key's end
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    M.lo[k] = (int32_t)fo[k];
    M.hi[k] = (int32_t)(fo[k] + ln[k]);
    M.src[k] = (k == 4 ? blobs : fields) + so[k];
  }
  return true;
}

// The message's data segments as a per-wave LDS table (4 words each: lo, hi, and the 64-bit
// source - lo), entry 5 empty, so a lane finds a segment's bounds and source with one ds_read_b128
// at its own index instead of a select chain over all five (the chain cost ~45 VALU a piece).
__device__ __forceinline__ void stream_seg_table(const StreamMsg& M, u32x4* tab, uint32_t lane) {
  __builtin_amdgcn_wave_barrier();  // one wave's LDS operations run in order: keep the program order
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const uint64_t dl = (uint64_t)M.src[k] - (uint64_t)(int64_t)M.lo[k];
      tab[k] = u32x4{(uint32_t)M.lo[k], (uint32_t)M.hi[k], (uint32_t)dl, (uint32_t)(dl >> 32)};
    }
    tab[5] = u32x4{0u, 0u, 0u, 0u};
  }
  __builtin_amdgcn_wave_barrier();
}

// The source of the 16-B output piece at message-relative dd (dd + m0 a multiple of 16) when the piece
// lies inside one data segment, else 0. The segments are in message order with lo nondecreasing, so
// the only one that can hold the piece is the last whose lo <= dd.
__device__ __forceinline__ uint64_t stream_piece_src(const StreamMsg& M, const u32x4* tab, int32_t dd) {
  const uint32_t k = (uint32_t)(dd >= M.lo[1]) + (uint32_t)(dd >= M.lo[2]) + (uint32_t)(dd >= M.lo[3]) +
                     (uint32_t)(dd >= M.lo[4]);
  const u32x4 e = tab[k];
  const bool in = dd >= (int32_t)e.x && dd + 16 <= (int32_t)e.y;
  const uint64_t src = (((uint64_t)e.w << 32) | e.z) + (uint64_t)(int64_t)dd;
  return in ? src : 0;
}

// A 16-B load from a source address held as an integer, kept in the global address space (a generic
// pointer would make it a flat load, which also counts on lgkmcnt, as the stores of crc_wave.h).
__device__ __forceinline__ u32x4 ld16ug(uint64_t a) { return *reinterpret_cast<const gu32x4*>(a); }

constexpr uint32_t kStreamSbs = 2;  // super-blocks a message's runs span: ceil((63 + kStreamPutMax) / 4096)
static_assert((63 + kStreamPutMax + kSuperBlock - 1) / kSuperBlock <= kStreamSbs, "streamed message spans");

// A wave per message (grid-stride over the waves of one 1024-thread workgroup per CU; the next
// message's descriptor loaded while this one runs). The message's output is 1 or 2 super-blocks of
// 4 KiB from its first 64-B run, four 1 KiB wave pieces each. All loads go out first: the source of
// each piece that lies inside one data segment, and the bytes of each segment whose piece is not
// inside it (at most 15 at either end; a lane each). Then the stores: those pieces (16 B each) and
// those edge bytes. Then the remaining pieces that touch the message are loaded back from the output,
// where put_layout_kernel wrote the gaps' bytes (the header, record prefixes) and this wave the edge
// bytes -- one wave's lanes, through the CU's one L1: no fence needed. Then, per super-block, the quad
// transpose and run_crc as region_runs_kernel hashes them, the 64 sums stored (16-B stores of the lanes
// whose runs overlap the message) into the message's run slots. A run that is not inside the message
// (its neighbours' bytes), or that holds a CRC field, is never summed: put_stream_seal_kernel re-reads
// those bytes once every field is written. (Software-pipelining two messages per wave measured slower:
// 128 VGPRs and spills, 0.79 against 0.70 ms.)
// Pipelined across messages: while message i's output is stored, its gap pieces loaded back and its
// runs hashed, message i+1's source loads are in flight. For the hash to wait only for message i's
// loads, the loads issued after them must be the same in number on every path (the compiler's wait
// counts are the least over the paths): so every edge-byte and piece load of the next message is
// issued, a lane or a message with nothing to load reading the table image instead, and the
// descriptors are read as dwords through the constant address space (scalar loads; a byte field
// read from a vector load would wait for every load in flight). Piece sources are not kept: a bit
// mask per lane says which of the 8 pieces came from a source. (The form without this pipelining
// lost its A/B, DESIGN.md §12.6 and §12.11: tools/probes/patches/put_stream_unpipelined.patch.)
namespace {
struct StreamUnit {  // wave-uniform: one message's output and its run slots
  uint8_t* out;      // the message's first byte
  int32_t p0b;       // (its first run's start) - (its first byte), <= 0
  int32_t len;
  uint32_t nruns;    // 0: no message
  uint32_t* rk;
};
}  // namespace

__global__ __launch_bounds__(1024) void put_stream_kernel(StreamPutArgs a) {
  fill_lds_slices(a.img);
  const uint32_t lane = threadIdx.x & 63u;
  const LaneConst k = make_lane_const(lane);
  uint32_t* buf = g_lds_runs + kSliceBytes / 4 + (threadIdx.x >> 6) * (kRunsBufBytes / 4);
  u32x4* const tab = reinterpret_cast<u32x4*>(buf + 128);  // the segment table (words 128..151 of the wave's buffer)
  const uint32_t slot = 16u * (lane & 3u) + (lane >> 2);
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint32_t wave = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) * gridDim.x + blockIdx.x);
  typedef __attribute__((address_space(4))) const uint32_t cword;
  static_assert(sizeof(ambrycrc_put_desc) == 80, "descriptor words");
  auto desc_at = [&](uint64_t j) {
    cword* w = (cword*)(uintptr_t)a.desc + 20 * j;
    uint32_t r[20];
#pragma unroll
    for (int t = 0; t < 20; ++t) r[t] = w[t];
    ambrycrc_put_desc d;
    __builtin_memcpy(&d, r, sizeof d);
    return d;
  };
  const uint64_t dummy = (uint64_t)(uintptr_t)a.img;  // loads with nothing to fetch read the table image

  // The next streamed message from i on (i advances past the job path's and invalid ones): its unit,
  // segment table, edge bytes and source pieces, every load issued, none waited for.
  uint64_t i = wave;
  auto start = [&](StreamUnit& u, int32_t (&ee)[3], uint32_t (&eb)[3], u32x4 (&x)[kStreamSbs][4], uint32_t& pm) {
    StreamMsg M;
    ambrycrc_put_desc d{};
    bool ok = false;
    for (; i < a.m && !ok; i += nwaves) {
      d = desc_at(i);
      ok = stream_msg(d, a.fields, a.blobs, M);  // else the job path's (or invalid: nothing written)
      if (ok) u.rk = a.rk + kRunPad + i * kStreamPutRuns;
    }
    const uint64_t m0 = a.oreg0 + d.out_off, S0 = m0 & ~uint64_t(63);
    const int32_t mis = (int32_t)(m0 & 15u);
    u.out = a.obase + m0;
    u.p0b = (int32_t)(S0 - m0);
    u.len = ok ? M.len : 0;
    u.nruns = ok ? (uint32_t)((m0 + M.len - S0 + 63) >> 6) : 0u;
    if (ok) stream_seg_table(M, tab, lane);
#pragma unroll
    for (uint32_t it = 0; it < 3; ++it) {
      const uint32_t idx = 64 * it + lane, s = idx >> 5, j = idx & 31u;
      const u32x4 t = tab[s < 5 ? s : 5];
      const int32_t lo = (int32_t)t.x, hi = (int32_t)t.y;
      const int32_t up = ((lo + mis + 15) & ~15) - mis, dn = ((hi + mis) & ~15) - mis;
      const int32_t e = j < 16 ? lo + (int32_t)j : (up > dn ? up : dn) + (int32_t)j - 16;
      const bool live = ok && s < 5 && (j < 16 ? e < (up < hi ? up : hi) : e < hi);
      ee[it] = live ? e : -1;
      eb[it] = *reinterpret_cast<const gu8*>(live ? (((uint64_t)t.w << 32) | t.z) + (uint64_t)(int64_t)e : dummy);
    }
    const int32_t p0 = u.p0b + 16 * (int32_t)lane;
    pm = 0;
#pragma unroll
    for (uint32_t sb = 0; sb < kStreamSbs; ++sb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint64_t src = ok ? stream_piece_src(M, tab, p0 + (int32_t)(kSuperBlock * sb + kBlockBytes * q)) : 0;
        x[sb][q] = ld16ug(src ? src : dummy);
        pm |= src ? 1u << (4 * sb + q) : 0u;
      }
    return ok;
  };

  StreamUnit un;
  int32_t een[3];
  uint32_t ebn[3];
  u32x4 xn[kStreamSbs][4];
  uint32_t pmn;
  bool more = start(un, een, ebn, xn, pmn);
  while (more) {
    const StreamUnit u = un;
    int32_t ee[3];
    uint32_t eb[3];
    u32x4 x[kStreamSbs][4];
    const uint32_t pm = pmn;
#pragma unroll
    for (int t = 0; t < 3; ++t) ee[t] = een[t], eb[t] = ebn[t];
#pragma unroll
    for (uint32_t sb = 0; sb < kStreamSbs; ++sb)
#pragma unroll
      for (int q = 0; q < 4; ++q) x[sb][q] = xn[sb][q];
    // this message's stores: the edge bytes, then its source pieces (one base per super-block, shared
    // with the load-backs below: an address computed between the stores and a load-back would reuse a
    // stored register and wait for that store to complete)
    const int32_t p0 = u.p0b + 16 * (int32_t)lane;
    uint8_t* pb[kStreamSbs] = {u.out + p0, u.out + p0 + kSuperBlock};
#pragma unroll
    for (uint32_t sb = 0; sb < kStreamSbs; ++sb) asm volatile("" : "+v"(pb[sb]));  // opaque: kept, not rematerialized
#pragma unroll
    for (uint32_t it = 0; it < 3; ++it)
      if (ee[it] >= 0) st8g(u.out + ee[it], eb[it]);
#pragma unroll
    for (uint32_t sb = 0; sb < kStreamSbs; ++sb)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (pm & (1u << (4 * sb + q))) st16u_nt(pb[sb] + kBlockBytes * q, x[sb][q]);
    // its gap pieces loaded back (the layout kernel's bytes and the edge bytes just stored); pieces
    // outside the message keep what the lane loaded (the table image): the runs they fall in cross the
    // message's ends or lie outside it, and are never summed
#pragma unroll
    for (uint32_t sb = 0; sb < kStreamSbs; ++sb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int32_t dd = p0 + (int32_t)(kSuperBlock * sb + kBlockBytes * q);
        if (!(pm & (1u << (4 * sb + q))) && dd + 16 > 0 && dd < u.len)
          x[sb][q] = ld16ug((uint64_t)(uintptr_t)(pb[sb] + kBlockBytes * q));
      }
    // the next message's parse and loads, in flight while this one is hashed
    more = start(un, een, ebn, xn, pmn);
#pragma unroll
    for (uint32_t sb = 0; sb < kStreamSbs; ++sb) {
      if (64 * sb >= u.nruns) break;
      quad_transpose_asm(x[sb]);
      buf[slot] = run_crc<4, 1>(x[sb], k, 0u);
      if (64 * sb + 4 * lane < u.nruns && lane < 16)  // runs 64 sb + 4 lane .. + 3, as region_runs_kernel's stores
        *reinterpret_cast<u32x4*>(u.rk + 64 * sb + 4 * lane) = *reinterpret_cast<const u32x4*>(buf + 4u * lane);
    }
  }
}

hipError_t launch_put_stream(const StreamPutArgs& a, int num_cu, hipStream_t s) {
  return launch_items(put_stream_kernel, a.m ? (uint32_t)num_cu : 0u, 1024, s, a);
}

size_t stream_put_rk_bytes(size_t m) { return ((kRunPad + (size_t)m * kStreamPutRuns) * sizeof(uint32_t) + 255) & ~size_t(255); }

// ---------------------------------------------------------------- streamed small messages
// Pass 2 of copy-mode serialization for messages of at most kStreamPutMax bytes (put_stream_kernel,
// above, wrote their bytes and the raw CRC of every 64-B output run): one thread per
// message computes the header CRC from the bytes it builds in registers and each record's CRC from the
// run sums (region::record_crc: the head and tail runs a record cuts re-read from the output), and
// writes the big-endian trailers -- the CRCs MessageFormatInputStream emits after each record
// (MessageFormatInputStream.java:85-93; PutMessageFormatInputStream.java:76-124). Two blocks per CU, as
// region_msg_kernel, so a thread's lines stay in L2 between its dependent reads.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(AMBRY_REGION_WPE))) void put_stream_seal_kernel(
    StreamPutArgs a) {
  __shared__ uint32_t tbl[1024];
  __shared__ uint32_t nib[region::kNibTotal];
  __shared__ uint32_t hm[kRegAuxWords], bt[kRegByteWords], un[kRegUnWords];
  stage_slice_tables(tbl, a.img);
  region::stage_nib(nib, a.img);
  region::stage_aux(hm, bt, un, a.img);
  __syncthreads();
  const region::Aux aux{hm, bt, un};
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.m; i += (uint64_t)gridDim.x * blockDim.x) {
    const ambrycrc_put_desc d = a.desc[i];
    PutLayout L;
    if (!put_layout(d, L) || L.length > kStreamPutMax) continue;
    const uint64_t m0 = a.oreg0 + d.out_off;
    uint8_t* msg = a.obase + m0;
    // message i's run slots, addressed by base-relative run index (record_crc's rk[k])
    const uint32_t* rk = reinterpret_cast<const uint32_t*>(
        reinterpret_cast<uintptr_t>(a.rk + kRunPad + i * kStreamPutRuns) - ((m0 >> 6) << 2));
    put_emit_header<false>(tbl, d, L, msg);
#pragma unroll 1
    for (uint32_t k = 1; k < kPutSlots; ++k) {
      uint64_t off, ln;
      bool present;
      put_crc_job(L, k, &off, &ln, &present);
      if (!present) continue;
      const uint32_t c = region::record_crc(region::TabC{tbl}, nib, a.obase, rk, m0 + off, ln, aux);
      put_be64(msg + off + ln, (uint64_t)c);
    }
  }
}

hipError_t launch_put_stream_seal(const StreamPutArgs& a, int num_cu, hipStream_t s) {
  return launch_items(put_stream_seal_kernel, blocks_for(a.m, num_cu, AMBRY_SEAL_BPC), 256, s, a);
}

// ---------------------------------------------------------------- gather copy
// Dword k of bytes [4Q + r, 4Q + r + 16) of the 32-byte concatenation a||b (little endian).
template <int Q>
__device__ __forceinline__ u32x4p shift_pair(const u32x4p& a, const u32x4p& b, uint32_t r) {
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  u32x4p o;
  if (r == 0) {
    o.x = w[Q];
    o.y = w[Q + 1];
    o.z = w[Q + 2];
    o.w = w[Q + 3];
  } else {
    o.x = __builtin_amdgcn_alignbyte(w[Q + 1], w[Q], r);
    o.y = __builtin_amdgcn_alignbyte(w[Q + 2], w[Q + 1], r);
    o.z = __builtin_amdgcn_alignbyte(w[Q + 3], w[Q + 2], r);
    o.w = __builtin_amdgcn_alignbyte(w[Q + 4], w[Q + 3], r);
  }
  return o;
}

// Copies n16 16-B pieces to the 16-B aligned dst from src (any alignment: shift = 4Q + r),
// lane-strided, 4 pieces per lane in flight. The second aligned source block of a piece holds
// bytes the piece needs whenever shift > 0, so every load touches the source range.
template <int Q>
__device__ __forceinline__ void copy_pieces(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint64_t n16,
                                            uint32_t r, uint32_t lane) {
  const uint32_t shift = 4 * Q + r;
  const u32x4p* s0 = reinterpret_cast<const u32x4p*>(src - shift);
  u32x4p* d0 = reinterpret_cast<u32x4p*>(dst);
  constexpr int U = 4;
  uint64_t p = lane;
  for (; p + 64 * (U - 1) < n16; p += 64 * U) {
    u32x4p a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      a[u] = __builtin_nontemporal_load(s0 + p + 64 * u);
      b[u] = shift ? __builtin_nontemporal_load(s0 + p + 64 * u + 1) : u32x4p{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int u = 0; u < U; ++u) __builtin_nontemporal_store(shift_pair<Q>(a[u], b[u], r), d0 + p + 64 * u);
  }
  for (; p < n16; p += 64) {
    const u32x4p a = __builtin_nontemporal_load(s0 + p);
    const u32x4p b = shift ? __builtin_nontemporal_load(s0 + p + 1) : u32x4p{0u, 0u, 0u, 0u};
    __builtin_nontemporal_store(shift_pair<Q>(a, b, r), d0 + p);
  }
}

// One wave copies n bytes src -> dst (wave-uniform arguments).
__device__ __forceinline__ void copy_range(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint64_t n,
                                           uint32_t lane) {
  const uint64_t head0 = (16 - ((uintptr_t)dst & 15)) & 15;
  const uint64_t head = head0 < n ? head0 : n;
  if (lane < head) dst[lane] = src[lane];
  const uint64_t body = n - head;
  const uint64_t n16 = body >> 4;
  uint8_t* d1 = dst + head;
  const uint8_t* s1 = src + head;
  if (n16) {
    const uint32_t shift = (uint32_t)((uintptr_t)s1 & 15);
    switch (shift >> 2) {
      case 0: copy_pieces<0>(d1, s1, n16, shift & 3, lane); break;
      case 1: copy_pieces<1>(d1, s1, n16, shift & 3, lane); break;
      case 2: copy_pieces<2>(d1, s1, n16, shift & 3, lane); break;
      default: copy_pieces<3>(d1, s1, n16, shift & 3, lane); break;
    }
  }
  const uint64_t t = body & 15;
  if (lane < t) d1[16 * n16 + lane] = s1[16 * n16 + lane];
}

// Persistent, cost-balanced copy of the jobs' bytes (cost_share_walk, wave_tools.h; start is the
// plan kernel's exclusive scan of len + kCopyJobCost).
__global__ __launch_bounds__(256) void gather_copy_kernel(CopyArgs a) {
  if (a.gate && *a.gate == 0) return;  // uniform
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint32_t wave = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) * gridDim.x + blockIdx.x);
  uint64_t w_src = 0, w_dst = 0;
  cost_share_walk(
      a.start, a.len, a.n, wave, nwaves, lane,
      [&](uint32_t i) {
        w_src = a.src[i];
        w_dst = a.dst_off[i];
      },
      [&](uint32_t j, uint64_t r0, uint64_t n) {
        copy_range(a.dst + readlane64(w_dst, j) + r0,
                   reinterpret_cast<const uint8_t*>((uintptr_t)readlane64(w_src, j)) + r0, n, lane);
      });
}

hipError_t launch_put_layout(const PutArgs& a, hipStream_t s) {
  return launch_items(put_layout_kernel, blocks_for(a.m), 256, s, a);
}

hipError_t launch_put_seal(const PutArgs& a, hipStream_t s) {
  return launch_items(put_seal_kernel, blocks_for(kPutSlots * a.m), 256, s, a);
}

hipError_t launch_gather_copy(const CopyArgs& a, int grid, hipStream_t s) {
  return launch_items(gather_copy_kernel, a.n ? (uint32_t)grid : 0u, 256, s, a);
}

}  // namespace ambrycrc
