// crc32_kernels.hip -- the batch CRC engine: the gfx950 (CDNA4) kernels for Ambry's blob CRC-32
// path and their launchers (launch_plan, launch_sweep, launch_sweep_copy, launch_verify,
// launch_fill). The wave primitives they are built from are in crc_wave.h; region mode, the PUT
// streamer and the bandwidth probes have kernel files of their own (region_kernels.hip,
// put_kernels.hip, bw_probe_kernels.hip).
//
// Replaces, for device-resident batches of chunks, the byte loop of
// ambry-utils/.../utils/Crc32.java:55-143 (and java.util.zip.CRC32.update, the
// same function) as called per router chunk (ambry-router/.../PutOperation.java:
// 1700-1703, 2033-2054) and per blob record (ambry-messageformat/.../
// MessageFormatRecord.java:1797-1832). Results are bit-exact CRC-32/ISO-HDLC.
//
// Work decomposition (default variant 29; variant 0 is the 16-B-piece fallback)
//   batch  -> the chunks viewed as one concatenated byte stream; wave w of the
//             persistent grid owns an equal share [w*S, (w+1)*S) of it (exact byte
//             balance for any chunk-size mix), cut points snapped to 16 B in memory.
//             Whole chunks <= 16 KiB (batches of >= 16,384 chunks) go to the group
//             phase first: G = 2/8/16 lanes per chunk by size class, 64/G chunks per wave
//   segment-> a (wave, chunk) intersection; the wave sweeps it in 4 KiB super-blocks:
//             four coalesced 1 KiB global_load_dwordx4 per lane, a quad transpose
//             leaving each lane a 64-B run
//   lane   -> slice-by-4 over its run using LDS byte tables that one v_perm_b32
//             addresses; the lane state hops one super-block with an x^(8*4096)
//             nibble-table multiply (independent of the run's own table walk)
//   wave   -> 6-level xor tree (DPP partners), shifts 64 B .. 2 KiB
//   segment-> shifted by its distance to the chunk end and atomically XORed into
//             out[chunk] (XOR is exact and order-free => deterministic)
//
// LDS layout: crc32_layout.h. One 1024-thread workgroup per CU (the image is
// ~150 KiB), persistent: each wave walks its own byte share.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crc32_gf2.h"
#include "crc32_layout.h"
#include "crc32_kernels.h"
#include "crc_wave.h"
#include "wave_tools.h"

namespace ambrycrc {

template <int DIAG>
__device__ __forceinline__ uint32_t fold(uint32_t s) {
  if constexpr (DIAG == 1) {
    return s ^ (s >> 7);  // diagnostic timing build: no LDS fold (wrong CRC)
  } else {
    return nib_mul(s, kFoldOff);
  }
}

// Two pieces whose first three table steps are independent of the running state,
// interleaved in source so a wave keeps two LDS dependency chains in flight.
template <int DIAG>
__device__ __forceinline__ uint32_t rpiece_pair_d(u32x4 w0, u32x4 w1, const LaneConst& k, uint32_t s) {
  uint32_t x0 = slice4(w0.x, k, w0.y);
  uint32_t x1 = slice4(w1.x, k, w1.y);
  x0 = slice4(x0, k, w0.z);
  x1 = slice4(x1, k, w1.z);
  x0 = slice4(x0, k, w0.w);
  x1 = slice4(x1, k, w1.w);
  s = slice4(x0, k, fold<DIAG>(s));
  return slice4(x1, k, fold<DIAG>(s));
}

// Block 0 of a body whose virtual start v0 = be - nb*1024 may precede bs: lane l's 16 B at
// v0 + 16l, zero where they lie before bs (zeros leave a zero register unchanged). Only
// lanes whose piece reaches bs form an address, so v0 may precede the allocation.
template <bool NT>
__device__ __forceinline__ u32x4 load_block0(const uint8_t* __restrict__ base, int64_t v0, uint64_t bs,
                                             uint32_t lane) {
  u32x4 w = {0u, 0u, 0u, 0u};
  const int64_t p = v0 + 16 * (int64_t)lane;
  if (p + 16 > (int64_t)bs) {  // => p >= floor16(bs) >= 0: inside the caller's buffer
    w = ld16<NT>(reinterpret_cast<const u32x4*>(base + p));
    if (p < (int64_t)bs) {
      const uint32_t cut = (uint32_t)(bs - p);  // 1..15 leading bytes to drop
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int lo = (int)cut - 4 * d;  // bytes of dword d to drop
        const uint32_t m = lo <= 0 ? 0xFFFFFFFFu : (lo >= 4 ? 0u : (0xFFFFFFFFu << (8 * lo)));
        w[d] &= m;
      }
    }
  }
  return w;
}

// Raw CRC of body [bs, be) (be 16-aligned, bs <= be arbitrary), returned in lane 63
// (other lanes: junk). Bytes below bs are treated as zeros, which leave a zero
// register unchanged, so the virtual range is aligned down to whole 1 KiB blocks.
template <int U, bool NT, int DIAG = 0>
__device__ __forceinline__ uint32_t body_crc(const uint8_t* __restrict__ base, uint64_t bs, uint64_t be,
                                             uint32_t lane, const LaneConst& k) {
  const uint64_t nb = (be - bs + kBlockBytes - 1) / kBlockBytes;
  if (nb == 0) return 0u;
  // The virtual start may precede the allocation (chunk in its first KiB): signed
  // arithmetic, and only lanes whose piece reaches bs ever form a load address.
  const int64_t v0 = (int64_t)be - (int64_t)(nb * kBlockBytes);
  const u32x4* q = reinterpret_cast<const u32x4*>(base + v0) + lane;

  uint32_t s = 0u;  // fold(0) == 0, so block 0 takes the same step as every other block
  {
    // Prime: blocks 0..min(U,nb)-1 are all issued before the first is used, so a short
    // segment (a 4 KiB record = 4 blocks) costs one memory round trip, not one per block.
    u32x4 buf[U];
    buf[0] = load_block0<NT>(base, v0, bs, lane);
#pragma unroll
    for (int u = 1; u < U; ++u) buf[u] = (uint64_t)u < nb ? ld16<NT>(q + u * (kBlockBytes / 16)) : u32x4{0u, 0u, 0u, 0u};
    // Rolling prefetch: the slot a piece is consumed from is refilled with the piece
    // U blocks ahead, so each lane keeps U x 16 B loads in flight continuously.
    uint64_t b = 0;
    for (; b + 2 * U <= nb; b += U) {
#pragma unroll
        for (int u = 0; u < U; u += 2) {
          const u32x4 w0 = buf[u], w1 = buf[u + 1];
          buf[u] = ld16<NT>(q + (b + U + u) * (kBlockBytes / 16));
          buf[u + 1] = ld16<NT>(q + (b + U + u + 1) * (kBlockBytes / 16));
          s = rpiece_pair_d<DIAG>(w0, w1, k, s);
        }
    }
    // Drain (nb - b < 2U): consume the slots, refilling each with its block U ahead if
    // there is one, then consume the refills. Predicates are wave-uniform.
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (b + u < nb) {
        const u32x4 w = buf[u];
        if (b + U + u < nb) buf[u] = ld16<NT>(q + (b + U + u) * (kBlockBytes / 16));
        s = rpiece(w, k, nib_mul(s, kFoldOff));
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (b + U + u < nb) s = rpiece(buf[u], k, nib_mul(s, kFoldOff));
  }

  // Lane l's stream ends 16(63-l) bytes before be: xor-tree with shifts 16*2^lvl,
  // partners delivered by DPP (no LDS round trip for the move itself).
  if constexpr (DIAG == 3) return s ^ __shfl_xor(s, 1);  // diagnostic timing build: no tree (wrong CRC)
  s = tree_level<0>(s, lane);
  s = tree_level<1>(s, lane);
  s = tree_level<2>(s, lane);
  s = tree_level<3>(s, lane);
  s = tree_level<4>(s, lane);
  s = tree_level<5>(s, lane);
  return s;
}

// ---- 64-B lane runs from coalesced loads (variant 12 and up) ----
// Per 4 KiB super-block each lane l = 4m+j issues 4 coalesced 1 KiB loads (block i, piece l),
// then a 4x4 transpose of 16-B elements inside its quad (two DPP quad_perm butterfly stages)
// leaves lane (m, j) holding the 64-B run [64m, 64m+64) of block j: the state hops once per
// 64 B (x^(8*4096) = POW[12]) instead of once per 16 B. Tree: lane bits 2..5 merge the runs of
// one block (shifts 64..512 B = POW[6..9]), bits 0..1 merge the blocks (1024, 2048 B).
template <int BIT, int POWK>
__device__ __forceinline__ uint32_t tree_level_t4(uint32_t s, uint32_t lane) {
  uint32_t o;
  if constexpr (BIT == 0) o = dpp<0x111, 0xf>(s);       // row_shr:1
  else if constexpr (BIT == 1) o = dpp<0x112, 0xf>(s);  // row_shr:2
  else if constexpr (BIT == 2) o = dpp<0x114, 0xf>(s);  // row_shr:4
  else if constexpr (BIT == 3) o = dpp<0x118, 0xf>(s);  // row_shr:8
  else o = __shfl_xor(s, 1 << BIT);                     // 16, 32: across rows
  const uint32_t sh = nib_mul(o, kPowOff + kNibSetBytes * POWK);
  return (lane & (1u << BIT)) ? (s ^ sh) : s;
}

template <int UB, bool NT, bool PRIO = false, bool COPY = false>
__device__ __forceinline__ uint32_t body_crc_t4(const uint8_t* __restrict__ base, uint64_t bs, uint64_t be,
                                                uint32_t lane, const LaneConst& k, uint8_t* dbase = nullptr) {
  constexpr uint64_t SB = 4 * (uint64_t)kBlockBytes;
  constexpr uint32_t kFold = kPowOff + kNibSetBytes * 12;
  const uint64_t nb = (be - bs + SB - 1) / SB;
  if (nb == 0) return 0u;
  const int64_t v0 = (int64_t)be - (int64_t)(nb * SB);  // may precede the allocation: signed
  u32x4 x[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    x[i] = u32x4{0u, 0u, 0u, 0u};
    const int64_t p = v0 + (int64_t)kBlockBytes * i + 16 * (int64_t)lane;
    if (p + 16 > (int64_t)bs) {  // => p >= floor16(bs) >= 0
      x[i] = ld16<NT>(reinterpret_cast<const u32x4*>(base + p));
      if constexpr (COPY) copy_piece(dbase, p, x[i], (int64_t)bs);
      if (p < (int64_t)bs) {
        const uint32_t cut = (uint32_t)(bs - p);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const int lo = (int)cut - 4 * d;
          const uint32_t m = lo <= 0 ? 0xFFFFFFFFu : (lo >= 4 ? 0u : (0xFFFFFFFFu << (8 * lo)));
          x[i][d] &= m;
        }
      }
    }
  }
  quad_transpose_asm(x);
  uint32_t s = run_crc<4>(x, k, 0u);
  const u32x4* q = reinterpret_cast<const u32x4*>(base + v0) + lane;  // super-block b, block i: q[b*256 + i*64]
  uint64_t b = 1;
  if (nb >= 1 + 2 * (uint64_t)UB) {
    u32x4 buf[UB][4];
#pragma unroll
    for (int u = 0; u < UB; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) buf[u][i] = ld16<NT>(q + (b + u) * 256 + i * 64);
    for (; b + 2 * UB <= nb; b += UB) {
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        u32x4 cur[4];
        if constexpr (PRIO) __builtin_amdgcn_s_setprio(3);  // loads first among the SIMD's waves
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          cur[i] = buf[u][i];
          buf[u][i] = ld16<NT>(q + (b + UB + u) * 256 + i * 64);
        }
        if constexpr (PRIO) __builtin_amdgcn_s_setprio(0);
        if constexpr (COPY) {
          if (dbase) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              st16u_nt(dbase + v0 + (int64_t)((b + u) * SB) + 1024 * i + 16 * lane, cur[i]);
          }
        }
        quad_transpose_asm(cur);
        s = run_crc<4>(cur, k, nib_mul(s, kFold));
      }
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      if constexpr (COPY) {
        if (dbase) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            st16u_nt(dbase + v0 + (int64_t)((b + u) * SB) + 1024 * i + 16 * lane, buf[u][i]);
        }
      }
      quad_transpose_asm(buf[u]);
      s = run_crc<4>(buf[u], k, nib_mul(s, kFold));
    }
    b += UB;
  }
  for (; b < nb; ++b) {
    u32x4 cur[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) cur[i] = ld16<NT>(q + b * 256 + i * 64);
    if constexpr (COPY) {
      if (dbase) {
#pragma unroll
        for (int i = 0; i < 4; ++i) st16u_nt(dbase + v0 + (int64_t)(b * SB) + 1024 * i + 16 * lane, cur[i]);
      }
    }
    quad_transpose_asm(cur);
    s = run_crc<4>(cur, k, nib_mul(s, kFold));
  }
  s = tree_level_t4<2, 6>(s, lane);
  s = tree_level_t4<3, 7>(s, lane);
  s = tree_level_t4<4, 8>(s, lane);
  s = tree_level_t4<5, 9>(s, lane);
  s = tree_level_t4<0, 10>(s, lane);
  s = tree_level_t4<1, 11>(s, lane);
  return s;
}

__device__ __forceinline__ uint64_t aligned_end(uint64_t s, uint64_t e) {
  uint64_t b = e & ~uint64_t(15);
  return b < s ? s : b;
}

// ---- group mode: whole small chunks, G lanes each, 64/G chunks per wave ----
// Per chunk the wave-mode fixed cost is a 6-level tree and the dependent LDS chain of
// each 1 KiB block; for 1-4 KiB chunks that, not HBM, sets the rate. A G-lane group
// takes a whole chunk instead: lane gl owns bytes [16gl, 16gl+16) of every 16G-byte
// block, fold x^(8*16G) = POW[log2 16G], a log2(G)-level tree, and 64/G chunks' chains
// run in the same instructions. The initial register ~crc_in is XORed into the chunk's
// first four bytes where they are loaded (plus ~crc_in >> 8len when len < 4), which
// removes the per-chunk shift over len. Model: tests/kernel_model.py group_crc.

// XOR the initial register's little-endian bytes (at addresses [cs, cs+4)) into the
// 16-B piece at address p.
__device__ __forceinline__ u32x4 xor_init(u32x4 w, int64_t p, uint64_t cs, uint32_t rinit) {
  const int64_t o = (int64_t)cs - p;  // init offset inside the piece
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const int64_t od = o - 4 * d;
    if (od >= 0 && od < 4) w[d] ^= rinit << (8 * (uint32_t)od);
    else if (od < 0 && od > -4) w[d] ^= rinit >> (8 * (uint32_t)(-od));
  }
  return w;
}

// The blocks of a group chunk, block b at p0 + b*BB (BB = 16G), through a ring of P struct
// members (no array, so nothing becomes a promoted vector that predicated writes copy
// whole): prime() issues blocks 0..P-1; a runtime loop steps P blocks at a time, member U
// folding block b0+U and refilling with block b0+U+P. P blocks in flight per lane, ~4P
// VGPRs, code size independent of the chunk-size cap. Bytes before cs read as zero; the
// piece holding [cs, cs+4) gets the initial register XORed in.
struct GroupCtx {
  const uint8_t* __restrict__ base;
  uint8_t* dbase;  // copy-through destination base (COPY builds)
  int64_t p0;
  uint64_t cs;
  bool body;
  uint32_t nbw;
  uint32_t rinit;
};

template <bool NT, int BB>
__device__ __forceinline__ u32x4 group_load(const GroupCtx& g, int b) {
  const int64_t p = g.p0 + (int64_t)b * BB;
  u32x4 w = {0u, 0u, 0u, 0u};
  if ((uint32_t)b < g.nbw && g.body && p + 16 > (int64_t)g.cs)  // => floor16(cs) <= p < cb
    w = ld16<NT>(reinterpret_cast<const u32x4*>(g.base + p));
  return w;
}

template <int U, int P, bool NT, int BB, bool COPY = false>
struct GroupRingT {
  u32x4 w;
  GroupRingT<U + 1, P, NT, BB, COPY> next;
  __device__ __forceinline__ void prime(const GroupCtx& g) {
    w = group_load<NT, BB>(g, U);
    next.prime(g);
  }
  // Blocks b0+U for U = 0..P-1: member U holds block b0+U and is refilled with b0+U+P.
  __device__ __forceinline__ uint32_t step(const GroupCtx& g, const LaneConst& k, uint32_t b0, uint32_t s,
                                           uint32_t fold_off) {
    const uint32_t b = b0 + U;
    if (b >= g.nbw) return s;
    u32x4 x = w;
    w = group_load<NT, BB>(g, (int)(b + P));
    const int64_t p = g.p0 + (int64_t)b * BB;
    if constexpr (COPY) {
      if (g.body) copy_piece(g.dbase, p, x, (int64_t)g.cs);
    }
    if (p < (int64_t)g.cs + 4 && p + 16 > (int64_t)g.cs) {
      x = xor_init(x, p, g.cs, g.rinit);
      if (p < (int64_t)g.cs) {
        const uint32_t cut = (uint32_t)((int64_t)g.cs - p);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const int lo = (int)cut - 4 * d;
          const uint32_t m = lo <= 0 ? 0xFFFFFFFFu : (lo >= 4 ? 0u : (0xFFFFFFFFu << (8 * lo)));
          x[d] &= m;
        }
      }
    }
    s = rpiece(x, k, b ? nib_mul(s, fold_off) : 0u);
    return next.step(g, k, b0, s, fold_off);
  }
};
template <int P, bool NT, int BB, bool COPY>
struct GroupRingT<P, P, NT, BB, COPY> {
  __device__ __forceinline__ void prime(const GroupCtx&) {}
  __device__ __forceinline__ uint32_t step(const GroupCtx&, const LaneConst&, uint32_t, uint32_t s, uint32_t) {
    return s;
  }
};

// List entries per wave for a class of ns chunks: a multiple of 64/G so every round fills all groups.
template <int G>
__device__ __forceinline__ uint64_t group_per(uint64_t ns, uint64_t nwaves) {
  return ((ns + nwaves - 1) / nwaves + 64 / G - 1) / (64 / G) * (64 / G);
}

// A wave's rounds of size class C [lo, hi): entries [i, i + 64/G) for i = i0, i0 + stride, ... < i1.
// Bit C of AMBRY_GRP_IL clear: a contiguous range of group_per entries per wave (stride 64/G);
// set: rounds interleaved over the waves (wave w takes rounds w, w + nwaves, ...), so all waves
// move through the class's list together. Default: class 2 (1-4 KiB) interleaved -- 4 KiB
// records 1.10x, 3000 B 1.03x, 2000 B 1.02x, 4 KiB PUT serialization 1.03x; interleaving classes
// 0 (100 B 0.96x) or 3 (4 KiB-blob message verify 0.94x) loses.
struct GroupRange {
  uint64_t i0, i1, stride;
};
template <int G, int C>
__device__ __forceinline__ GroupRange group_range(uint64_t lo, uint64_t hi, uint64_t wave, uint64_t nwaves) {
  constexpr uint64_t S = 64 / G;
  if constexpr ((AMBRY_GRP_IL >> C) & 1) {
    return GroupRange{lo + wave * S, hi, nwaves * S};
  } else {
    const uint64_t per = group_per<G>(hi - lo, nwaves);
    const uint64_t i0 = lo + wave * per;
    return GroupRange{i0, i0 + per < hi ? i0 + per : hi, S};
  }
}

// ---- class-sized, class-balanced group phase (variant 26) ----
// group_phase gives every wave an equal COUNT of list entries, and the list is sorted by
// size class, so a batch of mixed records (a PUT message's 60 B properties, 1 KiB user
// metadata, 4 KiB blob) puts all the 4 KiB records on a third of the waves; and it runs
// every class with G = 16, so a 100 B chunk pays a 256 B block and a 4-level tree. Here
// each class is spread over all waves separately, with a group width sized to the class:
//   class 0 (<= 256 B): G = 2,  32 B blocks, 32 chunks per round (was G = 4: a round is
//                       latency-bound, so twice the chunks per round wins over a shorter chain)
//   class 1 (<= 1 KiB): G = 8, 128 B blocks,  8 chunks per round
//   class 2 (<= 4 KiB): G = 16, 256 B blocks, 4 chunks per round; class 3 (<= 16 KiB) too.
// The trailing t < 16 bytes go 16/G per lane: lane gl takes the bytes at distance
// k in [16/G*(G-1-gl), 16/G*(G-gl)) from the chunk end, T_{k&3}[b], then one shift by
// x^(32*(k>>2)) per lane, then an xor over the group.

template <int G>
__device__ __forceinline__ constexpr uint32_t group_fold_off() {  // x^(8*16G) = POW[log2 16G]
  return kPowOff + kNibSetBytes * (G == 1 ? 4u : G == 2 ? 5u : G == 4 ? 6u : G == 8 ? 7u : G == 16 ? 8u : 9u);
}

// xor over the G lanes of each group; result in every lane of the group
template <int G>
__device__ __forceinline__ uint32_t group_xor(uint32_t v) {
  if constexpr (G == 16) {  // whole rows: row_ror 8, 4, 2, 1
    v ^= dpp<0x128, 0xf>(v);
    v ^= dpp<0x124, 0xf>(v);
    v ^= dpp<0x122, 0xf>(v);
    v ^= dpp<0x121, 0xf>(v);
  } else {
    static_assert(G == 1 || G == 2 || G == 4 || G == 8, "group width");
    if constexpr (G >= 2) v ^= dppq<0xB1>(v);  // lane ^ 1
    if constexpr (G >= 4) v ^= dppq<0x4E>(v);  // lane ^ 2
    if constexpr (G == 8) v ^= (uint32_t)__shfl_xor((int)v, 4);
  }
  return v;
}

template <int G, int NB, bool NT, bool COPY = false>
__device__ __forceinline__ uint32_t group_crc_g(const uint8_t* __restrict__ base, uint64_t cs, uint64_t len,
                                                uint32_t cin, uint32_t nbw, uint32_t lane, const LaneConst& k,
                                                uint8_t* dbase = nullptr) {
  constexpr uint32_t BB = 16u * G;
  constexpr uint32_t BPL = 16u / G;  // trailing bytes per lane
  const uint32_t gl = lane & (G - 1);
  const uint32_t rinit = ~cin;
  const uint64_t ce = cs + len;
  const uint64_t cb = aligned_end(cs, ce);
  const bool body = cb > cs;
  const int64_t p0 = (int64_t)cb - (int64_t)nbw * BB + 16 * (int64_t)gl;
  const GroupCtx g{base, dbase, p0, cs, body, nbw, rinit};
  const uint32_t t = (uint32_t)(ce - cb);  // trailing < 16 bytes
  const uint32_t k0 = BPL * (G - 1 - gl);  // this lane's bytes sit at distance k0..k0+BPL-1 from the end
  // the trailing bytes are loaded with the blocks, not after the chain (one round trip)
  uint32_t tb[BPL];
#pragma unroll
  for (uint32_t i = 0; i < BPL; ++i) tb[i] = k0 + i < t ? base[ce - 1 - (k0 + i)] : 0u;
  if constexpr (COPY) {
#pragma unroll
    for (uint32_t i = 0; i < BPL; ++i)
      if (dbase && k0 + i < t) st8g(dbase + (ce - 1 - (k0 + i)), tb[i]);
  }
  constexpr int P = NB < 8 ? NB : 8;
  GroupRingT<0, P, NT, (int)BB, COPY> ring;
  ring.prime(g);
  uint32_t s = 0;
#pragma unroll 1
  for (uint32_t b0 = 0; b0 < nbw; b0 += P) s = ring.step(g, k, b0, s, group_fold_off<G>());
  uint32_t r = s;
  if (nbw) {
    if constexpr (G >= 2) r = tree_level<0>(r, lane);
    if constexpr (G >= 4) r = tree_level<1>(r, lane);
    if constexpr (G >= 8) r = tree_level<2>(r, lane);
    if constexpr (G >= 16) r = tree_level<3>(r, lane);
    if constexpr (G >= 32) r = tree_level<4>(r, lane);
  }
  r = __shfl(r, (int)(lane | (G - 1)));  // the group's body CRC, from its last lane
  if (t & 1u) r = nib_mul(r, kPowOff + kNibSetBytes * 0);
  if (t & 2u) r = nib_mul(r, kPowOff + kNibSetBytes * 1);
  if (t & 4u) r = nib_mul(r, kPowOff + kNibSetBytes * 2);
  if (t & 8u) r = nib_mul(r, kPowOff + kNibSetBytes * 3);
  // vq[q]: the lane's bytes 4q..4q+3 (16/G > 4 for G < 4), each quad one x^(8*4) further
  constexpr uint32_t NQ = (BPL + 3) / 4;
  uint32_t vq[NQ];
#pragma unroll
  for (uint32_t q = 0; q < NQ; ++q) vq[q] = 0;
  uint32_t v = 0;
  if (k0 < t) {
#pragma unroll
    for (uint32_t i = 0; i < BPL; ++i) {
      const uint32_t kk = k0 + i;
      if (kk < t) {
        const uint64_t at = ce - 1 - kk;
        uint32_t byte = tb[i];
        if (at < cs + 4) byte ^= (rinit >> (8 * (uint32_t)(at - cs))) & 0xFFu;
        const uint32_t j = kk & 3;
        vq[i / 4] ^= lds_rd(((j >> 1) << 16) | (byte << 8) | ((j & 1) << 7) | ((lane & 31) << 2));
      }
    }
    v = vq[NQ - 1];
#pragma unroll
    for (int q = (int)NQ - 2; q >= 0; --q) v = vq[q] ^ nib_mul(v, kPowOff + kNibSetBytes * 2);
    if (k0 & 4) v = nib_mul(v, kPowOff + kNibSetBytes * 2);  // x^(8*4)
    if (k0 & 8) v = nib_mul(v, kPowOff + kNibSetBytes * 3);  // x^(8*8)
  }
  v = group_xor<G>(v);
  uint32_t crc = r ^ v ^ 0xFFFFFFFFu;
  if (len < 4) crc ^= rinit >> (8 * (uint32_t)len);
  return crc;
}

// Group body with 64-B lane runs (G = 8 for class 1, G = 16 for classes 2-3): the wave-mode
// transpose inside each G-lane group (G = 16 shown). A 1 KiB super-block is 4 loads per lane (load i:
// lane gl <- bytes [16gl, 16gl+16) of 256-B block i, 256 B contiguous per group); the quad
// transpose leaves lane gl = 4m + j holding the 64-B run [64m, 64m+64) of block j, which
// it walks as one 16-step slice-by-4 chain; the lane state hops one super-block with
// FOLD = x^(8*1024). Tree: gl bits 2, 3 merge the runs of a block (64, 128 B = POW[6, 7]),
// bits 0, 1 the blocks (256, 512 B = POW[8, 9]). 18 LDS reads per 16 B-lane piece... per
// KiB of chunk, against 24 for the 16-B-piece body; one super-block prefetched
// (group_class_t4s below).
template <bool NT>
__device__ __forceinline__ void group_fix_piece(u32x4& w, int64_t p, uint64_t cs, uint32_t rinit) {
  if (p + 16 <= (int64_t)cs) w = u32x4{0u, 0u, 0u, 0u};  // loaded from the dummy address (t4_load)
  if (p < (int64_t)cs + 4 && p + 16 > (int64_t)cs) {
    w = xor_init(w, p, cs, rinit);
    if (p < (int64_t)cs) {
      const uint32_t cut = (uint32_t)((int64_t)cs - p);
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int lo = (int)cut - 4 * d;
        const uint32_t m = lo <= 0 ? 0xFFFFFFFFu : (lo >= 4 ? 0u : (0xFFFFFFFFu << (8 * lo)));
        w[d] &= m;
      }
    }
  }
}

// Merge of the lanes' run states inside a group: gl bits 2.. (the runs of one block, shifts
// 64 B * 2^b = POW[6 + b]), then bits 0, 1 (the blocks, 16G B * 2^b = POW[log2(16G) + b]).
template <int G>
__device__ __forceinline__ uint32_t group_tree_t4(uint32_t r, uint32_t lane) {
  constexpr uint32_t LB = G == 8 ? 7u : 8u;  // log2(16G)
  r = tree_level_t4<2, 6>(r, lane);
  if constexpr (G == 16) r = tree_level_t4<3, 7>(r, lane);
  r = tree_level_t4<0, LB>(r, lane);
  r = tree_level_t4<1, LB + 1>(r, lane);
  return r;
}

// ---- streamed 64-B-run group path (classes 1-3) ----
// Run per round (descriptors, first super-block, steps, tree), a wave pays a bubble at every
// round start: the round's first super-block is only issued once the round begins, after two
// dependent descriptor loads, so a wave whose rounds are 1-4 steps long spends up to three
// memory round trips per round with nothing in flight. Here a wave's rounds form one stream
// of steps: the step that ends round r issues round r+1's first super-block (and its trailing
// bytes and stored CRC), so one super-block per group is always in flight, across round
// boundaries as within a round. Chunk descriptors are loaded a round ahead and list entries
// two rounds ahead (an entry past the wave's range re-reads its first: always loaded, never
// used).
// Every load here is issued unconditionally: a lane whose piece lies outside its chunk reads
// 16 B of the (cache-resident) table image instead, zeroed in group_fix_piece. A load under a
// lane-divergent branch is skipped when no lane takes it, so the number of loads in flight
// would depend on the path and the compiler would wait for all of them (vmcnt(0)) before
// using any: the prefetched super-block would be waited for before the current one is used.
struct T4Round {
  int64_t p0;        // this lane's first piece address (virtual start + 16 gl)
  uint64_t cs, ce, cb;
  uint32_t nbw;      // super-blocks this round (max over the wave's groups)
  uint32_t rinit, t, ci;
  bool act;
  uint64_t dsh;      // copy-through: the destination of source offset p is (uint8_t*)dsh + p
};

template <int G>
__device__ __forceinline__ T4Round t4_round(uint32_t ci, uint64_t len, uint64_t off, uint32_t cin, bool act,
                                            uint32_t lane) {
  T4Round r;
  len = act ? len : 0;
  off = act ? off : 0;
  r.cs = off;
  r.ce = off + len;
  r.cb = aligned_end(off, r.ce);
  const uint32_t nb = (uint32_t)((r.cb - off + 64 * G - 1) / (64 * G));
  uint32_t nbw = 0;
#pragma unroll
  for (uint32_t q = 0; q < 64 / G; ++q) {
    const uint32_t x = __builtin_amdgcn_readlane(nb, q * G);
    nbw = x > nbw ? x : nbw;
  }
  r.nbw = nbw;
  r.p0 = (int64_t)r.cb - (int64_t)nbw * (64 * G) + 16 * (int64_t)(lane & (G - 1));
  r.rinit = ~(act ? cin : 0u);
  r.t = (uint32_t)(r.ce - r.cb);
  r.ci = ci;
  r.act = act;
  r.dsh = 0;
  return r;
}

// Super-block sb of a round given by its fields (passed by value: a select between two rounds'
// structs through a reference would put both on the stack).
template <bool NT, int G>
__device__ __forceinline__ void t4_load(const uint8_t* __restrict__ base, const uint8_t* __restrict__ dummy,
                                        int64_t p0, uint64_t cs, uint64_t cb, uint32_t nbw, uint32_t sb,
                                        u32x4 (&x)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t p = p0 + (int64_t)sb * (64 * G) + (16 * G) * i;
    const bool in = sb < nbw && cb > cs && p + 16 > (int64_t)cs;  // => floor16(cs) <= p < cb
    x[i] = ld16<NT>(reinterpret_cast<const u32x4*>(in ? base + p : dummy));
  }
}

// The round's trailing bytes (16/G per lane) and, for message verify, its stored CRC.
template <int G>
__device__ __forceinline__ uint64_t t4_aux(const SweepArgs& a, const uint8_t* __restrict__ dummy, const T4Round& r,
                                           uint32_t lane, uint32_t (&tb)[16 / G]) {
  constexpr uint32_t BPL = 16u / G;
  const uint32_t k0 = BPL * (G - 1 - (lane & (G - 1)));
#pragma unroll
  for (uint32_t i = 0; i < BPL; ++i) tb[i] = *(k0 + i < r.t ? a.base + (r.ce - 1 - (k0 + i)) : dummy);
  uint64_t stored = 0;
  if (a.exp_fill) {
    const bool leader = (lane & (G - 1)) == 0 && r.act;
    __builtin_memcpy(&stored, leader ? a.base + r.ce : dummy, 8);
  }
  return stored;
}

// The round's CRCs from the lanes' chain states: tree over the group, trailing bytes, xor-out.
template <int G>
__device__ __forceinline__ uint32_t t4_finish(const T4Round& r, uint32_t s, const uint32_t (&tb)[16 / G],
                                              uint32_t lane) {
  constexpr uint32_t BPL = 16u / G;
  const uint32_t k0 = BPL * (G - 1 - (lane & (G - 1)));
  uint32_t rr = r.nbw ? group_tree_t4<G>(s, lane) : 0u;
  rr = __shfl(rr, (int)(lane | (G - 1)));
  const uint32_t t = r.t;
  if (t & 1u) rr = nib_mul(rr, kPowOff + kNibSetBytes * 0);
  if (t & 2u) rr = nib_mul(rr, kPowOff + kNibSetBytes * 1);
  if (t & 4u) rr = nib_mul(rr, kPowOff + kNibSetBytes * 2);
  if (t & 8u) rr = nib_mul(rr, kPowOff + kNibSetBytes * 3);
  uint32_t v = 0;
  if (k0 < t) {
#pragma unroll
    for (uint32_t i = 0; i < BPL; ++i) {
      const uint32_t kk = k0 + i;
      if (kk < t) {
        const uint64_t at = r.ce - 1 - kk;
        uint32_t byte = tb[i];
        if (at < r.cs + 4) byte ^= (r.rinit >> (8 * (uint32_t)(at - r.cs))) & 0xFFu;
        const uint32_t j = kk & 3;
        v ^= lds_rd(((j >> 1) << 16) | (byte << 8) | ((j & 1) << 7) | ((lane & 31) << 2));
      }
    }
    if (k0 & 4) v = nib_mul(v, kPowOff + kNibSetBytes * 2);
    if (k0 & 8) v = nib_mul(v, kPowOff + kNibSetBytes * 3);
  }
  v = group_xor<G>(v);
  uint32_t crc = rr ^ v ^ 0xFFFFFFFFu;
  const uint64_t len = r.ce - r.cs;
  if (len < 4) crc ^= r.rinit >> (8 * (uint32_t)len);
  return crc;
}

template <int G, int C, bool NT, bool COPY = false>
__device__ __forceinline__ void group_class_t4s(const SweepArgs& a, uint64_t lo, uint64_t hi, uint32_t wave,
                                                uint64_t nwaves, uint32_t lane, const LaneConst& k) {
  static_assert(G == 8 || G == 16, "64-B run groups are 8 or 16 lanes");
  constexpr uint32_t BPL = 16u / G;
  constexpr uint32_t kFold = G == 16 ? kFoldOff : kPowOff + kNibSetBytes * 9;  // x^(8*64G)
  if (hi <= lo) return;
  const GroupRange gr = group_range<G, C>(lo, hi, wave, nwaves);
  const uint64_t i0 = gr.i0, i1 = gr.i1, D = gr.stride;
  if (i0 >= hi) return;
  const uint32_t gi = lane / G;
  const uint8_t* dummy = reinterpret_cast<const uint8_t*>(a.img);
  auto idx_at = [&](uint64_t i) -> uint32_t { return a.small_idx[i + gi < i1 ? i + gi : i0]; };
  const uint32_t ci0 = idx_at(i0);
  uint32_t ci_n = idx_at(i0 + D);
  T4Round r = t4_round<G>(ci0, a.len[ci0], a.off[ci0], a.crc_in ? a.crc_in[ci0] : 0u, i0 + gi < i1, lane);
  if constexpr (COPY) {
    const uint64_t co = a.copy_off[ci0];
    r.dsh = co == kCopySkip ? 0 : (uint64_t)(uintptr_t)a.copy_dst + co - r.cs;
  }
  uint32_t tb[BPL];
  uint64_t stored = t4_aux<G>(a, dummy, r, lane, tb);
  uint64_t len_n = a.len[ci_n], off_n = a.off[ci_n];
  uint32_t cin_n = a.crc_in ? a.crc_in[ci_n] : 0u;
  uint64_t dst_n = COPY ? a.copy_off[ci_n] : 0;
  uint32_t ci_nn = idx_at(i0 + 2 * D);
  u32x4 nx[4];
  t4_load<NT, G>(a.base, dummy, r.p0, r.cs, r.cb, r.nbw, 0, nx);
  T4Round rn = r;
  uint32_t tbn[BPL];
  uint64_t stored_n = 0;
  uint64_t i = i0;
  uint32_t sb = 0, s = 0;
#pragma unroll 1
  while (true) {
    u32x4 x[4] = {nx[0], nx[1], nx[2], nx[3]};
    const bool last = sb + 1 >= r.nbw;  // wave-uniform
    if (last) {  // descriptors of round r+1 (loaded a round ago); start loading r+2's and r+3's entry
      rn = t4_round<G>(ci_n, len_n, off_n, cin_n, i + D + gi < i1, lane);
      if constexpr (COPY) rn.dsh = dst_n == kCopySkip ? 0 : (uint64_t)(uintptr_t)a.copy_dst + dst_n - rn.cs;
      stored_n = t4_aux<G>(a, dummy, rn, lane, tbn);
      ci_n = ci_nn;
      len_n = a.len[ci_n];
      off_n = a.off[ci_n];
      cin_n = a.crc_in ? a.crc_in[ci_n] : 0u;
      if constexpr (COPY) dst_n = a.copy_off[ci_n];
      ci_nn = idx_at(i + 3 * D);
    }
    // the next step, whichever round it is in
#if AMBRY_GRP_PRIO
    __builtin_amdgcn_s_setprio(3);
#endif
    t4_load<NT, G>(a.base, dummy, last ? rn.p0 : r.p0, last ? rn.cs : r.cs, last ? rn.cb : r.cb,
                   last ? rn.nbw : r.nbw, last ? 0u : sb + 1, nx);
#if AMBRY_GRP_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
    if constexpr (COPY) {
      if (r.cb > r.cs) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          copy_piece(reinterpret_cast<uint8_t*>(r.dsh), r.p0 + (int64_t)sb * (64 * G) + (16 * G) * q, x[q],
                     (int64_t)r.cs);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      group_fix_piece<NT>(x[q], r.p0 + (int64_t)sb * (64 * G) + (16 * G) * q, r.cs, r.rinit);
    quad_transpose_asm(x);
    s = run_crc<4>(x, k, sb ? nib_mul(s, kFold) : 0u);
    if (!last) {
      ++sb;
      continue;
    }
    const uint32_t crc = t4_finish<G>(r, r.nbw ? s : 0u, tb, lane);
    if constexpr (COPY) {  // the round's trailing bytes
      const uint32_t k0 = BPL * (G - 1 - (lane & (G - 1)));
#pragma unroll
      for (uint32_t q = 0; q < BPL; ++q)
        if (r.dsh && k0 + q < r.t) st8g(reinterpret_cast<uint8_t*>(r.dsh) + (r.ce - 1 - (k0 + q)), tb[q]);
    }
    if ((lane & (G - 1)) == 0 && r.act) {
      a.out[r.ci] = crc;
      if (a.exp_fill) {
        const uint64_t st = __builtin_bswap64(stored);
        a.exp_fill[r.ci] = (st >> 32) ? ~crc : (uint32_t)st;
      }
    }
    i += D;
    if (i >= i1) break;
    r = rn;
    stored = stored_n;
#pragma unroll
    for (uint32_t q = 0; q < BPL; ++q) tb[q] = tbn[q];
    sb = 0;
  }
}

// One size class [lo, hi) of the list, spread over all waves: wave w takes entries
// [lo + w*per, lo + (w+1)*per), per a multiple of 64/G.
template <int G, int NB, bool NT, bool COPY = false>
__device__ __forceinline__ void group_class(const SweepArgs& a, uint64_t lo, uint64_t hi, uint32_t wave,
                                            uint64_t nwaves, uint32_t lane, const LaneConst& k) {
  constexpr uint32_t S = 64 / G;
  if (hi <= lo) return;
  const GroupRange gr = group_range<G, 0>(lo, hi, wave, nwaves);
  const uint64_t i1 = gr.i1;
  const uint32_t gi = lane / G;
#pragma unroll 1
  for (uint64_t i = gr.i0; i < i1; i += gr.stride) {
    const bool act = i + gi < i1;
    const uint32_t ci = act ? a.small_idx[i + gi] : 0u;
    uint64_t len = 0, off = 0;
    uint32_t cin = 0;
    if (act) {
      len = a.len[ci];
      off = a.off[ci];
      cin = a.crc_in ? a.crc_in[ci] : 0u;
    }
    const uint64_t cb = aligned_end(off, off + len);
    constexpr uint32_t BLK = 16 * G;  // bytes per chain step
    const uint32_t nb = (uint32_t)((cb - off + BLK - 1) / BLK);
    uint32_t nbw = 0;
#pragma unroll
    for (uint32_t q = 0; q < S; ++q) {
      const uint32_t x = __builtin_amdgcn_readlane(nb, q * G);
      nbw = x > nbw ? x : nbw;
    }
    const bool leader = (lane & (G - 1)) == 0 && act;
    uint64_t stored = 0;
    if (a.exp_fill && leader) {  // message verify: the record's stored CRC follows its bytes
      __builtin_memcpy(&stored, a.base + off + len, 8);  // issued now, used after the chain
      stored = __builtin_bswap64(stored);
    }
    uint8_t* dbase = nullptr;
    if constexpr (COPY) {  // dst of source offset p: dbase + p
      const uint64_t co = a.copy_off[ci];
      dbase = act && co != kCopySkip ? a.copy_dst + (co - off) : nullptr;
    }
    const uint32_t crc = group_crc_g<G, NB, NT, COPY>(a.base, off, len, cin, nbw, lane, k, dbase);
    if (leader) {
      a.out[ci] = crc;
      if (a.exp_fill) a.exp_fill[ci] = (stored >> 32) ? ~crc : (uint32_t)stored;
    }
  }
}

// Class 0's group width and ring depth (A/B knobs for tools/ab_build.sh AB_FLAGS): 2-lane groups,
// 8 blocks in flight, 32 chunks per round -- measured 1.57x faster than 4-lane groups on 100 B
// records. Class 1 at G = 4 or 2 measured slower (1.1x, 1.75x).

// class bounds from the plan: small_total = {total, start of class 1, 2, 3}
__device__ __forceinline__ bool group_cls_has_work(const SweepArgs& a, uint32_t first_wave, uint64_t nwaves) {
  const uint64_t c0 = 0, c1 = a.small_total[1], c2 = a.small_total[2], c3 = a.small_total[3];
  const uint64_t c4 = a.small_total[0];
  return (c1 > c0 && group_range<AMBRY_C0_G, 0>(c0, c1, first_wave, nwaves).i0 < c1) ||
         (c2 > c1 && group_range<8, 1>(c1, c2, first_wave, nwaves).i0 < c2) ||
         (c3 > c2 && group_range<16, 2>(c2, c3, first_wave, nwaves).i0 < c3) ||
         (c4 > c3 && group_range<16, 3>(c3, c4, first_wave, nwaves).i0 < c4);
}

// Class 0 (<= 256 B) in 2-lane groups of 16-B pieces; classes 1-3 with 64-B lane runs in 8- and
// 16-lane groups.
template <bool NT, bool COPY = false>
__device__ __forceinline__ void group_phase_cls(const SweepArgs& a, uint32_t wave, uint64_t nwaves, uint32_t lane,
                                                const LaneConst& k) {
  const uint64_t c1 = a.small_total[1], c2 = a.small_total[2], c3 = a.small_total[3], c4 = a.small_total[0];
  group_class<AMBRY_C0_G, AMBRY_C0_NB, NT, COPY>(a, 0, c1, wave, nwaves, lane, k);
  group_class_t4s<8, 1, NT, COPY>(a, c1, c2, wave, nwaves, lane, k);
  group_class_t4s<16, 2, NT, COPY>(a, c2, c3, wave, nwaves, lane, k);
  group_class_t4s<16, 3, NT, COPY>(a, c3, c4, wave, nwaves, lane, k);
}

// Chunk-relative cut for global stream position g inside chunk c (0 < r < len):
// snapped so the memory address is 16-B aligned. Pure function of (g, chunk), so the
// two waves meeting at g agree on it.
__device__ __forceinline__ uint64_t snap_cut(uint64_t cs, uint64_t len, uint64_t r) {
  const uint64_t a = (cs + r + 15) & ~uint64_t(15);
  const uint64_t rr = a - cs;
  return rr < len ? rr : len;
}

// Persistent sweep: wave w owns global bytes [w*share, (w+1)*share) of the batch viewed
// as one concatenated stream (byte_start = exclusive scan of len), i.e. an equal share of
// bytes whatever the chunk-size mix. Each (wave, chunk) intersection is a segment whose
// raw CRC is shifted to the chunk end and XORed into out[chunk].
//   T4 = false (variant 0): 16-B pieces per lane, 8 blocks in flight, two pieces interleaved
//   T4 = true  (variant 29): 64-B lane runs from coalesced 4 KiB super-blocks (quad transpose),
//                one super-block prefetched, s_setprio 3 around its loads
//   GROUP: whole chunks <= 16 KiB go to the class-sized group phase first (same launch)
//   COPY: copy-through (SweepArgs::copy_dst), T4 and GROUP only
template <bool T4, bool GROUP, int DIAG = 0, bool COPY = false>
__global__ __launch_bounds__(1024) void crc32_sweep_kernel(SweepArgs a) {
  static_assert(!COPY || (T4 && DIAG == 0), "copy-through is built for the 64-B-run sweep only");
  if (COPY && a.gate && *a.gate == 0) return;  // the transform's gated general path (uniform)
  // Shares are wave-major over workgroups (share i -> wave i / gridDim.x of workgroup
  // i % gridDim.x), so when a batch has fewer shares than waves they spread over every
  // CU. A share is at least kMinShare bytes: a lone large chunk is cut into ~total/16 KiB
  // segments, not one per wave (each segment ends in an atomic on the chunk's word).
  const uint32_t waves_per_block = blockDim.x >> 6;
  const uint64_t nwaves = (uint64_t)gridDim.x * waves_per_block;
  const uint64_t total = a.byte_start[a.n];
  uint64_t share = ((total + nwaves - 1) / nwaves + kShareQuantum - 1) & ~uint64_t(kShareQuantum - 1);
  share = share < kMinShare ? kMinShare : share;
  // Fused group phase: the workgroup first takes its part of each class of the small-chunk list.
  const uint64_t ns = GROUP ? *a.small_total : 0;
  const bool grp = GROUP && ns > 0 && group_cls_has_work(a, blockIdx.x, nwaves);
  if ((uint64_t)blockIdx.x * share >= total && !grp) return;  // uniform: no work for this workgroup
  fill_lds(a.img);

  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) * gridDim.x + blockIdx.x);
  if constexpr (GROUP) {
    if (grp) group_phase_cls<true, COPY>(a, wave, nwaves, lane, make_lane_const(lane));
  }
  // Rounds (SweepArgs::window): equal shares sized so R rounds of nwaves shares cover the
  // batch; wave w takes shares w, w + nwaves, ... A 256 GiB batch read as one round of
  // 16 MiB shares ran at 95.5 % of a 32 GiB batch's read rate (TLB reach of the spread).
  uint64_t S = share;
  uint64_t round_step = 0;
  if (a.window && total > a.window) {
    const uint64_t R = (total + a.window - 1) / a.window;
    S = ((total + R * nwaves - 1) / (R * nwaves) + kShareQuantum - 1) & ~uint64_t(kShareQuantum - 1);
    S = S < kMinShare ? kMinShare : S;
    round_step = nwaves * S;
  }
  uint64_t g0 = (uint64_t)wave * S;
  if (g0 >= total) return;
  uint64_t g1 = g0 + S < total ? g0 + S : total;
  const uint32_t* xpow2 = a.img + kLdsBytes / 4;
  const LaneConst k = make_lane_const(lane);

  uint64_t init_len = ~0ull;  // one-entry cache of the init term for crc_in == 0
  uint32_t init_term = 0;

  // One segment: raw CRC of its body, shifted to the chunk end, + tail + init (wave-uniform).
  // *whole: the segment is the entire chunk, so no other wave contributes to out[ci].
  // dsh (COPY): the destination of source offset p is (uint8_t*)dsh + p
  auto segment = [&](uint64_t bsc, uint64_t len, uint64_t cs, uint32_t cin, uint64_t dsh, bool* whole) -> uint32_t {
    const uint64_t ce = cs + len;
    const uint64_t cb = aligned_end(cs, ce);
    const uint64_t r0 = g0 > bsc ? snap_cut(cs, len, g0 - bsc) : 0;
    const uint64_t r1 = g1 - bsc < len ? snap_cut(cs, len, g1 - bsc) : len;
    *whole = r0 == 0 && r1 == len;
    if (r0 >= r1) return 0u;
    const uint64_t sa = cs + r0, se = cs + r1;
    const uint64_t be = se == ce ? cb : se;  // 16-B aligned body end
    uint32_t r = 0;
    if (sa < be) {
      if constexpr (T4) {
        r = body_crc_t4<1, true, true, COPY>(a.base, sa, be, lane, k, reinterpret_cast<uint8_t*>(dsh));
      } else {
        r = body_crc<8, true, DIAG>(a.base, sa, be, lane, k);
      }
      r = __builtin_amdgcn_readlane(r, 63);
      r = shift_bytes(r, ce - be, xpow2);
    }
    if (se == ce && ce > cb) {  // trailing < 16 bytes, lane-parallel
      const uint64_t t0 = sa > cb ? sa : cb;
      r ^= __builtin_amdgcn_readlane(tail_crc(a.base + t0, (uint32_t)(ce - t0), lane), 0);
      if constexpr (COPY) {
        if (dsh && lane < ce - t0) st8g(reinterpret_cast<uint8_t*>(dsh) + t0 + lane, a.base[t0 + lane]);
      }
    }
    if (r0 == 0) {  // initial register ~crc_in advanced over the chunk, plus xor-out
      if (cin == 0) {
        if (len != init_len) {
          init_term = shift_bytes(0xFFFFFFFFu, len, xpow2) ^ 0xFFFFFFFFu;
          init_len = len;
        }
        r ^= init_term;
      } else {
        r ^= shift_bytes(~cin, len, xpow2) ^ 0xFFFFFFFFu;
      }
    }
    return r;
  };
  // A partial segment shares its chunk with a neighbouring wave: combine by XOR.
  auto emit_partial = [&](uint32_t ci, uint32_t r) {
    if constexpr (DIAG == 2) {  // diagnostic timing build: no per-segment atomic (wrong CRCs)
      if (lane == 0 && r == 0x9E3779B9u) a.out[ci] = r;
    } else {
      if (lane == 0) atomicXor(&a.out[ci], r);
    }
  };

  for (;;) {
    uint32_t c = __builtin_amdgcn_readfirstlane(find_start(a.byte_start, a.n, g0, lane));
    // Descriptors fetched 64 at a time (lane j <- chunk c+j), read back with readlane:
    // one load round trip per 64 chunks. byte_start only seeds a scalar running sum, so
    // 5 VGPRs stay live across the body.
    bool done = false;
    while (!done && c < a.n) {
      const uint32_t cnt = a.n - c < 64u ? a.n - c : 64u;
      uint64_t w_bs = ~0ull, w_len = 0, w_off = 0, w_dst = 0;
      uint32_t w_cin = 0;
      if (lane < cnt) {
        w_bs = a.byte_start[c + lane];
        w_len = a.len[c + lane];
        w_off = a.off[c + lane];
        w_cin = a.crc_in ? a.crc_in[c + lane] : 0u;
        if constexpr (COPY) {
          const uint64_t co = a.copy_off[c + lane];
          w_dst = co == kCopySkip ? 0 : (uint64_t)(uintptr_t)a.copy_dst + co - w_off;
        }
      }
      uint64_t bsc = readlane64(w_bs, 0);
      bool work = false;
      for (uint32_t j = 0; j < cnt;) {
        if (bsc >= g1) {
          done = true;
          break;
        }
        const uint64_t len = readlane64(w_len, j);
        const uint64_t span = len > a.small_max ? len : 0;  // small chunks: group phase
        if (span != 0) {  // empty chunks are finished by the plan kernel
          work = true;
          bool whole;
          const uint32_t r = segment(bsc, len, readlane64(w_off, j), __builtin_amdgcn_readlane(w_cin, j),
                                     COPY ? readlane64(w_dst, j) : 0, &whole);
          if (whole && DIAG != 2) {
            if (lane == 0) a.out[c + j] = r;  // no other wave contributes to this chunk
          } else {
            emit_partial(c + j, r);
          }
        }
        bsc += span;
        ++j;
      }
      // A window with no byte share (empty chunks, or small ones the group phase took) may head a
      // long run of them at one byte position: jump to the run's end (the chunk holding byte bsc)
      // instead of walking it 64 descriptors at a time.
      uint32_t next = c + cnt;
      if (!work && !done && next < a.n) {
        const uint32_t far = __builtin_amdgcn_readfirstlane(find_start(a.byte_start, a.n, bsc, lane));
        next = far > next ? far : next;
      }
      c = next;
    }
    if (round_step == 0) break;
    g0 += round_step;
    if (g0 >= total) break;
    g1 = g0 + S < total ? g0 + S : total;
  }
}

// ------------------------------------------------------------------ planning
// byte_start = exclusive scan of len (64-bit), in two small launches: count (per-block
// sums) and scan (block-local scans + carry of earlier blocks). Blocks of 256 threads
// own kPlanPerBlock consecutive chunks, loaded in rounds of 256 (coalesced). The scan
// also initialises out[]: 0 for chunks the sweep will XOR into, crc_in (the CRC of
// nothing continued from crc_in) for empty chunks; chunks the group phase takes whole
// (small) are left alone, it stores their CRC.
// Inclusive wave scan of a 64-bit value with DPP: row_shr 1/2/4/8 inside 16-lane rows,
// then row_bcast:15 (rows 1, 3) and row_bcast:31 (rows 2, 3). VALU only -- a __shfl_up
// ladder is 12 dependent ds_bpermute round trips per 64-bit scan.
__device__ __forceinline__ uint64_t wave_scan64(uint64_t v) {
#define AMBRY_SCAN_STEP(C, R)                                  \
  {                                                            \
    const uint32_t lo = dpp<C, R>((uint32_t)v);                \
    const uint32_t hi = dpp<C, R>((uint32_t)(v >> 32));        \
    v += ((uint64_t)hi << 32) | lo;                            \
  }
  AMBRY_SCAN_STEP(0x111, 0xf)
  AMBRY_SCAN_STEP(0x112, 0xf)
  AMBRY_SCAN_STEP(0x114, 0xf)
  AMBRY_SCAN_STEP(0x118, 0xf)
  AMBRY_SCAN_STEP(0x142, 0xa)
  AMBRY_SCAN_STEP(0x143, 0xc)
#undef AMBRY_SCAN_STEP
  return v;
}

// Inclusive scans of N values across a 256-thread block, one pair of barriers for all N:
// v[i] becomes the inclusive prefix, total[i] the block total.
template <int N>
__device__ __forceinline__ void block_scan256(uint64_t (&v)[N], uint64_t (&total)[N]) {
  __shared__ uint64_t wsum[4][N];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    v[i] = wave_scan64(v[i]);
    if (lane == 63) wsum[wv][i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) {
    uint64_t before = 0;
    for (uint32_t w = 0; w < wv; ++w) before += wsum[w][i];
    total[i] = wsum[0][i] + wsum[1][i] + wsum[2][i] + wsum[3][i];
    v[i] += before;
  }
  __syncthreads();
}

// Bytes a chunk contributes to the sweep's byte shares: chunks the group kernel takes
// whole (len <= small_max) contribute none.
__device__ __forceinline__ uint64_t share_len(uint64_t len, uint64_t small_max) {
  return len > small_max ? len : 0u;
}

__device__ __forceinline__ bool is_small(uint64_t len, uint64_t small_max) { return len != 0 && len <= small_max; }

// Size class of a small chunk (<= 256 B, 1 KiB, 4 KiB, more): the compacted list is
// ordered by class, so a group-phase round (64/G consecutive entries) holds chunks of
// similar length and its chain -- the longest chunk's block count -- wastes little.
__device__ __forceinline__ uint32_t small_class(uint64_t len) {
  return len <= 256 ? 0u : len <= AMBRY_C1_MAX ? 1u : len <= 4096 ? 2u : 3u;
}
// Per-chunk class indicator packed as 16-bit fields (a plan block has <= kPlanPerBlock <= 65535 chunks).
__device__ __forceinline__ uint64_t class_onehot(uint64_t len, uint64_t small_max) {
  return is_small(len, small_max) ? (1ull << (16 * small_class(len))) : 0ull;
}
__device__ __forceinline__ uint64_t field16(uint64_t v, uint32_t c) { return (v >> (16 * c)) & 0xFFFFu; }

__global__ __launch_bounds__(256) void crc32_plan_count_kernel(PlanArgs a) {
  if (a.gate && *a.gate == 0) return;
  const uint32_t base = blockIdx.x * kPlanPerBlock;
  uint64_t len[kPlanPerBlock / 256];  // every round's load in flight before the first use
#pragma unroll
  for (uint32_t r = 0; r < kPlanPerBlock / 256; ++r) {
    const uint32_t c = base + r * 256 + threadIdx.x;
    len[r] = c < a.n ? a.len[c] : 0u;
  }
  uint64_t v[2] = {0, 0}, total[2];
#pragma unroll
  for (uint32_t r = 0; r < kPlanPerBlock / 256; ++r) {
    v[0] += share_len(len[r], a.small_max);
    v[1] += class_onehot(len[r], a.small_max);
  }
  block_scan256<2>(v, total);
  if (threadIdx.x == 0) {
    a.block_sum[blockIdx.x] = total[0];
    a.block_small[blockIdx.x] = total[1];  // packed: 4 x 16-bit class counts
  }
}

// Scan: a thread owns R = kPlanPerBlock / 256 consecutive chunks. Lengths arrive in coalesced
// rounds of 256 (with crc_in; out[] is initialised right there, it needs no scan), are transposed
// through LDS (runs padded to R + 1 words: conflict-free strided reads), summed serially per
// thread and scanned once across the block; byte_start goes back through the same LDS slots to
// coalesced stores. One block scan per block instead of two wave scans per round: 94 VGPRs
// (5 waves per SIMD) against 164 (3 waves) for the round-by-round form.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void crc32_plan_scan_kernel(PlanArgs a) {
  if (a.gate && *a.gate == 0) return;
  constexpr uint32_t R = kPlanPerBlock / 256;
  constexpr uint32_t P = R + 1;
  __shared__ uint64_t lds[256 * P];
  const uint32_t nblocks = gridDim.x;
  const uint32_t base = blockIdx.x * kPlanPerBlock;
  const uint32_t tid = threadIdx.x;
  {
    uint64_t len[R];  // every round's load in flight before the first use (clamped index)
    uint32_t cin[R];
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) {
      const uint32_t c = base + r * 256 + tid;
      const uint32_t cc = c < a.n ? c : a.n - 1;
      len[r] = a.len[cc];
      cin[r] = a.crc_in ? a.crc_in[cc] : 0u;  // read before out[c] is written (out may alias crc_in)
    }
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) {
      const uint32_t i = r * 256 + tid, c = base + i;
      const bool in = c < a.n;
      lds[(i / R) * P + i % R] = in ? len[r] : 0u;  // chunks past n: length 0 (no share, no class)
      if (in) {
        if (a.crc_stage) a.crc_stage[c] = cin[r];
        // small chunks: the group phase stores their CRC whole (no XOR into out), so no init
        if (!is_small(len[r], a.small_max)) a.out[c] = len[r] ? 0u : cin[r];
      }
    }
  }
  __syncthreads();
  uint64_t tsum = 0, tcls = 0;
#pragma unroll
  for (uint32_t j = 0; j < R; ++j) {
    const uint64_t ln = lds[tid * P + j];
    tsum += share_len(ln, a.small_max);
    tcls += class_onehot(ln, a.small_max);
  }
  // One 7-value block scan: v[0] = byte carry of earlier blocks; v[1], v[2] class counts of earlier
  // blocks and v[3], v[4] of all blocks, two 32-bit fields each (classes 0|1, 2|3; their totals are
  // what is used); v[5] / v[6] this thread's bytes / packed 16-bit class counts (their prefixes
  // place the thread's run).
  uint64_t v[7] = {0, 0, 0, 0, 0, 0, 0}, tot[7];
  int any_share = 0;  // some block has share bytes
  if (nblocks > 1) {
    // four entries per thread per pass, every load issued (clamped index) before any is used
    for (uint32_t i0 = tid; i0 < nblocks; i0 += 1024) {
      uint64_t bs[4], bm[4];
#pragma unroll
      for (uint32_t u = 0; u < 4; ++u) {
        const uint32_t i = i0 + 256 * u;
        const uint32_t ic = i < nblocks ? i : 0u;
        bs[u] = a.block_sum[ic];
        bm[u] = a.small_max ? a.block_small[ic] : 0u;
      }
#pragma unroll
      for (uint32_t u = 0; u < 4; ++u) {
        const uint32_t i = i0 + 256 * u;
        const bool in = i < nblocks, earlier = i < blockIdx.x;  // earlier implies in
        const uint64_t lo = field16(bm[u], 0) | (field16(bm[u], 1) << 32);
        const uint64_t hi = field16(bm[u], 2) | (field16(bm[u], 3) << 32);
        v[0] += earlier ? bs[u] : 0u;
        v[1] += earlier ? lo : 0u;
        v[2] += earlier ? hi : 0u;
        v[3] += in ? lo : 0u;
        v[4] += in ? hi : 0u;
        any_share |= in && bs[u] != 0;
      }
    }
  }
  v[5] = tsum;
  v[6] = tcls;
  block_scan256<7>(v, tot);
  uint64_t cls_total[4], cls_carry[4];
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t sh = 32 * (k & 1);
    cls_total[k] = nblocks > 1 ? (tot[3 + (k >> 1)] >> sh) & 0xFFFFFFFFu : field16(tot[6], k);  // one block: its own
    cls_carry[k] = nblocks > 1 ? (tot[1 + (k >> 1)] >> sh) & 0xFFFFFFFFu : 0u;
  }
  // class c's list entries start at base[c] = chunks of classes < c
  uint64_t cls_base[4];
  cls_base[0] = 0;
  cls_base[1] = cls_total[0];
  cls_base[2] = cls_base[1] + cls_total[1];
  cls_base[3] = cls_base[2] + cls_total[2];
  const uint64_t before_cls = v[6] - tcls;  // earlier threads of this block, packed
  uint64_t pos[4];
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) pos[k] = cls_base[k] + cls_carry[k] + field16(before_cls, k);
  uint64_t b = tot[0] + v[5] - tsum;  // bytes of earlier blocks and of earlier threads
#pragma unroll
  for (uint32_t j = 0; j < R; ++j) {
    const uint64_t ln = lds[tid * P + j];  // the thread's own slots: read, then reused for byte_start
    const uint32_t c = base + tid * R + j;
    lds[tid * P + j] = b;
    b += share_len(ln, a.small_max);
    if (is_small(ln, a.small_max)) {  // implies c < n (lengths past n are 0)
      const uint32_t k = small_class(ln);
      const uint64_t p = k == 0 ? pos[0] : k == 1 ? pos[1] : k == 2 ? pos[2] : pos[3];
      a.small_idx[p] = c;
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) pos[q] += q == k ? 1u : 0u;
    }
    if (c == a.n - 1) a.byte_start[a.n] = b;
  }
  // A batch the group phase takes whole (no share bytes at all): the sweep reads byte_start[n]
  // (total 0) and nothing below it, so the per-chunk starts are not stored -- 8 of the 20 B per
  // chunk this kernel moves for small records. (small_max == 0: byte_start is a plain scan that
  // the PUT and transform paths read.)
  const bool store_starts = a.small_max == 0 || (nblocks > 1 ? __syncthreads_or(any_share) != 0 : tot[5] != 0);
  __syncthreads();
  if (store_starts) {
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) {
      const uint32_t i = r * 256 + tid, c = base + i;
      if (c < a.n) a.byte_start[c] = lds[(i / R) * P + i % R];
    }
  }
  if (blockIdx.x == 0 && tid == 0) {
    a.small_total[4] = 0;
    a.small_total[0] = cls_base[3] + cls_total[3];
    a.small_total[1] = cls_base[1];
    a.small_total[2] = cls_base[2];
    a.small_total[3] = cls_base[3];
  }
}

__global__ void crc32_verify_kernel(const uint32_t* __restrict__ crc, const uint32_t* __restrict__ expected,
                                    uint8_t* __restrict__ mismatch, uint32_t* __restrict__ count, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool bad = crc[i] != expected[i];
  if (mismatch) mismatch[i] = bad ? 1 : 0;
  if (bad && count) atomicAdd(count, 1u);
}

// Synthetic bytes: byte i of the stream = byte (i&7) of splitmix64(seed + ((i>>3)+1)*golden).
__device__ __forceinline__ uint64_t splitmix_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ void fill_splitmix_kernel(uint8_t* __restrict__ dst, uint64_t nbytes, uint64_t seed, uint64_t stream_off) {
  // Requires dst 16-B aligned and stream_off % 16 == 0 (checked on the host).
  const uint64_t n16 = nbytes / 16;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
    const uint64_t word = (stream_off >> 3) + 2 * i;
    const uint64_t w0 = splitmix_mix(seed + (word + 1) * 0x9E3779B97F4A7C15ull);
    const uint64_t w1 = splitmix_mix(seed + (word + 2) * 0x9E3779B97F4A7C15ull);
    u32x4 v = {(uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32)};
    reinterpret_cast<u32x4*>(dst)[i] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x < (nbytes & 15)) {
    const uint64_t pos = stream_off + n16 * 16 + threadIdx.x;
    const uint64_t w = splitmix_mix(seed + ((pos >> 3) + 1) * 0x9E3779B97F4A7C15ull);
    dst[n16 * 16 + threadIdx.x] = (uint8_t)(w >> (8 * (pos & 7)));
  }
}

// ---------------------------------------------------------------- launchers
hipError_t launch_plan(const PlanArgs& a, hipStream_t s) {
  const uint32_t blocks = blocks_for(a.n, 0, 0, kPlanPerBlock);
  // one planning block needs no per-block sums (its carry is 0)
  if (blocks > 1) hipLaunchKernelGGL(crc32_plan_count_kernel, dim3(blocks), dim3(256), 0, s, a);
  return launch_items(crc32_plan_scan_kernel, blocks, 256, s, a);
}

hipError_t launch_sweep_copy(const SweepArgs& a, int grid, int num_cu, int variant, hipStream_t s) {
#ifdef AMBRY_AB_SPLIT_GROUP
  if (variant == kVariantSplit) {
    if (a.small_max) {
      const hipError_t e = launch_group(a, num_cu, s);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((crc32_sweep_kernel<true, false, 0, true>), dim3(grid), dim3(1024), 0, s, a);
    return hipGetLastError();
  }
#endif
  (void)variant;
  (void)num_cu;
  hipLaunchKernelGGL((crc32_sweep_kernel<true, true, 0, true>), dim3(grid), dim3(1024), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sweep(const SweepArgs& a, int grid, int num_cu, int variant, hipStream_t s) {
  (void)num_cu;
  switch (variant) {
    // 0: 16-B pieces, every chunk in the sweep (no group phase): the fallback shape
    case kVariantPieces: hipLaunchKernelGGL((crc32_sweep_kernel<false, false>), dim3(grid), dim3(1024), 0, s, a); break;
    // 29 (default): 64-B lane runs + the class-sized group phase for whole chunks <= 16 KiB
    case kVariantDefault: hipLaunchKernelGGL((crc32_sweep_kernel<true, true>), dim3(grid), dim3(1024), 0, s, a); break;
    // 32: the group kernel (two workgroups per CU), then the sweep without its group phase
#ifdef AMBRY_AB_SPLIT_GROUP
    case kVariantSplit:
      if (a.small_max) {
        const hipError_t e = launch_group(a, num_cu, s);
        if (e != hipSuccess) return e;
      }
      hipLaunchKernelGGL((crc32_sweep_kernel<true, false>), dim3(grid), dim3(1024), 0, s, a);
      break;
#endif
#ifdef AMBRYCRC_DIAGNOSTICS
    // timing-only diagnostics (wrong CRCs; debug builds only): 100 FOLD lookups removed, 101 no
    // per-segment atomic, 102 no wave tree
    case kDiagNoFold: hipLaunchKernelGGL((crc32_sweep_kernel<false, false, 1>), dim3(grid), dim3(1024), 0, s, a); break;
    case kDiagNoFold + 1: hipLaunchKernelGGL((crc32_sweep_kernel<false, false, 2>), dim3(grid), dim3(1024), 0, s, a); break;
    case kDiagNoFold + 2: hipLaunchKernelGGL((crc32_sweep_kernel<false, false, 3>), dim3(grid), dim3(1024), 0, s, a); break;
#endif
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_verify(const uint32_t* crc, const uint32_t* expected, uint8_t* mismatch, uint32_t* count,
                         uint32_t n, hipStream_t s) {
  return launch_items(crc32_verify_kernel, blocks_for(n), 256, s, crc, expected, mismatch, count, n);
}

hipError_t launch_fill(uint8_t* dst, uint64_t nbytes, uint64_t seed, uint64_t stream_off, hipStream_t s) {
  if (nbytes == 0) return hipSuccess;
  uint64_t n16 = nbytes / 16;
  uint64_t blocks = (n16 + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  if (blocks == 0) blocks = 1;
  hipLaunchKernelGGL(fill_splitmix_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, dst, nbytes, seed, stream_off);
  return hipGetLastError();
}

}  // namespace ambrycrc
