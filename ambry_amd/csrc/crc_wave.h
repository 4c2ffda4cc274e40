// crc_wave.h -- the CRC wave primitives every kernel file builds its hashing from, once each: the
// two LDS table images and their LDS-DMA staging, the slice-by-4 step and the nibble-table
// multiply over them, the DPP partner moves and the wave tree level, the 16-B load and store
// helpers, and the 64-B lane run of the 4 KiB super-block kernels (quad transpose + run_crc).
// Users: the batch engine (crc32_kernels.hip), region mode (region_kernels.hip), the PUT streamer
// (put_kernels.hip), the bandwidth probes (bw_probe_kernels.hip) and tools/probes. What only the
// sweep uses (the block bodies, fold<DIAG>, the group phase) stays beside the sweep.
// Included by .hip files only. The LDS arrays have internal linkage, so each kernel file gets its
// own pair and a kernel allocates only the one it references.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crc32_gf2.h"
#include "crc32_layout.h"

namespace ambrycrc {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// The full table image (crc32_layout.h): the batch engine's kernels.
static __shared__ __attribute__((aligned(16))) uint32_t g_lds[kLdsBytes / 4];

// Stage the table image into LDS with LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave
// instruction, no VGPR round trip), all of a wave's ~10 loads in flight together, then one
// wait and a barrier. A load -> ds_write loop serialises on vmcnt(0) per iteration: ~10
// memory round trips, which was most of a single-chunk call's sweep-kernel time.
__device__ __forceinline__ void fill_lds(const uint32_t* __restrict__ img) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  constexpr uint32_t kChunks = (kLdsBytes + 1023) / 1024;
  for (uint32_t c = wave; c < kChunks; c += nw) {
    const uint32_t byte = c * 1024 + lane * 16;
    if (byte < kLdsBytes)
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(reinterpret_cast<const uint8_t*>(img) + byte),
          (__attribute__((address_space(3))) void*)(reinterpret_cast<uint8_t*>(g_lds) + c * 1024), 16, 0, 0);
  }
  __builtin_amdgcn_s_waitcnt(0);  // vmcnt(0) expcnt(0) lgkmcnt(0): the DMA writes have landed
  __syncthreads();
}

// The run-sum kernels (region_runs_kernel, region_fused_kernel, put_stream_kernel) stage only the
// slice tables, plus a 1 KiB buffer per wave for their run sums: their own LDS array, so those
// kernels are not sized by the full image.
constexpr uint32_t kRunsBufBytes = 1024;
static __shared__ __attribute__((aligned(16))) uint32_t g_lds_runs[(kSliceBytes + 16 * kRunsBufBytes) / 4];

// LDS-DMA of the slice tables (image bytes [0, 128 KiB)) into g_lds_runs, as fill_lds. The issue
// half alone is for a kernel that stages more before its one wait (region_fused_kernel).
__device__ __forceinline__ void issue_lds_slices(const uint32_t* __restrict__ img) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (uint32_t c = wv; c < kSliceBytes / 1024; c += nw)
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(reinterpret_cast<const uint8_t*>(img) + c * 1024 + lane * 16),
        (__attribute__((address_space(3))) void*)(reinterpret_cast<uint8_t*>(g_lds_runs) + c * 1024), 16, 0, 0);
}

__device__ __forceinline__ void fill_lds_slices(const uint32_t* __restrict__ img) {
  issue_lds_slices(img);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
}

// W = 0: the full image (g_lds); W = 1: the slice tables of region_runs_kernel (g_lds_runs).
template <int W = 0>
__device__ __forceinline__ uint32_t lds_rd(uint32_t byte_addr) {
  const char* base = W == 0 ? reinterpret_cast<const char*>(g_lds) : reinterpret_cast<const char*>(g_lds_runs);
  return *reinterpret_cast<const uint32_t*>(base + byte_addr);
}

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// Cross-lane moves without LDS: DPP row shifts / broadcasts (lanes with no source read 0).
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xf, false);
}

// Value of lane (l - 2^lvl) delivered to every lane l with bit lvl set (the tree's left partner):
// row_shr:1/2/4/8 inside 16-lane rows, then row_bcast:15 (rows 1,3) and row_bcast:31 (rows 2,3).
template <int LVL>
__device__ __forceinline__ uint32_t tree_partner(uint32_t v) {
  if constexpr (LVL < 4) return dpp<0x110 + (1 << LVL), 0xf>(v);
  else if constexpr (LVL == 4) return dpp<0x142, 0xa>(v);
  else return dpp<0x143, 0xc>(v);
}

// Per-lane address constants for slice table j: region bit, (j&1)*128, lane column.
struct LaneConst {
  uint32_t L0, L1, L2, L3;
};

__device__ __forceinline__ LaneConst make_lane_const(uint32_t lane) {
  const uint32_t col = (lane & 31u) << 2;
  LaneConst k;
  k.L0 = (0u << 16) | (0u << 7) | col;
  k.L1 = (0u << 16) | (1u << 7) | col;
  k.L2 = (1u << 16) | (0u << 7) | col;
  k.L3 = (1u << 16) | (1u << 7) | col;
  return k;
}

// One slice-by-4 step on x = state ^ word: T3[x.b0]^T2[x.b1]^T1[x.b2]^T0[x.b3] ^ xin.
// perm(L, x, sel): result byte0 = L.b0 (lane column), byte1 = x.b_k, byte2 = L.b2 (region), byte3 = 0.
template <int W = 0>
__device__ __forceinline__ uint32_t slice4(uint32_t x, const LaneConst& k, uint32_t xin) {
  const uint32_t a0 = __builtin_amdgcn_perm(k.L3, x, 0x0C060004u);
  const uint32_t a1 = __builtin_amdgcn_perm(k.L2, x, 0x0C060104u);
  const uint32_t a2 = __builtin_amdgcn_perm(k.L1, x, 0x0C060204u);
  const uint32_t a3 = __builtin_amdgcn_perm(k.L0, x, 0x0C060304u);
  const uint32_t t = xor3(lds_rd<W>(a0), lds_rd<W>(a1), lds_rd<W>(a2));
  return xor3(t, lds_rd<W>(a3), xin);
}

// Raw CRC (zero register, no xor-out) of one 16-B piece, xor xin.
__device__ __forceinline__ uint32_t rpiece(u32x4 w, const LaneConst& k, uint32_t xin) {
  uint32_t s = slice4(w.x, k, w.y);
  s = slice4(s, k, w.z);
  s = slice4(s, k, w.w);
  return slice4(s, k, xin);
}

// v * C mod P where C's nibble tables sit at kNibBase + set_off (conflict-free, 8 lookups).
__device__ __forceinline__ uint32_t nib_mul(uint32_t v, uint32_t set_off) {
  uint32_t t[8];
#pragma unroll
  for (int n = 0; n < 8; ++n)
    t[n] = lds_rd(kNibBase + set_off + 64u * n + (__builtin_amdgcn_ubfe(v, 4 * n, 4) << 2));
  return xor3(xor3(t[0], t[1], t[2]), xor3(t[3], t[4], t[5]), t[6] ^ t[7]);
}

// v * x^(8n) mod P for a wave-uniform n (register advanced over n zero bytes).
__device__ __forceinline__ uint32_t shift_bytes(uint32_t v, uint64_t n, const uint32_t* __restrict__ xpow2) {
  while (n) {
    const uint32_t k = (uint32_t)__builtin_ctzll(n);
    n &= n - 1;
    v = (k < kPowTables) ? nib_mul(v, kPowOff + kNibSetBytes * k) : gf2_mul(v, xpow2[k]);
  }
  return v;
}

template <bool NT>
__device__ __forceinline__ u32x4 ld16(const u32x4* p) {
  if constexpr (NT) {
    return __builtin_nontemporal_load(p);
  } else {
    return *p;
  }
}

// ---- copy-through (SweepArgs::copy_dst): every byte read for a chunk is also stored to the
// chunk's destination, dbase + (its source offset), so a serialization moves each field once.
// 16-B stores at any destination alignment (gfx9 global memory runs in unaligned mode; the
// memcpy becomes one global_store_dwordx4); a piece that starts before the chunk stores only
// its bytes from `lo` on.
// The destination pointers are built from integers (SweepArgs::copy_off), which leaves them in
// the generic address space: a store through one is a flat_store, which counts on lgkmcnt as well
// as vmcnt, so every LDS wait of the CRC chain would also wait for the outstanding stores. The
// casts keep them global_store.
typedef __attribute__((address_space(1))) u32x4 gu32x4;
typedef __attribute__((address_space(1))) uint8_t gu8;
__device__ __forceinline__ void st8g(uint8_t* d, uint32_t v) { *(gu8*)d = (uint8_t)v; }
__device__ __forceinline__ void st16u(uint8_t* d, const u32x4& v) { *(gu32x4*)d = v; }
// Wave-mode bodies (large chunks) stream their stores nontemporal: 3-5 % faster there, 18 %
// slower in the group phase's short records (r02x A/B), which keep the plain store.
__device__ __forceinline__ void st16u_nt(uint8_t* d, const u32x4& v) { __builtin_nontemporal_store(v, (gu32x4*)d); }

__device__ __forceinline__ void copy_piece(uint8_t* dbase, int64_t p, const u32x4& v, int64_t lo) {
  if (!dbase || p + 16 <= lo) return;  // null: a chunk read but not copied (kCopySkip)
  if (p >= lo) {
    st16u(dbase + p, v);
    return;
  }
#pragma unroll
  for (int b = 0; b < 16; ++b)
    if (p + b >= lo) st8g(dbase + p + b, v[b >> 2] >> (8 * (b & 3)));
}

template <int LVL>
__device__ __forceinline__ uint32_t tree_level(uint32_t s, uint32_t lane) {
  const uint32_t sh = nib_mul(tree_partner<LVL>(s), kTreeOff + kNibSetBytes * LVL);
  return (lane & (1u << LVL)) ? (s ^ sh) : s;
}

// Raw CRC (zero register) of the t < 16 bytes at p, lane-parallel: lane j holds byte j, whose
// contribution is T0[b] advanced over the t-1-j bytes after it = T_{k&3}[b] * x^(32*(k>>2)),
// k = t-1-j; then an XOR over the 16 lanes of row 0. Result valid in every lane of row 0.
__device__ __forceinline__ uint32_t tail_crc(const uint8_t* __restrict__ p, uint32_t t, uint32_t lane) {
  uint32_t v = 0;
  if (lane < t) {
    const uint32_t b = p[lane];
    const uint32_t k = t - 1 - lane;
    const uint32_t j = k & 3;
    v = lds_rd(((j >> 1) << 16) | (b << 8) | ((j & 1) << 7) | ((lane & 31) << 2));
    if (k & 4) v = nib_mul(v, kPowOff + kNibSetBytes * 2);  // x^(8*4)
    if (k & 8) v = nib_mul(v, kPowOff + kNibSetBytes * 3);  // x^(8*8)
  }
  v ^= dpp<0x128, 0xf>(v);  // row_ror:8
  v ^= dpp<0x124, 0xf>(v);  // row_ror:4
  v ^= dpp<0x122, 0xf>(v);  // row_ror:2
  v ^= dpp<0x121, 0xf>(v);  // row_ror:1
  return v;
}

// Raw CRC of a lane's run of R consecutive 16-B pieces (R slice-by-4 chains of 4 steps, back
// to back), xor xin into the last step.
template <int R, int W = 0>
__device__ __forceinline__ uint32_t run_crc(const u32x4 (&w)[R], const LaneConst& k, uint32_t xin) {
  uint32_t x = w[0].x;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    x = slice4<W>(x, k, w[r].y);
    x = slice4<W>(x, k, w[r].z);
    x = slice4<W>(x, k, w[r].w);
    x = slice4<W>(x, k, r + 1 < R ? w[r + 1].x : xin);
  }
  return x;
}

template <int CTRL>
__device__ __forceinline__ uint32_t dppq(uint32_t v) {  // quad_perm: every lane has a source
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, true);
}

// A 4x4 transpose of 16-B elements inside each lane quad, with the lane selects fused into the DPP moves: v_cndmask_b32_dpp
// computes vcc ? src1 : dpp(src0), so each stage is 4 VALU ops per dword instead of 4 DPP
// moves + 4 v_cndmask_b32_e64 (the compiler cannot fuse them: its selects take the lane
// mask from an SGPR pair, the VOP3 form, which has no DPP encoding on gfx9). 8 VALU per
// dword per transpose instead of 16. s_nop 1 on entry and exit covers the gfx9 hazard of
// a DPP read within 2 wait states of the VALU write of its source.
__device__ __forceinline__ void quad_transpose_asm(u32x4 (&x)[4]) {
  const uint64_t m1 = 0xAAAAAAAAAAAAAAAAull, n1 = 0x5555555555555555ull;  // lane & 1 set / clear
  const uint64_t m2 = 0xCCCCCCCCCCCCCCCCull, n2 = 0x3333333333333333ull;  // lane & 2 set / clear
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    uint32_t a0, a1, a2, a3, y0, y1, y2, y3;
    asm volatile(
        "s_nop 1\n\t"
        "s_mov_b64 vcc, %[n1]\n\t"
        "v_cndmask_b32_dpp %[a0], %[x1], %[x0], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32_dpp %[a2], %[x3], %[x2], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_mov_b64 vcc, %[m1]\n\t"
        "v_cndmask_b32_dpp %[a1], %[x0], %[x1], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32_dpp %[a3], %[x2], %[x3], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_mov_b64 vcc, %[n2]\n\t"
        "v_cndmask_b32_dpp %[y0], %[a2], %[a0], vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32_dpp %[y1], %[a3], %[a1], vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "s_mov_b64 vcc, %[m2]\n\t"
        "v_cndmask_b32_dpp %[y2], %[a0], %[a2], vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32_dpp %[y3], %[a1], %[a3], vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1"
        : [a0] "=&v"(a0), [a1] "=&v"(a1), [a2] "=&v"(a2), [a3] "=&v"(a3), [y0] "=&v"(y0), [y1] "=&v"(y1),
          [y2] "=&v"(y2), [y3] "=&v"(y3)
        : [x0] "v"(x[0][d]), [x1] "v"(x[1][d]), [x2] "v"(x[2][d]), [x3] "v"(x[3][d]), [m1] "s"(m1), [n1] "s"(n1),
          [m2] "s"(m2), [n2] "s"(n2)
        : "vcc");
    x[0][d] = y0;
    x[1][d] = y1;
    x[2][d] = y2;
    x[3][d] = y3;
  }
}

}  // namespace ambrycrc
