// seg_verify.hip -- probe: the single-read region verify. Can the record CRCs of
// a region of small PUT messages be had from ONE stream of the region -- run sums hashed in registers
// as region_runs_kernel hashes them, each record's pieces combined inside the wave by a segmented
// scan over its runs -- instead of pass 1's run-sum stores and pass 2's re-reads (DESIGN.md §11.4,
// §11.7)? Three kernels:
//   parse    a thread per message reads its V3 header (PutMessageFormatInputStream.java:76-124 layout;
//            MessageFormatRecord.java:951-981) and writes its 8 record boundaries (the header, blob
//            properties, user metadata and blob records' starts and last bytes): one line a message.
//   stream   a wave per contiguous range of 4 KiB super-blocks, the next one in flight: the quad
//            transpose and run_crc<4,1> as pass 1 (a lane per 64-B run); the chunk of boundaries
//            inside the super-block from the parse's list; per run, masked hashes at its boundaries
//            (region::hash_run_m, the bytes below the boundary); records inside one run finished at
//            once; for the others each run's contribution to the record open at its end, a
//            segmented scan over the 64 runs in run order (x^(8*64*2^k) per level, ds_bpermute
//            partners, head flags from one ballot), the carry to the next super-block; a record
//            ending in a run takes the scan value of the run before it; un-shift to the record end
//            (region_crc.h's sets), complement: the CRC.
//   fix      a thread per wave: the one record open across the start of its range, from the
//            previous wave's carry (x^(8*64*n) by the image's power sets).
// Messages: key 24 B, properties payload 75 B, user metadata 1,000 B, blob 100 B / 1 KiB / 4 KiB
// (S = 1284 / 2208 / 5280 B, as tools/probes/direct_lane.hip and tools/bench_messages.py's
// regions), random bytes, trailers from zlib. Every record's CRC is checked against zlib; the JSON
// line per size gives each kernel's median time over 7 passes and the mismatch count.
// Scope of the probe: V3 headers, no encryption key, records of >= 4 B, at most 3 boundaries in a
// 64-B run (these layouts have no more), no record longer than a
// wave's range; the stored trailers are not compared in the kernel (the CRCs go to an array).
// Build (from the repo root, after `make -C ambry_amd`):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -o tools/probes/seg_verify tools/probes/seg_verify.hip -ldl -lz
// Run: tools/probes/seg_verify [ambry_amd/libambrycrc.so]
#include <dlfcn.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <vector>

#include "../../ambry_amd/csrc/crc32_kernels.h"
#include "../../ambry_amd/csrc/crc32_layout.h"
#include "../../ambry_amd/csrc/crc_wave.h"
#include "../../ambry_amd/csrc/region_crc.h"

#define CK(e)                                                          \
  do {                                                                 \
    hipError_t r_ = (e);                                               \
    if (r_ != hipSuccess) {                                            \
      printf("HIP error %s at %d\n", hipGetErrorString(r_), __LINE__); \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

namespace seg {
using namespace ambrycrc;
constexpr int kMaxEv = 3;  // boundaries a run may hold (more: counted in stats[1], CRCs wrong)

struct Args {
  const uint8_t* base;   // the region (padded by 8 KiB of zeros)
  uint64_t nsb;          // 4 KiB super-blocks over the region
  const uint32_t* ev;    // 8 boundary keys a message: record starts, and last bytes (end - 1)
  uint64_t nev;
  const uint32_t* img;   // the library's table image
  uint32_t* out;         // a CRC a record
  uint32_t* fix;         // per wave: record, V, runs, d (4 words; record ~0: none)
  uint32_t* cout;        // per wave: the scan value at the range's end
  uint32_t* stats;       // [0]: super-blocks with 64 boundaries or more (overflow), [1]: runs with > kMaxEv
};

constexpr uint32_t kPowFirst = 4;  // s_nib holds the image's x^(8*2^k) sets, k = 4..11
__shared__ uint32_t s_nib[8 * region::kNibWords];
__shared__ uint32_t s_un[kRegUnWords];
__shared__ uint32_t s_hm[kRegAuxWords];

__device__ __forceinline__ uint32_t be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

__global__ __launch_bounds__(256) void parse_kernel(const uint8_t* base, uint64_t m, uint64_t S, uint32_t* ev) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint64_t m0 = i * S;
  const uint8_t* h = base + m0;
  const uint32_t bp = be32(h + 16), um = be32(h + 24), bl = be32(h + 28);
  const uint64_t total = ((uint64_t)be32(h + 4) << 32) | be32(h + 8);
  const uint32_t end = (uint32_t)(m0 + bp + total);
  const uint32_t a = (uint32_t)m0;
  u32x4* o = reinterpret_cast<u32x4*>(ev + 8 * i);
  o[0] = u32x4{a, a + 31, a + bp, a + um - 9};
  o[1] = u32x4{a + um, a + bl - 9, a + bl, end - 9};
}

__device__ __forceinline__ uint32_t unshift(uint32_t v, uint32_t d) {
  return region::nmul(s_un, region::nmul(s_un, v, d & 7u), 8u + (d >> 3));
}

// First index in k[0, n) whose key is >= x (k sorted).
__device__ __forceinline__ uint32_t lower_bound_lds(const uint32_t* k, uint32_t n, uint32_t x) {
  uint32_t lo = 0, len = n;
  while (len) {
    const uint32_t half = len >> 1;
    if (k[lo + half] < x) {
      lo += half + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  return lo;
}

__device__ __forceinline__ u32x4 sb_load(const Args& a, uint64_t s, uint32_t lane, int i) {
  return __builtin_nontemporal_load(
      reinterpret_cast<const u32x4*>(a.base + s * kSuperBlock + (uint64_t)kBlockBytes * i + 16u * lane));
}

__global__ __launch_bounds__(1024) void stream_kernel(Args a) {
  {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (uint32_t c = wv; c < kSliceBytes / 1024; c += nw)
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(reinterpret_cast<const uint8_t*>(a.img) + c * 1024 + lane * 16),
          (__attribute__((address_space(3))) void*)(reinterpret_cast<uint8_t*>(g_lds_runs) + c * 1024), 16, 0, 0);
    for (uint32_t i = threadIdx.x; i < 8 * region::kNibWords; i += blockDim.x)
      s_nib[i] = a.img[(kNibBase + kPowOff + kNibSetBytes * kPowFirst) / 4 + i];
    const uint32_t* reg = a.img + kImgRegOff / 4;
    for (uint32_t i = threadIdx.x; i < kRegUnWords; i += blockDim.x) s_un[i] = reg[kRegAuxWords + kRegByteWords + i];
    for (uint32_t i = threadIdx.x; i < kRegAuxWords; i += blockDim.x) s_hm[i] = reg[i];
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }
  const uint32_t lane = threadIdx.x & 63u;
  const LaneConst k = make_lane_const(lane);
  const region::TabR tab{reinterpret_cast<const uint8_t*>(g_lds_runs), (lane & 31u) << 2};
  uint32_t* wb = g_lds_runs + kSliceBytes / 4 + (threadIdx.x >> 6) * (kRunsBufBytes / 4);
  uint32_t* evk = wb;        // the chunk's keys
  uint32_t* cb = wb + 64;    // contributions in run order
  uint32_t* hb = wb + 128;   // head flags in run order
  const uint32_t r = 16u * (lane & 3u) + (lane >> 2);  // the run this lane holds after the transpose
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint32_t wave = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) * gridDim.x + blockIdx.x);
  const uint64_t first = a.nsb * wave / nwaves, end = a.nsb * (wave + 1) / nwaves;
  if (first >= end) return;
  // the first boundary at or after the range start (wave-uniform binary search)
  uint64_t cursor;
  {
    const uint32_t x = (uint32_t)(first * kSuperBlock);
    uint64_t lo = 0, len = a.nev;
    while (len) {
      const uint64_t half = len >> 1;
      if (a.ev[lo + half] < x) {
        lo += half + 1;
        len -= half + 1;
      } else {
        len = half;
      }
    }
    cursor = lo;
  }
  uint32_t carry = 0;
  bool fresh = true;
  uint32_t key = cursor + lane < a.nev ? a.ev[cursor + lane] : 0xFFFFFFFFu;  // no record has started since the range start
  u32x4 x[4], xn[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) x[i] = sb_load(a, first, lane, i);
  for (uint64_t s = first; s < end; ++s) {
    if (s + 1 < end) {
#pragma unroll
      for (int i = 0; i < 4; ++i) xn[i] = sb_load(a, s + 1, lane, i);
    }
    const uint32_t S = (uint32_t)(s * kSuperBlock);
    const uint64_t inb = __ballot(key < S + (uint32_t)kSuperBlock);
    const uint32_t nch = (uint32_t)__builtin_popcountll(inb);
    if (nch == 64 && lane == 0) atomicAdd(&a.stats[0], 1u);
    evk[lane] = key;
    {  // the next chunk's keys, in flight while this super-block is hashed
      const uint64_t gn = cursor + nch + lane;
      key = gn < a.nev ? a.ev[gn] : 0xFFFFFFFFu;
    }
    quad_transpose_asm(x);
    const uint32_t R = run_crc<4, 1>(x, k, 0u);
    const uint32_t rs = S + 64u * r;
    const uint32_t lo_r = lower_bound_lds(evk, nch, rs), hi_r = lower_bound_lds(evk, nch, rs + 64u);
    const uint32_t cnt = hi_r - lo_r;
    if (cnt > (uint32_t)kMaxEv) atomicAdd(&a.stats[1], 1u);
    const uint64_t g0 = cursor + lo_r;  // global index of the run's first boundary
    // boundary offsets in the run (starts: first byte; ends: one past the last byte) and the masked
    // hashes of the bytes below each
    uint32_t off[kMaxEv], P[kMaxEv];
#pragma unroll
    for (int j = 0; j < kMaxEv; ++j) {
      off[j] = 0;
      P[j] = 0;
      if (__ballot(cnt > (uint32_t)j) == 0) continue;
      if (cnt > (uint32_t)j) {
        off[j] = evk[lo_r + j] - rs + (uint32_t)((g0 + j) & 1u);
        P[j] = region::hash_run_m<true>(tab, s_nib, s_hm, x, 0, (int)off[j]);
      }
    }
    const bool open_start = (g0 & 1u) != 0, open_end = ((cursor + hi_r) & 1u) != 0;
    // records inside this run: a start at j followed by its end at j + 1
#pragma unroll
    for (int j = 0; j + 1 < kMaxEv; ++j) {
      if ((uint32_t)j + 1 < cnt && ((g0 + j) & 1u) == 0) {
        const uint32_t V = P[j + 1] ^ P[j] ^ s_hm[kRegH0 + off[j]];
        a.out[(g0 + j) >> 1] = ~unshift(V, 64u - off[j + 1]);
      }
    }
    // the contribution to the record open at the run's end, and whether it starts here
    uint32_t c = 0, h = 1;
    if (open_end) {
      if (cnt > 0) {
        uint32_t ps = P[0], so = off[0];
#pragma unroll
        for (int j = 1; j < kMaxEv; ++j)
          if ((uint32_t)j == cnt - 1) ps = P[j], so = off[j];
        const uint32_t tin = 64u - so;
        c = R ^ ps ^ s_hm[kRegH0 + so] ^ (tin < 4 ? 0xFFFFFFFFu >> (8 * tin) : 0u);
      } else {
        c = R;
        h = 0;
      }
    }
    cb[r] = c;
    hb[r] = h;
    __builtin_amdgcn_wave_barrier();
    uint32_t A = cb[lane];
    const uint64_t H = __ballot(hb[lane] != 0);  // bit i: run i starts a segment
    if (lane == 0 && !(H & 1u)) A ^= region::nmul(s_nib, carry, 2);  // x^(8*64)
#pragma unroll
    for (int lv = 0; lv < 6; ++lv) {
      const uint32_t d = 1u << lv;
      const uint32_t p = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(4 * (lane >= d ? lane - d : 0)), (int)A);
      const uint64_t win = lane >= d ? (H >> (lane + 1 - d)) & ((1ull << d) - 1) : 1;  // heads in (lane - d, lane]
      const uint32_t add = region::nmul(s_nib, p, 2 + lv);
      if (lane >= d && win == 0) A ^= add;
    }
    // the record that ends here but started before: the scan value of the run before, shifted by one
    const uint32_t Aprev = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(4 * (r > 0 ? r - 1 : 0)), (int)A);
    const uint32_t prev = r > 0 ? Aprev : carry;
    if (open_start && cnt > 0) {
      const uint32_t V = region::nmul(s_nib, prev, 2) ^ P[0];
      const uint32_t d = 64u - off[0];
      const uint64_t rec = g0 >> 1;
      const uint64_t below = r > 0 ? (H & ((1ull << r) - 1)) : 0;  // run-order heads before run r
      if (fresh && below == 0) {  // open since before the range: the fix kernel completes it
        const uint32_t n = (uint32_t)((s - first) * 64 + r + 1);
        *reinterpret_cast<u32x4*>(a.fix + 4 * wave) = u32x4{(uint32_t)rec, V, n, d};
      } else {
        a.out[rec] = ~unshift(V, d);
      }
    }
    carry = (uint32_t)__builtin_amdgcn_readlane((int)A, 63);
    if (H) fresh = false;
    cursor += nch;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = xn[i];
  }
  if (lane == 0) a.cout[wave] = carry;
}

__global__ void fix_kernel(Args a, uint32_t nwaves) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w == 0 || w >= nwaves) return;
  const uint32_t* f = a.fix + 4 * w;
  if (f[0] == 0xFFFFFFFFu) return;
  const uint32_t* pw = a.img + (kNibBase + kPowOff) / 4;  // x^(8*2^k) sets
  const uint32_t* un = a.img + kImgRegOff / 4 + kRegAuxWords + kRegByteWords;
  uint32_t c = a.cout[w - 1], n = f[2];
  for (uint32_t b = 0; n; ++b, n >>= 1)
    if (n & 1u) c = region::nmul(pw, c, 6 + b);  // x^(8*64*2^b)
  uint32_t V = f[1] ^ c;
  V = region::nmul(un, region::nmul(un, V, f[3] & 7u), 8u + (f[3] >> 3));
  a.out[f[0]] = ~V;
}


// ---- variant "cap": no masked re-hash. The run's chain (16 slice-by-4 steps, one word each) keeps
// the register at each boundary's word (T(o): the raw register of the run's bytes [0, o) at o, the
// boundary's 0-3 bytes of that word added by byte steps); every piece is then a register at its own
// position, moved by x^(8j) (j <= 64: up to 3 zero-byte steps and one of 16 nibble sets x^(32q),
// built at kernel start): a record inside a run is T(e) ^ (T(s) ^ ~0) x^(8(e-s)); the piece that
// opens a record carries R ^ (T(s) ^ ~0) x^(8(64-s)) to the run end; a record ending at e after
// earlier runs is A x^(8e) ^ T(e) -- no un-shift, and the initial register is the ~0 itself.
__shared__ uint32_t s_q[16 * region::kNibWords];  // x^(32q), q = 1..16

template <class Tab>
__device__ __forceinline__ uint32_t zbytes(const Tab& t, uint32_t v, uint32_t n) {  // n <= 3 zero bytes
#pragma unroll
  for (uint32_t i = 0; i < 3; ++i)
    if (i < n) v = t.t0(v & 0xffu) ^ (v >> 8);
  return v;
}

template <class Tab>
__device__ __forceinline__ uint32_t mulx8(const Tab& t, uint32_t v, uint32_t j) {  // v x^(8j), j <= 64
  v = zbytes(t, v, j & 3u);
  const uint32_t q = j >> 2;
  return q ? region::nmul(s_q, v, q - 1) : v;
}

__global__ __launch_bounds__(1024) void stream_cap_kernel(Args a) {
  {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (uint32_t c = wv; c < kSliceBytes / 1024; c += nw)
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(reinterpret_cast<const uint8_t*>(a.img) + c * 1024 + lane * 16),
          (__attribute__((address_space(3))) void*)(reinterpret_cast<uint8_t*>(g_lds_runs) + c * 1024), 16, 0, 0);
    for (uint32_t i = threadIdx.x; i < 8 * region::kNibWords; i += blockDim.x)
      s_nib[i] = a.img[(kNibBase + kPowOff + kNibSetBytes * kPowFirst) / 4 + i];
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    // s_q: entry (n, u) of set q-1 = (u << 4n) moved over 4q zero bytes by the T0 table
    const region::TabR t{reinterpret_cast<const uint8_t*>(g_lds_runs), (lane & 31u) << 2};
    for (uint32_t i = threadIdx.x; i < 16 * region::kNibWords; i += blockDim.x) {
      const uint32_t q = i / region::kNibWords + 1, e = i % region::kNibWords;
      uint32_t v = (e & 15u) << (4 * (e >> 4));
      for (uint32_t z = 0; z < 4 * q; ++z) v = t.t0(v & 0xffu) ^ (v >> 8);
      s_q[i] = v;
    }
    __syncthreads();
  }
  const uint32_t lane = threadIdx.x & 63u;
  const LaneConst k = make_lane_const(lane);
  const region::TabR tab{reinterpret_cast<const uint8_t*>(g_lds_runs), (lane & 31u) << 2};
  uint32_t* wb = g_lds_runs + kSliceBytes / 4 + (threadIdx.x >> 6) * (kRunsBufBytes / 4);
  uint32_t* evk = wb;
  uint32_t* cb = wb + 64;
  uint32_t* hb = wb + 128;
  const uint32_t r = 16u * (lane & 3u) + (lane >> 2);
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint32_t wave = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) * gridDim.x + blockIdx.x);
  const uint64_t first = a.nsb * wave / nwaves, end = a.nsb * (wave + 1) / nwaves;
  if (first >= end) return;
  uint64_t cursor;
  {
    const uint32_t x = (uint32_t)(first * kSuperBlock);
    uint64_t lo = 0, len = a.nev;
    while (len) {
      const uint64_t half = len >> 1;
      if (a.ev[lo + half] < x) {
        lo += half + 1;
        len -= half + 1;
      } else {
        len = half;
      }
    }
    cursor = lo;
  }
  uint32_t carry = 0;
  bool fresh = true;
  uint32_t key = cursor + lane < a.nev ? a.ev[cursor + lane] : 0xFFFFFFFFu;
  u32x4 x[4], xn[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) x[i] = sb_load(a, first, lane, i);
  for (uint64_t s = first; s < end; ++s) {
    if (s + 1 < end) {
#pragma unroll
      for (int i = 0; i < 4; ++i) xn[i] = sb_load(a, s + 1, lane, i);
    }
    const uint32_t S = (uint32_t)(s * kSuperBlock);
    const uint64_t inb = __ballot(key < S + (uint32_t)kSuperBlock);
    const uint32_t nch = (uint32_t)__builtin_popcountll(inb);
    if (nch == 64 && lane == 0) atomicAdd(&a.stats[0], 1u);
    evk[lane] = key;
    {
      const uint64_t gn = cursor + nch + lane;
      key = gn < a.nev ? a.ev[gn] : 0xFFFFFFFFu;
    }
    quad_transpose_asm(x);
    const uint32_t rs = S + 64u * r;
    const uint32_t lo_r = lower_bound_lds(evk, nch, rs), hi_r = lower_bound_lds(evk, nch, rs + 64u);
    const uint32_t cnt = hi_r - lo_r;
    if (cnt > (uint32_t)kMaxEv) atomicAdd(&a.stats[1], 1u);
    const uint64_t g0 = cursor + lo_r;
    uint32_t off[kMaxEv], wj[kMaxEv], cap[kMaxEv], cw[kMaxEv];
#pragma unroll
    for (int j = 0; j < kMaxEv; ++j) {
      off[j] = (uint32_t)j < cnt ? evk[lo_r + j] - rs + (uint32_t)((g0 + j) & 1u) : 64u;
      wj[j] = off[j] >> 2;  // 16: the run end (T = R)
      cap[j] = 0;
      cw[j] = 0;
    }
    // the run's chain, keeping the register and the word at each boundary's word
    uint32_t st = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const uint32_t w = x[q][d];
#pragma unroll
        for (int j = 0; j < kMaxEv; ++j) {
          const bool at = wj[j] == (uint32_t)(4 * q + d);
          cap[j] = at ? st : cap[j];
          cw[j] = at ? w : cw[j];
        }
        st = slice4<1>(st ^ w, k, 0u);
      }
    const uint32_t R = st;
    uint32_t T[kMaxEv];
#pragma unroll
    for (int j = 0; j < kMaxEv; ++j) {
      uint32_t t = cap[j];
      const uint32_t b = off[j] & 3u;
#pragma unroll
      for (uint32_t i = 0; i < 3; ++i)
        if (i < b) t = tab.t0((t ^ (cw[j] >> (8 * i))) & 0xffu) ^ (t >> 8);
      T[j] = wj[j] >= 16 ? R : t;
    }
    const bool open_start = (g0 & 1u) != 0, open_end = ((cursor + hi_r) & 1u) != 0;
#pragma unroll
    for (int j = 0; j + 1 < kMaxEv; ++j) {
      if ((uint32_t)j + 1 < cnt && ((g0 + j) & 1u) == 0) {
        const uint32_t V = T[j + 1] ^ mulx8(tab, T[j] ^ 0xFFFFFFFFu, off[j + 1] - off[j]);
        a.out[(g0 + j) >> 1] = ~V;
      }
    }
    uint32_t c = 0, h = 1;
    if (open_end) {
      if (cnt > 0) {
        uint32_t ts = T[0], so = off[0];
#pragma unroll
        for (int j = 1; j < kMaxEv; ++j)
          if ((uint32_t)j == cnt - 1) ts = T[j], so = off[j];
        c = R ^ mulx8(tab, ts ^ 0xFFFFFFFFu, 64u - so);
      } else {
        c = R;
        h = 0;
      }
    }
    cb[r] = c;
    hb[r] = h;
    __builtin_amdgcn_wave_barrier();
    uint32_t A = cb[lane];
    const uint64_t H = __ballot(hb[lane] != 0);
    if (lane == 0 && !(H & 1u)) A ^= region::nmul(s_nib, carry, 2);  // x^(8*64)
#pragma unroll
    for (int lv = 0; lv < 6; ++lv) {
      const uint32_t d = 1u << lv;
      const uint32_t p = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(4 * (lane >= d ? lane - d : 0)), (int)A);
      const uint64_t win = lane >= d ? (H >> (lane + 1 - d)) & ((1ull << d) - 1) : 1;
      const uint32_t add = region::nmul(s_nib, p, 2 + lv);
      if (lane >= d && win == 0) A ^= add;
    }
    const uint32_t Aprev = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(4 * (r > 0 ? r - 1 : 0)), (int)A);
    const uint32_t prev = r > 0 ? Aprev : carry;
    if (open_start && cnt > 0) {
      const uint64_t rec = g0 >> 1;
      const uint64_t below = r > 0 ? (H & ((1ull << r) - 1)) : 0;
      if (fresh && below == 0) {  // the fix kernel adds the previous wave's carry over these bytes
        const uint32_t nb = (uint32_t)((s - first) * kSuperBlock + 64u * r + off[0]);
        *reinterpret_cast<u32x4*>(a.fix + 4 * wave) = u32x4{(uint32_t)rec, mulx8(tab, prev, off[0]) ^ T[0], nb, 0u};
      } else {
        a.out[rec] = ~(mulx8(tab, prev, off[0]) ^ T[0]);
      }
    }
    carry = (uint32_t)__builtin_amdgcn_readlane((int)A, 63);
    if (H) fresh = false;
    cursor += nch;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = xn[i];
  }
  if (lane == 0) a.cout[wave] = carry;
}

__global__ void fix_cap_kernel(Args a, uint32_t nwaves) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w == 0 || w >= nwaves) return;
  const uint32_t* f = a.fix + 4 * w;
  if (f[0] == 0xFFFFFFFFu) return;
  const uint32_t* pw = a.img + (kNibBase + kPowOff) / 4;  // x^(8*2^k) sets
  uint32_t c = a.cout[w - 1], n = f[2];
  for (uint32_t b = 0; n; ++b, n >>= 1)
    if (n & 1u) c = region::nmul(pw, c, b);  // x^(8*2^b)
  a.out[f[0]] = ~(f[1] ^ c);
}

}  // namespace seg

static void put_be(uint8_t* p, uint64_t v, int n) {
  for (int i = 0; i < n; ++i) p[i] = (uint8_t)(v >> (8 * (n - 1 - i)));
}

int main(int argc, char** argv) {
  const char* lib = argc > 1 ? argv[1] : "ambry_amd/libambrycrc.so";
  void* h = dlopen(lib, RTLD_NOW | RTLD_LOCAL);
  if (!h) {
    printf("dlopen %s: %s\n", lib, dlerror());
    return 1;
  }
  auto timg = (long (*)(uint32_t*, size_t))dlsym(h, "ambrycrc_debug_table_image");
  std::vector<uint32_t> img(ambrycrc::kImgBytes / 4);
  if (!timg || timg(img.data(), img.size()) <= 0) {
    printf("no table image\n");
    return 1;
  }
  uint32_t* d_img;
  CK(hipMalloc(&d_img, img.size() * 4));
  CK(hipMemcpy(d_img, img.data(), img.size() * 4, hipMemcpyHostToDevice));
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const int ncu = prop.multiProcessorCount;
  const uint64_t region_target = 1384120320ull;  // the 4 KiB-blob verify region of tools/bench_messages.py
  for (uint32_t blob : {4096u, 1024u, 100u}) {
    const uint32_t key = 24, props = 75, um = 1000;
    const uint32_t hs = 40, bp = hs + key, umr = bp + 2 + props + 8, blr = umr + 6 + um + 8;
    const uint64_t S = blr + 13 + blob + 8;
    const uint64_t m = region_target / S, nbytes = m * S;
    std::vector<uint8_t> host(nbytes + 8192, 0);
    std::vector<uint32_t> want(4 * m);
    uint64_t seed = 0x9E3779B97F4A7C15ull ^ blob;
    auto rnd = [&]() {
      seed ^= seed << 13;
      seed ^= seed >> 7;
      seed ^= seed << 17;
      return seed;
    };
    for (uint64_t i = 0; i < m; ++i) {
      uint8_t* p = host.data() + i * S;
      for (uint64_t b = hs; b + 8 <= S; b += 8) {
        const uint64_t v = rnd();
        memcpy(p + b, &v, 8);
      }
      put_be(p, 3, 2);
      put_be(p + 2, i & 3, 2);
      put_be(p + 4, S - bp, 8);
      put_be(p + 12, 0xFFFFFFFFull, 4);
      put_be(p + 16, bp, 4);
      put_be(p + 20, 0xFFFFFFFFull, 4);
      put_be(p + 24, umr, 4);
      put_be(p + 28, blr, 4);
      put_be(p + bp, 1, 2);
      put_be(p + umr, 1, 2);
      put_be(p + umr + 2, um, 4);
      put_be(p + blr, 3, 2);
      put_be(p + blr + 2, 0, 2);
      p[blr + 4] = 0;
      put_be(p + blr + 5, blob, 8);
      const uint32_t rs[4] = {0, bp, umr, blr}, re[4] = {32, umr - 8, blr - 8, (uint32_t)S - 8};
      for (int k = 0; k < 4; ++k) {
        const uint32_t c = (uint32_t)crc32(0, p + rs[k], re[k] - rs[k]);
        put_be(p + re[k], c, 8);
        want[4 * i + k] = c;
      }
    }
    uint8_t* d_base;
    uint32_t *d_ev, *d_out, *d_fix, *d_cout, *d_stats;
    const uint64_t nsb = (nbytes + ambrycrc::kSuperBlock - 1) / ambrycrc::kSuperBlock;
    const uint32_t grid = (uint32_t)ncu, nwaves = grid * 16;
    CK(hipMalloc(&d_base, host.size()));
    CK(hipMemcpy(d_base, host.data(), host.size(), hipMemcpyHostToDevice));
    CK(hipMalloc(&d_ev, 8 * m * 4));
    CK(hipMalloc(&d_out, 4 * m * 4));
    CK(hipMalloc(&d_fix, 4 * nwaves * 4));
    CK(hipMalloc(&d_cout, nwaves * 4));
    CK(hipMalloc(&d_stats, 64));
    CK(hipMemset(d_stats, 0, 64));
    seg::Args a{d_base, nsb, d_ev, 8 * m, d_img, d_out, d_fix, d_cout, d_stats};
    hipEvent_t e[4];
    for (auto& x : e) CK(hipEventCreate(&x));
    for (int var = 0; var < 2; ++var) {
    CK(hipMemset(d_stats, 0, 64));
    std::vector<float> tp, ts, tf;
    uint64_t bad = 0;
    for (int rep = 0; rep < 8; ++rep) {
      CK(hipMemset(d_out, 0, 4 * m * 4));
      CK(hipMemset(d_fix, 0xFF, 4 * nwaves * 4));
      CK(hipEventRecord(e[0], 0));
      hipLaunchKernelGGL(seg::parse_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, 0, d_base, m, S, d_ev);
      CK(hipEventRecord(e[1], 0));
      if (var == 0)
        hipLaunchKernelGGL(seg::stream_kernel, dim3(grid), dim3(1024), 0, 0, a);
      else
        hipLaunchKernelGGL(seg::stream_cap_kernel, dim3(grid), dim3(1024), 0, 0, a);
      CK(hipEventRecord(e[2], 0));
      if (var == 0)
        hipLaunchKernelGGL(seg::fix_kernel, dim3((nwaves + 255) / 256), dim3(256), 0, 0, a, nwaves);
      else
        hipLaunchKernelGGL(seg::fix_cap_kernel, dim3((nwaves + 255) / 256), dim3(256), 0, 0, a, nwaves);
      CK(hipEventRecord(e[3], 0));
      CK(hipGetLastError());
      CK(hipEventSynchronize(e[3]));
      float x0, x1, x2;
      CK(hipEventElapsedTime(&x0, e[0], e[1]));
      CK(hipEventElapsedTime(&x1, e[1], e[2]));
      CK(hipEventElapsedTime(&x2, e[2], e[3]));
      if (rep) tp.push_back(x0), ts.push_back(x1), tf.push_back(x2);
      if (rep == 0) {
        std::vector<uint32_t> got(4 * m);
        CK(hipMemcpy(got.data(), d_out, got.size() * 4, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < got.size(); ++i) bad += got[i] != want[i];
      }
    }
    uint32_t st[2];
    CK(hipMemcpy(st, d_stats, 8, hipMemcpyDeviceToHost));
    auto med = [](std::vector<float> v) {
      std::sort(v.begin(), v.end());
      return v[v.size() / 2];
    };
    const double mp = med(tp), ms = med(ts), mf = med(tf);
    printf("{\"probe\": \"seg_verify\", \"variant\": \"%s\", \"blob\": %u, \"message_bytes\": %lu, \"messages\": %lu, \"region_bytes\": %lu, "
           "\"ms_parse\": %.4f, \"ms_stream\": %.4f, \"ms_fix\": %.4f, \"ms_total\": %.4f, \"GBps_region\": %.1f, "
           "\"records\": %lu, \"mismatches\": %lu, \"overflow_superblocks\": %u, \"runs_over_4\": %u}\n",
           var ? "cap" : "rehash", blob, (unsigned long)S, (unsigned long)m, (unsigned long)nbytes, mp, ms, mf, mp + ms + mf,
           nbytes / ((mp + ms + mf) * 1e6), (unsigned long)(4 * m), (unsigned long)bad, st[0], st[1]);
    fflush(stdout);
    }
    CK(hipFree(d_base));
    CK(hipFree(d_ev));
    CK(hipFree(d_out));
    CK(hipFree(d_fix));
    CK(hipFree(d_cout));
    CK(hipFree(d_stats));
  }
  return 0;
}
