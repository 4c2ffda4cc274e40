// bw_probe_kernels.hip -- the read- and copy-bandwidth probe kernels behind the measurement entry
// of ambrycrc.cpp (launch_readbw): the access shapes of the sweep, the group phase and the message
// processors without their arithmetic, for the roofs the product kernels are compared against.
// No product path launches them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crc32_kernels.h"
#include "crc32_layout.h"
#include "crc_wave.h"

namespace ambrycrc {

// ------------------------------------------------------- read-bandwidth probe
// Same grid, occupancy and per-lane access pattern as crc32_sweep_kernel (256 KiB
// tiles per wave, lane l reading bytes [16l, 16l+16) of each KiB, rolling U=8
// prefetch) with the CRC arithmetic replaced by an XOR: the achievable read roof
// for this access shape. Variant 1 uses nontemporal loads; variant 2 is a plain
// grid-stride dwordx4 stream over 8x more, smaller workgroups.
template <bool NT>
__global__ __launch_bounds__(1024) void readbw_tiles_kernel(const uint8_t* __restrict__ base, uint64_t nbytes,
                                                            uint32_t* __restrict__ out) {
  constexpr int U = 8;
  constexpr uint64_t kTile = 256u << 10;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
  const uint64_t ntiles = nbytes / kTile;
  uint32_t x = 0;
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    const u32x4* q = reinterpret_cast<const u32x4*>(base + t * kTile) + lane;
    constexpr uint64_t nb = kTile / kBlockBytes;
    u32x4 buf[U];
#pragma unroll
    for (int u = 0; u < U; ++u) buf[u] = ld16<NT>(q + u * 64);
    for (uint64_t b = 0; b + 2 * U <= nb; b += U) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const u32x4 w = buf[u];
        buf[u] = ld16<NT>(q + (b + U + u) * 64);
        x ^= w.x ^ w.y ^ w.z ^ w.w;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) x ^= buf[u].x ^ buf[u].y ^ buf[u].z ^ buf[u].w;
  }
  out[blockIdx.x * blockDim.x + threadIdx.x] = x;
}

// Contiguous per-wave shares (the sweep's layout: share = nbytes / waves, in 1 KiB
// blocks), optionally entered at a wave-dependent rotation so concurrent waves sit at
// different offsets of their shares (probes for channel/bank hot spots).
template <bool ROT>
__global__ __launch_bounds__(1024) void readbw_share_kernel(const uint8_t* __restrict__ base, uint64_t nbytes,
                                                            uint32_t* __restrict__ out) {
  constexpr int U = 8;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) * gridDim.x + blockIdx.x);
  const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
  const uint64_t nb = nbytes / kBlockBytes / nwaves;  // blocks per wave
  const u32x4* q = reinterpret_cast<const u32x4*>(base + (uint64_t)wave * nb * kBlockBytes) + lane;
  const uint64_t rot = ROT ? ((uint64_t)wave * 97u) % (nb ? nb : 1) : 0;
  uint32_t x = 0;
  uint64_t b = 0;
  for (; b + U <= nb; b += U) {
    u32x4 w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      uint64_t bb = b + u + rot;
      bb = bb >= nb ? bb - nb : bb;
      w[u] = __builtin_nontemporal_load(q + bb * 64);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) x ^= w[u].x ^ w[u].y ^ w[u].z ^ w[u].w;
  }
  out[blockIdx.x * blockDim.x + threadIdx.x] = x;
}

__global__ __launch_bounds__(256) void readbw_stream_kernel(const u32x4* __restrict__ p, uint64_t n16,
                                                            uint32_t* __restrict__ out) {
  constexpr int U = 8;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint32_t x = 0;
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + (U - 1) * stride < n16; i += U * stride) {
    u32x4 w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) w[u] = __builtin_nontemporal_load(p + i + u * stride);
#pragma unroll
    for (int u = 0; u < U; ++u) x ^= w[u].x ^ w[u].y ^ w[u].z ^ w[u].w;
  }
  for (; i < n16; i += stride) x ^= p[i].x;
  out[blockIdx.x * blockDim.x + threadIdx.x] = x;
}

// The group phase's access shape without its arithmetic: chunks of `chunk` bytes back to back,
// 64/G per wave round (one per G-lane group), wave w taking an equal run of the chunk list; each
// lane loads its 16 B of four 16G-byte blocks per 64G-byte super-block (t4_load), one
// super-block prefetched. The read roof the 4 KiB records' group rounds are compared against.
// COPY: also store every piece at dst + (its source offset) -- the group phase's copy-through
// store shape, for the copy roof of that shape (variants 32+ of launch_readbw).
template <int G, bool COPY = false>
__global__ __launch_bounds__(1024) void readbw_group_kernel(const uint8_t* __restrict__ base, uint64_t nbytes,
                                                            uint32_t chunk, uint32_t* __restrict__ out,
                                                            uint8_t* __restrict__ dst = nullptr) {
  constexpr uint32_t S = 64 / G;
  const uint32_t lane = threadIdx.x & 63u, gl = lane & (G - 1), gi = lane / G;
  const uint32_t wave = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) * gridDim.x + blockIdx.x);
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint64_t n = nbytes / chunk;
  const uint64_t per = ((n + nwaves - 1) / nwaves + S - 1) / S * S;
  const uint64_t i0 = wave * per, i1 = i0 + per < n ? i0 + per : n;
  const uint32_t nsb = (chunk + 64 * G - 1) / (64 * G);
  uint32_t x = 0;
  for (uint64_t i = i0; i < i1; i += S) {
    const uint64_t c = i + gi < i1 ? i + gi : i;
    const u32x4* q = reinterpret_cast<const u32x4*>(base + c * chunk) + gl;
    u32x4 nx[4], cur[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) nx[j] = ld16<true>(q + G * j);
    for (uint32_t sb = 0; sb < nsb; ++sb) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        cur[j] = nx[j];
        if (sb + 1 < nsb) nx[j] = ld16<true>(q + (sb + 1) * 4 * G + G * j);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if constexpr (COPY) {
          if (sb * 4 * G + G * j + gl < chunk / 16)
            st16u(dst + c * chunk + 16 * ((uint64_t)sb * 4 * G + G * j + gl), cur[j]);
        }
        x ^= cur[j].x ^ cur[j].y ^ cur[j].z ^ cur[j].w;
      }
    }
  }
  out[blockIdx.x * blockDim.x + threadIdx.x] = x;
}

// Grid-stride copy over many small blocks (the guide's float4-copy shape): variant 49 plain
// stores, 50 nontemporal stores.
template <bool NTS>
__global__ __launch_bounds__(256) void copybw_gridstride_kernel(const u32x4* __restrict__ src, uint64_t n16,
                                                               uint8_t* __restrict__ dst) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
    const u32x4 v = ld16<true>(src + i);
    if constexpr (NTS) st16u_nt(dst + 16 * i, v);
    else st16u(dst + 16 * i, v);
  }
}

// Contiguous copy: each wave copies an equal contiguous share of [0, n16) 16-B pieces, four per
// lane in flight (the plain copy roof of launch_readbw variant 48).
__global__ __launch_bounds__(1024) void copybw_stream_kernel(const u32x4* __restrict__ src, uint64_t n16,
                                                             uint8_t* __restrict__ dst) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (threadIdx.x >> 6) * (uint64_t)gridDim.x + blockIdx.x;
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint64_t per = ((n16 + nwaves - 1) / nwaves + 255) / 256 * 256;
  const uint64_t i0 = wave * per, i1 = i0 + per < n16 ? i0 + per : n16;
  for (uint64_t i = i0 + lane; i < i1; i += 256) {
    u32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = ld16<true>(src + (i + 64 * u < i1 ? i + 64 * u : i));
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i + 64 * u < i1) st16u(dst + 16 * (i + 64 * u), v[u]);
  }
}

// FETCH_SIZE calibration probe for scattered reads (variants 60 / 61 / 62): every 128-B line of
// [0, nbytes) is read exactly once, in a scattered order (line = t * odd stride mod lines, lines a
// power of two), by one 16-B / 4-B / 8-B load at the line start -- the access shape of the message
// processors' header, field and stored-CRC reads. FETCH_SIZE of a pass over a buffer larger than
// the Infinity Cache against nbytes gives the multiplier for those reads.
template <int W>
__global__ __launch_bounds__(256) void readbw_scatter_kernel(const uint8_t* __restrict__ base, uint64_t lines,
                                                             uint32_t* __restrict__ out) {
  uint32_t acc = 0;
  const uint64_t n = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < lines; t += n) {
    const uint64_t line = (t * 0x9E3779B1ull) & (lines - 1);
    const uint8_t* p = base + line * 128;
    if constexpr (W == 16) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(p);
      acc ^= v.x ^ v.y ^ v.z ^ v.w;
    } else if constexpr (W == 8) {
      uint64_t v;
      __builtin_memcpy(&v, p + 3, 8);  // unaligned, as the parse's big-endian long reads
      acc ^= (uint32_t)v ^ (uint32_t)(v >> 32);
    } else {
      acc ^= *reinterpret_cast<const uint32_t*>(p);
    }
  }
  if (acc == 0x9E3779B9u) out[0] = acc;  // keeps the loads
}

hipError_t launch_readbw(const uint8_t* base, uint64_t nbytes, uint32_t* out, int grid, int variant, hipStream_t s) {
  if (variant >= 60 && variant <= 62) {
    uint64_t lines = 1;
    while (lines * 2 * 128 <= nbytes) lines *= 2;
    const uint32_t blocks = (uint32_t)grid * 8;
    if (variant == 60) hipLaunchKernelGGL(readbw_scatter_kernel<16>, dim3(blocks), dim3(256), 0, s, base, lines, out);
    else if (variant == 61) hipLaunchKernelGGL(readbw_scatter_kernel<4>, dim3(blocks), dim3(256), 0, s, base, lines, out);
    else hipLaunchKernelGGL(readbw_scatter_kernel<8>, dim3(blocks), dim3(256), 0, s, base, lines, out);
    return hipGetLastError();
  }
  if (variant >= 32) {  // copy probes: read [0, nbytes/2), write from nbytes/2 (+ 11 B for 40..44)
    const uint64_t half = nbytes / 2 - 4096;
    uint8_t* dst = const_cast<uint8_t*>(base) + nbytes / 2 + (variant >= 40 && variant < 48 ? 11 : 0);
    if (variant == 49 || variant == 50) {
      if (variant == 49)
        hipLaunchKernelGGL(copybw_gridstride_kernel<false>, dim3(grid * 32), dim3(256), 0, s,
                           reinterpret_cast<const u32x4*>(base), half / 16, dst);
      else
        hipLaunchKernelGGL(copybw_gridstride_kernel<true>, dim3(grid * 32), dim3(256), 0, s,
                           reinterpret_cast<const u32x4*>(base), half / 16, dst);
      return hipGetLastError();
    }
    if (variant == 48) {
      hipLaunchKernelGGL(copybw_stream_kernel, dim3(grid), dim3(1024), 0, s, reinterpret_cast<const u32x4*>(base),
                         half / 16, dst);
      return hipGetLastError();
    }
    if (variant > 44) return hipErrorInvalidValue;  // 45..47, 51+: none
    const uint32_t chunk = 1024u << ((variant - 32) & 7);
    hipLaunchKernelGGL((readbw_group_kernel<16, true>), dim3(grid), dim3(1024), 0, s, base, half, chunk, out, dst);
    return hipGetLastError();
  }
  if (variant >= 16) {  // group shape: variant = 16 + log2(chunk bytes / 1024) for G = 16 (4 KiB: 18)
    const uint32_t chunk = 1024u << (variant - 16);
    hipLaunchKernelGGL(readbw_group_kernel<16>, dim3(grid), dim3(1024), 0, s, base, nbytes, chunk, out);
    return hipGetLastError();
  }
  switch (variant) {
    case 0: hipLaunchKernelGGL(readbw_tiles_kernel<false>, dim3(grid), dim3(1024), 0, s, base, nbytes, out); break;
    case 1: hipLaunchKernelGGL(readbw_tiles_kernel<true>, dim3(grid), dim3(1024), 0, s, base, nbytes, out); break;
    case 3: hipLaunchKernelGGL(readbw_share_kernel<false>, dim3(grid), dim3(1024), 0, s, base, nbytes, out); break;
    case 4: hipLaunchKernelGGL(readbw_share_kernel<true>, dim3(grid), dim3(1024), 0, s, base, nbytes, out); break;
    case 2:
      hipLaunchKernelGGL(readbw_stream_kernel, dim3(grid * 4 * 8), dim3(256), 0, s,
                         reinterpret_cast<const u32x4*>(base), nbytes / 16, out);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace ambrycrc
