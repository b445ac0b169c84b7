// Audit chunk gather: the chunks a storage challenge names, copied out of
// every fragment of an HBM-resident batch so they can be hashed and proven.
//
// Reference: a fragment is CHUNK_COUNT = 1024 chunks (primitives/common/src/lib.rs:62), i.e.
// 8 KiB chunks of an 8 MiB fragment; a challenge names CHUNK_COUNT * 46 / 1000 = 47 distinct
// chunk indices (c-pallets/audit/src/lib.rs:955-964, NetSnapShot.random_index_list,
// types.rs:21). The PoDR2 tag arithmetic over those chunks runs in the TEE and is not in the
// reference; this is the byte-exact part: addressing and gathering.
//
// One lane moves 16 bytes; blockIdx.x walks (index, tile of the chunk), blockIdx.y the fragment.
// Pure HBM streaming: read + write nfrag * nidx * chunk_len bytes.
//
// Two addressings of the same column: fragments of a batch layout (k_chunk_gather,
// cec_audit_chunks) and fragments at arbitrary device addresses listed in a table
// (k_chunk_gather_tab, cec_audit_chunks_ptrs: a miner holds one fragment of many segments, each
// in its own allocation). For the hashes of scattered chunks nothing is gathered: k_chunk_addrs
// writes every chunk's address (8 bytes per chunk) and the SHA-256 kernels read the chunks where
// they lie.
#include "dev_util.h"
#include "kernels.h"

namespace cec {

typedef u32x4 __attribute__((address_space(1))) gv16;

__device__ __forceinline__ u32x4 ld16(const uint8_t* p, uint64_t v) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p) + v);
}
__device__ __forceinline__ u32x4 ld16(const gu8* p, uint64_t v) {
  return __builtin_nontemporal_load((const gv16*)p + v);
}

// One workgroup's piece of one chunk, shared by the in-layout and the table-addressed kernel
// (which differ only in where `src` comes from): lane v of tile `tile` moves 16 bytes (V16) or
// one byte of the chunk_len bytes at src to dst.
template <bool V16, class Src>
__device__ __forceinline__ void chunk_column(Src src, uint8_t* __restrict__ dst, uint32_t tile,
                                             uint64_t chunk_len) {
  if constexpr (V16) {
    const uint64_t v = (uint64_t)tile * 256 + threadIdx.x;
    if (v * 16 < chunk_len)
      __builtin_nontemporal_store(ld16(src, v), reinterpret_cast<u32x4*>(dst) + v);
  } else {
    const uint64_t b = (uint64_t)tile * 256 + threadIdx.x;
    if (b < chunk_len) dst[b] = src[b];
  }
}

template <bool V16>
__global__ __launch_bounds__(256) void k_chunk_gather(Layout L, int nshards,
                                                      const uint32_t* __restrict__ idx,
                                                      uint32_t nidx, uint64_t chunk_len,
                                                      uint32_t tiles, uint32_t frag0,
                                                      uint8_t* __restrict__ out) {
  const uint32_t j = blockIdx.x / tiles, tile = blockIdx.x - j * tiles;
  const uint32_t frag = frag0 + blockIdx.y;
  const uint32_t seg = frag / nshards, sh = frag - seg * nshards;
  const uint8_t* src = shard_ptr(L, (int)sh, seg) + (uint64_t)idx[j] * chunk_len;
  uint8_t* dst = out + ((uint64_t)frag * nidx + j) * chunk_len;
  chunk_column<V16>(src, dst, tile, chunk_len);
}

// The table-addressed form (cec_audit_chunks_ptrs): fragment f lies at frags[f] (a device table of
// 64-bit addresses, read through the constant address space as the other pointer tables are, one
// scalar load per workgroup), wherever the caller has it. Same grid, same column.
template <bool V16>
__global__ __launch_bounds__(256) void k_chunk_gather_tab(const uint64_t* __restrict__ frags,
                                                          const uint32_t* __restrict__ idx,
                                                          uint32_t nidx, uint64_t chunk_len,
                                                          uint32_t tiles, uint32_t frag0,
                                                          uint8_t* __restrict__ out) {
  const uint32_t j = blockIdx.x / tiles, tile = blockIdx.x - j * tiles;
  const uint32_t frag = frag0 + blockIdx.y;
  const gu8* src = gptr(tab_row(frags, frag, 1)[0]) + (uint64_t)idx[j] * chunk_len;
  uint8_t* dst = out + ((uint64_t)frag * nidx + j) * chunk_len;
  chunk_column<V16>(src, dst, tile, chunk_len);
}

// addrs[f * nidx + j] = frags[f] + idx[j] * chunk_len: the address of every challenged chunk,
// the per-chain array the SHA-256 kernels read (launch_sha256_hex's `ptrs`), so the chunks are
// hashed where they lie.
__global__ __launch_bounds__(256) void k_chunk_addrs(const uint64_t* __restrict__ frags,
                                                     const uint32_t* __restrict__ idx,
                                                     uint32_t nidx, uint64_t chunk_len, uint64_t n,
                                                     uint64_t* __restrict__ addrs) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t f = i / nidx;
  addrs[i] = frags[f] + (uint64_t)idx[i - f * nidx] * chunk_len;
}

void launch_chunk_gather(const Layout& L, int nshards, uint64_t nfrag, const uint32_t* d_idx,
                         uint32_t nidx, uint64_t chunk_len, uint8_t* out, hipStream_t st) {
  if (nfrag == 0 || nidx == 0 || chunk_len == 0) return;
  const uintptr_t bits = (uintptr_t)L.data | (uintptr_t)L.parity | L.shard_stride |
                         L.data_seg_stride | L.par_seg_stride | chunk_len | (uintptr_t)out;
  const bool v16 = (bits & 15) == 0;
  const uint64_t per_tile = v16 ? 256 * 16 : 256;
  const uint32_t tiles = (uint32_t)((chunk_len + per_tile - 1) / per_tile);
  for_y_chunks(nfrag, [&](uint32_t f0, uint32_t ny) {
    if (v16)
      hipLaunchKernelGGL(k_chunk_gather<true>, dim3(tiles * nidx, ny), dim3(256), 0, st, L,
                         nshards, d_idx, nidx, chunk_len, tiles, f0, out);
    else
      hipLaunchKernelGGL(k_chunk_gather<false>, dim3(tiles * nidx, ny), dim3(256), 0, st, L,
                         nshards, d_idx, nidx, chunk_len, tiles, f0, out);
  });
}

void launch_chunk_gather_tab(const uint64_t* d_frags, uint64_t nfrag, const uint32_t* d_idx,
                             uint32_t nidx, uint64_t chunk_len, uint8_t* out, bool vec_ok,
                             hipStream_t st) {
  if (nfrag == 0 || nidx == 0 || chunk_len == 0) return;
  const uint64_t per_tile = vec_ok ? 256 * 16 : 256;
  const uint32_t tiles = (uint32_t)((chunk_len + per_tile - 1) / per_tile);
  for_y_chunks(nfrag, [&](uint32_t f0, uint32_t ny) {
    if (vec_ok)
      hipLaunchKernelGGL(k_chunk_gather_tab<true>, dim3(tiles * nidx, ny), dim3(256), 0, st,
                         d_frags, d_idx, nidx, chunk_len, tiles, f0, out);
    else
      hipLaunchKernelGGL(k_chunk_gather_tab<false>, dim3(tiles * nidx, ny), dim3(256), 0, st,
                         d_frags, d_idx, nidx, chunk_len, tiles, f0, out);
  });
}

void launch_chunk_addrs(const uint64_t* d_frags, uint64_t nfrag, const uint32_t* d_idx,
                        uint32_t nidx, uint64_t chunk_len, uint64_t* d_addrs, hipStream_t st) {
  const uint64_t n = nfrag * nidx;
  if (n == 0) return;
  hipLaunchKernelGGL(k_chunk_addrs, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, d_frags,
                     d_idx, nidx, chunk_len, n, d_addrs);
}

}  // namespace cec
