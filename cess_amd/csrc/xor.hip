// Byte-stream kernels beside the codec. XOR reduction (the partial-product
// exchange of a degraded read): the decoder of a segment adds, in GF(2^8), the partial rebuilds
// other GPUs computed from the survivors they hold (cec_reconstruct_partial_batch) into its own
// partial: dst ^= src[0] ^ ... ^ src[nsrc-1].
// Addition in GF(2^8) is XOR, so this is the whole combine step; RCCL has no XOR reduction
// (rccl.h ncclRedOp_t), which is why the partials travel point to point and meet here.
//
// One lane owns 16 bytes of dst and walks the sources: read (nsrc + 1) * len, write len, all
// streaming (nontemporal). HBM-bound.
#include "dev_util.h"
#include "kernels.h"

namespace cec {

template <bool V16>
__global__ __launch_bounds__(256) void k_xor_reduce(uint8_t* __restrict__ dst,
                                                    const uint8_t* __restrict__ src, uint32_t nsrc,
                                                    uint64_t stride, uint64_t len) {
  // a grid-stride walk: the launcher caps the grid (kXorMaxBlocks), one step for shorter buffers
  const uint64_t step = (uint64_t)gridDim.x * 256;
  const uint64_t n = V16 ? len / 16 : len;  // V16: len is a 16-byte multiple
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
    if constexpr (V16) {
      u32x4 acc = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(dst) + i);
      for (uint32_t j = 0; j < nsrc; ++j)
        acc ^= __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + j * stride) + i);
      __builtin_nontemporal_store(acc, reinterpret_cast<u32x4*>(dst) + i);
    } else {
      uint8_t acc = dst[i];
      for (uint32_t j = 0; j < nsrc; ++j) acc ^= src[j * stride + i];
      dst[i] = acc;
    }
  }
}

// HIP refuses a launch of 2^32 or more work items in one dimension (gridDim.x * blockDim.x; the
// byte path of a 4 GiB buffer is 2^24 blocks of 256), so the grid stops at 2^22 blocks and the
// lanes walk the rest: 1 GiB of bytes, or 16 GiB of 16-byte columns, per step.
constexpr uint64_t kXorMaxBlocks = 1u << 22;

void launch_xor_reduce(uint8_t* dst, const uint8_t* src, uint32_t nsrc, uint64_t stride,
                       uint64_t len, hipStream_t st) {
  if (len == 0 || nsrc == 0) return;
  const bool v16 = (((uintptr_t)dst | (uintptr_t)src | stride | len) & 15) == 0;
  const uint64_t per_block = v16 ? 256 * 16 : 256;
  uint64_t blocks = (len + per_block - 1) / per_block;
  if (blocks > kXorMaxBlocks) blocks = kXorMaxBlocks;
  if (v16)
    hipLaunchKernelGGL(k_xor_reduce<true>, dim3((uint32_t)blocks), dim3(256), 0, st, dst, src,
                       nsrc, stride, len);
  else
    hipLaunchKernelGGL(k_xor_reduce<false>, dim3((uint32_t)blocks), dim3(256), 0, st, dst, src,
                       nsrc, stride, len);
}

// The scattered form (cec_xor_ptrs): every workgroup row (blockIdx.y) owns one row {dst, nsrc
// sources} of 64-bit words in a device table, so destinations and partials lie wherever the
// caller has them (receive buffers, output tensors) and rows may have different numbers of
// partials: a zero word is skipped. The row is read through the constant address space, as the
// pointer tables of kernels.hip are: the addresses arrive as wave-uniform scalar loads, the skip
// is a wave-uniform branch, and the words become address_space(1) pointers, so the accesses stay
// global_load / global_store. One lane owns 16 bytes, streaming as above; the last block of a row
// also takes the byte tail, and with vec_ok == 0 (some address of the call is not 16-byte aligned)
// the grid covers the row byte by byte.
typedef const uint64_t __attribute__((address_space(4))) xcu64;
typedef uint8_t __attribute__((address_space(1))) xgu8;
typedef u32x4 __attribute__((address_space(1))) xgv16;

__global__ __launch_bounds__(256) void k_xor_rows(const uint64_t* __restrict__ tab, uint32_t row0,
                                                  uint32_t nsrc, uint64_t len, int vec_ok) {
  const xcu64* __restrict__ row =
      (const xcu64*)(uintptr_t)tab + ((uint64_t)row0 + blockIdx.y) * ((uint64_t)nsrc + 1);
  xgu8* const dst = (xgu8*)row[0];
  if (vec_ok) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < len / 16) {
      u32x4 acc = __builtin_nontemporal_load((const xgv16*)dst + v);
      for (uint32_t j = 0; j < nsrc; ++j) {
        const uint64_t a = row[1 + j];
        if (a) acc ^= __builtin_nontemporal_load((const xgv16*)a + v);  // wave-uniform
      }
      __builtin_nontemporal_store(acc, (xgv16*)dst + v);
    }
    if (!(len % 16) || blockIdx.x != gridDim.x - 1) return;
  }
  // byte path: whole row (vec_ok == 0, grid covers len) or the tail (last block)
  const uint64_t i = vec_ok ? (len - len % 16) + threadIdx.x
                            : (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  uint8_t acc = dst[i];
  for (uint32_t j = 0; j < nsrc; ++j) {
    const uint64_t a = row[1 + j];
    if (a) acc ^= ((const xgu8*)a)[i];
  }
  dst[i] = acc;
}

void launch_xor_rows(const uint64_t* tab, uint32_t nrows, uint32_t nsrc, uint64_t len,
                     bool vec_ok, hipStream_t st) {
  if (len == 0 || nsrc == 0 || nrows == 0) return;
  uint64_t gx = vec_ok ? (len / 16 + 255) / 256 : (len + 255) / 256;
  if (gx == 0) gx = 1;  // shorter than one column: the tail's block
  for_y_chunks(nrows, [&](uint32_t r0, uint32_t ny) {
    hipLaunchKernelGGL(k_xor_rows, dim3((uint32_t)gx, ny), dim3(256), 0, st, tab, r0, nsrc, len,
                       vec_ok ? 1 : 0);
  });
}

// Per-segment equality of two [nseg][seg_bytes] device arrays (cec_verify_batch: recomputed
// parity against the stored parity): ok[seg] was set to 1 before; a lane that finds a differing
// 16-byte piece (or byte, unaligned) stores 0 there. Read-only streaming otherwise.
template <bool V16>
__global__ __launch_bounds__(256) void k_cmp_segments(const uint8_t* __restrict__ a,
                                                      const uint8_t* __restrict__ b,
                                                      uint64_t seg_bytes, uint8_t* __restrict__ ok,
                                                      uint32_t seg0) {
  const uint32_t seg = seg0 + blockIdx.y;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint8_t* pa = a + seg * seg_bytes;
  const uint8_t* pb = b + seg * seg_bytes;
  bool diff;
  if constexpr (V16) {
    if (i * 16 >= seg_bytes) return;
    const u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(pa) + i);
    const u32x4 y = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(pb) + i);
    const u32x4 z = x ^ y;
    diff = (z.x | z.y | z.z | z.w) != 0;
  } else {
    if (i >= seg_bytes) return;
    diff = pa[i] != pb[i];
  }
  if (diff) ok[seg] = 0;
}

void launch_cmp_segments(const uint8_t* a, const uint8_t* b, uint64_t seg_bytes, uint64_t nseg,
                         uint8_t* ok, hipStream_t st) {
  if (seg_bytes == 0 || nseg == 0) return;
  const bool v16 = (((uintptr_t)a | (uintptr_t)b | seg_bytes) & 15) == 0;
  const uint64_t per_block = v16 ? 256 * 16 : 256;
  const uint64_t gx = (seg_bytes + per_block - 1) / per_block;
  for_y_chunks(nseg, [&](uint32_t s0, uint32_t ny) {
    if (v16)
      hipLaunchKernelGGL(k_cmp_segments<true>, dim3((uint32_t)gx, ny), dim3(256), 0, st, a, b,
                         seg_bytes, ok, s0);
    else
      hipLaunchKernelGGL(k_cmp_segments<false>, dim3((uint32_t)gx, ny), dim3(256), 0, st, a, b,
                         seg_bytes, ok, s0);
  });
}

}  // namespace cec
