// Device helpers, and the launchers' grid-y chunking, shared by the HIP translation units of
// libcessec.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace cec {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint8_t* shard_ptr(const Layout& L, int idx, uint32_t seg) {
  return idx < L.k ? L.data + seg * L.data_seg_stride + (uint64_t)idx * L.shard_stride
                   : L.parity + seg * L.par_seg_stride + (uint64_t)(idx - L.k) * L.shard_stride;
}

// Pointer-table rows (kernels.h "Pointer-table addressing") are read through the constant address
// space: they are never written while a kernel runs, so their words arrive as wave-uniform scalar
// loads. The words are turned into address_space(1) pointers, not generic ones: the accesses stay
// global_load / global_store (a flat access counts on lgkmcnt too and would serialise with the
// scalar reads).
typedef const uint64_t __attribute__((address_space(4))) cu64;
typedef uint8_t __attribute__((address_space(1))) gu8;

__device__ __forceinline__ const cu64* tab_row(const uint64_t* tab, uint64_t row, uint32_t rs) {
  return (const cu64*)(uintptr_t)tab + row * rs;
}
__device__ __forceinline__ gu8* gptr(uint64_t a) { return (gu8*)a; }

// Host: a grid is at most kMaxGridY workgroup rows high, so `n` rows (segments, table rows,
// fragments) take f(first row, row count) once per launch of at most that many.
constexpr uint32_t kMaxGridY = 65535;
template <class F>
void for_y_chunks(uint64_t n, F f) {
  for (uint64_t r0 = 0; r0 < n; r0 += kMaxGridY)
    f((uint32_t)r0, (uint32_t)(n - r0 < kMaxGridY ? n - r0 : kMaxGridY));
}

// v_bitop3 with truth table 0x96: a ^ b ^ c in one VALU op.
__device__ __forceinline__ uint32_t xor3_u32(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

}  // namespace cec
