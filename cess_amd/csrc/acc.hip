// Parity accumulated shard by shard (cec_encode_idx_batch, cec_update_batch, and on scattered
// shards cec_encode_idx_ptrs, cec_update_ptrs: k_acc_ptrs below): the one primitive
//   parity[o] ^= XOR_j c[j][o] * x_j        (overwrite mode: parity[o] = ...)
// where x_j is a data shard (EncodeIdx) or old_j ^ new_j of a changed data shard (Update).
//
// One lane owns 16-byte columns of the launch's parity shards: it loads them into the accumulators
// (not in overwrite mode), folds each input column in as k_rt does (the xtime powers up to the
// column's highest coefficient bit, one v_bitop3 acc ^= pow_b & mask per (output, bit)), and stores
// them. A lane reads and writes only its own parity columns, so accumulating in place needs no
// ordering between lanes. The next input's loads are issued before the current one is folded in.
//
// A launch takes at most kRtMaxOut outputs and kAccMaxIn inputs, and its coefficients, input
// slots and bit bounds travel in the kernel arguments: the kernels read no codec-owned device
// memory (no program cache entry, nothing to retire behind stream marks). The arrays are read
// through the kernarg segment (constant address space), so indexing them with the run-time input
// index stays a scalar load and makes no private copy; the 32-bit masks are expanded from the
// coefficient bytes on the SALU.
//
// Bytes moved per segment of F-byte shards, m parity shards: EncodeIdx (1 + 2m) F accumulating,
// (1 + m) F overwriting; Update of c shards (2c + 2m) F. EncodeIdx of RS(32,32) spends about 1.1
// VALU ops per byte moved (8 bits x 32 outputs of v_bitop3 per input dword, 65 dwords moved).
#include <cstring>

#include "dev_util.h"
#include "kernels.h"

namespace cec {

namespace {

constexpr uint32_t kAccAccumulate = 1;  // AccArgs::flags: read the parity before writing it
constexpr uint32_t kAccVec16 = 2;       // every base and stride allows 16-byte columns

struct AccArgs {
  const uint8_t* in_a;  // the shard (EncodeIdx) or the old bytes (Update)
  const uint8_t* in_b;  // the new bytes (Update)
  uint8_t* par;         // first parity shard of the launch, segment 0
  uint64_t len;
  uint64_t in_seg_stride, in_slot_stride;
  uint64_t par_seg_stride, par_shard_stride;
  uint32_t seg0, nin, nout, flags;
  uint32_t slot[kAccMaxIn];                 // input j is slot[j] of in_a (and of in_b)
  int32_t hb[kAccMaxIn];                    // highest set bit over coef[j][*], -1 for none
  uint32_t coef[kAccMaxIn][kRtMaxOut / 4];  // coef[j][o / 4] byte o % 4 = coefficient of
                                            // (output o, input j); zero past nout
};

typedef const AccArgs __attribute__((address_space(4))) AccArgsK;

// The kernel's only argument sits at offset 0 of the kernarg segment.
__device__ __forceinline__ const AccArgsK* acc_kernargs() {
  return (const AccArgsK*)__builtin_amdgcn_kernarg_segment_ptr();
}

// 2*x in GF(2^8)/0x11D on four packed bytes (kernels.hip xt).
__device__ __forceinline__ uint32_t xt(uint32_t x) {
  const uint32_t sign = __builtin_amdgcn_perm(x, x << 8, 0x0B090A08u);
  return __builtin_amdgcn_bitop3_b32((x & 0x7f7f7f7fu) << 1, sign, 0x1d1d1d1du, 0x78);  // a ^ (b & c)
}
__device__ __forceinline__ u32x4 xt(u32x4 x) {
  return u32x4{xt(x.x), xt(x.y), xt(x.z), xt(x.w)};
}
// a ^ (b & m)
__device__ __forceinline__ uint32_t bitop3_xand(uint32_t a, uint32_t b, uint32_t m) {
  return __builtin_amdgcn_bitop3_b32(a, b, m, 0x78);
}
__device__ __forceinline__ u32x4 bitop3_xand(u32x4 a, u32x4 b, uint32_t m) {
  return u32x4{bitop3_xand(a.x, b.x, m), bitop3_xand(a.y, b.y, m), bitop3_xand(a.z, b.z, m),
               bitop3_xand(a.w, b.w, m)};
}
__device__ __forceinline__ u32x4 ld16(const uint8_t* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
}
__device__ __forceinline__ void st16(uint8_t* p, u32x4 v) {
  __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
}

#define CEC_AI __attribute__((always_inline))

// The product over one lane's U columns. ld_in(which, slot, u): column u of input slot `slot` of
// in_a (which = 0) or in_b (1); ld_par / st_par(o, u): column u of parity shard o.
// K: the launch's arguments in the kernarg segment (AccArgs or AccPtrArgs: slot, hb, coef).
template <int NOB, int U, bool UPD, class T, class KA, class LI, class LP, class SP>
__device__ __forceinline__ void acc_fold(const KA* __restrict__ K, uint32_t nin,
                                         uint32_t nout, bool accumulate, LI ld_in, LP ld_par,
                                         SP st_par) {
  T acc[NOB][U];
  T cur_a[U], cur_b[U], nxt_a[U], nxt_b[U];
  {
    const uint32_t s0 = K->slot[0];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      cur_a[u] = ld_in(0, s0, u);
      if constexpr (UPD) cur_b[u] = ld_in(1, s0, u);
    }
  }
  // One wave-uniform branch for all the parity loads (a branch per output makes the compiler copy
  // the accumulators at every join). The accumulators padded up to the bucket have no shard: they
  // load the last real one again and are never stored.
  if (accumulate) {
#pragma unroll
    for (int o = 0; o < NOB; ++o) {
      const uint32_t oc = (uint32_t)o < nout ? (uint32_t)o : nout - 1;
#pragma unroll
      for (int u = 0; u < U; ++u) acc[o][u] = ld_par(oc, u);
    }
  } else {
#pragma unroll
    for (int o = 0; o < NOB; ++o)
#pragma unroll
      for (int u = 0; u < U; ++u) acc[o][u] = T(0);
  }
  for (uint32_t j = 0; j < nin; ++j) {
    if (j + 1 < nin) {
      const uint32_t sn = K->slot[j + 1];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        nxt_a[u] = ld_in(0, sn, u);
        if constexpr (UPD) nxt_b[u] = ld_in(1, sn, u);
      }
    }
    const int hb = K->hb[j];
    uint32_t w[(NOB + 3) / 4];
#pragma unroll
    for (int q = 0; q < (NOB + 3) / 4; ++q) w[q] = K->coef[j][q];
    T p[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if constexpr (UPD) p[u] = cur_a[u] ^ cur_b[u];
      else p[u] = cur_a[u];
    }
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      if (b > hb) break;  // wave-uniform: no higher coefficient bit in this column
      if (b > 0) {
#pragma unroll
        for (int u = 0; u < U; ++u) p[u] = xt(p[u]);
      }
#pragma unroll
      for (int o = 0; o < NOB; ++o) {
        const uint32_t m = 0u - ((w[o >> 2] >> (8 * (o & 3) + b)) & 1u);  // SALU
#pragma unroll
        for (int u = 0; u < U; ++u) acc[o][u] = bitop3_xand(acc[o][u], p[u], m);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      cur_a[u] = nxt_a[u];
      if constexpr (UPD) cur_b[u] = nxt_b[u];
    }
  }
#pragma unroll
  for (int o = 0; o < NOB; ++o) {
    if (o < (int)nout) {
#pragma unroll
      for (int u = 0; u < U; ++u) st_par(o, u, acc[o][u]);
    }
  }
}

// Grid x: tiles of 256 * U 16-byte columns (vec16) or of 256 bytes; grid y: segments from seg0.
template <int NOB, int U, bool UPD>
__global__ __launch_bounds__(256) void k_acc(AccArgs a) {
  const AccArgsK* __restrict__ K = acc_kernargs();
  const uint32_t seg = a.seg0 + blockIdx.y;
  const uint8_t* __restrict__ ia = a.in_a + seg * a.in_seg_stride;
  const uint8_t* __restrict__ ib = UPD ? a.in_b + seg * a.in_seg_stride : nullptr;
  uint8_t* __restrict__ par = a.par + seg * a.par_seg_stride;
  const bool accumulate = (a.flags & kAccAccumulate) != 0;
  const bool vec = (a.flags & kAccVec16) != 0;
  const uint64_t nvec = a.len / 16;
  if (vec && nvec) {
    // Lanes past the last column read that column again and store nothing: a branch around their
    // loads would make the input loop's control flow divergent and the argument reads vector loads.
    const uint64_t base = (uint64_t)blockIdx.x * (256 * U) + threadIdx.x;
    auto col = [&](int u) CEC_AI -> uint64_t {
      const uint64_t v = base + (uint64_t)u * 256;
      return (v < nvec ? v : nvec - 1) * 16;
    };
    auto ld_in = [&](int which, uint32_t slot, int u) CEC_AI -> u32x4 {
      return ld16((which ? ib : ia) + (uint64_t)slot * a.in_slot_stride + col(u));
    };
    auto ld_par = [&](uint32_t o, int u) CEC_AI -> u32x4 {
      return ld16(par + (uint64_t)o * a.par_shard_stride + col(u));
    };
    auto st_par = [&](int o, int u, u32x4 y) CEC_AI {
      if (base + (uint64_t)u * 256 < nvec) st16(par + (uint64_t)o * a.par_shard_stride + col(u), y);
    };
    acc_fold<NOB, U, UPD, u32x4>(K, a.nin, a.nout, accumulate, ld_in, ld_par, st_par);
  }
  if (vec && (!(a.len % 16) || blockIdx.x != gridDim.x - 1)) return;
  // byte path: the whole shard (grid covers len) or the tail after the last full column
  const uint64_t i = vec ? (a.len - a.len % 16) + threadIdx.x
                         : (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.len) return;
  auto ld_in = [&](int which, uint32_t slot, int) CEC_AI -> uint32_t {
    return ((which ? ib : ia) + (uint64_t)slot * a.in_slot_stride)[i];
  };
  auto ld_par = [&](uint32_t o, int) CEC_AI -> uint32_t {
    return (par + (uint64_t)o * a.par_shard_stride)[i];
  };
  auto st_par = [&](int o, int, uint32_t y) CEC_AI {
    (par + (uint64_t)o * a.par_shard_stride)[i] = (uint8_t)y;
  };
  acc_fold<NOB, 1, UPD, uint32_t>(K, a.nin, a.nout, accumulate, ld_in, ld_par, st_par);
}

template <int NOB, bool UPD>
void run_acc(AccArgs a, uint64_t nseg, hipStream_t st) {
  constexpr int U = 1;
  uint64_t gx = (a.flags & kAccVec16) ? (a.len / 16 + 256 * U - 1) / (256 * U) : (a.len + 255) / 256;
  if (gx == 0) gx = 1;  // tail-only shard
  for_y_chunks(nseg, [&](uint32_t s0, uint32_t ny) {
    a.seg0 = s0;
    hipLaunchKernelGGL((k_acc<NOB, U, UPD>), dim3((unsigned)gx, ny), dim3(256), 0, st, a);
  });
}

template <bool UPD>
void run_acc_bucket(int nob, const AccArgs& a, uint64_t nseg, hipStream_t st) {
  switch (nob) {
    case 1: run_acc<1, UPD>(a, nseg, st); break;
    case 2: run_acc<2, UPD>(a, nseg, st); break;
    case 3: run_acc<3, UPD>(a, nseg, st); break;
    case 4: run_acc<4, UPD>(a, nseg, st); break;
    case 5: run_acc<5, UPD>(a, nseg, st); break;
    case 6: run_acc<6, UPD>(a, nseg, st); break;
    case 7: run_acc<7, UPD>(a, nseg, st); break;
    case 8: run_acc<8, UPD>(a, nseg, st); break;
    case 12: run_acc<12, UPD>(a, nseg, st); break;
    case 16: run_acc<16, UPD>(a, nseg, st); break;
    case 24: run_acc<24, UPD>(a, nseg, st); break;
    default: run_acc<32, UPD>(a, nseg, st); break;
  }
}

// The table-addressed form (cec_encode_idx_ptrs, cec_update_ptrs): every workgroup row
// (blockIdx.y) owns one row of 64-bit words in a device table, {nin input addresses [, the nin
// new-data addresses (Update)], nout parity addresses}, rows `rs` words apart, so every shard lies
// wherever the caller has it. The row is read through the constant address space and its words
// become address_space(1) pointers (dev_util.h): scalar loads ahead of global_load / global_store.
// The product, the column clamp and the byte tail are k_acc's.
struct AccPtrArgs {
  const uint64_t* tab;
  uint64_t len;
  uint32_t row0, rs, nin, nout, flags, pad_;
  uint32_t slot[kAccMaxIn];                 // input j is word slot[j] of the row (its new bytes
                                            // word nin + slot[j])
  int32_t hb[kAccMaxIn];                    // as AccArgs
  uint32_t coef[kAccMaxIn][kRtMaxOut / 4];  // as AccArgs
};

typedef const AccPtrArgs __attribute__((address_space(4))) AccPtrArgsK;
typedef u32x4 __attribute__((address_space(1))) gv16;

__device__ __forceinline__ u32x4 ld16(const gu8* p) {
  return __builtin_nontemporal_load((const gv16*)p);
}
__device__ __forceinline__ void st16(gu8* p, u32x4 v) {
  __builtin_nontemporal_store(v, (gv16*)p);
}

// Grid x: as k_acc; grid y: table rows from row0.
template <int NOB, int U, bool UPD>
__global__ __launch_bounds__(256) void k_acc_ptrs(AccPtrArgs a) {
  const AccPtrArgsK* __restrict__ K =
      (const AccPtrArgsK*)__builtin_amdgcn_kernarg_segment_ptr();  // the only argument: offset 0
  const cu64* __restrict__ row = tab_row(a.tab, (uint64_t)a.row0 + blockIdx.y, a.rs);
  const uint32_t par0 = UPD ? 2 * a.nin : a.nin;  // the row's first parity word
  const bool accumulate = (a.flags & kAccAccumulate) != 0;
  const bool vec = (a.flags & kAccVec16) != 0;
  const uint64_t nvec = a.len / 16;
  if (vec && nvec) {
    // lanes past the last column read it again and store nothing, as in k_acc
    const uint64_t base = (uint64_t)blockIdx.x * (256 * U) + threadIdx.x;
    auto col = [&](int u) CEC_AI -> uint64_t {
      const uint64_t v = base + (uint64_t)u * 256;
      return (v < nvec ? v : nvec - 1) * 16;
    };
    auto ld_in = [&](int which, uint32_t slot, int u) CEC_AI -> u32x4 {
      return ld16(gptr(row[slot + (which ? a.nin : 0)]) + col(u));
    };
    auto ld_par = [&](uint32_t o, int u) CEC_AI -> u32x4 {
      return ld16(gptr(row[par0 + o]) + col(u));
    };
    auto st_par = [&](int o, int u, u32x4 y) CEC_AI {
      if (base + (uint64_t)u * 256 < nvec) st16(gptr(row[par0 + o]) + col(u), y);
    };
    acc_fold<NOB, U, UPD, u32x4>(K, a.nin, a.nout, accumulate, ld_in, ld_par, st_par);
  }
  if (vec && (!(a.len % 16) || blockIdx.x != gridDim.x - 1)) return;
  // byte path: the whole shard (grid covers len) or the tail after the last full column
  const uint64_t i = vec ? (a.len - a.len % 16) + threadIdx.x
                         : (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.len) return;
  auto ld_in = [&](int which, uint32_t slot, int) CEC_AI -> uint32_t {
    return gptr(row[slot + (which ? a.nin : 0)])[i];
  };
  auto ld_par = [&](uint32_t o, int) CEC_AI -> uint32_t { return gptr(row[par0 + o])[i]; };
  auto st_par = [&](int o, int, uint32_t y) CEC_AI { gptr(row[par0 + o])[i] = (uint8_t)y; };
  acc_fold<NOB, 1, UPD, uint32_t>(K, a.nin, a.nout, accumulate, ld_in, ld_par, st_par);
}

template <int NOB, bool UPD>
void run_acc_ptrs(AccPtrArgs a, uint64_t nrows, hipStream_t st) {
  constexpr int U = 1;
  uint64_t gx = (a.flags & kAccVec16) ? (a.len / 16 + 256 * U - 1) / (256 * U) : (a.len + 255) / 256;
  if (gx == 0) gx = 1;  // tail-only shard
  for_y_chunks(nrows, [&](uint32_t r0, uint32_t ny) {
    a.row0 = r0;
    hipLaunchKernelGGL((k_acc_ptrs<NOB, U, UPD>), dim3((unsigned)gx, ny), dim3(256), 0, st, a);
  });
}

template <bool UPD>
void run_acc_ptrs_bucket(int nob, const AccPtrArgs& a, uint64_t nrows, hipStream_t st) {
  switch (nob) {
    case 1: run_acc_ptrs<1, UPD>(a, nrows, st); break;
    case 2: run_acc_ptrs<2, UPD>(a, nrows, st); break;
    case 3: run_acc_ptrs<3, UPD>(a, nrows, st); break;
    case 4: run_acc_ptrs<4, UPD>(a, nrows, st); break;
    case 5: run_acc_ptrs<5, UPD>(a, nrows, st); break;
    case 6: run_acc_ptrs<6, UPD>(a, nrows, st); break;
    case 7: run_acc_ptrs<7, UPD>(a, nrows, st); break;
    case 8: run_acc_ptrs<8, UPD>(a, nrows, st); break;
    case 12: run_acc_ptrs<12, UPD>(a, nrows, st); break;
    case 16: run_acc_ptrs<16, UPD>(a, nrows, st); break;
    case 24: run_acc_ptrs<24, UPD>(a, nrows, st); break;
    default: run_acc_ptrs<32, UPD>(a, nrows, st); break;
  }
}

}  // namespace

void launch_acc_ptrs(const uint64_t* tab, uint32_t nrows, const uint8_t* coef, int nin, int nout,
                     bool update, bool accumulate, uint64_t len, bool vec_ok, hipStream_t st) {
  if (nrows == 0 || len == 0 || nin <= 0 || nout <= 0 || nin > kAccMaxIn || nout > kRtMaxOut)
    return;
  AccPtrArgs a;
  std::memset(&a, 0, sizeof(a));
  a.tab = tab;
  a.len = len;
  a.rs = (uint32_t)((update ? 2 : 1) * nin + nout);
  a.nin = (uint32_t)nin;
  a.nout = (uint32_t)nout;
  a.flags = (accumulate ? kAccAccumulate : 0) | (vec_ok ? kAccVec16 : 0);
  for (int j = 0; j < nin; ++j) {
    a.slot[j] = (uint32_t)j;
    unsigned any = 0;
    for (int o = 0; o < nout; ++o) {
      const unsigned c = coef[(size_t)j * nout + o];
      any |= c;
      a.coef[j][o >> 2] |= (uint32_t)c << (8 * (o & 3));
    }
    a.hb[j] = any ? 31 - __builtin_clz(any) : -1;
  }
  if (update) run_acc_ptrs_bucket<true>(rt_bucket(nout), a, nrows, st);
  else run_acc_ptrs_bucket<false>(rt_bucket(nout), a, nrows, st);
}

void launch_acc(const uint8_t* in_a, const uint8_t* in_b, uint64_t in_seg_stride,
                uint64_t in_slot_stride, uint8_t* parity, uint64_t par_seg_stride,
                uint64_t par_shard_stride, uint64_t len, const uint32_t* slots,
                const uint8_t* coef, int nin, int nout, bool accumulate, uint64_t nseg,
                hipStream_t st) {
  if (nseg == 0 || len == 0 || nin <= 0 || nout <= 0) return;
  uint32_t max_slot = 0;
  for (int j = 0; j < nin; ++j) max_slot = slots[j] > max_slot ? slots[j] : max_slot;
  // a stride counts only where it is multiplied by something nonzero
  uint64_t bits = (uintptr_t)in_a | (uintptr_t)in_b | (uintptr_t)parity;
  if (nseg > 1) bits |= in_seg_stride | par_seg_stride;
  if (max_slot > 0) bits |= in_slot_stride;
  if (nout > 1) bits |= par_shard_stride;
  const bool vec = (bits & 15) == 0;
  for (int o0 = 0; o0 < nout; o0 += kRtMaxOut) {
    const int no = nout - o0 < kRtMaxOut ? nout - o0 : kRtMaxOut;
    for (int j0 = 0; j0 < nin; j0 += kAccMaxIn) {
      const int ni = nin - j0 < kAccMaxIn ? nin - j0 : kAccMaxIn;
      AccArgs a;
      std::memset(&a, 0, sizeof(a));
      a.in_a = in_a;
      a.in_b = in_b;
      a.par = parity + (uint64_t)o0 * par_shard_stride;
      a.len = len;
      a.in_seg_stride = in_seg_stride;
      a.in_slot_stride = in_slot_stride;
      a.par_seg_stride = par_seg_stride;
      a.par_shard_stride = par_shard_stride;
      a.nin = (uint32_t)ni;
      a.nout = (uint32_t)no;
      // every input chunk after the first adds to what the first one left
      a.flags = ((accumulate || j0 > 0) ? kAccAccumulate : 0) | (vec ? kAccVec16 : 0);
      for (int j = 0; j < ni; ++j) {
        a.slot[j] = slots[j0 + j];
        unsigned any = 0;
        for (int o = 0; o < no; ++o) {
          const unsigned c = coef[(size_t)(j0 + j) * nout + o0 + o];
          any |= c;
          a.coef[j][o >> 2] |= (uint32_t)c << (8 * (o & 3));
        }
        a.hb[j] = any ? 31 - __builtin_clz(any) : -1;
      }
      if (in_b) run_acc_bucket<true>(rt_bucket(no), a, nseg, st);
      else run_acc_bucket<false>(rt_bucket(no), a, nseg, st);
    }
  }
}

}  // namespace cec
