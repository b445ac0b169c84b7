// Decode rows from flags, solved per segment (cec_repair_flagged_multi_ptrs, cec_flag_solve, and
// with read_plan.h cec_read_flagged_ptrs): the pieces of the planner kernels k_flag_plan_multi and
// k_read_plan (kernels.hip: plan_wave), as host and device inline functions without HIP types.
// The solve (fs_solve_begin, fs_solve_column) and the row writers are called by the kernels' lanes
// and by the host's loop (fs_plan_segment_as), so what is checked on a CPU is the code the kernels
// compile (tests/native/flag_solve.cpp, tests/native/read_plan.cpp, tests/test_flag_solve.py).
// What a repair and a read do differently is a rule type: FsRepair here, RpRead in read_plan.h.
//
// gf256.h fixes E = V * inv(V[0:k]) with V[r][c] = r^c: shard r of a segment is f(r) for one
// polynomial f of degree < k over GF(2^8), the evaluation points being the shard indices 0..n-1
// taken as field elements. The decode row of a lost shard j over any k survivors S_0 < ... <
// S_{k-1} is therefore the Lagrange basis at j,
//   c_t(j) = prod_{u != t} (j ^ S_u) / prod_{u != t} (S_t ^ S_u),
// with no matrix inversion and O(k) products per coefficient. With
//   D_t = prod_{u != t} (S_t ^ S_u)   and   N_j = prod_u (j ^ S_u)
// it is c_t(j) = N_j / ((j ^ S_t) * D_t). j is not a survivor and the survivors are distinct, so
// every factor, and with it every coefficient, is non-zero: a rebuild has no zero column.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CEC_FS_HD __host__ __device__ inline
#else
#define CEC_FS_HD inline
#endif
#if defined(__clang__)
#define CEC_FS_UNROLL _Pragma("unroll")
#else
#define CEC_FS_UNROLL
#endif

namespace cec {

constexpr int kFlagMultiMax = 4;  // CEC_FLAG_MULTI_MAX: the bit-plane product's widest bucket
// The chunk layout of kernels.h as far as the table kernels read it: header {nin, nout, nob, 0},
// hb[nin] at word kFsHbWord, masks[nin][8][nob] at kFsHeaderWords. The in / out index arrays
// between header and hb are not read through a table row and stay unwritten; there is no Horner
// section (header word 3 is zero).
constexpr uint32_t kFsHbWord = 4 + 512;
constexpr uint32_t kFsHeaderWords = 4 + 256 + 256 + 256;
CEC_FS_HD uint32_t fs_chunk_words(uint32_t k, uint32_t e) { return kFsHeaderWords + k * 8 * e; }

// a * b in GF(2^8) mod 0x11D (a, b < 256): the carry-less product, then the seven high bits
// folded down. No table, so host and device run the same code.
CEC_FS_HD uint32_t fs_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 8; ++i) p ^= (0u - ((b >> i) & 1u)) & (a << i);
  for (int i = 14; i >= 8; --i) p ^= (0u - ((p >> i) & 1u)) & (0x11Du << (i - 8));
  return p;
}
// 1 / a (a != 0) as a^254 = a^2 * a^4 * ... * a^128
CEC_FS_HD uint32_t fs_inv(uint32_t a) {
  uint32_t r = 1, s = a;
  for (int i = 1; i < 8; ++i) {
    s = fs_mul(s, s);
    r = fs_mul(r, s);
  }
  return r;
}

// The rule of cec_flag_status_multi on a segment's counts. The codes are the CEC_FLAG_* values
// (asserted where cess_ec.h is in sight).
constexpr uint32_t kFsClean = 0, kFsRebuilt = 1, kFsMany = 2, kFsLost = 3;
CEC_FS_HD uint32_t fs_status(uint32_t nbad, uint32_t ngood, uint32_t k, uint32_t max_bad) {
  return nbad == 0 ? kFsClean : ngood < k ? kFsLost : nbad <= max_bad ? kFsRebuilt : kFsMany;
}

// D_t over the survivor list S[0..k)
CEC_FS_HD uint32_t fs_denom(const uint8_t* S, uint32_t k, uint32_t t) {
  const uint32_t st = S[t];
  uint32_t d = 1;
  for (uint32_t u = 0; u < k; ++u)
    if (u != t) d = fs_mul(d, st ^ S[u]);
  return d;
}
// N_j for a shard j that is not in S
CEC_FS_HD uint32_t fs_numer(const uint8_t* S, uint32_t k, uint32_t j) {
  uint32_t nj = 1;
  for (uint32_t u = 0; u < k; ++u) nj = fs_mul(nj, j ^ S[u]);
  return nj;
}
// c_t(j) from N_j, S_t and D_t
CEC_FS_HD uint32_t fs_coef(uint32_t nj, uint32_t j, uint32_t st, uint32_t dt) {
  return fs_mul(nj, fs_inv(fs_mul(j ^ st, dt)));
}

// The chunk of a rebuild of e outputs from k survivors: its header ...
CEC_FS_HD void fs_put_header(uint32_t* chunk, uint32_t k, uint32_t e) {
  chunk[0] = k;
  chunk[1] = e;
  chunk[2] = e;
  chunk[3] = 0;
}
// ... and input column t: col holds c_t(out_o) in byte o (o < e <= 4). hb[t] is the highest set
// bit over the column's coefficients, masks[t][b][o] all ones where bit b of c_t(out_o) is set.
CEC_FS_HD void fs_put_column(uint32_t* chunk, uint32_t e, uint32_t t, uint32_t col) {
  uint32_t any = 0;
  for (uint32_t o = 0; o < e; ++o) any |= (col >> (8 * o)) & 0xFFu;
  uint32_t top = 0;
  for (uint32_t b = 1; b < 8; ++b)
    if ((any >> b) & 1u) top = b;
  chunk[kFsHbWord + t] = any ? top : 0xFFFFFFFFu;
  uint32_t* mk = chunk + kFsHeaderWords + (size_t)t * 8 * e;
  for (uint32_t b = 0; b < 8; ++b)
    for (uint32_t o = 0; o < e; ++o) mk[b * e + o] = 0u - ((col >> (8 * o + b)) & 1u);
}

// The solve of a rebuilt segment, the same code for a kernel's lanes and the host's loops. S: the
// first k good indices; lost: the e shards to rebuild, ascending, a byte each of one word.
CEC_FS_HD uint32_t fs_lost(uint32_t lost, uint32_t o) { return (lost >> (8 * o)) & 0xFFu; }
// N_j of every output and, with `chunk`, the chunk's header (a kernel passes it from one lane)
CEC_FS_HD void fs_solve_begin(const uint8_t* S, uint32_t k, uint32_t e, uint32_t lost,
                              uint32_t* nj, uint32_t* chunk) {
  CEC_FS_UNROLL
  for (uint32_t o = 0; o < (uint32_t)kFlagMultiMax; ++o)
    nj[o] = o < e ? fs_numer(S, k, fs_lost(lost, o)) : 0;
  if (chunk) fs_put_header(chunk, k, e);
}
// Input column t (a kernel: t = lane, lane + 64, ...; the host: t = 0..k): c_t(out_o) in byte o
// of what it returns and, with `chunk`, written into it
CEC_FS_HD uint32_t fs_solve_column(const uint8_t* S, uint32_t k, uint32_t e, uint32_t lost,
                                   const uint32_t* nj, uint32_t t, uint32_t* chunk) {
  const uint32_t dt = fs_denom(S, k, t);
  uint32_t col = 0;
  CEC_FS_UNROLL
  for (uint32_t o = 0; o < (uint32_t)kFlagMultiMax; ++o)
    if (o < e) col |= fs_coef(nj[o], fs_lost(lost, o), S[t], dt) << (8 * o);
  if (chunk) fs_put_column(chunk, e, t, col);
  return col;
}

// Bucket b's product rows: [nseg][k + 1 + b] = {program chunk, k survivors, b outputs} (TableAddr
// of kernels.hip); a product leaves a row whose word 0 is zero. `lane` of `lanes` writers.
CEC_FS_HD uint32_t fs_row_words(uint32_t k, uint32_t b) { return k + 1 + b; }
CEC_FS_HD void fs_put_idle(uint64_t* row, uint32_t words, uint32_t lane, uint32_t lanes) {
  for (uint32_t t = lane; t < words; t += lanes) row[t] = 0;
}
CEC_FS_HD void fs_put_chunk(uint64_t* row, uint64_t chunk) { row[0] = chunk; }
CEC_FS_HD void fs_put_in(uint64_t* row, uint32_t t, uint64_t addr) { row[1 + t] = addr; }
CEC_FS_HD void fs_put_out(uint64_t* row, uint32_t k, uint32_t o, uint64_t addr) {
  row[1 + k + o] = addr;
}

// What a planner does differently for a repair and for a read (read_plan.h: RpRead) is a rule
// type, the same one for the wave (kernels.hip: plan_wave) and for the host's loop below. The
// repair: a held shard that is not good is lost and is rebuilt where it lies; the row of a segment
// in a bucket that is not its own is idle in word 0 and otherwise unwritten; no copy rows.
struct FsRepair {
  static constexpr bool kCopies = false;
  template <class W>
  static CEC_FS_HD bool lost(bool held, bool good, uint32_t, uint32_t, const W*) {
    return held && !good;
  }
  static CEC_FS_HD uint64_t out_addr(const uint64_t* seg, const uint64_t*, uint32_t j) {
    return seg[j];
  }
  static CEC_FS_HD void put_idle(uint64_t* row, uint32_t, uint32_t lane, uint32_t) {
    if (lane == 0) fs_put_chunk(row, 0);
  }
};

// One segment, host only, the planner's lanes played by loops. held, flags: n bytes; wanted: k
// bytes where the rule reads them. The status by fs_status over the rule's lost shards; for a
// REBUILT segment those shards (out_idx, ascending, *nout of them, kFlagMultiMax bytes at the
// most), the first k good ones (in_idx, ascending), the rows (rows[o * k + t] = c_t(out_idx[o]))
// and, with `chunk` (fs_chunk_words(k, *nout) words), the program chunk as the kernel writes it.
// With copy rows, copy_idx[0 .. *ncopy) (k bytes) are the shards the rule copies, ascending. With
// `tab` (seg: n addresses, 0: not held; dst: k addresses, 0: not wanted) the tables are written
// as the kernel writes them: copy_rows and bucket_rows[b - 1] (fs_row_words(k, b) words each,
// null: no table for bucket b). Any output pointer but status and nout (and ncopy, with copy rows)
// may be null. Nothing else is written for a segment that is not REBUILT.
struct FsTables {
  const uint64_t* seg;
  const uint64_t* dst;
  uint64_t* copy_rows;
  uint64_t* bucket_rows[kFlagMultiMax];
  uint64_t chunk_addr;  // what word 0 of the segment's product row holds
};
template <class Rule>
inline void fs_plan_segment_as(uint32_t k, uint32_t n, const uint8_t* held, const uint8_t* flags,
                               const uint8_t* wanted, uint32_t max_bad, uint32_t* status,
                               uint32_t* nout, uint8_t* out_idx, uint8_t* in_idx, uint8_t* rows,
                               uint32_t* chunk, uint8_t* copy_idx, uint32_t* ncopy,
                               const FsTables* tab) {
  uint8_t S[256];
  uint32_t nlost = 0, ngood = 0, lost = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const bool good = held[i] && flags[i];
    if (good) {
      if (ngood < k) S[ngood] = (uint8_t)i;
      ++ngood;
    }
    if (Rule::lost(held[i] != 0, good, i, k, wanted)) {
      if (nlost < (uint32_t)kFlagMultiMax) lost |= i << (8 * nlost);
      ++nlost;
    }
  }
  const uint32_t st = fs_status(nlost, ngood, k, max_bad);
  *status = st;
  const uint32_t e = st == kFsRebuilt ? nlost : 0;
  *nout = e;
  if constexpr (Rule::kCopies) {
    uint32_t nc = 0;
    for (uint32_t j = 0; j < k; ++j) {
      const bool go = Rule::copied(st, wanted[j] != 0, held[j] && flags[j]);
      if (go && copy_idx) copy_idx[nc] = (uint8_t)j;
      nc += go;
      if (tab && tab->copy_rows) Rule::put_copy(tab->copy_rows, j, go, tab->seg[j], tab->dst[j]);
    }
    *ncopy = nc;
  }
  uint64_t* row = nullptr;
  if (tab)
    for (uint32_t b = 1; b <= (uint32_t)kFlagMultiMax; ++b) {
      uint64_t* const rb = tab->bucket_rows[b - 1];
      if (b == e) row = rb;
      else if (rb) Rule::put_idle(rb, fs_row_words(k, b), 0, 1);
    }
  if (!e) return;
  uint32_t nj[kFlagMultiMax];
  fs_solve_begin(S, k, e, lost, nj, chunk);
  if (row) fs_put_chunk(row, tab->chunk_addr);
  for (uint32_t o = 0; o < e; ++o) {
    if (out_idx) out_idx[o] = (uint8_t)fs_lost(lost, o);
    if (row) fs_put_out(row, k, o, Rule::out_addr(tab->seg, tab->dst, fs_lost(lost, o)));
  }
  for (uint32_t t = 0; t < k; ++t) {  // the lanes
    const uint32_t col = fs_solve_column(S, k, e, lost, nj, t, chunk);
    if (in_idx) in_idx[t] = S[t];
    if (rows)
      for (uint32_t o = 0; o < e; ++o) rows[(size_t)o * k + t] = (uint8_t)(col >> (8 * o));
    if (row) fs_put_in(row, t, tab->seg[S[t]]);
  }
}
inline void fs_plan_segment(uint32_t k, uint32_t n, const uint8_t* held, const uint8_t* flags,
                            uint32_t max_bad, uint32_t* status, uint32_t* nout, uint8_t* out_idx,
                            uint8_t* in_idx, uint8_t* rows, uint32_t* chunk) {
  fs_plan_segment_as<FsRepair>(k, n, held, flags, nullptr, max_bad, status, nout, out_idx, in_idx,
                               rows, chunk, nullptr, nullptr, nullptr);
}

}  // namespace cec
