// Decode rows from flags, solved per segment (cec_repair_flagged_multi_ptrs, cec_flag_solve): the
// pieces of the planner kernel k_flag_plan_multi (kernels.hip), as host and device inline
// functions without HIP types, so the arithmetic the kernel compiles is checked on a CPU
// (tests/native/flag_solve.cpp, tests/test_flag_solve.py).
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

// One segment, host only, the planner's lanes played by loops: the status by fs_status, and for a
// REBUILT segment the bad shards (out_idx, ascending, *nout of them), the first k good ones
// (in_idx, ascending), the rows (rows[o * k + t] = c_t(out_idx[o])) and, with `chunk`
// (fs_chunk_words(k, *nout) words), the program chunk as the kernel writes it. Any output pointer
// but status and nout may be null. Nothing but *status and *nout (0) is written for a segment that
// is not REBUILT.
inline void fs_plan_segment(uint32_t k, uint32_t n, const uint8_t* held, const uint8_t* flags,
                            uint32_t max_bad, uint32_t* status, uint32_t* nout, uint8_t* out_idx,
                            uint8_t* in_idx, uint8_t* rows, uint32_t* chunk) {
  uint8_t S[256], lost[kFlagMultiMax] = {};
  uint32_t nbad = 0, ngood = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (!held[i]) continue;
    if (flags[i]) {
      if (ngood < k) S[ngood] = (uint8_t)i;
      ++ngood;
    } else {
      if (nbad < (uint32_t)kFlagMultiMax) lost[nbad] = (uint8_t)i;
      ++nbad;
    }
  }
  *status = fs_status(nbad, ngood, k, max_bad);
  const uint32_t e = *status == kFsRebuilt ? nbad : 0;
  *nout = e;
  if (!e) return;
  uint32_t nj[kFlagMultiMax] = {};
  for (uint32_t o = 0; o < e; ++o) {
    nj[o] = fs_numer(S, k, lost[o]);
    if (out_idx) out_idx[o] = lost[o];
  }
  if (chunk) fs_put_header(chunk, k, e);
  for (uint32_t t = 0; t < k; ++t) {  // the lanes
    const uint32_t dt = fs_denom(S, k, t);
    uint32_t col = 0;
    for (uint32_t o = 0; o < e; ++o) col |= fs_coef(nj[o], lost[o], S[t], dt) << (8 * o);
    if (in_idx) in_idx[t] = S[t];
    if (rows)
      for (uint32_t o = 0; o < e; ++o) rows[(size_t)o * k + t] = (uint8_t)(col >> (8 * o));
    if (chunk) fs_put_column(chunk, e, t, col);
  }
}

}  // namespace cec
