// A degraded read decided from flags (cec_read_flagged_ptrs, cec_read_status, cec_read_solve):
// the pieces of the planner kernels k_read_plan and k_read_plan21 (kernels.hip) that are not
// already in flag_solve.h, as host and device inline functions without HIP types, so the
// arithmetic and the row writers the kernels compile are checked on a CPU
// (tests/native/read_plan.cpp, tests/test_read_solve.py).
//
// What differs from the repair's plan: a shard is *missing* when it is a wanted data shard that is
// not good (not held, or held with flag 0); the outputs of a rebuild are the missing shards and
// their addresses come from the caller's destinations; and every wanted data shard that is good is
// copied, through one copy row {src, dst} per data shard. The survivors are the first k good
// shards in index order and the rows the Lagrange form of flag_solve.h, as in the repair.
#pragma once
#include "flag_solve.h"

namespace cec {

// good, and missing, of one shard
CEC_FS_HD bool rp_good(bool held, uint32_t flag) { return held && flag != 0; }
CEC_FS_HD bool rp_missing(bool wanted, bool good) { return wanted && !good; }
// The rule on a segment's counts: fs_status with the missing wanted data shards in the place of
// the bad ones.
CEC_FS_HD uint32_t rp_status(uint32_t nmiss, uint32_t ngood, uint32_t k, uint32_t max_bad) {
  return fs_status(nmiss, ngood, k, max_bad);
}
// whether the good wanted data shards of a segment of this status are copied
CEC_FS_HD bool rp_copies(uint32_t status) { return status == kFsClean || status == kFsRebuilt; }

// The tables, all of 64-bit words. Copy rows: [nseg][k][2], row (s, j) = {src, dst} of data shard
// j, zero in both words where there is nothing to copy.
constexpr uint32_t kRpCopyWords = 2;
CEC_FS_HD void rp_put_copy(uint64_t* copy_rows, uint32_t j, bool go, uint64_t src, uint64_t dst) {
  copy_rows[(size_t)j * kRpCopyWords] = go ? src : 0;
  copy_rows[(size_t)j * kRpCopyWords + 1] = go ? dst : 0;
}
// Bucket b's product rows: [nseg][k + 1 + b] = {program chunk, k survivors, b destinations}
// (TableAddr of kernels.hip); an idle row is zero in every word. `lane` of `lanes` writers.
CEC_FS_HD uint32_t rp_row_words(uint32_t k, uint32_t b) { return k + 1 + b; }
CEC_FS_HD void rp_put_idle(uint64_t* row, uint32_t words, uint32_t lane, uint32_t lanes) {
  for (uint32_t t = lane; t < words; t += lanes) row[t] = 0;
}
CEC_FS_HD void rp_put_chunk(uint64_t* row, uint64_t chunk) { row[0] = chunk; }
CEC_FS_HD void rp_put_in(uint64_t* row, uint32_t t, uint64_t addr) { row[1 + t] = addr; }
CEC_FS_HD void rp_put_out(uint64_t* row, uint32_t k, uint32_t o, uint64_t addr) {
  row[1 + k + o] = addr;
}

// RS(2,1), the closed forms of k_ptr21: row {input 0, input 1, output, case}, case j in {0, 1} =
// data shard j from (the other data shard, the parity); an idle row is {0, 0, 0, 3}. a[3] are the
// shard addresses (0: not held), f[3] the flags (f[i] is not looked at when a[i] is 0), d[2] the
// destinations (0: not wanted). Two missing shards leave one good at the most, so a REBUILT
// segment has exactly one. Returns the status; row: 4 words, copy_rows: 2 * kRpCopyWords words.
constexpr uint32_t kRp21RowWords = 4, kRp21Idle = 3;
CEC_FS_HD uint32_t rp_plan21(const uint64_t* a, const uint8_t* f, const uint64_t* d,
                             uint32_t max_bad, uint64_t* row, uint64_t* copy_rows) {
  const bool g0 = a[0] && f[0], g1 = a[1] && f[1], g2 = a[2] && f[2];
  const bool m0 = rp_missing(d[0] != 0, g0), m1 = rp_missing(d[1] != 0, g1);
  const uint32_t st = rp_status((uint32_t)m0 + m1, (uint32_t)g0 + g1 + g2, 2, max_bad);
  const bool go = st == kFsRebuilt;
  const uint32_t j = m0 ? 0 : 1;
  row[0] = !go ? 0 : j == 0 ? a[1] : a[0];
  row[1] = !go ? 0 : a[2];
  row[2] = !go ? 0 : d[j];
  row[3] = go ? j : kRp21Idle;
  const bool cp = rp_copies(st);
  rp_put_copy(copy_rows, 0, cp && d[0] && g0, a[0], d[0]);
  rp_put_copy(copy_rows, 1, cp && d[1] && g1, a[1], d[1]);
  return st;
}

// One segment, host only, the planner's lanes played by loops. held, flags: n bytes; wanted: k
// bytes. The status by rp_status; for a REBUILT segment the missing shards (out_idx, ascending,
// *nout of them, kFlagMultiMax bytes), the first k good shards (in_idx, k bytes), the rows
// (rows[o * k + t] = c_t(out_idx[o]), kFlagMultiMax * k bytes) and, with `chunk`
// (fs_chunk_words(k, *nout) words), the program chunk as the kernel writes it. For a CLEAN or
// REBUILT segment copy_idx[0 .. *ncopy) (k bytes) are the wanted good data shards, ascending;
// *ncopy is 0 for LOST and MANY. With `seg` (n addresses, 0: not held) and `dst` (k addresses, 0:
// not wanted) the tables are written as the kernel writes them: copy_rows (k * kRpCopyWords
// words) and bucket_rows[b - 1] (rp_row_words(k, b) words each, null: no table for bucket b).
// Any output pointer but status, nout and ncopy may be null.
struct RpTables {
  const uint64_t* seg;
  const uint64_t* dst;
  uint64_t* copy_rows;
  uint64_t* bucket_rows[kFlagMultiMax];
  uint64_t chunk_addr;  // what word 0 of the segment's product row holds
};
inline void rp_plan_segment(uint32_t k, uint32_t n, const uint8_t* held, const uint8_t* flags,
                            const uint8_t* wanted, uint32_t max_bad, uint32_t* status,
                            uint32_t* nout, uint8_t* out_idx, uint8_t* in_idx, uint8_t* rows,
                            uint32_t* chunk, uint8_t* copy_idx, uint32_t* ncopy,
                            const RpTables* tab) {
  uint8_t S[256], lost[kFlagMultiMax] = {};
  uint32_t nmiss = 0, ngood = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const bool good = rp_good(held[i] != 0, held[i] ? flags[i] : 0);
    if (good) {
      if (ngood < k) S[ngood] = (uint8_t)i;
      ++ngood;
    }
    if (i < k && rp_missing(wanted[i] != 0, good)) {
      if (nmiss < (uint32_t)kFlagMultiMax) lost[nmiss] = (uint8_t)i;
      ++nmiss;
    }
  }
  const uint32_t st = rp_status(nmiss, ngood, k, max_bad);
  *status = st;
  const uint32_t e = st == kFsRebuilt ? nmiss : 0;
  *nout = e;
  uint32_t nc = 0;
  for (uint32_t j = 0; j < k; ++j) {
    const bool go =
        rp_copies(st) && wanted[j] && rp_good(held[j] != 0, held[j] ? flags[j] : 0);
    if (go && copy_idx) copy_idx[nc] = (uint8_t)j;
    nc += go;
    if (tab && tab->copy_rows) rp_put_copy(tab->copy_rows, j, go, tab->seg[j], tab->dst[j]);
  }
  *ncopy = nc;
  uint64_t* row = nullptr;
  if (tab)
    for (uint32_t b = 1; b <= (uint32_t)kFlagMultiMax; ++b) {
      uint64_t* const rb = tab->bucket_rows[b - 1];
      if (b == e) row = rb;
      else if (rb) rp_put_idle(rb, rp_row_words(k, b), 0, 1);
    }
  if (!e) return;
  uint32_t nj[kFlagMultiMax] = {};
  for (uint32_t o = 0; o < e; ++o) {
    nj[o] = fs_numer(S, k, lost[o]);
    if (out_idx) out_idx[o] = lost[o];
    if (row) rp_put_out(row, k, o, tab->dst[lost[o]]);
  }
  if (chunk) fs_put_header(chunk, k, e);
  if (row) rp_put_chunk(row, tab->chunk_addr);
  for (uint32_t t = 0; t < k; ++t) {  // the lanes
    const uint32_t dt = fs_denom(S, k, t);
    uint32_t col = 0;
    for (uint32_t o = 0; o < e; ++o) col |= fs_coef(nj[o], lost[o], S[t], dt) << (8 * o);
    if (in_idx) in_idx[t] = S[t];
    if (rows)
      for (uint32_t o = 0; o < e; ++o) rows[(size_t)o * k + t] = (uint8_t)(col >> (8 * o));
    if (chunk) fs_put_column(chunk, e, t, col);
    if (row) rp_put_in(row, t, tab->seg[S[t]]);
  }
}

}  // namespace cec
