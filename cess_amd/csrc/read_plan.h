// A degraded read decided from flags (cec_read_flagged_ptrs, cec_read_status, cec_read_solve):
// what the planner kernels k_read_plan and k_read_plan21 (kernels.hip) have that flag_solve.h
// does not: the rule of a read, the copy rows and RS(2,1)'s closed form, as host and device inline
// functions without HIP types, checked on a CPU (tests/native/read_plan.cpp,
// tests/test_read_solve.py).
//
// What differs from the repair's plan: a shard is *missing* when it is a wanted data shard that is
// not good (not held, or held with flag 0); the outputs of a rebuild are the missing shards and
// their addresses come from the caller's destinations; and every wanted data shard that is good is
// copied, through one copy row {src, dst} per data shard. The survivors are the first k good
// shards in index order and the rows the Lagrange form of flag_solve.h, as in the repair.
#pragma once
#include "flag_solve.h"

namespace cec {

// missing, of one shard (good: held with a flag that is not 0)
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
// The read as a planner's rule (flag_solve.h: FsRepair is the repair's): a wanted data shard
// that is not good is lost and is rebuilt at its destination; the row of a segment in a bucket
// that is not its own is zero in every word; the good wanted data shards of a segment that is
// read have copy rows.
struct RpRead {
  static constexpr bool kCopies = true;
  template <class W>
  static CEC_FS_HD bool lost(bool, bool good, uint32_t i, uint32_t k, const W* wanted) {
    return i < k && rp_missing(wanted[i] != 0, good);
  }
  static CEC_FS_HD uint64_t out_addr(const uint64_t*, const uint64_t* dst, uint32_t j) {
    return dst[j];
  }
  static CEC_FS_HD void put_idle(uint64_t* row, uint32_t words, uint32_t lane, uint32_t lanes) {
    fs_put_idle(row, words, lane, lanes);
  }
  static CEC_FS_HD bool copied(uint32_t status, bool wanted, bool good) {
    return rp_copies(status) && wanted && good;
  }
  static CEC_FS_HD void put_copy(uint64_t* copy_rows, uint32_t j, bool go, uint64_t src,
                                 uint64_t dst) {
    rp_put_copy(copy_rows, j, go, src, dst);
  }
};

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

// One segment, host only: fs_plan_segment_as under the read's rule (wanted: k bytes; *ncopy is 0
// for LOST and MANY). The tables and a product row's width under the names the read's callers
// (tests/native/read_plan.cpp) have for them.
using RpTables = FsTables;
CEC_FS_HD uint32_t rp_row_words(uint32_t k, uint32_t b) { return fs_row_words(k, b); }
inline void rp_plan_segment(uint32_t k, uint32_t n, const uint8_t* held, const uint8_t* flags,
                            const uint8_t* wanted, uint32_t max_bad, uint32_t* status,
                            uint32_t* nout, uint8_t* out_idx, uint8_t* in_idx, uint8_t* rows,
                            uint32_t* chunk, uint8_t* copy_idx, uint32_t* ncopy,
                            const RpTables* tab) {
  fs_plan_segment_as<RpRead>(k, n, held, flags, wanted, max_bad, status, nout, out_idx, in_idx,
                             rows, chunk, copy_idx, ncopy, tab);
}

}  // namespace cec
