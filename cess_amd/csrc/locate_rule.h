// Which held shard of a segment is corrupt, from parity alone (cec_locate_ptrs, cec_locate_host,
// cec_locate_rows): the rule of the kernels k_syn, k_locate_plan and k_locate_finish (kernels.hip)
// as host and device inline functions without HIP types, in the manner of flag_solve.h and
// read_plan.h, checked on a CPU (tests/native/locate_model.cpp, tests/test_locate_rule.py).
//
// gf256.h's convention makes shard i of a segment f(i) for one polynomial f of degree < k (see
// flag_solve.h). The h held shards of a segment, at the points H, are therefore a codeword of a
// generalised Reed-Solomon code of dimension k, whose dual gives h - k checks on every byte offset:
//   S_a = XOR_{i in H} u_i * i^a * v_i = 0      a = 0 .. h-k-1
//   u_i = 1 / prod_{i' in H, i' != i} (i ^ i')  0^0 = 1
// (sum_i u_i g(i) is the leading coefficient of the interpolant of g through H, zero for every g of
// degree < h - 1, and i^a f(i) has degree < k + a.) One bad shard j with error e gives S_a =
// u_j j^a e: S_1 = j S_0, the ratio is the shard index. With j known,
//   T_a = S_{a+1} ^ j S_a = XOR_i u_i (i ^ j) i^a v_i
// has coefficient zero at shard j and is, up to the non-zero factors (i ^ j), the syndrome a of the
// held set without j: T_0 .. T_{r-2} zero at every byte says the other held shards agree.
//
// The rule, per segment, with r = min(nsyn, h - k) syndromes computed (nsyn in [1, kLocateSynMax]):
//   UNCHECKED  h <= k: no redundancy is held, no shard byte is read          held flags 1
//   CLEAN      r >= 1 and S_0 .. S_{r-1} zero at every byte offset           held flags 1
//   FOUND      dirty, r >= 2, and (a) some byte offset has S_0 != 0, (b) x is the lowest such,
//              (c) exactly one j in H has S_1(x) = j S_0(x), (d) T_0 .. T_{r-2} for that j are
//              zero at every byte offset                                     held 1, shard j 0
//   AMBIGUOUS  dirty and not FOUND, every dirty segment with r = 1 included  held flags 0
// Flags of shards that are not held are 0. AMBIGUOUS marks every held shard bad on purpose: the
// flagged repairs then report LOST and write nothing, the flagged read refuses the segment, and
// the where-add can hash exactly those fragments (gate = kLocAmbiguous).
//
// The guarantee, and its limit. If exactly one held shard of a segment differs from the codeword
// of the others, the segment is FOUND with that shard, for any r >= 2: S_0 = u_j e is non-zero
// wherever e is, the ratio is j at every such offset and at no other index, and T is zero. If b
// held shards differ, 2 <= b <= r - 1, the segment is never FOUND: FOUND with j would make the
// held set without j, a code of distance r (over the r - 1 checks T), contain an error of weight
// <= b < r at some offset, and T would be non-zero there. With b >= r a wrong FOUND is possible:
// errors in several shards at the same byte offsets can imitate one. That is what
// cec_confirm_flagged is for. The rule speaks of the mutual consistency of the held shards, not of
// their recorded hashes: k + 1 shards replaced by another codeword's are CLEAN.
#pragma once
#include <vector>

#include "flag_solve.h"

namespace cec {

constexpr int kLocateSynMax = 4;  // CEC_LOCATE_SYN_MAX: the bit-plane product's widest bucket
constexpr uint32_t kLocClean = 0, kLocFound = 1, kLocAmbiguous = 2, kLocUnchecked = 3;
constexpr uint32_t kLocNone = 0xFFFFFFFFu;           // no candidate
constexpr uint64_t kLocNoWitness = ~(uint64_t)0;     // no byte offset with S_0 != 0 seen

// syndromes computed for a held set of h shards
CEC_FS_HD uint32_t loc_r(uint32_t h, uint32_t k, uint32_t nsyn) {
  return h <= k ? 0u : (nsyn < h - k ? nsyn : h - k);
}
// i^a, 0^0 = 1
CEC_FS_HD uint32_t loc_pow(uint32_t i, uint32_t a) {
  uint32_t p = 1;
  for (uint32_t t = 0; t < a; ++t) p = fs_mul(p, i);
  return p;
}
// u_t of held shard H[t] over the held list H[0 .. h), ascending
CEC_FS_HD uint32_t loc_u(const uint8_t* H, uint32_t h, uint32_t t) {
  return fs_inv(fs_denom(H, h, t));
}
// Input column t of the syndrome product: u_t * H[t]^a in byte a, a < kLocateSynMax
CEC_FS_HD uint32_t loc_column(const uint8_t* H, uint32_t h, uint32_t t) {
  uint32_t c = loc_u(H, h, t), col = 0;
  CEC_FS_UNROLL
  for (uint32_t a = 0; a < (uint32_t)kLocateSynMax; ++a) {
    col |= c << (8 * a);
    c = fs_mul(c, H[t]);
  }
  return col;
}
// The program chunk of a held set (the layout of flag_solve.h: header {h, r, r, 0}, hb, masks),
// fs_chunk_words(h, r) words: r outputs from the h held shards in index order.
inline void loc_put_chunk(uint32_t* chunk, const uint8_t* H, uint32_t h, uint32_t r) {
  fs_put_header(chunk, h, r);
  const uint32_t keep = r >= 4 ? 0xFFFFFFFFu : (1u << (8 * r)) - 1u;
  for (uint32_t t = 0; t < h; ++t) fs_put_column(chunk, r, t, loc_column(H, h, t) & keep);
}

// The planner's table of a held set, bytes: {h in bytes 0 and 1, little-endian, r in byte 2, five
// bytes of zero}, then four arrays of n bytes: idx[t] = H[t] (t < h), c0[t] = u_t, c1[t] = u_t * H[t],
// pos[i] = 1 where shard i is held, else 0.
constexpr uint32_t kLocSetHead = 8;
CEC_FS_HD uint32_t loc_set_bytes(uint32_t n) { return (kLocSetHead + 4 * n + 7) & ~7u; }
inline void loc_put_set(uint8_t* set, const uint8_t* held, uint32_t n, uint32_t r) {
  uint8_t H[256];
  uint32_t h = 0;
  for (uint32_t i = 0; i < n; ++i) {
    set[kLocSetHead + 3 * n + i] = held[i] ? 1 : 0;
    if (held[i]) H[h++] = (uint8_t)i;
  }
  set[0] = (uint8_t)h, set[1] = (uint8_t)(h >> 8), set[2] = (uint8_t)r, set[3] = 0;
  set[4] = set[5] = set[6] = set[7] = 0;
  for (uint32_t t = 0; t < n; ++t) {
    const uint32_t col = t < h ? loc_column(H, h, t) : 0;
    set[kLocSetHead + t] = t < h ? H[t] : 0;
    set[kLocSetHead + n + t] = (uint8_t)col;
    set[kLocSetHead + 2 * n + t] = (uint8_t)(col >> 8);
  }
}
CEC_FS_HD uint32_t loc_set_h(const uint8_t* set) { return set[0] | (uint32_t)set[1] << 8; }
CEC_FS_HD uint32_t loc_set_r(const uint8_t* set) { return set[2]; }

// (c): whether held shard i is a candidate for the witness syndromes S_0 != 0 and S_1
CEC_FS_HD bool loc_matches(uint32_t i, uint32_t s0, uint32_t s1) { return fs_mul(i, s0) == s1; }
// T_a of one byte from S_a and S_{a+1}
CEC_FS_HD uint32_t loc_t(uint32_t j, uint32_t sa, uint32_t sa1) { return sa1 ^ fs_mul(j, sa); }

// The table above: dirty = some S_a != 0 somewhere, cand = the candidate of (c) or kLocNone (also
// without a witness, or with r < 2), dirty2 = some T_a != 0 somewhere.
CEC_FS_HD uint32_t loc_status(uint32_t h, uint32_t k, uint32_t r, bool dirty, uint32_t cand,
                              bool dirty2) {
  if (h <= k) return kLocUnchecked;
  if (!dirty) return kLocClean;
  return r >= 2 && cand != kLocNone && !dirty2 ? kLocFound : kLocAmbiguous;
}
// the flag byte of shard i
CEC_FS_HD uint32_t loc_flag(uint32_t status, bool held, uint32_t i, uint32_t cand) {
  if (!held || status == kLocAmbiguous) return 0;
  return status == kLocFound && i == cand ? 0u : 1u;
}

// Host only: every product a * b by fs_mul, once per process, [a * 256 + b].
inline const uint8_t* loc_mul_table() {
  static const std::vector<uint8_t> tab = [] {
    std::vector<uint8_t> t(256 * 256);
    for (uint32_t a = 0; a < 256; ++a)
      for (uint32_t b = 0; b < 256; ++b) t[a * 256 + b] = (uint8_t)fs_mul(a, b);
    return t;
  }();
  return tab.data();
}

// One segment on host memory, the kernels' passes played by loops: shards[i] (len bytes) or null
// where shard i is not held. *found = the shard of a FOUND segment, else -1.
inline void loc_segment_host(uint32_t k, uint32_t n, const uint8_t* const* shards, size_t len,
                             uint32_t nsyn, uint32_t* status, int* found) {
  uint8_t H[256];
  uint32_t h = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (shards[i]) H[h++] = (uint8_t)i;
  const uint32_t r = loc_r(h, k, nsyn);
  *found = -1;
  if (r == 0) {
    *status = loc_status(h, k, r, false, kLocNone, false);
    return;
  }
  uint32_t col[256];
  for (uint32_t t = 0; t < h; ++t) col[t] = loc_column(H, h, t);
  const uint8_t* const mul = loc_mul_table();
  auto syndromes = [&](size_t x, uint32_t* S) {
    for (uint32_t a = 0; a < r; ++a) S[a] = 0;
    for (uint32_t t = 0; t < h; ++t) {
      const uint32_t v = shards[H[t]][x];
      if (!v) continue;
      for (uint32_t a = 0; a < r; ++a) S[a] ^= mul[((col[t] >> (8 * a)) & 0xFFu) * 256 + v];
    }
  };
  // the locate pass: dirty, and the witness as the lowest offset with S_0 != 0
  bool dirty = false;
  uint64_t witness = kLocNoWitness;
  uint32_t S[kLocateSynMax];
  for (size_t x = 0; x < len; ++x) {
    syndromes(x, S);
    uint32_t any = 0;
    for (uint32_t a = 0; a < r; ++a) any |= S[a];
    dirty |= any != 0;
    if (S[0] && witness == kLocNoWitness) witness = x;
  }
  // the planner: S_0 and S_1 at the witness from the table's rows 0 and 1
  uint32_t cand = kLocNone;
  if (dirty && r >= 2 && witness != kLocNoWitness) {
    uint32_t s0 = 0, s1 = 0, hits = 0;
    for (uint32_t t = 0; t < h; ++t) {
      const uint32_t v = shards[H[t]][witness];
      s0 ^= fs_mul(col[t] & 0xFFu, v);
      s1 ^= fs_mul((col[t] >> 8) & 0xFFu, v);
    }
    for (uint32_t t = 0; t < h; ++t)
      if (loc_matches(H[t], s0, s1)) {
        cand = H[t];
        ++hits;
      }
    if (hits != 1) cand = kLocNone;
  }
  // the confirm pass
  bool dirty2 = false;
  if (cand != kLocNone)
    for (size_t x = 0; x < len && !dirty2; ++x) {
      syndromes(x, S);
      for (uint32_t a = 0; a + 1 < r; ++a) dirty2 |= loc_t(cand, S[a], S[a + 1]) != 0;
    }
  *status = loc_status(h, k, r, dirty, cand, dirty2);
  if (*status == kLocFound) *found = (int)cand;
}

}  // namespace cec
