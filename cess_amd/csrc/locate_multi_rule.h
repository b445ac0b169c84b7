// Which one or two held shards of a segment are corrupt, from parity alone (cec_locate_multi_ptrs,
// cec_locate_multi_host): the rule of the kernels k_pair_syn, k_pair_plan and k_pair_finish
// (kernels.hip) as host and device inline functions without HIP types, over locate_rule.h's
// helpers and in its notation, checked on a CPU (tests/native/locate_multi_model.cpp,
// tests/test_locate_multi_rule.py).
//
// H is the held set, h = |H|, u_i = 1 / prod_{i' in H, i' != i} (i ^ i'),
//   S_a(x) = XOR_{i in H} u_i * i^a * v_i(x)      a = 0 .. r-1,  0^0 = 1,  r = min(nsyn, h - k).
// Bad shards B with errors e_i give S_a = XOR_{i in B} u_i i^a e_i: a power-sum syndrome with the
// shard indices as locators. The pair rule applies to a segment when max_bad >= 2 and r = 4; every
// other segment gets steps 1-3 with its r and is AMBIGUOUS past them.
//   1. Locate pass. dirty = some S_a != 0 somewhere; the witness x1 is the lowest byte offset at
//      which ANY of S_0 .. S_{r-1} is non-zero. (Not cec_locate_ptrs' "S_0 != 0": two bad shards
//      can cancel S_0 at every offset, u_1 e_1 = u_2 e_2, and that witness would never appear.)
//   2. Column solve at x1, from the shard bytes there and coefficient rows 0..3 of the set.
//      One index: S_0 != 0 and exactly one held j has S_{a+1} = j S_a for every a < r - 1 (j = 0
//      is a legal shard). Then J = {j}.
//      Two indices (r = 4, the one-index test failed): det = S_1^2 ^ S_0 S_2 != 0,
//      sigma1 = (S_1 S_2 ^ S_0 S_3) / det, sigma2 = (S_1 S_3 ^ S_2^2) / det, and exactly two held i
//      satisfy i^2 ^ sigma1 i ^ sigma2 = 0 (the locator polynomial (z ^ j1)(z ^ j2)). Then J is
//      those two. Neither: AMBIGUOUS.
//   3. Confirm with |J| = 1. T_a = S_{a+1} ^ j S_a, a < r - 1. Zero everywhere: FOUND {j}.
//      Otherwise, without the pair rule: AMBIGUOUS. With it, x2 is the lowest offset at which any
//      T_a is non-zero; a second solve there needs T_0 != 0 and exactly one held i != j with
//      T_1 = i T_0 and T_2 = i T_1. Then J = {j, i}, sigma1 = j ^ i, sigma2 = j i. Else AMBIGUOUS.
//   4. Confirm with |J| = 2. U_a = S_{a+2} ^ sigma1 S_{a+1} ^ sigma2 S_a, a = 0, 1. Zero
//      everywhere: FOUND J. Otherwise AMBIGUOUS.
// A clean segment is read once; one bad shard, or two that meet at the first dirty offset, twice;
// two that do not meet there three times.
//
// FOUND: the shards of J have flag 0, the other held shards 1. AMBIGUOUS: every held flag 0. Not
// held: flag 0. nbad = |J| for FOUND, else 0.
//
// The guarantee, and its limit. With r = 4 the four checks define a code of distance 5 on H. If
// the held shards that differ from the codeword of the others are a set B with |B| <= 2, the
// result is FOUND with exactly B: the column at x1 has error weight 1 or 2 inside B and decoding
// is unique within radius 2, so the solve names the shard or shards in error there and nothing
// else; T is the syndrome of the held set without j (three checks, distance 4), so a single
// remaining bad shard is named uniquely at x2; U = XOR_i u_i (i ^ j1)(i ^ j2) i^a v_i has
// coefficient zero at both shards of J and is zero when the rest agree. A wrong FOUND needs, at
// every offset where an error outside J exists, an error of weight >= 3 outside J (U holds two
// checks, distance 3, on H without J), so it needs |B| >= 3: cec_confirm_flagged covers that case,
// as it does for the single rule at |B| >= r.
#pragma once
#include "locate_rule.h"

namespace cec {

constexpr int kLocateBadMax = 2;  // CEC_LOCATE_BAD_MAX

// A segment's candidate word between the passes: J in bytes 0 and 1 (byte 1 repeats byte 0 for
// one shard), sigma2 in byte 2, |J| in byte 3; kLocNone without a candidate.
CEC_FS_HD uint32_t loc2_pack1(uint32_t j) { return j | j << 8 | 1u << 24; }
CEC_FS_HD uint32_t loc2_pack2(uint32_t j, uint32_t i) {
  return j | i << 8 | fs_mul(j, i) << 16 | 2u << 24;
}
CEC_FS_HD uint32_t loc2_nbad(uint32_t cand) { return cand == kLocNone ? 0u : cand >> 24; }
CEC_FS_HD uint32_t loc2_j0(uint32_t cand) { return cand & 0xFFu; }
CEC_FS_HD uint32_t loc2_j1(uint32_t cand) { return (cand >> 8) & 0xFFu; }
CEC_FS_HD uint32_t loc2_sigma1(uint32_t cand) { return loc2_j0(cand) ^ loc2_j1(cand); }
CEC_FS_HD uint32_t loc2_sigma2(uint32_t cand) { return (cand >> 16) & 0xFFu; }

// The planner's table of a held set with all four coefficient rows, bytes: loc_put_set's header,
// then six arrays of n bytes: idx[t] = H[t] (t < h), c_a[t] = u_t * H[t]^a for a = 0..3 (zero for
// a >= r: the planner sees the syndromes the product computes), pos[i] = 1 where shard i is held,
// else 0.
CEC_FS_HD uint32_t loc2_set_bytes(uint32_t n) { return (kLocSetHead + 6 * n + 7) & ~7u; }
inline void loc2_put_set(uint8_t* set, const uint8_t* held, uint32_t n, uint32_t r) {
  uint8_t H[256];
  uint32_t h = 0;
  for (uint32_t i = 0; i < n; ++i) {
    set[kLocSetHead + 5 * n + i] = held[i] ? 1 : 0;
    if (held[i]) H[h++] = (uint8_t)i;
  }
  set[0] = (uint8_t)h, set[1] = (uint8_t)(h >> 8), set[2] = (uint8_t)r, set[3] = 0;
  set[4] = set[5] = set[6] = set[7] = 0;
  for (uint32_t t = 0; t < n; ++t) {
    const uint32_t col = t < h ? loc_column(H, h, t) : 0;
    set[kLocSetHead + t] = t < h ? H[t] : 0;
    for (uint32_t a = 0; a < 4; ++a)
      set[kLocSetHead + (1 + a) * n + t] = a < r ? (uint8_t)(col >> (8 * a)) : 0;
  }
}
CEC_FS_HD const uint8_t* loc2_set_idx(const uint8_t* set) { return set + kLocSetHead; }
CEC_FS_HD const uint8_t* loc2_set_coef(const uint8_t* set, uint32_t n, uint32_t a) {
  return set + kLocSetHead + (1 + a) * n;
}
CEC_FS_HD const uint8_t* loc2_set_pos(const uint8_t* set, uint32_t n) {
  return set + kLocSetHead + 5 * n;
}

// One held shard's byte v at a witness offset into the packed syndromes S_0..S_3 (byte a = S_a):
// a lane's share, or the host's loop body.
CEC_FS_HD uint32_t loc2_term(const uint8_t* set, uint32_t n, uint32_t t, uint32_t v) {
  uint32_t s = 0;
  CEC_FS_UNROLL
  for (uint32_t a = 0; a < 4; ++a) s |= fs_mul(loc2_set_coef(set, n, a)[t], v) << (8 * a);
  return s;
}
CEC_FS_HD uint32_t loc2_s(uint32_t packed, uint32_t a) { return (packed >> (8 * a)) & 0xFFu; }

// Step 2, one index: whether held shard i satisfies S_{a+1} = i S_a for every a < r - 1 (the
// caller has S_0 != 0 and r >= 2).
CEC_FS_HD bool loc2_one_matches(uint32_t i, uint32_t S, uint32_t r) {
  bool ok = true;
  for (uint32_t a = 0; a + 1 < r; ++a) ok = ok && fs_mul(i, loc2_s(S, a)) == loc2_s(S, a + 1);
  return ok;
}
// Step 2, two indices (r = 4): the locator's coefficients as sigma1 | sigma2 << 8, or kLocNone
// where det = 0. (Inlined by force: with the inverse's loops the compiler would otherwise leave a
// call in the planner kernel.)
CEC_FS_HD __attribute__((always_inline)) uint32_t loc2_locator(uint32_t S) {
  const uint32_t s0 = loc2_s(S, 0), s1 = loc2_s(S, 1), s2 = loc2_s(S, 2), s3 = loc2_s(S, 3);
  const uint32_t det = fs_mul(s1, s1) ^ fs_mul(s0, s2);
  if (det == 0) return kLocNone;
  const uint32_t inv = fs_inv(det);
  const uint32_t sg1 = fs_mul(fs_mul(s1, s2) ^ fs_mul(s0, s3), inv);
  const uint32_t sg2 = fs_mul(fs_mul(s1, s3) ^ fs_mul(s2, s2), inv);
  return sg1 | sg2 << 8;
}
CEC_FS_HD bool loc2_is_root(uint32_t i, uint32_t locator) {
  return (fs_mul(i, i) ^ fs_mul(locator & 0xFFu, i) ^ (locator >> 8)) == 0;
}
// Step 3: the packed T_0..T_2 of one byte column for the candidate j (byte a = T_a, a < 3), and
// whether held shard i != j is the second index.
CEC_FS_HD uint32_t loc2_t(uint32_t j, uint32_t S) {
  uint32_t T = 0;
  CEC_FS_UNROLL
  for (uint32_t a = 0; a < 3; ++a) T |= loc_t(j, loc2_s(S, a), loc2_s(S, a + 1)) << (8 * a);
  return T;
}
CEC_FS_HD bool loc2_second_matches(uint32_t i, uint32_t j, uint32_t T) {
  return i != j && fs_mul(i, loc2_s(T, 0)) == loc2_s(T, 1) &&
         fs_mul(i, loc2_s(T, 1)) == loc2_s(T, 2);
}
// Step 4: U_a of one byte for a = 0, 1
CEC_FS_HD uint32_t loc2_u(uint32_t cand, uint32_t sa, uint32_t sa1, uint32_t sa2) {
  return sa2 ^ fs_mul(loc2_sigma1(cand), sa1) ^ fs_mul(loc2_sigma2(cand), sa);
}

// Which steps apply. The first solve runs for a dirty segment with r >= 2 and a witness; the
// second for one whose single candidate left T dirty, under the pair rule.
CEC_FS_HD bool loc2_pair_rule(uint32_t r, uint32_t max_bad) { return max_bad >= 2 && r == 4; }
// The first solve's verdict from the ballots' counts: `ones` shards passed the one-index test
// (first of them j), else `roots` roots of the locator were held (the first two i0, i1).
CEC_FS_HD uint32_t loc2_solve1(uint32_t ones, uint32_t j, uint32_t roots, uint32_t i0,
                               uint32_t i1) {
  if (ones == 1) return loc2_pack1(j);
  return roots == 2 ? loc2_pack2(i0, i1) : kLocNone;
}

// The status table: dirty = some S_a != 0, cand as packed above, dirtyT = some T_a != 0 for a
// one-shard candidate, dirtyU = some U_a != 0 for a pair.
CEC_FS_HD uint32_t loc2_status(uint32_t h, uint32_t k, bool dirty, uint32_t cand, bool dirtyT,
                               bool dirtyU) {
  if (h <= k) return kLocUnchecked;
  if (!dirty) return kLocClean;
  const uint32_t nb = loc2_nbad(cand);
  if (nb == 1) return dirtyT ? kLocAmbiguous : kLocFound;
  if (nb == 2) return dirtyU ? kLocAmbiguous : kLocFound;
  return kLocAmbiguous;
}
CEC_FS_HD uint32_t loc2_flag(uint32_t status, bool held, uint32_t i, uint32_t cand) {
  if (!held || status == kLocAmbiguous) return 0;
  return status == kLocFound && (i == loc2_j0(cand) || i == loc2_j1(cand)) ? 0u : 1u;
}

// One segment on host memory, the kernels' passes played by loops: shards[i] (len bytes) or null
// where shard i is not held. found[0..2): the shards of a FOUND segment ascending, unused -1.
inline void loc2_segment_host(uint32_t k, uint32_t n, const uint8_t* const* shards, size_t len,
                              uint32_t nsyn, uint32_t max_bad, uint32_t* status, int* nfound,
                              int* found) {
  uint8_t held[256], H[256];
  uint32_t h = 0;
  for (uint32_t i = 0; i < n; ++i) {
    held[i] = shards[i] ? 1 : 0;
    if (shards[i]) H[h++] = (uint8_t)i;
  }
  const uint32_t r = loc_r(h, k, nsyn);
  *nfound = 0;
  found[0] = found[1] = -1;
  if (r == 0) {
    *status = loc2_status(h, k, false, kLocNone, false, false);
    return;
  }
  std::vector<uint8_t> setv(loc2_set_bytes(n));
  uint8_t* const set = setv.data();
  loc2_put_set(set, held, n, r);
  const uint32_t keep = r >= 4 ? 0xFFFFFFFFu : (1u << (8 * r)) - 1u;
  const uint8_t* const mul = loc_mul_table();
  uint32_t col[256];
  for (uint32_t t = 0; t < h; ++t) col[t] = loc_column(H, h, t) & keep;
  auto syndromes = [&](size_t x) {  // the product's view: packed S_0..S_{r-1}
    uint32_t S = 0;
    for (uint32_t t = 0; t < h; ++t) {
      const uint32_t v = shards[H[t]][x];
      if (!v) continue;
      for (uint32_t a = 0; a < r; ++a)
        S ^= (uint32_t)mul[((col[t] >> (8 * a)) & 0xFFu) * 256 + v] << (8 * a);
    }
    return S;
  };
  auto at_witness = [&](size_t x) {  // the planner's view
    uint32_t S = 0;
    for (uint32_t t = 0; t < h; ++t) S ^= loc2_term(set, n, t, shards[H[t]][x]);
    return S;
  };
  // 1. the locate pass
  bool dirty = false;
  uint64_t x1 = kLocNoWitness;
  for (size_t x = 0; x < len; ++x)
    if (syndromes(x)) {
      dirty = true;
      x1 = x;
      break;
    }
  // 2. the column solve at x1
  uint32_t cand = kLocNone;
  if (dirty && r >= 2) {
    const uint32_t S = at_witness((size_t)x1);
    uint32_t ones = 0, j = 0, roots = 0, i01[2] = {0, 0};
    if (loc2_s(S, 0))
      for (uint32_t t = 0; t < h; ++t)
        if (loc2_one_matches(H[t], S, r) && ones++ == 0) j = H[t];
    if (ones != 1 && loc2_pair_rule(r, max_bad)) {
      const uint32_t locator = loc2_locator(S);
      if (locator != kLocNone)
        for (uint32_t t = 0; t < h; ++t)
          if (loc2_is_root(H[t], locator)) {
            if (roots < 2) i01[roots] = H[t];
            ++roots;
          }
    }
    cand = loc2_solve1(ones, j, roots, i01[0], i01[1]);
  }
  // 3. the T confirm, with the second witness, and the second solve
  bool dirtyT = false, dirtyU = false;
  if (loc2_nbad(cand) == 1) {
    const uint32_t j = loc2_j0(cand);
    uint64_t x2 = kLocNoWitness;
    for (size_t x = 0; x < len; ++x) {
      const uint32_t S = syndromes(x);
      uint32_t T = 0;
      for (uint32_t a = 0; a + 1 < r; ++a) T |= loc_t(j, loc2_s(S, a), loc2_s(S, a + 1));
      if (T) {
        dirtyT = true;
        x2 = x;
        break;
      }
    }
    if (dirtyT && loc2_pair_rule(r, max_bad)) {
      const uint32_t T = loc2_t(j, at_witness((size_t)x2));
      uint32_t hits = 0, i2 = 0;
      if (loc2_s(T, 0))
        for (uint32_t t = 0; t < h; ++t)
          if (loc2_second_matches(H[t], j, T) && hits++ == 0) i2 = H[t];
      cand = hits == 1 ? loc2_pack2(j, i2) : kLocNone;
    }
  }
  // 4. the U confirm
  if (loc2_nbad(cand) == 2)
    for (size_t x = 0; x < len && !dirtyU; ++x) {
      const uint32_t S = syndromes(x);
      for (uint32_t a = 0; a < 2; ++a)
        dirtyU |= loc2_u(cand, loc2_s(S, a), loc2_s(S, a + 1), loc2_s(S, a + 2)) != 0;
    }
  *status = loc2_status(h, k, dirty, cand, dirtyT, dirtyU);
  if (*status == kLocFound) {
    const uint32_t nb = loc2_nbad(cand), a = loc2_j0(cand), b = loc2_j1(cand);
    *nfound = (int)nb;
    found[0] = (int)(a < b ? a : b);
    if (nb == 2) found[1] = (int)(a < b ? b : a);
  }
}

}  // namespace cec
