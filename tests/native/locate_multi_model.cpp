// The rule of cec_locate_multi_ptrs (csrc/locate_multi_rule.h) in a program of its own, built
// with -fsanitize=address,undefined by tests/test_locate_multi_rule.py: codewords from gf256.h's
// encode matrix in buffers of exactly their length, one and two bad shards in every shape under
// four checks, two under fewer, three against nothing but memory safety, the candidate word, the
// status table, and the four-row set table written into a buffer of exactly its stated size.
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../cess_amd/csrc/gf256.h"
#include "../../cess_amd/csrc/locate_multi_rule.h"

using namespace cec;
using Big = Mat<kMaxShards, kMaxShards>;
using Work = Mat<kMaxShards, 2 * kMaxShards>;

static int g_fail = 0;
#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);     \
      ++g_fail;                                                    \
    }                                                              \
  } while (0)

struct Segment {
  int k, m;
  size_t len;
  std::vector<std::vector<uint8_t>> cw;
};

static Segment make_segment(int k, int m, size_t len, std::mt19937& rng) {
  auto E = std::make_unique<Big>();
  auto top = std::make_unique<Big>();
  auto topinv = std::make_unique<Big>();
  auto work = std::make_unique<Work>();
  CHECK(gf_encode_matrix(k, m, *E, *top, *topinv, *work));
  Segment s{k, m, len, {}};
  s.cw.assign(k + m, std::vector<uint8_t>(len, 0));
  for (int i = 0; i < k; ++i)
    for (auto& b : s.cw[i]) b = (uint8_t)rng();
  for (int p = k; p < k + m; ++p)
    for (size_t x = 0; x < len; ++x) {
      uint8_t acc = 0;
      for (int c = 0; c < k; ++c) acc ^= gf_mul(E->v[p][c], s.cw[c][x]);
      s.cw[p][x] = acc;
    }
  return s;
}

// exact-size copies, so a read past a shard's end is seen
struct Held {
  std::vector<std::unique_ptr<uint8_t[]>> own;
  std::vector<const uint8_t*> ptr;
};
static Held view(const Segment& s, const std::vector<uint8_t>& held) {
  Held v;
  for (int i = 0; i < s.k + s.m; ++i) {
    if (!held[i]) {
      v.own.emplace_back();
      v.ptr.push_back(nullptr);
      continue;
    }
    v.own.emplace_back(new uint8_t[s.len]);
    std::memcpy(v.own.back().get(), s.cw[i].data(), s.len);
    v.ptr.push_back(v.own.back().get());
  }
  return v;
}

struct Result {
  uint32_t st;
  int nfound, found[2];
};
static Result run(const Segment& s, const Held& v, int nsyn, int max_bad) {
  Result r{9, 9, {9, 9}};
  loc2_segment_host((uint32_t)s.k, (uint32_t)(s.k + s.m), v.ptr.data(), s.len, (uint32_t)nsyn,
                    (uint32_t)max_bad, &r.st, &r.nfound, r.found);
  return r;
}
static bool found_is(const Result& r, int a, int b) {
  return r.st == kLocFound && r.nfound == (b < 0 ? 1 : 2) && r.found[0] == a && r.found[1] == b;
}
static bool ambiguous(const Result& r) {
  return r.st == kLocAmbiguous && r.nfound == 0 && r.found[0] == -1 && r.found[1] == -1;
}

static uint8_t nz(std::mt19937& rng) { return (uint8_t)(1 + rng() % 255); }

// shape 0: both whole; 1: one byte each, a first; 2: b first; 3: one offset; 4: S_0 cancels
static void corrupt_pair(const Segment& s, Held& w, const uint8_t* H, uint32_t hh, uint32_t ta,
                         uint32_t tb, int shape, std::mt19937& rng) {
  uint8_t* a = w.own[H[ta]].get();
  uint8_t* b = w.own[H[tb]].get();
  const size_t x = rng() % s.len, y = s.len > 1 ? (x + 1 + rng() % (s.len - 1)) % s.len : x;
  const size_t lo = x < y ? x : y, hi = x < y ? y : x;
  if (shape == 0) {
    for (size_t i = 0; i < s.len; ++i) a[i] ^= nz(rng), b[i] ^= nz(rng);
  } else if (shape == 1) {
    a[lo] ^= nz(rng), b[hi] ^= nz(rng);
  } else if (shape == 2) {
    b[lo] ^= nz(rng), a[hi] ^= nz(rng);
  } else if (shape == 3) {
    a[x] ^= nz(rng), b[x] ^= nz(rng);
  } else {
    const uint32_t ratio = fs_mul(loc_u(H, hh, ta), fs_inv(loc_u(H, hh, tb)));
    for (size_t i = 0; i < s.len; ++i) {
      const uint8_t e = i == x ? nz(rng) : (uint8_t)rng();
      a[i] ^= e;
      b[i] ^= (uint8_t)fs_mul(ratio, e);
    }
  }
}

static void sweep(int k, int m, size_t len, std::mt19937& rng) {
  const int n = k + m;
  const Segment s = make_segment(k, m, len, rng);
  for (int h : {n, k + 4, k + 3, k + 2, k + 1, k}) {
    if (h > n) continue;
    std::vector<uint8_t> held(n, 0);
    {
      std::vector<int> idx(n);
      for (int i = 0; i < n; ++i) idx[i] = i;
      for (int i = 0; i < h; ++i) std::swap(idx[i], idx[i + rng() % (n - i)]);
      for (int i = 0; i < h; ++i) held[idx[i]] = 1;
    }
    uint8_t H[256];
    uint32_t hh = 0;
    for (int i = 0; i < n; ++i)
      if (held[i]) H[hh++] = (uint8_t)i;
    const uint32_t r = loc_r(hh, (uint32_t)k, kLocateSynMax);
    // the four-row table in a buffer of exactly its stated size, against the two-row one
    {
      std::unique_ptr<uint8_t[]> set(new uint8_t[loc2_set_bytes((uint32_t)n)]);
      std::unique_ptr<uint8_t[]> set1(new uint8_t[loc_set_bytes((uint32_t)n)]);
      loc2_put_set(set.get(), held.data(), (uint32_t)n, r);
      loc_put_set(set1.get(), held.data(), (uint32_t)n, r);
      CHECK(loc_set_h(set.get()) == hh && loc_set_r(set.get()) == r);
      CHECK(std::memcmp(set.get(), set1.get(), kLocSetHead) == 0);
      for (uint32_t t = 0; t < hh; ++t) {
        CHECK(loc2_set_idx(set.get())[t] == H[t]);
        for (uint32_t a = 0; a < 4; ++a)
          CHECK(loc2_set_coef(set.get(), (uint32_t)n, a)[t] ==
                (a < r ? (loc_column(H, hh, t) >> (8 * a)) & 0xFFu : 0u));
      }
      for (int i = 0; i < n; ++i) CHECK(loc2_set_pos(set.get(), (uint32_t)n)[i] == held[i]);
    }
    Held v = view(s, held);
    Result res = run(s, v, 4, 2);
    CHECK(res.st == (h <= k ? kLocUnchecked : kLocClean) && res.nfound == 0 && res.found[0] == -1);
    if (hh < 2 || r == 0) continue;
    // one bad shard: found for r >= 2 under both max_bad
    for (int trial = 0; trial < 4; ++trial) {
      const uint32_t t = trial == 0 ? 0 : rng() % hh;
      Held w = view(s, held);
      if (trial & 1) {
        for (size_t x = 0; x < s.len; ++x) w.own[H[t]].get()[x] ^= nz(rng);
      } else {
        w.own[H[t]].get()[rng() % s.len] ^= nz(rng);
      }
      for (int max_bad = 1; max_bad <= 2; ++max_bad) {
        res = run(s, w, 4, max_bad);
        if (r == 1) CHECK(ambiguous(res));
        else CHECK(found_is(res, H[t], -1));
      }
    }
    // two bad shards, every shape
    for (int trial = 0; trial < 10; ++trial) {
      uint32_t ta = trial < 5 ? 0 : rng() % hh, tb = (ta + 1 + rng() % (hh - 1)) % hh;
      if (ta > tb) std::swap(ta, tb);
      const int shape = trial % 5;
      if (s.len < 2 && (shape == 1 || shape == 2)) continue;
      Held w = view(s, held);
      corrupt_pair(s, w, H, hh, ta, tb, shape, rng);
      res = run(s, w, 4, 2);
      if (r == 4) CHECK(found_is(res, H[ta], H[tb]));
      else if (r == 1 && shape == 4) CHECK(res.st == kLocClean);  // the one check is S_0
      else if (r == 3 || shape != 3) CHECK(ambiguous(res) || (r == 2 && s.len == 1));
      else CHECK(res.nfound <= 1);
      res = run(s, w, 4, 1);  // the single rule: never two
      CHECK(res.nfound <= 1 && (r < 3 || ambiguous(res)));  // two are past the single rule
      if (r == 4) {  // fewer checks asked for
        res = run(s, w, 3, 2);
        CHECK(ambiguous(res));
      }
    }
    // three bad shards: whatever the verdict, it is well-formed
    for (int trial = 0; trial < 4 && hh >= 3; ++trial) {
      Held w = view(s, held);
      const size_t x = rng() % s.len;
      const uint32_t t0 = rng() % hh;
      for (uint32_t d = 0; d < 3; ++d) w.own[H[(t0 + d) % hh]].get()[x] ^= nz(rng);
      res = run(s, w, 4, 2);
      CHECK(res.st == kLocAmbiguous || res.st == kLocFound);
      CHECK(res.st == kLocFound ? (res.nfound >= 1 && res.found[0] >= 0) : ambiguous(res));
    }
  }
}

int main() {
  std::mt19937 rng(20261022);
  // the candidate word
  CHECK(loc2_nbad(kLocNone) == 0 && loc2_nbad(loc2_pack1(0)) == 1 && loc2_nbad(loc2_pack2(0, 7)) == 2);
  CHECK(loc2_j0(loc2_pack1(255)) == 255 && loc2_j1(loc2_pack1(255)) == 255);
  CHECK(loc2_pack1(255) != kLocNone && loc2_pack2(255, 254) != kLocNone);
  CHECK(loc2_sigma1(loc2_pack2(3, 5)) == 6 && loc2_sigma2(loc2_pack2(3, 5)) == fs_mul(3, 5));
  CHECK(loc2_sigma2(loc2_pack2(0, 9)) == 0 && loc2_is_root(0, 9 | 0 << 8) && loc2_is_root(9, 9));
  // the status table and the flags
  CHECK(loc2_status(4, 4, true, loc2_pack1(1), false, false) == kLocUnchecked);
  CHECK(loc2_status(8, 4, false, kLocNone, false, false) == kLocClean);
  CHECK(loc2_status(8, 4, true, kLocNone, false, false) == kLocAmbiguous);
  CHECK(loc2_status(8, 4, true, loc2_pack1(3), false, false) == kLocFound);
  CHECK(loc2_status(8, 4, true, loc2_pack1(3), true, false) == kLocAmbiguous);
  CHECK(loc2_status(8, 4, true, loc2_pack2(3, 0), true, false) == kLocFound);
  CHECK(loc2_status(8, 4, true, loc2_pack2(3, 0), true, true) == kLocAmbiguous);
  const uint32_t pr = loc2_pack2(3, 0);
  CHECK(loc2_flag(kLocFound, true, 3, pr) == 0 && loc2_flag(kLocFound, true, 0, pr) == 0);
  CHECK(loc2_flag(kLocFound, true, 2, pr) == 1 && loc2_flag(kLocFound, false, 2, pr) == 0);
  CHECK(loc2_flag(kLocFound, true, 0, loc2_pack1(3)) == 1);
  CHECK(loc2_flag(kLocAmbiguous, true, 2, kLocNone) == 0 && loc2_flag(kLocClean, true, 255, kLocNone) == 1);
  CHECK(loc2_pair_rule(4, 2) && !loc2_pair_rule(3, 2) && !loc2_pair_rule(4, 1));
  const int codes[][2] = {{4, 4}, {10, 4}, {2, 4}, {4, 5}, {4, 2}, {32, 32}, {200, 56}};
  for (auto& km : codes)
    for (size_t len : {(size_t)1, (size_t)2, (size_t)7, (size_t)40}) {
      if (km[0] + km[1] > 64 && len != 7) continue;
      sweep(km[0], km[1], len, rng);
    }
  if (g_fail) {
    std::printf("locate_multi_model: %d failures\n", g_fail);
    return 1;
  }
  std::printf("locate_multi_model ok\n");
  return 0;
}
