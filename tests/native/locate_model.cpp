// The rule of cec_locate_ptrs (csrc/locate_rule.h) in a program of its own, built with
// -fsanitize=address,undefined by tests/test_locate_rule.py: codewords from gf256.h's encode
// matrix, the check rows against them, every held shard as the single bad one, the held-set edges,
// two bad shards under three checks, and the set table and program chunk the host uploads, written
// into buffers of exactly their stated sizes.
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../cess_amd/csrc/gf256.h"
#include "../../cess_amd/csrc/locate_rule.h"

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
  std::vector<std::vector<uint8_t>> cw;  // the codeword, every shard
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

static std::vector<uint8_t> random_held(int n, int h, std::mt19937& rng) {
  std::vector<int> idx(n);
  for (int i = 0; i < n; ++i) idx[i] = i;
  for (int i = 0; i < h; ++i) std::swap(idx[i], idx[i + rng() % (n - i)]);
  std::vector<uint8_t> held(n, 0);
  for (int i = 0; i < h; ++i) held[idx[i]] = 1;
  return held;
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

static void run(const Segment& s, const Held& v, int nsyn, uint32_t* st, int* found) {
  loc_segment_host((uint32_t)s.k, (uint32_t)(s.k + s.m), v.ptr.data(), s.len, (uint32_t)nsyn, st,
                   found);
}

static void sweep(int k, int m, std::mt19937& rng) {
  const int n = k + m;
  const Segment s = make_segment(k, m, 19, rng);
  for (int h : {n, k + 2, k + 1, k}) {
    if (h > n) continue;
    const std::vector<uint8_t> held = random_held(n, h, rng);
    uint8_t H[256];
    uint32_t hh = 0;
    for (int i = 0; i < n; ++i)
      if (held[i]) H[hh++] = (uint8_t)i;
    const uint32_t r = loc_r(hh, (uint32_t)k, kLocateSynMax);
    CHECK(r == (uint32_t)(h <= k ? 0 : h - k < 4 ? h - k : 4));
    // the check rows annihilate the codeword
    for (uint32_t a = 0; a < r; ++a)
      for (size_t x = 0; x < s.len; ++x) {
        uint32_t acc = 0;
        for (uint32_t t = 0; t < hh; ++t)
          acc ^= fs_mul((loc_column(H, hh, t) >> (8 * a)) & 0xFFu, s.cw[H[t]][x]);
        CHECK(acc == 0);
      }
    // the uploads, in buffers of exactly their stated sizes
    {
      std::unique_ptr<uint8_t[]> set(new uint8_t[loc_set_bytes((uint32_t)n)]);
      loc_put_set(set.get(), held.data(), (uint32_t)n, r);
      CHECK(loc_set_h(set.get()) == hh && loc_set_r(set.get()) == r);
      for (uint32_t t = 0; t < hh; ++t) {
        CHECK(set[kLocSetHead + t] == H[t]);
        CHECK(set[kLocSetHead + n + t] == (loc_column(H, hh, t) & 0xFFu));
        CHECK(set[kLocSetHead + 2 * n + t] == ((loc_column(H, hh, t) >> 8) & 0xFFu));
      }
      for (int i = 0; i < n; ++i) CHECK(set[kLocSetHead + 3 * n + i] == held[i]);
      if (r) {
        const uint32_t words = fs_chunk_words(hh, r);
        std::unique_ptr<uint32_t[]> chunk(new uint32_t[words]);
        std::memset(chunk.get(), 0xAB, words * sizeof(uint32_t));
        loc_put_chunk(chunk.get(), H, hh, r);
        CHECK(chunk[0] == hh && chunk[1] == r && chunk[2] == r && chunk[3] == 0);
        for (uint32_t t = 0; t < hh; ++t)
          for (uint32_t b = 0; b < 8; ++b)
            for (uint32_t o = 0; o < r; ++o)
              CHECK(chunk[kFsHeaderWords + (t * 8 + b) * r + o] ==
                    0u - ((loc_column(H, hh, t) >> (8 * o + b)) & 1u));
      }
    }
    uint32_t st = 9;
    int found = 9;
    Held v = view(s, held);
    run(s, v, kLocateSynMax, &st, &found);
    CHECK(st == (h <= k ? kLocUnchecked : kLocClean) && found == -1);
    // every held shard as the single bad one: one bit, or the whole shard
    for (uint32_t t = 0; t < hh; ++t) {
      if (n > 64 && H[t] != 0 && H[t] < k && t % 23) continue;  // shard 0, parity, a sample
      Held w = view(s, held);
      uint8_t* bad = w.own[H[t]].get();
      if (t & 1) {
        for (size_t x = 0; x < s.len; ++x) bad[x] ^= (uint8_t)(1 + rng() % 255);
      } else {
        bad[rng() % s.len] ^= (uint8_t)(1u << (rng() % 8));
      }
      for (int nsyn = 1; nsyn <= kLocateSynMax; ++nsyn) {
        run(s, w, nsyn, &st, &found);
        const uint32_t rr = loc_r(hh, (uint32_t)k, (uint32_t)nsyn);
        if (rr == 0) CHECK(st == kLocUnchecked && found == -1);
        else if (rr == 1) CHECK(st == kLocAmbiguous && found == -1);
        else CHECK(st == kLocFound && found == (int)H[t]);
      }
    }
    // two bad shards at one byte offset: never FOUND with three or more checks
    if (r >= 3)
      for (int trial = 0; trial < 8; ++trial) {
        Held w = view(s, held);
        const uint32_t a = rng() % hh, b = (a + 1 + rng() % (hh - 1)) % hh;
        const size_t x = rng() % s.len;
        w.own[H[a]].get()[x] ^= (uint8_t)(1 + rng() % 255);
        w.own[H[b]].get()[x] ^= (uint8_t)(1 + rng() % 255);
        for (int nsyn = 3; nsyn <= kLocateSynMax; ++nsyn) {
          run(s, w, nsyn, &st, &found);
          CHECK(st == kLocAmbiguous && found == -1);
        }
      }
  }
}

int main() {
  std::mt19937 rng(20261021);
  // the status table and the flags
  CHECK(loc_status(4, 4, 0, true, 1, false) == kLocUnchecked);
  CHECK(loc_status(6, 4, 2, false, kLocNone, false) == kLocClean);
  CHECK(loc_status(6, 4, 2, true, 3, false) == kLocFound);
  CHECK(loc_status(6, 4, 2, true, 3, true) == kLocAmbiguous);
  CHECK(loc_status(6, 4, 2, true, kLocNone, false) == kLocAmbiguous);
  CHECK(loc_status(5, 4, 1, true, 3, false) == kLocAmbiguous);
  CHECK(loc_flag(kLocFound, true, 3, 3) == 0 && loc_flag(kLocFound, true, 2, 3) == 1);
  CHECK(loc_flag(kLocFound, false, 2, 3) == 0 && loc_flag(kLocAmbiguous, true, 2, kLocNone) == 0);
  CHECK(loc_flag(kLocClean, true, 0, kLocNone) == 1 && loc_flag(kLocUnchecked, true, 0, 0) == 1);
  CHECK(loc_pow(0, 0) == 1 && loc_pow(0, 1) == 0 && loc_pow(2, 8) == 0x1D);
  const int codes[][2] = {{2, 1}, {2, 2}, {4, 2}, {10, 4}, {17, 3}, {32, 32}, {200, 56}};
  for (auto& km : codes) sweep(km[0], km[1], rng);
  if (g_fail) {
    std::printf("locate_model: %d failures\n", g_fail);
    return 1;
  }
  std::printf("locate_model ok\n");
  return 0;
}
