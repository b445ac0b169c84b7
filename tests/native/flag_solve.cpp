// The planner's arithmetic and chunk writer (cess_amd/csrc/flag_solve.h) on a CPU, built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_flag_solve.py. Cases come on stdin,
// one per line: "k m max_bad" and then the n = k + m held bytes and the n flag bytes, all decimal.
// Every case is planned twice: into a heap block of exactly fs_chunk_words(k, e) words (the
// sanitizer's red zones stand around it) and into the middle of a block with 64 guard words on
// either side. Printed per case: status and output count, out / in indices, the rows, and of the
// chunk the header, hb[0..k) and the k * 8 * e mask words; "clean 1" when the guards, and the
// chunk words the planner must not write (the in / out index arrays, hb past k), kept their fill.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../cess_amd/csrc/flag_solve.h"

int main() {
  constexpr uint32_t kFill = 0xDEADBEEFu, kGuard = 64;
  int k, m, max_bad;
  while (std::scanf("%d %d %d", &k, &m, &max_bad) == 3) {
    const int n = k + m;
    std::vector<uint8_t> held(n), flags(n);
    for (int pass = 0; pass < 2; ++pass)
      for (int i = 0; i < n; ++i) {
        int v;
        if (std::scanf("%d", &v) != 1) return 2;
        (pass ? flags : held)[i] = (uint8_t)v;
      }
    uint32_t st = 0, e = 0;
    // exact sizes: in_idx k bytes, rows e * k, out_idx e, so any overrun meets a red zone
    cec::fs_plan_segment(k, n, held.data(), flags.data(), max_bad, &st, &e, nullptr, nullptr,
                         nullptr, nullptr);
    std::unique_ptr<uint8_t[]> out(new uint8_t[e ? e : 1]), in(new uint8_t[k]),
        rows(new uint8_t[e ? (size_t)e * k : 1]);
    const size_t words = e ? cec::fs_chunk_words(k, e) : 0;
    std::unique_ptr<uint32_t[]> exact(new uint32_t[words ? words : 1]);
    std::vector<uint32_t> guarded(words + 2 * kGuard, kFill);
    for (size_t w = 0; w < words; ++w) exact[w] = kFill;
    uint32_t st2 = 0, e2 = 0;
    cec::fs_plan_segment(k, n, held.data(), flags.data(), max_bad, &st2, &e2, out.get(), in.get(),
                         rows.get(), e ? exact.get() : nullptr);
    cec::fs_plan_segment(k, n, held.data(), flags.data(), max_bad, &st2, &e2, nullptr, nullptr,
                         nullptr, e ? guarded.data() + kGuard : nullptr);
    if (st2 != st || e2 != e) return 3;
    std::printf("status %u %u\n", st, e);
    if (!e) continue;
    std::printf("out");
    for (uint32_t o = 0; o < e; ++o) std::printf(" %u", out[o]);
    std::printf("\nin");
    for (int t = 0; t < k; ++t) std::printf(" %u", in[t]);
    for (uint32_t o = 0; o < e; ++o) {
      std::printf("\nrow");
      for (int t = 0; t < k; ++t) std::printf(" %u", rows[(size_t)o * k + t]);
    }
    const uint32_t* c = exact.get();
    bool clean = std::memcmp(c, guarded.data() + kGuard, words * sizeof(uint32_t)) == 0;
    for (uint32_t g = 0; g < kGuard; ++g)
      clean = clean && guarded[g] == kFill && guarded[kGuard + words + g] == kFill;
    for (uint32_t w = 4; w < cec::kFsHbWord; ++w) clean = clean && c[w] == kFill;
    for (uint32_t w = cec::kFsHbWord + k; w < cec::kFsHeaderWords; ++w)
      clean = clean && c[w] == kFill;
    std::printf("\nhdr %u %u %u %u\nhb", c[0], c[1], c[2], c[3]);
    for (int t = 0; t < k; ++t) std::printf(" %u", c[cec::kFsHbWord + t]);
    std::printf("\nmask");
    for (size_t w = cec::kFsHeaderWords; w < words; ++w) std::printf(" %x", c[w]);
    std::printf("\nclean %d\n", clean ? 1 : 0);
  }
  return 0;
}
