// The read planner's pieces (cess_amd/csrc/read_plan.h) on a CPU, built with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_read_solve.py. Cases come on stdin, one per line:
// "k m max_bad", then the n = k + m held bytes, the n flag bytes and the k wanted bytes, all
// decimal. Shard i, when held, lies at address 0x1000 * (i + 1); data shard j, when wanted, goes
// to 0x100000 + 0x1000 * j; the chunk's address is 0xC0000. Every buffer is a heap block of
// exactly its documented size, so the sanitizer's red zones stand around it: out_idx e bytes,
// in_idx k, rows e * k, copy_idx k, the chunk fs_chunk_words(k, e) words, the copy rows
// k * kRpCopyWords words, bucket b's row rp_row_words(k, b). Printed per case: status, output
// count and copy count; the copy indices; the copy rows; the four bucket rows (hex words; a word
// the planner left alone prints as its fill); for a rebuild out / in / rows and of the chunk the
// header, hb[0..k) and the mask words. RS(2,1) cases also print rp_plan21's status, row and copy
// rows over the same addresses.
#include <cstdio>
#include <memory>
#include <vector>

#include "../../cess_amd/csrc/read_plan.h"

int main() {
  constexpr uint64_t kFill64 = 0xDEADBEEFDEADBEEFull;
  constexpr uint32_t kFill = 0xDEADBEEFu;
  int k, m, max_bad;
  while (std::scanf("%d %d %d", &k, &m, &max_bad) == 3) {
    const int n = k + m;
    std::vector<uint8_t> held(n), flags(n), wanted(k);
    for (int pass = 0; pass < 3; ++pass)
      for (int i = 0; i < (pass == 2 ? k : n); ++i) {
        int v;
        if (std::scanf("%d", &v) != 1) return 2;
        (pass == 0 ? held : pass == 1 ? flags : wanted)[i] = (uint8_t)v;
      }
    std::unique_ptr<uint64_t[]> seg(new uint64_t[n]), dst(new uint64_t[k]);
    for (int i = 0; i < n; ++i) seg[i] = held[i] ? 0x1000ull * (i + 1) : 0;
    for (int j = 0; j < k; ++j) dst[j] = wanted[j] ? 0x100000ull + 0x1000ull * j : 0;
    uint32_t st = 0, e = 0, nc = 0;
    cec::rp_plan_segment(k, n, held.data(), flags.data(), wanted.data(), max_bad, &st, &e, nullptr,
                         nullptr, nullptr, nullptr, nullptr, &nc, nullptr);
    std::unique_ptr<uint8_t[]> out(new uint8_t[e ? e : 1]), in(new uint8_t[k]),
        rows(new uint8_t[e ? (size_t)e * k : 1]), cidx(new uint8_t[k]);
    const size_t words = e ? cec::fs_chunk_words(k, e) : 0;
    std::unique_ptr<uint32_t[]> chunk(new uint32_t[words ? words : 1]);
    for (size_t w = 0; w < words; ++w) chunk[w] = kFill;
    const size_t cw = (size_t)k * cec::kRpCopyWords;
    std::unique_ptr<uint64_t[]> copy(new uint64_t[cw]);
    for (size_t w = 0; w < cw; ++w) copy[w] = kFill64;
    std::unique_ptr<uint64_t[]> bucket[cec::kFlagMultiMax];
    cec::RpTables tab{};
    tab.seg = seg.get();
    tab.dst = dst.get();
    tab.copy_rows = copy.get();
    tab.chunk_addr = 0xC0000;
    for (int b = 1; b <= cec::kFlagMultiMax; ++b) {
      const uint32_t rw = cec::rp_row_words(k, b);
      bucket[b - 1].reset(new uint64_t[rw]);
      for (uint32_t w = 0; w < rw; ++w) bucket[b - 1][w] = kFill64;
      tab.bucket_rows[b - 1] = bucket[b - 1].get();
    }
    uint32_t st2 = 0, e2 = 0, nc2 = 0;
    cec::rp_plan_segment(k, n, held.data(), flags.data(), wanted.data(), max_bad, &st2, &e2,
                         out.get(), in.get(), rows.get(), e ? chunk.get() : nullptr, cidx.get(),
                         &nc2, &tab);
    if (st2 != st || e2 != e || nc2 != nc) return 3;
    std::printf("status %u %u %u\ncidx", st, e, nc);
    for (uint32_t c = 0; c < nc; ++c) std::printf(" %u", cidx[c]);
    std::printf("\ncrow");
    for (size_t w = 0; w < cw; ++w) std::printf(" %llx", (unsigned long long)copy[w]);
    for (int b = 1; b <= cec::kFlagMultiMax; ++b) {
      std::printf("\nb%d", b);
      for (uint32_t w = 0; w < cec::rp_row_words(k, b); ++w)
        std::printf(" %llx", (unsigned long long)bucket[b - 1][w]);
    }
    std::printf("\n");
    if (k == 2 && m == 1) {
      std::unique_ptr<uint64_t[]> row21(new uint64_t[cec::kRp21RowWords]),
          copy21(new uint64_t[2 * cec::kRpCopyWords]);
      const uint32_t s21 =
          cec::rp_plan21(seg.get(), flags.data(), dst.get(), max_bad, row21.get(), copy21.get());
      std::printf("p21 %u", s21);
      for (uint32_t w = 0; w < cec::kRp21RowWords; ++w)
        std::printf(" %llx", (unsigned long long)row21[w]);
      for (uint32_t w = 0; w < 2 * cec::kRpCopyWords; ++w)
        std::printf(" %llx", (unsigned long long)copy21[w]);
      std::printf("\n");
    }
    if (!e) continue;
    std::printf("out");
    for (uint32_t o = 0; o < e; ++o) std::printf(" %u", out[o]);
    std::printf("\nin");
    for (int t = 0; t < k; ++t) std::printf(" %u", in[t]);
    for (uint32_t o = 0; o < e; ++o) {
      std::printf("\nrow");
      for (int t = 0; t < k; ++t) std::printf(" %u", rows[(size_t)o * k + t]);
    }
    const uint32_t* c = chunk.get();
    bool clean = true;  // the chunk words the planner must not write
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
