// The placement arithmetic of k_hashq_admit (cess_amd/csrc/hashq_where.h) on a CPU, built under
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_hashq_where_plan.py. The buffers have
// exactly the sizes the plan is given, on the heap, so a read or write past them is reported.
//
// stdin, one case per line:  n per gate gated  held...  flags...  gate_bytes...
// (n bytes each of held and flags, ceil(n / per) gate bytes when gated is 1, as decimal numbers).
// stdout per case:  nsel pos...
// A line "rule status ok..." prints confirm_rule's code for that segment instead.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../cess_amd/csrc/hashq_where.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    if (line.rfind("rule", 0) == 0) {
      std::string word;
      unsigned status = 0, v = 0, zeros = 0, ones = 0;
      in >> word >> status;
      while (in >> v) {
        zeros += v == 0;
        ones += v == 1;
      }
      std::printf("%u\n", cec::confirm_rule(status == 1, zeros, ones));
      continue;
    }
    size_t n = 0, per = 0;
    unsigned gate = 0, gated = 0, v = 0;
    if (!(in >> n >> per >> gate >> gated)) continue;
    std::vector<uint8_t> held(n), flags(n), gates(gated ? (n + per - 1) / per : 0);
    for (auto* vec : {&held, &flags, &gates})
      for (auto& b : *vec) {
        in >> v;
        b = (uint8_t)v;
      }
    std::vector<uint32_t> pos(n, 0xEEEEEEEEu);
    size_t nsel = ~(size_t)0;
    cec::where_plan(held.data(), flags.data(), n, per, gated ? gates.data() : nullptr, gate,
                    pos.data(), &nsel);
    std::printf("%zu", nsel);
    for (uint32_t p : pos) std::printf(" %u", p);
    std::printf("\n");
  }
  return 0;
}
