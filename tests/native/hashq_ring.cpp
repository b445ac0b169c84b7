// The hash queue's ring (cess_amd/csrc/hashq_ring.h) on a CPU, under AddressSanitizer +
// UndefinedBehaviorSanitizer: built and run by tests/test_hashq_ring.py, which compares what this
// prints with a Python model. It drives the ring the way hashq.cpp does, without the launches.
//   hashq_ring CAPACITY < operations, one per line:
//     add n blocks parts part_blocks    n chains of `blocks` blocks, over `parts` buffers of
//                                       part_blocks blocks each (parts <= 1: a plain add)
//     tick T                            at most T blocks per chain (0: drain)
// Printed per operation: "ticket t" or "refused" for an add; for a tick one "launch head span step
// live" per launch, each followed by its "rebase ticket part" lines; then "state head tail live
// left" and "done" with one digit per ticket 0..next_ticket.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cess_amd/csrc/hashq_ring.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  cec::HashqRing r;
  r.cap = std::strtoull(argv[1], nullptr, 10);
  char line[256];
  while (std::fgets(line, sizeof line, stdin)) {
    unsigned long long n, blocks, parts, part_blocks, T;
    if (std::sscanf(line, "add %llu %llu %llu %llu", &n, &blocks, &parts, &part_blocks) == 4) {
      if (n == 0) {
        std::printf("ticket 0\n");
      } else if (!r.room(n)) {
        std::printf("refused\n");
      } else if (parts > 1) {  // addresses the ring keeps and never reads
        std::vector<const uint8_t*> ptrs(n * parts, reinterpret_cast<const uint8_t*>(64));
        std::printf("ticket %llu\n",
                    (unsigned long long)r.push(n, blocks, parts, part_blocks, std::move(ptrs)));
      } else {
        std::printf("ticket %llu\n", (unsigned long long)r.push(n, blocks));
      }
    } else if (std::sscanf(line, "tick %llu", &T) == 1) {
      if (!r.adds.empty()) {
        if (T == 0) T = r.drain_blocks();
        for (uint64_t left = T; left && !r.adds.empty();) {
          const cec::HashqRing::Launch l = r.next(left);
          std::printf("launch %llu %u %u %llu\n", (unsigned long long)l.head, l.span, l.step,
                      (unsigned long long)l.live);
          if (l.step == 0 || l.step > left) return 3;  // the loop would not end
          r.advance(l.step, [](const cec::HashqRing::Add& a, uint64_t p) {
            if (a.ptrs.size() != a.n * a.parts || p >= a.parts) std::abort();
            std::printf("rebase %llu %llu\n", (unsigned long long)a.ticket, (unsigned long long)p);
            return 0;
          });
          left -= l.step;
        }
      }
    } else {
      std::fprintf(stderr, "bad line: %s", line);
      return 2;
    }
    std::printf("state %llu %llu %llu %llu\ndone ", (unsigned long long)r.head,
                (unsigned long long)r.tail, (unsigned long long)r.live_chains(),
                (unsigned long long)r.blocks_left());
    for (uint64_t t = 0; t <= r.next_ticket; ++t) std::putchar(r.done(t) ? '1' : '0');
    std::putchar('\n');
  }
  return 0;
}
