// The hash queue's bookkeeping (hashq.cpp): which adds hold which slots of the ring, how far the
// ticks have taken them, and how a tick is cut into launches. Host arithmetic only: no HIP, no
// locks, so it is checked on a CPU (tests/native/hashq_ring.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <deque>
#include <utility>
#include <vector>

namespace cec {

struct HashqRing {
  struct Add {
    uint64_t slot0, n, blocks, done, ticket;
    // concat adds (cec_hashq_add_concat_ptrs): chains of `parts` buffers of part_blocks blocks
    // each, the queue's copy of their n * parts addresses (chain-major). parts == 0: a plain add.
    uint64_t parts = 0, part_blocks = 0;
    std::vector<const uint8_t*> ptrs;
  };
  std::deque<Add> adds;  // adds not yet complete, in slot order
  uint64_t cap = 0;
  uint64_t head = 0, tail = 0;  // absolute slot numbers; live slots are [head, tail)
  uint64_t next_ticket = 1;

  bool room(uint64_t n) const { return tail + n - head <= cap; }

  // List n chains of `blocks` blocks in slots tail..; the add's ticket.
  uint64_t push(uint64_t n, uint64_t blocks, uint64_t parts = 0, uint64_t part_blocks = 0,
                std::vector<const uint8_t*> ptrs = {}) {
    adds.push_back({tail, n, blocks, 0, next_ticket, parts, part_blocks, std::move(ptrs)});
    tail += n;
    return next_ticket++;
  }

  // an add is complete once it is no longer listed (tickets are increasing along the deque)
  bool done(uint64_t ticket) const {
    for (const auto& a : adds)
      if (a.ticket == ticket) return a.done == a.blocks;
    return ticket < next_ticket;
  }
  uint64_t live_chains() const {
    uint64_t live = 0;
    for (const auto& a : adds)
      if (a.done < a.blocks) live += a.n;
    return live;
  }
  uint64_t blocks_left() const {
    uint64_t left = 0;
    for (const auto& a : adds) left = std::max(left, a.blocks - a.done);
    return left;
  }
  // max_blocks of a drain: enough to complete every live chain (a tick counts in 32 bits)
  uint32_t drain_blocks() const { return (uint32_t)std::min<uint64_t>(blocks_left(), 0xFFFFFFFFull); }

  // Blocks until the chains of a concat add stand at the start of a part other than their first
  // (0: none ahead; the last part needs no boundary after it, its tail and the padding blocks are
  // read, or not read, by the ticks as for any chain).
  static uint64_t to_boundary(const Add& a) {
    if (a.parts < 2 || a.done == a.blocks) return 0;
    const uint64_t p = a.done / a.part_blocks + 1;
    return p < a.parts ? p * a.part_blocks - a.done : 0;
  }

  // The next launch of a tick with `left` blocks still to issue: slots head.. (span of them), `live`
  // chains among them, step blocks. The tick kernels read a chain as flat src + blk * 64, so no
  // launch may take a concat chain across a part boundary: the step is cut at the nearest one over
  // all live concat adds.
  struct Launch {
    uint64_t head;
    uint32_t span, step;
    uint64_t live;
  };
  Launch next(uint64_t left) const {
    uint64_t step = left;
    for (const auto& a : adds)
      if (const uint64_t b = to_boundary(a)) step = std::min(step, b);
    return {head, (uint32_t)(tail - head), (uint32_t)step, live_chains()};
  }

  // After that launch: every add is `step` blocks further (or complete). rebase(add, p) is called
  // for each concat add that now stands at the start of its part p, which its chains have to be
  // pointed at before the next launch; a non-zero result ends the call at once and is returned.
  // Completed adds then retire from the front, so the tick range starts at the oldest live chain.
  template <class F>
  int advance(uint64_t step, F rebase) {
    for (auto& a : adds) {
      const uint64_t adv = std::min(step, a.blocks - a.done);
      a.done += adv;
      if (adv && a.parts > 1 && a.done % a.part_blocks == 0 && a.done / a.part_blocks < a.parts)
        if (int rc = rebase(a, a.done / a.part_blocks)) return rc;
    }
    while (!adds.empty() && adds.front().done == adds.front().blocks) adds.pop_front();
    head = adds.empty() ? tail : adds.front().slot0;
    return 0;
  }
};

}  // namespace cec
