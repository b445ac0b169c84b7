// Chains the device admits (cec_hashq_add_check_where_ptrs): the rule and the placement arithmetic
// of the admit kernel k_hashq_admit (sha256.hip), as host and device inline functions without HIP
// types, so what the kernel compiles is checked on a CPU (tests/native/hashq_where.cpp,
// tests/test_hashq_where_plan.py). The rule of cec_confirm_flagged (k_confirm_flagged,
// kernels.hip) stands here too.
//
// A tick wave costs the same with one live lane as with 64, so sparse admission alone saves
// nothing: the admitted chains of an add are packed into its front slots and the others are
// parked (complete from the start) in its back slots. With n chains, the j-th admitted one in
// index order takes slot offset j, the j-th one not admitted n - 1 - j. The add runs as launches
// of one workgroup over chunks of kWhereChunk chains in index order, on one stream: a launch
// ranks its chains within each wave of kWhereWave from a ballot, sums the waves before it, and
// adds the totals its predecessors left. No atomic, and the same placement every run.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CEC_HW_HD __host__ __device__ inline
#else
#define CEC_HW_HD inline
#endif

namespace cec {

constexpr uint32_t kWhereChunk = 256;  // chains per launch: the addresses of one argument block
constexpr uint32_t kWhereWave = 64;
constexpr uint32_t kWhereWaves = kWhereChunk / kWhereWave;

// d_ok of a chain that was not admitted (CEC_HASHQ_SKIPPED) and the codes of cec_confirm_flagged
// (CEC_CONFIRM_*), asserted equal where cess_ec.h is in sight.
constexpr uint32_t kWhereSkipped = 2;
constexpr uint32_t kConfirmNone = 0, kConfirmProven = 1, kConfirmRefuted = 2;

// The rule: a chain with a buffer, whose flag byte is zero and whose group's gate byte (if the
// add has gate bytes) equals `gate`.
CEC_HW_HD bool where_admit(bool has_buf, uint32_t flag, bool gated, uint32_t gate_byte,
                           uint32_t gate) {
  return has_buf && flag == 0 && (!gated || gate_byte == gate);
}

CEC_HW_HD uint32_t where_count(uint64_t ballot) { return (uint32_t)__builtin_popcountll(ballot); }
// Lanes of a wave below `lane` whose bit is set in the wave's ballot: what mbcnt gives the device.
CEC_HW_HD uint32_t where_rank(uint64_t ballot, uint32_t lane) {
  return where_count(ballot & ((1ull << lane) - 1));
}

// Admitted chains of the chunk in the waves before `wave`, from the waves' own counts.
CEC_HW_HD uint32_t where_waves_before(const uint32_t (&count)[kWhereWaves], uint32_t wave) {
  uint32_t s = 0;
  for (uint32_t w = 0; w < kWhereWaves; ++w) s += w < wave ? count[w] : 0;
  return s;
}

// Slot offset within an add of n chains for chain `t` of a chunk (t = its index in the chunk),
// given the admitted and parked totals of the chunks before and `sel_rank`, the admitted chains
// of this chunk before t.
CEC_HW_HD uint32_t where_pos(bool admitted, uint32_t n, uint32_t sel_before, uint32_t park_before,
                             uint32_t t, uint32_t sel_rank) {
  return admitted ? sel_before + sel_rank : n - 1 - (park_before + (t - sel_rank));
}

// cec_confirm_rule on a segment's counts: zeros and ones among its n ok bytes.
CEC_HW_HD uint32_t confirm_rule(bool rebuilt, uint32_t zeros, uint32_t ones) {
  return !rebuilt ? kConfirmNone : zeros ? kConfirmRefuted : ones ? kConfirmProven : kConfirmNone;
}

// cec_hashq_where_plan: the kernel's launches with loops in place of lanes. held[i] != 0: chain i
// has a buffer. gate_bytes null: no gate. pos[i]: chain i's slot offset; *nsel: admitted chains.
inline void where_plan(const uint8_t* held, const uint8_t* flags, size_t n, size_t per,
                       const uint8_t* gate_bytes, uint32_t gate, uint32_t* pos, size_t* nsel) {
  uint32_t totals[2] = {0, 0};  // the queue's two words: admitted, parked
  for (size_t i0 = 0; i0 < n; i0 += kWhereChunk) {
    const uint32_t cnt = (uint32_t)(n - i0 < kWhereChunk ? n - i0 : kWhereChunk);
    uint64_t ballot[kWhereWaves] = {};
    uint32_t count[kWhereWaves] = {};
    auto admitted = [&](uint32_t t) {
      const size_t i = i0 + t;
      return t < cnt && where_admit(held[i] != 0, flags[i], gate_bytes != nullptr,
                                    gate_bytes ? gate_bytes[i / per] : 0, gate);
    };
    for (uint32_t t = 0; t < kWhereChunk; ++t)
      if (admitted(t)) ballot[t / kWhereWave] |= 1ull << (t % kWhereWave);
    for (uint32_t w = 0; w < kWhereWaves; ++w) count[w] = where_count(ballot[w]);
    for (uint32_t t = 0; t < cnt; ++t) {
      const uint32_t w = t / kWhereWave;
      const uint32_t rank = where_waves_before(count, w) + where_rank(ballot[w], t % kWhereWave);
      pos[i0 + t] = where_pos(admitted(t), (uint32_t)n, totals[0], totals[1], t, rank);
    }
    const uint32_t sel = where_waves_before(count, kWhereWaves);
    totals[0] += sel;
    totals[1] += cnt - sel;
  }
  if (nsel) *nsel = totals[0];
}

}  // namespace cec
