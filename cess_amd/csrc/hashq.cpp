// libcessec hash queue: streaming SHA-256 of many long device buffers (the fragment and segment
// hashes of SegmentList, c-pallets/file-bank/src/types.rs:13-16).
//
// A fragment's SHA-256 is one serial chain: on a GPU its rate is one wave's instruction issue
// (about 35 MB/s per chain), so throughput comes only from chains in flight. The queue keeps
// every chain's state in HBM (ShaChain, kernels.h) in a ring of slots; cec_hashq_add appends
// chains (one small kernel, no host->device copy), cec_hashq_tick advances every live chain by
// at most max_blocks blocks in one launch. A producer that adds a batch per step and ticks once
// per step therefore hashes a window of batches at once, and each batch's hex lands a known
// number of ticks later: completion is tracked on the host from the lengths alone, so nothing
// is read back.
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "../../include/cess_ec.h"
#include "hashq_ring.h"
#include "hashq_where.h"
#include "host_util.h"
#include "kernels.h"

struct cec_hashq {
  int device = 0;
  hipStream_t stream = nullptr;
  cec::ShaChain* tab = nullptr;
  uint32_t* totals = nullptr;  // two words behind the table: k_hashq_admit's running counts
  cec::HashqRing ring;  // which slots are live and how far along: all of the host's bookkeeping
  int tick_mode = 0;    // CEC_HQOPT_TICK
  uint32_t mask() const { return (uint32_t)(ring.cap - 1); }
};

namespace {

// What every add does once its own arguments are checked. `launch(slot0)` writes the n chain
// records in the slots after the tail: they are not live until the push, so a failed launch
// leaves the ring as it was. `keep` (concat adds of parts > 1): the n * parts addresses the queue
// copies, since parts 1.. are needed when the chains get there, long after the caller has its
// array back.
template <class L>
int add_chains(cec_hashq* q, size_t n, uint64_t blocks, uint64_t* ticket, L launch,
               size_t parts = 0, size_t part_blocks = 0, const uint8_t* const* keep = nullptr) {
  if (n == 0) {
    if (ticket) *ticket = 0;
    return CEC_OK;
  }
  if (!q->ring.room(n))
    return cec::set_error(CEC_ENOMEM, "hash queue full: tick until chains complete");
  std::vector<const uint8_t*> ptrs;
  if (keep) {
    try {
      ptrs.assign(keep, keep + n * parts);
    } catch (const std::bad_alloc&) {
      return cec::set_error(CEC_ENOMEM, "hashq concat addresses");
    }
  }
  CEC_HIP_TRY(hipSetDevice(q->device));
  launch(q->ring.tail);
  int rc = cec::check_launch("launch");
  if (rc) return rc;
  // a prefix digest is written before its chain completes, so tracking the add by its full
  // length is conservative for it
  const uint64_t t = q->ring.push(n, blocks, parts, part_blocks, std::move(ptrs));
  if (ticket) *ticket = t;
  return CEC_OK;
}

// The recorded hashes a checking add compares with and the flags it writes (both null: no check).
struct Check {
  const uint8_t* expect = nullptr;
  size_t expect_outer = 0;
  uint8_t* ok = nullptr;
  size_t ok_outer = 0;
};

// What the checking adds ask of their own arguments, before anything else is looked at.
int check_args(const cec_hashq* q, size_t n, const uint8_t* d_expect, const uint8_t* d_ok) {
  if (!q) return cec::set_error(CEC_EINVAL, "null");
  if (n && (!d_expect || !d_ok))
    return cec::set_error(CEC_EINVAL, "a checking add needs d_expect and d_ok");
  if ((uintptr_t)d_expect & 3) return cec::set_error(CEC_EINVAL, "d_expect must be 4-byte aligned");
  return CEC_OK;
}

// Strided chains (cec_hashq_add_prefix, cec_hashq_add_resume, cec_hashq_add_check): pre_blk with
// d_prefix_hex, blk0 with d_states, the check with c.ok.
int add_strided(cec_hashq* q, const uint8_t* d_base, size_t n, size_t per, size_t outer_stride,
                size_t inner_stride, size_t len, uint8_t* d_hex, size_t hex_outer, uint64_t pre_blk,
                uint8_t* d_prefix_hex, size_t prefix_hex_outer, const uint32_t* d_states,
                uint64_t blk0, const Check& c, uint64_t* ticket) {
  return add_chains(q, n, cec::sha256_blocks(len) - blk0, ticket, [&](uint64_t slot0) {
    cec::launch_hashq_add(q->tab, q->mask(), slot0, (uint32_t)n, d_base, (uint32_t)per,
                          outer_stride, inner_stride, len, d_hex, hex_outer, pre_blk, d_prefix_hex,
                          prefix_hex_outer, c.expect, c.expect_outer, c.ok, c.ok_outer, q->stream,
                          d_states, blk0);
  });
}

// Chains by address table (cec_hashq_add_ptrs: parts = 1, no prefix; cec_hashq_add_concat_ptrs;
// cec_hashq_add_check_concat_ptrs: either, checked against c.expect + 64 * i into c.ok + i):
// the first parts' addresses go in the kernel arguments, so the array is the caller's again on
// return and nothing waits for the ticks queued before. One part: nothing to move to, nothing
// kept.
int add_table(cec_hashq* q, const uint8_t* const* d_parts, size_t n, size_t parts,
              size_t part_blocks, size_t len, uint8_t* d_hex, uint8_t* d_prefix_hex,
              const Check& c, uint64_t* ticket) {
  const bool concat = parts > 1;
  return add_chains(
      q, n, cec::sha256_blocks(len), ticket,
      [&](uint64_t slot0) {
        cec::launch_hashq_add_concat(q->tab, q->mask(), slot0, n, d_parts, parts, len, d_hex,
                                     part_blocks, d_prefix_hex, c.expect, c.ok, q->stream);
      },
      concat ? parts : 0, concat ? part_blocks : 0, concat ? d_parts : nullptr);
}

// The argument checks and the add of cec_hashq_add_ptrs and of cec_hashq_add_concat_ptrs, shared
// with their checking form.
int add_ptrs(cec_hashq* q, const uint8_t* const* d_bufs, size_t n, size_t len, uint8_t* d_hex,
             const Check& c, uint64_t* ticket) {
  if (!q || (n && !d_bufs)) return cec::set_error(CEC_EINVAL, "null");
  if (n > 0xFFFFFFFFull) return cec::set_error(CEC_EINVAL, "n too large");
  for (size_t i = 0; i < n; ++i)
    if (!d_bufs[i]) return cec::set_error(CEC_EINVAL, "null buffer");
  return add_table(q, d_bufs, n, 1, 0, len, d_hex, nullptr, c, ticket);
}

int add_concat_ptrs(cec_hashq* q, const uint8_t* const* d_parts, size_t n, size_t parts,
                    size_t part_len, size_t len, uint8_t* d_hex, uint8_t* d_prefix_hex,
                    const Check& c, uint64_t* ticket) {
  if (!q || (n && !d_parts)) return cec::set_error(CEC_EINVAL, "null");
  if (parts == 0) return cec::set_error(CEC_EINVAL, "parts == 0");
  if (part_len == 0 || (part_len & 63))
    return cec::set_error(CEC_EINVAL, "part_len must be a nonzero multiple of 64");
  if (parts > ~(size_t)0 / part_len) return cec::set_error(CEC_EINVAL, "parts * part_len overflows");
  if (len == 0) len = parts * part_len;
  if (len <= (parts - 1) * part_len || len > parts * part_len)
    return cec::set_error(CEC_EINVAL, "len must end inside the last part");
  if (d_prefix_hex && len < part_len)
    return cec::set_error(CEC_EINVAL, "the prefix digest needs a whole first part");
  if (n > 0xFFFFFFFFull) return cec::set_error(CEC_EINVAL, "n too large");
  if (n && parts > ~(size_t)0 / sizeof(void*) / n)
    return cec::set_error(CEC_EINVAL, "n * parts overflows");
  for (size_t i = 0; i < n * parts; ++i)
    if (!d_parts[i]) return cec::set_error(CEC_EINVAL, "null buffer");
  return add_table(q, d_parts, n, parts, part_len >> 6, len, d_hex, d_prefix_hex, c, ticket);
}

}  // namespace

extern "C" {

int cec_hashq_create(int device, size_t capacity, void* hip_stream, cec_hashq** out) {
  if (!out) return cec::set_error(CEC_EINVAL, "null out");
  *out = nullptr;
  if (capacity == 0 || capacity > (1u << 31) || (capacity & (capacity - 1)))
    return cec::set_error(CEC_EINVAL, "capacity must be a power of two in [1, 2^31]");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return cec::set_error(CEC_ENODEV, "no HIP device");
  if (device < 0 || device >= ndev) return cec::set_error(CEC_EINVAL, "bad device");
  CEC_HIP_TRY(hipSetDevice(device));
  auto* q = new (std::nothrow) cec_hashq;
  if (!q) return cec::set_error(CEC_ENOMEM, "hashq");
  q->device = device;
  q->stream = reinterpret_cast<hipStream_t>(hip_stream);
  q->ring.cap = capacity;
  // stream-ordered (hipFree would synchronise the whole device at destroy): every use of the
  // table is a launch on q->stream
  hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&q->tab),
                                capacity * sizeof(cec::ShaChain) + 2 * sizeof(uint32_t),
                                q->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(q->stream);
  if (e != hipSuccess) {
    delete q;
    return cec::set_error(CEC_ENOMEM, std::string("hashq table: ") + hipGetErrorString(e));
  }
  q->totals = reinterpret_cast<uint32_t*>(q->tab + capacity);
  *out = q;
  return CEC_OK;
}

void cec_hashq_destroy(cec_hashq* q) {
  if (!q) return;
  (void)hipSetDevice(q->device);
  // freed in stream order, after the launches still queued on the stream that read the table
  (void)hipFreeAsync(q->tab, q->stream);
  delete q;
}

int cec_hashq_add_prefix(cec_hashq* q, const uint8_t* d_base, size_t n, size_t per,
                         size_t outer_stride, size_t inner_stride, size_t len, uint8_t* d_hex,
                         size_t hex_outer, size_t prefix_len, uint8_t* d_prefix_hex,
                         size_t prefix_hex_outer, uint64_t* ticket) {
  if (!q || (n && !d_base) || per == 0) return cec::set_error(CEC_EINVAL, "null or per == 0");
  if (n > 0xFFFFFFFFull) return cec::set_error(CEC_EINVAL, "n too large");
  if (d_prefix_hex && (prefix_len == 0 || (prefix_len & 63) || prefix_len > len))
    return cec::set_error(CEC_EINVAL, "prefix_len must be a nonzero multiple of 64 <= len");
  return add_strided(q, d_base, n, per, outer_stride, inner_stride, len, d_hex, hex_outer,
                     d_prefix_hex ? prefix_len >> 6 : 0, d_prefix_hex, prefix_hex_outer, nullptr, 0,
                     Check{}, ticket);
}

int cec_hashq_add_resume(cec_hashq* q, const uint8_t* d_base, size_t n, size_t per,
                         size_t outer_stride, size_t inner_stride, size_t len, size_t start_len,
                         const uint32_t* d_states, uint8_t* d_hex, size_t hex_outer,
                         uint64_t* ticket) {
  if (!q || (n && (!d_base || !d_states)) || per == 0)
    return cec::set_error(CEC_EINVAL, "null or per == 0");
  if (n > 0xFFFFFFFFull) return cec::set_error(CEC_EINVAL, "n too large");
  if ((start_len & 63) || start_len > (len & ~(size_t)63))
    return cec::set_error(CEC_EINVAL, "start_len must be a multiple of 64 within len's full blocks");
  return add_strided(q, d_base, n, per, outer_stride, inner_stride, len, d_hex, hex_outer, 0,
                     nullptr, 0, d_states, start_len >> 6, Check{}, ticket);
}

int cec_hashq_add(cec_hashq* q, const uint8_t* d_base, size_t n, size_t per, size_t outer_stride,
                  size_t inner_stride, size_t len, uint8_t* d_hex, size_t hex_outer,
                  uint64_t* ticket) {
  return cec_hashq_add_prefix(q, d_base, n, per, outer_stride, inner_stride, len, d_hex,
                              hex_outer, 0, nullptr, 0, ticket);
}

int cec_hashq_add_ptrs(cec_hashq* q, const uint8_t* const* d_bufs, size_t n, size_t len,
                       uint8_t* d_hex, uint64_t* ticket) {
  return add_ptrs(q, d_bufs, n, len, d_hex, Check{}, ticket);
}

int cec_hashq_add_concat_ptrs(cec_hashq* q, const uint8_t* const* d_parts, size_t n, size_t parts,
                              size_t part_len, size_t len, uint8_t* d_hex, uint8_t* d_prefix_hex,
                              uint64_t* ticket) {
  return add_concat_ptrs(q, d_parts, n, parts, part_len, len, d_hex, d_prefix_hex, Check{},
                         ticket);
}

int cec_hashq_add_check(cec_hashq* q, const uint8_t* d_base, size_t n, size_t per,
                        size_t outer_stride, size_t inner_stride, size_t len,
                        const uint8_t* d_expect, size_t expect_outer, uint8_t* d_ok, size_t ok_outer,
                        uint8_t* d_hex, size_t hex_outer, uint64_t* ticket) {
  int rc = check_args(q, n, d_expect, d_ok);
  if (rc) return rc;
  if ((n && !d_base) || per == 0) return cec::set_error(CEC_EINVAL, "null or per == 0");
  if (n > 0xFFFFFFFFull) return cec::set_error(CEC_EINVAL, "n too large");
  return add_strided(q, d_base, n, per, outer_stride, inner_stride, len, d_hex, hex_outer, 0,
                     nullptr, 0, nullptr, 0, Check{d_expect, expect_outer, d_ok, ok_outer}, ticket);
}

int cec_hashq_add_check_concat_ptrs(cec_hashq* q, const uint8_t* const* d_parts, size_t n,
                                    size_t parts, size_t part_len, size_t len,
                                    const uint8_t* d_expect, uint8_t* d_ok, uint8_t* d_hex,
                                    uint8_t* d_prefix_hex, uint64_t* ticket) {
  int rc = check_args(q, n, d_expect, d_ok);
  if (rc) return rc;
  const Check c{d_expect, 0, d_ok, 0};
  // one buffer per chain is cec_hashq_add_ptrs: any len, part_len not used, no prefix to give
  if (parts == 1 && !d_prefix_hex) return add_ptrs(q, d_parts, n, len, d_hex, c, ticket);
  return add_concat_ptrs(q, d_parts, n, parts, part_len, len, d_hex, d_prefix_hex, c, ticket);
}

static_assert(CEC_HASHQ_SKIPPED == cec::kWhereSkipped && CEC_CONFIRM_NONE == cec::kConfirmNone &&
                  CEC_CONFIRM_PROVEN == cec::kConfirmProven &&
                  CEC_CONFIRM_REFUTED == cec::kConfirmRefuted,
              "hashq_where.h restates the codes of cess_ec.h");

int cec_hashq_add_check_where_ptrs(cec_hashq* q, const uint8_t* const* d_bufs, size_t n, size_t len,
                                   const uint8_t* d_expect, const uint8_t* d_flags, size_t per,
                                   const uint8_t* d_gate, int gate, uint8_t* d_ok, uint8_t* d_hex,
                                   uint64_t* ticket) {
  int rc = check_args(q, n, d_expect, d_ok);
  if (rc) return rc;
  if (n && (!d_bufs || !d_flags)) return cec::set_error(CEC_EINVAL, "null");
  if (d_gate && per == 0) return cec::set_error(CEC_EINVAL, "gate bytes need per > 0");
  if (gate < 0 || gate > 255) return cec::set_error(CEC_EINVAL, "gate must be a byte value");
  if (n > 0xFFFFFFFFull) return cec::set_error(CEC_EINVAL, "n too large");
  // i < 2^32 - 1, so any per from 2^32 - 1 on puts every chain in group 0
  const uint32_t per32 = (uint32_t)(per < 0xFFFFFFFFull ? per : 0xFFFFFFFFull);
  // the host knows no chain's fate: n slots, n chains of the whole length, a plain add
  return add_chains(q, n, cec::sha256_blocks(len), ticket, [&](uint64_t slot0) {
    cec::launch_hashq_admit(q->tab, q->mask(), slot0, n, d_bufs, len, d_expect, d_flags, per32,
                            d_gate, (uint32_t)gate, d_ok, d_hex, q->totals, q->stream);
  });
}

int cec_hashq_where_plan(const uint8_t* held, const uint8_t* flags, size_t n, size_t per,
                         const uint8_t* gate_bytes, int gate, uint32_t* pos, size_t* nsel) {
  if (n && (!held || !flags || !pos)) return cec::set_error(CEC_EINVAL, "null");
  if (gate_bytes && per == 0) return cec::set_error(CEC_EINVAL, "gate bytes need per > 0");
  if (gate < 0 || gate > 255) return cec::set_error(CEC_EINVAL, "gate must be a byte value");
  if (n > 0xFFFFFFFFull) return cec::set_error(CEC_EINVAL, "n too large");
  cec::where_plan(held, flags, n, per, gate_bytes, (uint32_t)gate, pos, nsel);
  return CEC_OK;
}

int cec_hashq_tick(cec_hashq* q, uint32_t max_blocks) {
  if (!q) return cec::set_error(CEC_EINVAL, "null");
  cec::HashqRing& r = q->ring;
  if (r.adds.empty()) return CEC_OK;
  if (max_blocks == 0) max_blocks = r.drain_blocks();
  CEC_HIP_TRY(hipSetDevice(q->device));
  // Every live chain of whatever kind advances by min(max_blocks, blocks left) in all: the ring
  // cuts the tick at the part boundaries of the concat adds and names the adds to move to their
  // next part after each launch. With no concat add live this is one launch.
  for (uint64_t left = max_blocks; left && !r.adds.empty();) {
    const cec::HashqRing::Launch l = r.next(left);
    cec::launch_sha256_tick(q->tick_mode, q->tab, q->mask(), l.head, l.span, l.step, l.live,
                            q->stream);
    int rc = cec::check_launch("launch");
    if (rc) return rc;
    // the chains of `a` stand at the start of part p: point them at it
    rc = r.advance(l.step, [&](const cec::HashqRing::Add& a, uint64_t p) {
      cec::launch_hashq_rebase(q->tab, q->mask(), a.slot0, a.n, a.ptrs.data() + p,
                               (size_t)a.parts, p * a.part_blocks * 64, q->stream);
      return cec::check_launch("launch");
    });
    if (rc) return rc;
    left -= l.step;
  }
  return CEC_OK;
}

int cec_hashq_finish(cec_hashq* q) {
  if (!q) return cec::set_error(CEC_EINVAL, "null");
  while (!q->ring.adds.empty()) {
    int rc = cec_hashq_tick(q, 0);
    if (rc) return rc;
  }
  return CEC_OK;
}

int cec_hashq_status(const cec_hashq* q, uint64_t ticket, int* done, size_t* live_chains,
                     uint64_t* blocks_left) {
  if (!q) return cec::set_error(CEC_EINVAL, "null");
  if (done) *done = q->ring.done(ticket);
  if (live_chains) *live_chains = (size_t)q->ring.live_chains();
  if (blocks_left) *blocks_left = q->ring.blocks_left();
  return CEC_OK;
}

int cec_hashq_set_option(cec_hashq* q, int option, int value) {
  if (!q) return cec::set_error(CEC_EINVAL, "null");
  if (option == CEC_HQOPT_TICK) {
    if (value < 0 || value > 4) return cec::set_error(CEC_EINVAL, "tick kernel must be 0..4");
    q->tick_mode = value;
    return CEC_OK;
  }
  return cec::set_error(CEC_EINVAL, "unknown hash queue option");
}

}  // extern "C"
