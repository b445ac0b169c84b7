// Host-side launch interface of the HIP kernels in kernels.hip (internal to libcessec).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cec {

// Where shard `i` of segment `s` lives in HBM. The batched device layout of the C ABI is
// [seg][shard][len] for data and for parity, i.e. for i < k:
//   data   + s * data_seg_stride + i * shard_stride
// and for i >= k:
//   parity + s * par_seg_stride + (i - k) * shard_stride.
struct Layout {
  uint8_t* data;
  uint8_t* parity;
  uint64_t len;              // bytes per shard
  uint64_t shard_stride;     // bytes between consecutive shards of one segment
  uint64_t data_seg_stride;  // bytes between consecutive segments in `data`
  uint64_t par_seg_stride;   // bytes between consecutive segments in `parity`
  int k;
};

// One run-time-coefficient program chunk in HBM: up to kRtMaxOut outputs from `nin` inputs.
// Layout (all uint32): header {nin, nout, nob, 0}, in[256], out[256], hb[256] (highest set
// coefficient bit of input column j, -1 for a zero column), then masks[nin][8][nob]:
// masks[j][b][o] = 0xFFFFFFFF when bit b of coef[o][j] is set (zero padded to the bucket nob).
// When nin <= kRthMaxIn, header[3] is the word offset of a Horner section used by the
// Horner-over-input-groups kernel (k_rth): top[32] (highest set coefficient bit of output row
// o, 0xFFFFFFFF for a zero row), then idx[32][8][8]: idx[o][b][g] = the 4-bit combination of
// input group g (inputs 4g..4g+3) whose coefficients in row o have bit b set.
constexpr int kRtMaxOut = 32;
constexpr int kRthMaxIn = 32;
constexpr size_t kRtHeaderWords = 4 + 256 + 256 + 256;
constexpr size_t kRthWords = 32 + 32 * 8 * 8;
inline size_t rt_chunk_bytes(int nin, int nob) {
  return (kRtHeaderWords + (size_t)nin * 8 * nob + (nin <= kRthMaxIn ? kRthWords : 0)) *
         sizeof(uint32_t);
}

// True when every shard start and the shard length allow 16-byte vector access.
bool layout_vec16_ok(const Layout& L);

// Kernel selection of one codec (cec_set_option). Held per codec, passed to every launcher: no
// process-wide state, so distinct codecs on distinct threads stay independent.
struct KernelOpts {
  int ct_variant = -1;  // compile-time kernel variant: -1 = default; others only in tuning
                        // builds (libcessec_tune.so, -DCEC_TUNING)
  int rt_mode = 0;      // run-time kernel: 0 Horner + index-mode XORs (4..32 inputs), 1 per-bit
                        // masks, 2 Horner + v_mov table reads, 3 bit-plane accumulators for
                        // chunks of <= 4 outputs (k_rtb)
  int sha_mode = 0;     // one-shot SHA-256: 0 auto, 1 one wave, 2 two waves per 64 buffers
};
// Whether a run-time chunk of bucket `nob` over `nin` inputs takes the bit-plane product (k_rtb,
// k_ptrb) where one exists for the bucket: asked for, or by default up to four outputs from four
// or more inputs.
inline bool rt_takes_rtb(const KernelOpts& o, int nob, int nin) {
  return o.rt_mode == 3 || (o.rt_mode == 0 && nob <= 4 && nin >= 4);
}
// Highest ct_variant this build instantiates (0 in the product library: default only).
int max_ct_variant();

// Compile-time-coefficient kernels. Return false if no specialised kernel exists for the
// request (caller then uses the run-time kernel).
bool launch_encode_ct(const KernelOpts& o, int k, int m, const Layout& L,
                      const uint32_t* seg_list, uint32_t nseg, hipStream_t st);
// Decode for a single erasure of RS(k, m) codes that have a specialised plan; `missing` is the
// erased shard index and `data_only` drops a parity output.
bool launch_decode_ct(const KernelOpts& o, int k, int m, int missing, const Layout& L,
                      const uint32_t* seg_list, uint32_t nseg, hipStream_t st);
// RS(2,1) single erasures, a different one per segment, in one launch: tagged[i] = segment |
// (erased index << 30) for the nseg segments of the launch. False if not applicable.
// tuning variant 90 (libcessec_tune.so only; false elsewhere): erasures in the kernel arguments
bool launch_decode1_mixed_kargs(int k, int m, const Layout& L, const uint8_t* erased,
                                uint32_t nseg, hipStream_t st);
bool launch_decode1_mixed(const KernelOpts& o, int k, int m, const Layout& L,
                          const uint32_t* tagged, uint32_t nseg, hipStream_t st);

// Verify fused with the recompute (RS(2,1), RS(32,32)): ok[s] = 0 where the stored parity differs
// (ok preset by the caller). False (nothing launched) for other codes or layouts.
bool launch_verify_ct(int k, int m, const Layout& L, uint8_t* ok, uint32_t nseg, hipStream_t st);

// RS(32,32) encode as an additive FFT on bit-sliced data (fft.hip). False (nothing launched)
// when the layout does not fit (shard_len % 1024, 16-byte alignment).
bool launch_fft_rs3232(const Layout& L, const uint32_t* seg_list, uint32_t nseg, int nt,
                       hipStream_t st);

// RS(32,32) verify by the same transform, compared with the stored parity (ok preset by the
// caller; ok[s] = 0 where segment s differs). False (nothing launched) where the layout does not fit.
bool launch_fft_rs3232_verify(const Layout& L, uint8_t* ok, uint32_t nseg, hipStream_t st);

// RS(32,32) erasure decode on the additive FFT (fftdec.hip) with plans of fftdec_plan.h: every
// segment uses `plan1`, or listed segment y uses plans[y] (all of the launch's plans take the same
// side and the same size class, fftdec_big of their syndrome slot count). False (nothing launched)
// when the layout does not fit (fftdec_layout_ok).
bool fftdec_layout_ok(const Layout& L);
bool fftdec_big(int nrs);
// form 0: the product's (every pair exchange through DPP); tuning build only: 1 + a mask of the
// exchanges through the LDS crossbar (bit 0 the IFFT's, 1 the FFT's last layer, 2 the nibble packs),
// 10 the product's without the skip of unread input slots.
bool launch_fftdec(const Layout& L, int side, bool big, const uint32_t* plan1,
                   const uint32_t* const* plans, const uint32_t* seg_list, uint32_t nseg,
                   hipStream_t st, int form = 0);
// The formal-derivative decoder (fftdec_d.hip, plans of fftdec_plan_d): same arguments, any side.
// form 0: one 512-column block per wave (k_fftdec_d, the product's). Tuning build only: 1 the
// persistent kernel that merges a block's output multiplication with the next block's input
// multiplication (k_fftdec_dp), 3 the same with wave priorities by remaining work (DESIGN.md §4:
// 9 % fewer VALU per block, slower overall), 4..10 k_fftdec_d with other masks of the phases whose
// quad exchanges go through the LDS crossbar (ds_swizzle) instead of DPP (fftdec_d.hip kFddSwz),
// 11 the product's without the skip of unread input slots.
bool launch_fftdec_d(const Layout& L, const uint32_t* plan1, const uint32_t* const* plans,
                     const uint32_t* seg_list, uint32_t nseg, hipStream_t st, int form = 0);

// Whether a compile-time single-erasure decode kernel exists for (k, m, missing).
bool has_decode_ct(int k, int m, int missing);

// Bucketed output count the run-time kernel is instantiated for (>= nout).
int rt_bucket(int nout);
// Run-time coefficient GF matvec: out[r] = XOR_j coef[j][r] * in[j]. Either every segment uses
// the chunk `chunk`, or listed segment y uses per_seg[y] (all chunks of one launch share the
// bucket `nob`). Chunks are device memory laid out as described at RtChunk above.
void launch_matvec_rt(const Layout& L, const uint32_t* chunk, const uint32_t* const* per_seg,
                      int nob, const uint32_t* seg_list, uint32_t nseg, hipStream_t st);
// Same product by bit-plane accumulators (k_rtb) for chunks of nob <= 4 outputs; false (nothing
// launched) for a wider bucket.
bool launch_matvec_rtb(const Layout& L, const uint32_t* chunk, const uint32_t* const* per_seg,
                       int nob, const uint32_t* seg_list, uint32_t nseg, hipStream_t st,
                       int variant = -1);
// Same product from the chunks' Horner sections (every chunk of the launch has nin <= nin_max
// <= kRthMaxIn). Returns false (nothing launched) if the form is disabled by the variant knob.
bool launch_matvec_rth(const KernelOpts& o, const Layout& L, const uint32_t* chunk,
                       const uint32_t* const* per_seg, int nin_max, const uint32_t* seg_list,
                       uint32_t nseg, hipStream_t st);

// Pointer-table addressing (scattered shards, the cec_*_ptrs calls): `tab` holds `nrows` rows of
// 64-bit words in HBM, one per workgroup row, the device addresses of a segment's inputs in
// program order, then of its outputs, each `len` bytes. vec_ok: every address in the rows is
// 16-byte aligned (else the byte path runs for the whole launch).
// What a launch does with the `len` bytes at every output position of its rows:
enum class PtrSink {
  store,      // writes the product there (rebuild, encode)
  compare,    // reads them as the expected bytes and compares: ok[segment] (device, preset to 1 by
              // the caller) = 0 for a row that differs, and nothing else is written. The rows
              // carry their segment (below). `ok` is read by this sink only.
  accumulate  // reads them, XORs the product in and writes them back
};
// RS(2,1), compile-time coefficients: row = {input 0, input 1, output, case} (compare: case |
// segment << 32), case 0 / 1 = rebuild data fragment 0 / 1 from (the other data fragment, the
// parity), 2 = encode from (d0, d1). Store and compare only (partials take the run-time rows):
// nothing is launched for accumulate.
void launch_ptrs_rs21(PtrSink sink, const uint64_t* tab, uint32_t nrows, uint64_t len, bool vec_ok,
                      uint8_t* ok, hipStream_t st);
// Run-time programs: row = {address of the segment's program chunk, its nin inputs, its nout
// outputs, ..., segment}, rows `rs` words apart (rs >= 1 + nin + nout; compare: the segment in
// word rs - 1, rs >= 2 + nin + nout), every chunk of the launch of bucket `nob`. The per-bit mask
// product (k_rt's) for any bucket, or with `bitplane` the bit-plane product (k_rtb's) where the
// bucket has one (nob <= 4).
void launch_ptrs_rt(PtrSink sink, bool bitplane, const uint64_t* tab, uint32_t nrows, uint32_t rs,
                    int nob, uint64_t len, bool vec_ok, uint8_t* ok, hipStream_t st);

// Rebuilds decided on the GPU (cec_repair_flagged_ptrs): a planner kernel reads per-fragment flags
// from device memory and writes the rows of the table above, which the next launches on the
// stream run. The per-segment rule is cec_flag_status's (cess_ec.h): bad = held and flag == 0,
// good = held and flag != 0; no bad: clean; one bad and >= k good: rebuilt; two or more bad and
// >= k good: many; else lost. The codes are the CEC_FLAG_* values.
enum : uint32_t { kFlagClean = 0, kFlagRebuilt = 1, kFlagMany = 2, kFlagLost = 3 };
struct FlagPlan {
  const uint64_t* segs;    // [nseg][n + 1]: a segment's n shard addresses (0: not held), then the
                           // index of its group (segments of one held set)
  const uint64_t* chunks;  // [group][n]: the program chunk that rebuilds shard j of the group's
                           // held set from the others (0: none; unused for RS(2,1) rows)
  const uint8_t* surv;     // [group][n][k]: that program's survivors, shard indices in its order
  const uint8_t* flags;    // [nseg][n], any alignment; bytes of shards not held are not read
  uint8_t* status;         // [nseg]: kFlag* per segment
  uint64_t* rows;          // the working table, row s for segment s (no compaction: the table
                           // does not depend on the order in which waves run)
  uint32_t nseg;
  int n, k;
};
// rs21: rows {input 0, input 1, output, case} for launch_ptrs_rs21, a segment that is not rebuilt
// gets {0, 0, 0, 3}, a case k_ptr21 leaves without touching an address (n == 3, one lane per
// segment). Otherwise rows {program chunk, k inputs, 1 output}, k + 2 words, for
// launch_ptrs_rt_flag, a segment that is not rebuilt gets an all-zero row (one wave per segment).
void launch_flag_plan(const FlagPlan& p, bool rs21, hipStream_t st);
// launch_ptrs_rt's store form for chunks of a bucket nob in 1..4 (nothing is launched for another)
// over rows a planner wrote: a row whose word 0 is zero is left before its program chunk or any
// of its addresses is looked at.
void launch_ptrs_rt_flag(bool bitplane, const uint64_t* tab, uint32_t nrows, uint32_t rs, int nob,
                         uint64_t len, bool vec_ok, hipStream_t st);

// Several bad shards per segment (cec_repair_flagged_multi_ptrs), and a degraded read decided on
// the GPU (cec_read_flagged_ptrs): the planner also solves the decode rows, per segment, from the
// flags (flag_solve.h: the Lagrange form, no inversion), so the host prepares no program. Both are
// one wave program under a rule (flag_solve.h FsRepair, read_plan.h RpRead) and take one plan.
// The repair's rule is cec_flag_status_multi's: up to max_bad (<= kFlagMultiMax) bad shards and
// >= k good ones: rebuilt, all of them, where they lie, from the first k good shards in index
// order. The read's is cec_read_status's, with the missing wanted data shards (wanted and not
// held, or held with flag 0) in the place of the bad ones: they are rebuilt at the caller's
// destinations and the good wanted ones copied there; nothing at `segs` is ever an output.
struct FlagPlanMulti {
  const uint64_t* segs;   // [nseg][n]: a segment's n shard addresses (0: not held)
  const uint8_t* flags;   // [nseg][n], any alignment; bytes of shards not held are not read
  uint8_t* status;        // [nseg]: kFlag* per segment
  uint64_t* rows[4];      // rows[b - 1]: the table of bucket b, [nseg][k + 1 + b] words; null: no
                          // segment of the call can have b shards rebuilt, no table. A read of
                          // RS(2,1): rows[0] is [nseg][4], k_ptr21's rows
  uint32_t* chunks;       // [nseg][chunk_words]: segment s's program chunk (flag_solve.h; unused
                          // for RS(2,1))
  uint32_t chunk_words;   // fs_chunk_words(k, the widest bucket with a table)
  uint32_t nseg;
  int n, k, max_bad;
  // a read only, null for a repair
  const uint64_t* dst;    // [nseg][k]: where data shard j is wanted (0: not wanted)
  uint64_t* copy;         // [nseg][k][2]: {src, dst} of every good wanted data shard of a clean or
                          // rebuilt segment, {0, 0} elsewhere
};
using ReadPlan = FlagPlanMulti;
// One wave per segment. A segment rebuilt with e shards gets the row {its chunk, the addresses of
// its first k good shards, of its e outputs} in bucket e's table and its chunk written (header
// {k, e, e, 0}, hb, masks); in every other table its row is idle: word 0 zero, and for a repair
// the rest unwritten, for a read zero in every word. Row s and chunk s are segment s's, written
// with plain stores: no atomics, no compaction, the tables of two runs are equal.
void launch_flag_plan_multi(const FlagPlanMulti& p, hipStream_t st);
// rs21: one lane per segment, rows {input 0, input 1, destination, case 0 / 1} or the idle {0, 0,
// 0, 3}. Otherwise the wave program above under the read's rule, which also writes the copy rows.
void launch_read_plan(const ReadPlan& p, bool rs21, hipStream_t st);
// The gated copy: `nrows` rows {src, dst}; a workgroup row whose src word is zero leaves after one
// scalar load, every other streams `len` bytes from src to dst (16-byte columns with a byte tail,
// or byte-wise for the whole launch without vec_ok).
void launch_read_copy(const uint64_t* tab, uint64_t nrows, uint64_t len, bool vec_ok,
                      hipStream_t st);

// The corrupt shard found from parity alone (cec_locate_ptrs; the rule is locate_rule.h's). The
// host knows every held set (the NULL pattern), so it uploads per distinct set one program chunk
// of the syndrome product (r outputs from the h held shards in index order) and one planner table
// (locate_rule.h loc_put_set), and per segment one row; nothing is written on the device but the
// results and the four small arrays below.
struct LocatePlan {
  const uint64_t* rows;  // [nseg][rs]: {the set's chunk (0: h <= k, unchecked), the held addresses
                         // in index order, ..., the set's index in word rs - 1}: TableAddr's view
  const uint8_t* sets;   // [set][set_bytes]
  uint64_t* witness;     // [nseg], preset to all ones: the lowest byte offset with S_0 != 0
  uint32_t* cand;        // [nseg]: the candidate shard, or 0xFFFFFFFF (written for every segment)
  uint8_t* dirty;        // [nseg], preset to 0: 1 where some syndrome byte is not zero
  uint8_t* dirty2;       // [nseg], preset to 0: 1 where some T byte is not zero for the candidate
  uint8_t* flags;        // [nseg][n], any alignment, written whole
  uint8_t* status;       // [nseg]: kLoc* per segment
  uint32_t rs, set_bytes;
  uint32_t nseg;
  int n, k;
};
// The syndrome product k_syn over all rows, for the rows whose chunk is of bucket `nob` (1..4;
// every other row is left after its chunk's header, an unchecked one before it). confirm false:
// the locate pass (dirty, witness). confirm true (nob >= 2): only rows with a candidate go on, and
// dirty2 is what they write. Nothing else is stored.
void launch_syn(const LocatePlan& p, int nob, bool confirm, uint64_t len, bool vec_ok,
                hipStream_t st);
// One wave per segment: the candidate from the shard bytes at the witness offset.
void launch_locate_plan(const LocatePlan& p, uint64_t len, hipStream_t st);
// One wave per segment: status and the n flag bytes.
void launch_locate_finish(const LocatePlan& p, hipStream_t st);

// One or two corrupt shards found from parity alone (cec_locate_multi_ptrs with max_bad = 2; the
// rule is locate_multi_rule.h's). Rows and chunks as in LocatePlan; the planner tables hold all
// four coefficient rows (loc2_put_set).
struct PairPlan {
  const uint64_t* rows;  // [nseg][rs], LocatePlan's
  const uint8_t* sets;   // [set][set_bytes], loc2_put_set
  uint64_t* witness;     // [nseg], preset to all ones: the lowest byte offset with some S_a != 0
  uint64_t* witness2;    // [nseg], preset to all ones: the lowest byte offset with some T_a != 0
                         // for a one-shard candidate (r = 4)
  uint32_t* cand;        // [nseg]: the candidate word (loc2_pack1 / loc2_pack2) or 0xFFFFFFFF,
                         // written for every segment by the first solve
  uint8_t* dirty;        // [nseg], preset to 0: 1 where some syndrome byte is not zero
  uint8_t* dirtyT;       // [nseg], preset to 0: 1 where some T byte is not zero
  uint8_t* dirtyU;       // [nseg], preset to 0: 1 where some U byte is not zero
  uint8_t* flags;        // [nseg][n], any alignment, written whole
  uint8_t* status;       // [nseg]: kLoc* per segment
  uint8_t* nbad;         // [nseg] or null: |J| of a FOUND segment, else 0
  uint32_t rs, set_bytes;
  uint32_t nseg;
  int n, k, max_bad;
};
// The syndrome product k_pair_syn over all rows of bucket `nob`. mode 0: the locate pass (dirty,
// witness: any syndrome). mode 1 (nob >= 2): the T confirm of the rows whose candidate is one
// shard (dirtyT, and witness2 for nob = 4). mode 2 (nob = 4): the U confirm of the rows whose
// candidate is a pair (dirtyU). Nothing else is stored.
void launch_pair_syn(const PairPlan& p, int nob, int mode, uint64_t len, bool vec_ok,
                     hipStream_t st);
// One wave per segment. step 0: the candidate word from the shard bytes at the witness. step 1:
// the second shard from the bytes at the second witness.
void launch_pair_plan(const PairPlan& p, uint64_t len, int step, hipStream_t st);
// One wave per segment: status, the n flag bytes and nbad.
void launch_pair_finish(const PairPlan& p, hipStream_t st);
// nbad[s] = 1 where status[s] is FOUND, else 0: the single rule's count.
void launch_pair_nbad_single(const uint8_t* status, uint8_t* nbad, uint64_t nseg, hipStream_t st);

// SHA-256 of `n` equal-length buffers, written as 64 lowercase hex characters each into
// `hex_out` (device, n * 64 bytes). If `ptrs` is null, buffer i is shard (i % nshards) of
// segment (i / nshards) in layout L.
void launch_sha256_hex(int sha_mode, const uint8_t* const* ptrs, const Layout* L, int nshards,
                       uint64_t n, uint64_t len, uint8_t* hex_out, hipStream_t st);

// One chain of the streaming SHA-256 queue (hashq.cpp), 128 bytes in HBM. `blk` counts the
// 64-byte blocks already compressed into `h`, padding blocks included; the chain is complete
// when blk == (len >> 6) + ((len & 63) >= 56 ? 2 : 1), and its hex (if `hex` is set) is written
// by the launch that completes it. Prefix digest: when `pre_blk` > 0 the chain also writes the
// SHA-256 hex of its first pre_blk * 64 bytes to `pre_hex`, from a copy of `h` taken right after
// block pre_blk - 1 and one padding block (a segment's chain gives its first fragment's hash).
// Check: when `ok` is set the completing launch also compares the 64 hex characters of the digest
// with the 64 bytes at `expect` (4-byte aligned, read as words) and stores *ok = 1 (equal) or 0;
// a launch that leaves the chain unfinished writes nothing there. The prefix digest is an output
// only: the record has room for one (expect, ok) pair.
struct ShaChain {
  const uint8_t* src;
  uint64_t len;
  uint64_t blk;
  uint8_t* hex;
  uint32_t h[8];
  uint8_t* pre_hex;
  uint64_t pre_blk;
  uint32_t pre_h[8];  // state after pre_blk blocks, parked by the one-wave tick until its loop ends
  const uint8_t* expect;  // the recorded hash to compare with, 64 lowercase hex chars (null with ok)
  uint8_t* ok;            // where the comparison's flag goes (null: no check)
};
static_assert(sizeof(ShaChain) == 128, "ShaChain is one 128-byte record");

__host__ __device__ inline uint64_t sha256_blocks(uint64_t len) { return (len >> 6) + ((len & 63) >= 56 ? 2 : 1); }

// Initialise n chains in slots slot0.. of the ring `tab` (capacity mask + 1, a power of two).
// pre_blk > 0: chain i also writes the hex of its first pre_blk blocks to
// pre_hex + ((i / per) * pre_hex_outer + i % per) * 64. ok set: chain i is checked against
// expect + ((i / per) * expect_outer + i % per) * 64, its flag goes to
// ok + (i / per) * ok_outer + i % per.
void launch_hashq_add(ShaChain* tab, uint32_t mask, uint64_t slot0, uint32_t n,
                      const uint8_t* base, uint32_t per, uint64_t outer, uint64_t inner,
                      uint64_t len, uint8_t* hex, uint64_t hex_outer, uint64_t pre_blk,
                      uint8_t* pre_hex, uint64_t pre_hex_outer, const uint8_t* expect,
                      uint64_t expect_outer, uint8_t* ok, uint64_t ok_outer, hipStream_t st,
                      const uint32_t* h0 = nullptr, uint64_t blk0 = 0);
// The same for n buffers at arbitrary device addresses (cec_hashq_add_ptrs: stride 1, no prefix)
// and for chains over several buffers back to back (cec_hashq_add_concat_ptrs): chain i starts at
// src[i * stride] (a HOST array; stride = parts, so these are the chains' first parts) with the
// whole chain's len, writes its hex to hex + 64 * i (hex null: no output) and, with pre_hex, the
// hex of its first pre_blk blocks to pre_hex + 64 * i; with ok, it is checked against
// expect + 64 * i and flagged in ok + i. The addresses are copied into the kernel
// arguments (a 2 KiB block, under the 4 KiB limit), one launch per 256 chains.
// This launcher and the next stop at a launch that fails: the caller's launch check reports it.
void launch_hashq_add_concat(ShaChain* tab, uint32_t mask, uint64_t slot0, uint64_t n,
                             const uint8_t* const* src, size_t stride, uint64_t len, uint8_t* hex,
                             uint64_t pre_blk, uint8_t* pre_hex, const uint8_t* expect,
                             uint8_t* ok, hipStream_t st);
// Point the n chains in slots slot0.. at their next part: chain i's src becomes
// addr[i * stride] - off (a HOST array, copied into the kernel arguments, one launch per 256
// chains), off being the byte position in the chain at which that part starts. The ticks then
// read the part as flat src + blk * 64; the host keeps a launch from crossing into a part its
// chains are not based on.
void launch_hashq_rebase(ShaChain* tab, uint32_t mask, uint64_t slot0, uint64_t n,
                         const uint8_t* const* addr, size_t stride, uint64_t off, hipStream_t st);
// Checked chains the device admits (cec_hashq_add_check_where_ptrs): n chains over src[0 .. n) (a
// HOST array, null entries allowed) take the n slots slot0.., chain i admitted iff src[i] is set,
// flags[i] == 0 and (gate_bytes null or gate_bytes[i / per] == gate), read on the device when the
// stream gets there. Admitted chains take the front slots in index order, checked against
// expect + 64 * i into ok + i, hex (if set) to hex + 64 * i; the others are parked complete in the
// back slots and get ok[i] = 2. totals: two words of device memory for the launches' running
// counts. One launch per 256 chains, ordered on st; stops at a launch that fails.
void launch_hashq_admit(ShaChain* tab, uint32_t mask, uint64_t slot0, uint64_t n,
                        const uint8_t* const* src, uint64_t len, const uint8_t* expect,
                        const uint8_t* flags, uint32_t per, const uint8_t* gate_bytes,
                        uint32_t gate, uint8_t* ok, uint8_t* hex, uint32_t* totals,
                        hipStream_t st);
// cec_confirm_flagged: confirm[s] from status[s] and ok[s * n .. s * n + n) (hashq_where.h
// confirm_rule), one wave per segment.
void launch_confirm_flagged(const uint8_t* status, const uint8_t* ok, uint64_t nseg, uint32_t n,
                            uint8_t* confirm, hipStream_t st);
// Advance the n chains in slots head.. by at most max_blocks blocks each; tick_mode 0 lets `live`
// (chains not yet complete among them) pick the kernel form, 1 or 2 = two waves with that many
// blocks prefetched, 3 = one wave per 64 chains.
void launch_sha256_tick(int tick_mode, ShaChain* tab, uint32_t mask, uint64_t head, uint32_t n,
                        uint32_t max_blocks, uint64_t live, hipStream_t st);

// Audit chunk gather (audit.hip): chunk idx[j] (chunk_len bytes) of fragment f, fragments in
// batch order (f = seg * nshards + shard, shards of layout L), to out[(f * nidx + j) * chunk_len].
void launch_chunk_gather(const Layout& L, int nshards, uint64_t nfrag, const uint32_t* d_idx,
                         uint32_t nidx, uint64_t chunk_len, uint8_t* out, hipStream_t st);
// The same gather of scattered fragments (cec_audit_chunks_ptrs): fragment f is the bytes at
// d_frags[f] (a device table of nfrag addresses). vec_ok: every fragment address, `out` and
// chunk_len are 16-byte multiples (16-byte columns; else byte-wise for the whole launch).
void launch_chunk_gather_tab(const uint64_t* d_frags, uint64_t nfrag, const uint32_t* d_idx,
                             uint32_t nidx, uint64_t chunk_len, uint8_t* out, bool vec_ok,
                             hipStream_t st);
// d_addrs[f * nidx + j] = d_frags[f] + d_idx[j] * chunk_len (nfrag * nidx < 2^32 words): the
// `ptrs` of launch_sha256_hex for hashing the challenged chunks in place.
void launch_chunk_addrs(const uint64_t* d_frags, uint64_t nfrag, const uint32_t* d_idx,
                        uint32_t nidx, uint64_t chunk_len, uint64_t* d_addrs, hipStream_t st);

// XOR reduction (xor.hip): dst[0..len) ^= src[j * stride ..][0..len) for j < nsrc.
void launch_xor_reduce(uint8_t* dst, const uint8_t* src, uint32_t nsrc, uint64_t stride,
                       uint64_t len, hipStream_t st);
// Scattered form (cec_xor_ptrs): row r of the device table `tab` is {dst, nsrc sources}, 1 + nsrc
// words; dst[0..len) ^= the len bytes at every non-zero source word. vec_ok: every address of the
// table is 16-byte aligned (16-byte columns and a byte tail; else byte-wise).
void launch_xor_rows(const uint64_t* tab, uint32_t nrows, uint32_t nsrc, uint64_t len,
                     bool vec_ok, hipStream_t st);

// Parity accumulation (acc.hip; cec_encode_idx_batch, cec_update_batch): for every segment s and
// output o < nout
//   par[o] ^= XOR_{j < nin} coef[j * nout + o] * x_j     (accumulate; else par[o] = ...)
// with par[o] at parity + s * par_seg_stride + o * par_shard_stride and x_j the len bytes at
// in_a + s * in_seg_stride + slots[j] * in_slot_stride, XORed with the bytes at the same offset
// from in_b when in_b is not null (Update: old ^ new). Host arrays `slots` and `coef` are copied
// into the kernel arguments (launches of at most kRtMaxOut outputs from kAccMaxIn inputs; input
// chunks after the first accumulate), so the kernels read no other device memory than the shards.
// 16-byte columns when every base and every stride in use is a 16-byte multiple (a length that is
// not gets a byte tail), byte-wise for the whole call otherwise.
constexpr int kAccMaxIn = 8;
void launch_acc(const uint8_t* in_a, const uint8_t* in_b, uint64_t in_seg_stride,
                uint64_t in_slot_stride, uint8_t* parity, uint64_t par_seg_stride,
                uint64_t par_shard_stride, uint64_t len, const uint32_t* slots,
                const uint8_t* coef, int nin, int nout, bool accumulate, uint64_t nseg,
                hipStream_t st);
// The same product on scattered shards (cec_encode_idx_ptrs, cec_update_ptrs): row r of the device
// table `tab` is {nin input addresses, with `update` the nin addresses of their new bytes, nout
// parity addresses}, (update ? 2 : 1) * nin + nout words, each address `len` bytes. One launch
// (per 65535 rows): nin <= kAccMaxIn, nout <= kRtMaxOut (the caller cuts the chunks; nothing is
// launched otherwise), coef[j * nout + o] copied into the kernel arguments. vec_ok: every address
// of the table is 16-byte aligned (16-byte columns and a byte tail; else byte-wise).
void launch_acc_ptrs(const uint64_t* tab, uint32_t nrows, const uint8_t* coef, int nin, int nout,
                     bool update, bool accumulate, uint64_t len, bool vec_ok, hipStream_t st);

// ok[s] = 0 for every segment s whose seg_bytes of a and b differ (ok preset by the caller).
void launch_cmp_segments(const uint8_t* a, const uint8_t* b, uint64_t seg_bytes, uint64_t nseg,
                         uint8_t* ok, hipStream_t st);

// Synthetic segment bytes: 64-bit word w of segment s = splitmix64(seed ^ (s << 32) ^ w),
// little-endian; segments are seg_bytes long and contiguous from `out`.
void launch_fill_splitmix(uint8_t* out, uint64_t seg_bytes, uint64_t nseg, uint64_t seg0,
                          uint64_t seed, hipStream_t st);

}  // namespace cec
