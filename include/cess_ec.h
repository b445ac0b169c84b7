/*
 * cess_ec.h — C ABI of libcessec, the MI355X (gfx950) Reed-Solomon codec for CESS's
 * segment -> fragment path.
 *
 * Reference interfaces replaced (see SURVEY.md §8b and INTEGRATION.md):
 *   The reference chain (/root/reference) holds no codec: it fixes the geometry and records the
 *   codec's outputs. Its interface for this path is the on-chain record
 *     FileBank::upload_declaration(file_hash, deal_info: BoundedVec<SegmentList>, user_brief)
 *       c-pallets/file-bank/src/lib.rs:423-428
 *     SegmentList { hash: Hash, fragment_list: BoundedVec<Hash, FragmentCount> }
 *       c-pallets/file-bank/src/types.rs:13-16
 *     Hash([u8; 64])                          primitives/common/src/lib.rs:16
 *     SEGMENT_SIZE = 16 MiB, FRAGMENT_SIZE = 8 MiB   primitives/common/src/lib.rs:60-61
 *     FRAGMENT_COUNT = 3                      runtime/src/lib.rs:1027
 *   and the restoral (repair) flow whose off-chain step is a single-fragment reconstruct
 *     generate_restoral_order / restoral_order_complete   c-pallets/file-bank/src/lib.rs:943-1122
 *   The entry points below mirror the off-chain codec API those records come from
 *   (klauspost/reedsolomon Encoder: New / Encode / EncodeIdx / Update / Reconstruct /
 *   ReconstructData / ReconstructSome / Verify / Split — not vendored in the reference), one function per operation,
 *   plus batched device-resident forms for HBM-resident segment batches.
 *
 * Conventions: GF(2^8), polynomial 0x11D, systematic Vandermonde matrix.
 * Shard i < k is data, i >= k parity. All functions return 0 or a negative CEC_E* code; no
 * exceptions cross the ABI. A codec is bound to one device and is not re-entrant; distinct
 * codecs are independent (cec_destroy waits only for the codec's own queued launches, never for
 * the device). Caller owns every shard / segment / hash buffer.
 */
#ifndef CESS_EC_H
#define CESS_EC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CEC_OK 0
#define CEC_EINVAL (-1)     /* bad k/m (k<1, m<1, k+m>256), null pointer, bad option */
#define CEC_ETOOFEW (-2)    /* fewer than k shards present (klauspost ErrTooFewShards) */
#define CEC_ESHARDLEN (-3)  /* zero or mismatched shard length (ErrShardSize / ErrShardNoData) */
#define CEC_EHIP (-4)       /* HIP runtime error (see cec_last_error) */
#define CEC_ENOMEM (-5)     /* device or host allocation failed */
#define CEC_ENCCL (-6)      /* RCCL error (multi-GPU paths) */
#define CEC_ESHORTDATA (-7) /* split of an empty segment (klauspost ErrShortData) */
#define CEC_ENODEV (-8)     /* no usable GPU */
#define CEC_ESEGCOUNT (-9)  /* more segments than the chain's SegmentCount bound (1000) */
#define CEC_ECALLBACK (-10) /* a pipeline callback returned an error */

typedef struct cec_codec cec_codec;

/* Library identity: "cessec <version> gfx950". */
const char* cec_version(void);
const char* cec_strerror(int code);
/* Detail text of the last error on this thread (HIP error string etc.). */
const char* cec_last_error(void);
/* Number of visible HIP devices (0 when none). */
int cec_device_count(void);

/* New(k, m): codec bound to `device`. Builds the (k+m) x k matrix; k >= 1, m >= 1, k+m <= 256. */
int cec_create(int k, int m, int device, cec_codec** out);
void cec_destroy(cec_codec* codec);
/* k, m and device of a codec (any output pointer may be NULL). */
int cec_codec_info(const cec_codec* codec, int* k, int* m, int* device);
/* Copy the (k+m) x k encode matrix, row-major, into `out`. Host only, no GPU work. */
int cec_matrix(const cec_codec* codec, uint8_t* out);

/* Host-buffer API (klauspost-shaped). `shards` holds k+m host pointers of shard_len bytes each.
 * The data is staged through HBM; calls are synchronous. */
int cec_encode(cec_codec* codec, uint8_t* const* shards, size_t shard_len);
/* present[i] != 0: shard i is valid. Missing shards are written in place; with data_only only
 * missing data shards are produced (ReconstructData). All present: no-op. Every rebuild (here and
 * in the batch calls) reads exactly the k survivors cec_survivors names, nothing else flagged
 * present: the first k present shards (klauspost's choice), or for RS(32,32) the set the
 * FFT-domain decoders rebuild from most cheaply. Any k survivors give the same bytes. */
int cec_reconstruct(cec_codec* codec, uint8_t* const* shards, const uint8_t* present,
                    size_t shard_len, int data_only);
/* Host only: the k survivors (ascending shard indices) a rebuild of the pattern `present`
 * (k + m flags) reads. A caller that moves survivors to the decoder (a multi-GPU gather, a
 * repair service fetching from peers) moves these. CEC_ETOOFEW below k present. */
int cec_survivors(int k, int m, const uint8_t* present, uint8_t* survivors);
/* *ok = 1 when every parity shard equals the encode of the data shards. */
int cec_verify(cec_codec* codec, uint8_t* const* shards, size_t shard_len, int* ok);

/* Batched device-resident API. d_data: [nseg][k][shard_len], d_parity: [nseg][m][shard_len],
 * both in HBM. Work is enqueued on `hip_stream` (NULL = the HIP null stream, as in the HIP API)
 * and the call returns without waiting.
 * HIP graph capture: the calls whose kernels take compile-time coefficients and read no
 * codec-owned memory may be captured (hipStreamBeginCapture on hip_stream) and replayed, after
 * one uncaptured call of the same shape: cec_encode_batch of RS(2,1) and RS(32,32), and
 * cec_reconstruct_batch of RS(2,1) with one pattern (per_segment = 0). Every other rebuild reads
 * a decode program from the codec's cache, which may evict it while a graph still points at it:
 * do not capture those, nor cec_reconstruct_some_batch, nor the pointer-table calls
 * (cec_reconstruct_ptrs, cec_encode_ptrs, cec_verify_ptrs, cec_reconstruct_partial_ptrs,
 * cec_xor_ptrs, cec_encode_idx_ptrs, cec_update_ptrs, cec_audit_chunks_ptrs: their kernels read a
 * codec-owned table that is retired once the call's launches complete). A single 16 MiB RS(2,1) segment's
 * encode + three rebuilds: 29.5 us eagerly, 24.8 us as one graph (profiles/r05/graph_probe.log). */
int cec_encode_batch(cec_codec* codec, const uint8_t* d_data, uint8_t* d_parity, size_t nseg,
                     size_t shard_len, void* hip_stream);
/* Rebuild missing shards in place in the same layout. `present` is a host array of k+m flags
 * (per_segment = 0: one pattern for every segment) or nseg*(k+m) flags (per_segment = 1).
 * Segments are grouped by erasure pattern; decode matrices are inverted on the host once per
 * pattern and cached. */
int cec_reconstruct_batch(cec_codec* codec, uint8_t* d_data, uint8_t* d_parity, size_t nseg,
                          size_t shard_len, const uint8_t* present, int per_segment,
                          int data_only, void* hip_stream);
/* Host only. Rows of the decode of `present` (k+m flags) for the shards flagged in `required`
 * (k+m flags; flags of present shards are ignored): *nreq outputs, out_idx[r] their shard indices
 * ascending, rows[r*k + j] the coefficient of survivor j (cec_survivors order).
 * CEC_ETOOFEW below k present. */
int cec_decode_rows(int k, int m, const uint8_t* present, const uint8_t* required,
                    uint8_t* rows, uint8_t* out_idx, int* nreq);
/* ReconstructSome on the batch layout: as cec_reconstruct_batch, but only missing shards flagged
 * in `required` (same shape as `present`) are written; other missing shards' memory is untouched.
 * The restoral flow's case: an order names one fragment, and rebuilding one lost fragment of a
 * wide segment costs less than rebuilding all of them. The survivors read are those of the
 * pattern (cec_survivors), whatever is required. Decode programs share the codec's LRU cache
 * under a key that also holds the required mask; a mask naming every missing shard is the full
 * rebuild's entry. RS(32,32) goes through the same cost model and FFT-domain decoders with the
 * real output count. */
int cec_reconstruct_some_batch(cec_codec* codec, uint8_t* d_data, uint8_t* d_parity, size_t nseg,
                               size_t shard_len, const uint8_t* present, const uint8_t* required,
                               int per_segment, void* hip_stream);
/* Scattered shards. src, dst: HOST arrays of nseg*(k+m) DEVICE pointers. src[s*n+i] NULL = shard i
 * of segment s is absent. dst[s*n+i] non-NULL = write shard i of segment s there (shard_len
 * bytes); dst entries of present shards are ignored.
 *  - Reads: only the k survivors cec_survivors names for each segment's pattern are read.
 *  - Writes: nothing but the shard_len bytes at each wanted dst is written. A segment with no
 *    wanted output costs nothing (it gets no workgroup, and its shards are not counted).
 *  - Validation: all segments are validated before anything is enqueued; on CEC_ETOOFEW,
 *    CEC_ESHARDLEN or CEC_EINVAL no byte is written. A NULL array, or a dst equal to a survivor
 *    address of its own segment, gives CEC_EINVAL. nseg == 0 is a no-op that returns CEC_OK.
 *  - Pointer arrays: the library copies them into a device table before returning, so both
 *    belong to the caller again on return. The work itself is enqueued on hip_stream and not
 *    waited for.
 *  - Alignment: any alignment and any shard_len >= 1 is correct. When every address the call
 *    reads or writes is 16-byte aligned the kernels take 16-byte (or 8-byte) columns, otherwise
 *    the whole call runs byte-wise (the fallback is per call).
 *  - HIP graph capture: not capturable. The kernels read the codec-owned pointer table and, for
 *    every code but RS(2,1), decode programs from the codec's cache (see the note above).
 * Every geometry runs table-addressed kernels: RS(2,1) the compile-time closed forms (mixed
 * patterns in one launch), otherwise the run-time bit-plane kernel for up to four outputs from
 * four or more inputs and the run-time mask kernel for the rest, RS(32,32) included: its
 * FFT-domain decoders address a coset through one buffer resource with 32-bit offsets and cannot
 * scatter. */
int cec_reconstruct_ptrs(cec_codec* codec, const uint8_t* const* src, uint8_t* const* dst,
                         size_t nseg, size_t shard_len, void* hip_stream);
/* Encode = the above with the k data shards as src and the m parity buffers as dst:
 * d_data_ptrs[s*k+i], d_parity_ptrs[s*m+o] (host arrays of device pointers, none NULL). */
int cec_encode_ptrs(cec_codec* codec, const uint8_t* const* d_data_ptrs,
                    uint8_t* const* d_parity_ptrs, size_t nseg, size_t shard_len,
                    void* hip_stream);
/* Partial rebuild (the partial-product exchange of a multi-GPU degraded read):
 * like cec_reconstruct_batch with per-segment patterns (present: nseg*(k+m) flags; survivors =
 * cec_survivors of each segment's pattern), but every missing shard receives only the
 * contribution of the survivors flagged in `held` (nseg*(k+m) flags; flags of non-survivors are
 * ignored): out = XOR over held survivors i of D[out][i] * shard_i. Only held survivors are read
 * (a segment with no held survivor gets zeros: its program multiplies one survivor slot of the
 * batch, whatever it holds, by zero coefficients). The rebuild is linear, so XOR-ing the partials
 * of a partition of the survivors (one per GPU holding some of them, cec_xor_batch) gives the
 * missing shard. A GPU then sends one partial per lost fragment instead of its survivors. */
int cec_reconstruct_partial_batch(cec_codec* codec, uint8_t* d_data, uint8_t* d_parity,
                                  size_t nseg, size_t shard_len, const uint8_t* present,
                                  const uint8_t* held, int data_only, void* hip_stream);
/* Verify for a batch (klauspost Verify over HBM): d_ok[s] (device, nseg bytes) = 1 when the
 * parity shards of segment s equal the encode of its data shards, else 0. The parity is
 * recomputed into codec-owned scratch and compared; nothing in the batch is written. */
int cec_verify_batch(cec_codec* codec, const uint8_t* d_data, const uint8_t* d_parity,
                     size_t nseg, size_t shard_len, uint8_t* d_ok, void* hip_stream);
/* Verify for scattered shards, in place and read-only. src, expect: HOST arrays of nseg*(k+m)
 * DEVICE pointers laid out as in cec_reconstruct_ptrs; d_ok: device memory of nseg bytes.
 * src[s*n+i] NULL = shard i of segment s is not a source. expect[s*n+i] non-NULL = recompute shard
 * i of segment s from the segment's survivors and compare it with the shard_len bytes there.
 * d_ok[s] = 1 when every expectation of segment s matched, or it had none; otherwise 0.
 * klauspost's Verify is src = the k data shards, expect = the m parity shards; any missing shard
 * may be the one checked, e.g. RS(4,2) with d1 lost: src = {d0, -, d2, d3, p0, -}, expect =
 * {-, -, -, -, -, p1} checks p1 against the others without rebuilding d1.
 *  - A shard is a source or an expectation, never both: src[s*n+i] and expect[s*n+i] both
 *    non-NULL gives CEC_EINVAL (ignoring one would report bytes verified that nobody compared).
 *  - Reads: only the k survivors cec_survivors names for the pattern of non-NULL src entries, and
 *    the expected buffers. Other sources may hold anything.
 *  - Writes: nothing but the nseg bytes of d_ok (preset to 1 on hip_stream ahead of the kernels,
 *    which clear the flag of a segment that differs). No scratch parity, no batch-sized
 *    allocation. A segment with no expectation gets no workgroup and d_ok[s] = 1.
 *  - Validation: everything is validated before anything is enqueued; on an error d_ok is not
 *    written. A NULL array, or a NULL d_ok, with nseg > 0: CEC_EINVAL. A segment with an
 *    expectation and fewer than k sources: CEC_ETOOFEW. shard_len == 0: CEC_ESHARDLEN. nseg == 0:
 *    CEC_OK. A segment with fewer than k sources and no expectation is no error, as a segment
 *    with no destination in cec_reconstruct_ptrs: its shards are not counted, and d_ok[s] = 1.
 *    Sources and expectations may alias, within and across segments: the call only reads them.
 *  - Pointer arrays, alignment: as cec_reconstruct_ptrs. Both arrays belong to the caller again
 *    on return; the work is enqueued on hip_stream and not waited for. Any alignment and any
 *    shard_len >= 1 is correct; 16-byte (or 8-, 4-byte) columns with a byte tail when every
 *    address read is 16-byte aligned, otherwise the whole call runs byte-wise.
 *  - HIP graph capture: not capturable, for the reasons given at cec_reconstruct_ptrs (the
 *    codec-owned table and, for every code but RS(2,1), the cached decode programs).
 * Decode programs come from the codec's LRU cache under the keys of cec_reconstruct_ptrs with the
 * expectation mask as the required mask: a verify and a rebuild of one pattern share an entry.
 * The kernels are the compare forms of the table-addressed ones (same column bodies, the store
 * replaced by a load and a compare); RS(32,32) takes the run-time kernels here too. */
int cec_verify_ptrs(cec_codec* codec, const uint8_t* const* src, const uint8_t* const* expect,
                    size_t nseg, size_t shard_len, uint8_t* d_ok, void* hip_stream);
/* GF(2^8) addition of device buffers: d_dst[0..len) ^= d_src[j*src_stride ..][0..len) for
 * j < nsrc (src_stride >= len when nsrc > 1). Enqueued on hip_stream, which must belong to the
 * device holding the buffers (no codec: the caller's current device and stream decide). Any
 * alignment; len up to 512 GiB (CEC_EINVAL past it) in one launch of a capped grid whose lanes
 * walk the buffer, so lengths of 4 GiB and more run on the byte path too. */
int cec_xor_batch(uint8_t* d_dst, const uint8_t* d_src, size_t nsrc, size_t src_stride,
                  size_t len, void* hip_stream);
/* Partial rebuild of scattered shards, in place: cec_reconstruct_partial_batch without the batch.
 * With n = k+m: present is a HOST array of nseg*n flags, the erasure pattern of each segment as
 * every party of the exchange knows it (its survivors are cec_survivors of its row). src, dst:
 * HOST arrays of nseg*n DEVICE pointers laid out as in cec_reconstruct_ptrs. src[s*n+i] non-NULL =
 * the caller holds shard i of segment s at that address. dst[s*n+i] non-NULL at a shard flagged
 * absent = that shard is a wanted output (shard_len bytes); dst entries of present shards are
 * ignored. Every wanted output i receives XOR over the held survivors j of D[i][j] * shard_j, D[i]
 * the decode row cec_decode_rows gives for the pattern. XOR-ing the results over any partition of
 * a segment's survivors gives the rebuilt shard (cec_xor_ptrs), as with the batch form.
 *  - accumulate == 0: dst = partial. A segment with wanted outputs and no held survivor gets
 *    zeros written (the neutral element, as in the batch form).
 *    accumulate != 0: dst ^= partial, a read-modify-write of exactly the shard_len bytes at each
 *    wanted dst. A segment with no held survivor gets no workgroup and is not touched.
 *  - Reads: only held shards that are survivors of their segment, and with accumulate the wanted
 *    dst. A held shard that is present but not one of the k survivors is never read and may hold
 *    anything.
 *  - Writes: nothing but the shard_len bytes at each wanted dst. A segment with no wanted output
 *    costs nothing (no workgroup, and its shards are not counted).
 *  - Validation: everything is validated before anything is enqueued; on an error no byte is
 *    written. CEC_EINVAL: a NULL codec; a NULL array with nseg > 0; src non-NULL at a shard
 *    flagged absent (the table and the flags are out of step); a wanted dst equal to a held
 *    survivor address of its own segment; the same wanted dst address twice in one call (two rows
 *    would race on it). Equal addresses are what is checked: ranges that overlap partially are
 *    the caller's duty to avoid. CEC_ETOOFEW: a segment with a wanted output and fewer than k
 *    shards flagged present. CEC_ESHARDLEN: shard_len == 0. nseg == 0: CEC_OK.
 *  - Pointer arrays: all three arrays belong to the caller again on return. The device table comes
 *    from the codec's pool and is retired once the launches complete, as in cec_reconstruct_ptrs;
 *    the work is enqueued on hip_stream and not waited for.
 *  - Alignment: any alignment and any shard_len >= 1 is correct. When every address read or
 *    written is 16-byte aligned the kernels take vector columns with a byte tail, otherwise the
 *    whole call runs byte-wise.
 *  - HIP graph capture: not capturable, for the reasons given at cec_reconstruct_ptrs.
 * Programs come from the codec's LRU cache under the partial keys of
 * cec_reconstruct_partial_batch extended by the wanted-output mask: a call whose outputs are every
 * lost shard shares its entry with the batch form of the same pattern and held set. Every geometry
 * runs the table-addressed run-time kernels (the store forms, or their accumulate forms): RS(2,1)
 * too, where a partial of one survivor is one multiplication and no closed form exists, and
 * RS(32,32), whose FFT-domain decoders never run partials. */
int cec_reconstruct_partial_ptrs(cec_codec* codec, const uint8_t* const* src,
                                 uint8_t* const* dst, const uint8_t* present, size_t nseg,
                                 size_t shard_len, int accumulate, void* hip_stream);
/* GF(2^8) addition of scattered device buffers, the combine step of the partials above where
 * they were received: dst is a HOST array of nrows DEVICE pointers, src a HOST array of
 * nrows*nsrc DEVICE pointers, and dst[r][0..len) ^= XOR over j < nsrc of src[r*nsrc+j][0..len).
 * A NULL src entry is skipped (rows have different numbers of partials). A NULL dst[r], or a row
 * with no source, gets no workgroup.
 *  - Reads: the len bytes at every non-NULL src of a row with a dst, and at that dst.
 *    Writes: nothing but the len bytes at those dst.
 *  - Validation: before anything is enqueued; on an error no byte is written. CEC_EINVAL: a NULL
 *    codec; a NULL array with work to do; the same dst address twice; any src address equal to
 *    any dst address of the call (equal addresses are what is checked, partial overlaps are the
 *    caller's duty). len == 0, nrows == 0 or nsrc == 0 is a no-op that returns CEC_OK, as in
 *    cec_xor_batch.
 *  - Pointer arrays, alignment, table: as cec_reconstruct_ptrs. Both arrays belong to the caller
 *    again on return; 16-byte columns with a byte tail when every address in use is 16-byte
 *    aligned, otherwise the whole call runs byte-wise; the device table comes from the codec's
 *    pool and is retired once the launches complete, so the call is not capturable. The work is
 *    enqueued on hip_stream and not waited for. */
int cec_xor_ptrs(cec_codec* codec, uint8_t* const* dst, const uint8_t* const* src, size_t nrows,
                 size_t nsrc, size_t len, void* hip_stream);
/* Heal flagged fragments: a rebuild whose "which shard is bad" comes from flags in DEVICE memory,
 * such as cec_hashq_add_check_concat_ptrs and cec_verify_ptrs leave there, decided per segment on
 * the GPU and done in place, on the stream that produced the flags, with no host round trip (the
 * off-chain half of generate_restoral_order / restoral_order_complete,
 * c-pallets/file-bank/src/lib.rs:943-1122, after a scrub). Per segment, one of: */
#define CEC_FLAG_CLEAN 0   /* no held shard flagged bad: nothing written */
#define CEC_FLAG_REBUILT 1 /* exactly one bad, >= k good: that shard rewritten in place */
#define CEC_FLAG_MANY 2    /* two or more bad, >= k good: nothing written (host path can rebuild) */
#define CEC_FLAG_LOST 3    /* at least one bad and fewer than k good: nothing written */
/* Host only: the rule the device applies to one segment. held, flags: k+m bytes each. bad = held
 * and flag == 0, good = held and flag != 0 (flags of shards not held are ignored). bad == 0:
 * CEC_FLAG_CLEAN, whatever the held count. bad == 1 and good >= k: CEC_FLAG_REBUILT, and *lost
 * (may be NULL) receives that shard's index; -1 for every other status. bad >= 2 and good >= k:
 * CEC_FLAG_MANY. Anything else: CEC_FLAG_LOST. */
int cec_flag_status(int k, int m, const uint8_t* held, const uint8_t* flags, int* status,
                    int* lost);
/* With n = k+m: shards is a HOST array of nseg*n DEVICE pointers laid out as in
 * cec_reconstruct_ptrs, NULL = the shard is not held here. d_flags: DEVICE memory of nseg*n bytes
 * at any alignment, d_flags[s*n+i] != 0 = held shard i of segment s is good, 0 = it is bad: the
 * layout cec_hashq_add_check_concat_ptrs writes when its chains are listed segment-major. d_status:
 * DEVICE memory of nseg bytes, receives one CEC_FLAG_* code per segment by the rule of
 * cec_flag_status. The bad shard j of a CEC_FLAG_REBUILT segment is recomputed from the k
 * survivors cec_survivors names for the pattern (held \ {j}) and written over the shard_len bytes
 * at shards[s*n+j]. For RS(2,1) one bad fragment per segment is all the code can repair; for
 * wider codes this is the single-failure case, and CEC_FLAG_MANY segments are reported untouched
 * for cec_reconstruct_ptrs to take.
 *  - Reads: d_flags (bytes of shards not held are not looked at), and for REBUILT segments only
 *    those k survivors. No shard of any other segment is read.
 *  - Writes: d_status, and the bad shard of each REBUILT segment. d_flags is not written.
 *  - Not waited for: everything that depends on the flags is enqueued on hip_stream and the call
 *    returns; the flags may still be in production by work queued earlier on that stream. The call
 *    neither synchronises hip_stream nor copies any flag to the host. (It waits for the codec's
 *    own upload stream, for its table, as the other _ptrs calls do.)
 *  - Validation: everything is validated before anything is enqueued; on an error no byte is
 *    written. CEC_EINVAL: a NULL codec; with nseg > 0 a NULL shards, d_flags or d_status; the same
 *    non-NULL shard address twice anywhere in the call (any of them may become a destination;
 *    equal addresses are what is checked, as in cec_xor_ptrs). CEC_ESHARDLEN: shard_len == 0.
 *    nseg == 0: CEC_OK.
 *  - Alignment: any alignment and any shard_len >= 1 is correct. When every held address is
 *    16-byte aligned the kernels take vector columns with a byte tail, otherwise the whole call
 *    runs byte-wise (the fallback is per call).
 *  - Pointer array: it belongs to the caller again on return. The device tables (the addresses, the
 *    candidate programs, the rows the planner kernel writes) come from the codec's pool and are
 *    retired behind the launches: CEC_STAT_POOL_BYTES does not grow across repeated calls.
 *  - HIP graph capture: not capturable, for the reasons given at cec_reconstruct_ptrs.
 * Decode programs (every code but RS(2,1) without CEC_OPT_FORCE_GENERIC, whose closed forms need
 * none): one per held set and held shard j, prepared before the flags are known, from the codec's
 * LRU cache under the keys cec_reconstruct_ptrs uses for (held \ {j}, required {j}), so the two
 * calls share entries; the call holds them until its launches are marked, so a cache capacity of
 * 1 stays correct. A planner kernel applies the rule and writes one table row per segment; the
 * table-addressed kernels then run over every row, and a segment that is not REBUILT costs one
 * row of workgroups that leave after one scalar load. */
int cec_repair_flagged_ptrs(cec_codec* codec, uint8_t* const* shards, const uint8_t* d_flags,
                            size_t nseg, size_t shard_len, uint8_t* d_status, void* hip_stream);
/* Several bad shards per segment: the same heal for the wider codes, where a miner exit takes
 * several fragments of a segment at once. Up to max_bad bad shards of a segment are rebuilt, the
 * decode rows solved on the GPU from the flags. The cap: */
#define CEC_FLAG_MULTI_MAX 4 /* the bit-plane product exists for one to four outputs */
/* Host only: the rule with a bound. bad and good as in cec_flag_status. bad == 0: CEC_FLAG_CLEAN.
 * good < k: CEC_FLAG_LOST. bad <= max_bad: CEC_FLAG_REBUILT, every bad shard is rewritten; *nlost
 * receives their count and lost[0 .. *nlost) (CEC_FLAG_MULTI_MAX bytes, may be NULL) their indices,
 * ascending. Otherwise CEC_FLAG_MANY. *nlost is 0 and lost is not written for every status but
 * REBUILT. No status value is added. max_bad must be in [1, CEC_FLAG_MULTI_MAX] (CEC_EINVAL); with
 * max_bad == 1 the rule is cec_flag_status's. */
int cec_flag_status_multi(int k, int m, const uint8_t* held, const uint8_t* flags, int max_bad,
                          int* status, int* nlost, uint8_t* lost);
/* Host only: what the device computes for one segment. Status and *nout as above; for a REBUILT
 * segment out_idx[0 .. *nout) (CEC_FLAG_MULTI_MAX bytes) are the bad shards, ascending, in_idx[0 .. k)
 * the survivors read, the first k good shards in index order, and rows (CEC_FLAG_MULTI_MAX * k
 * bytes) the decode rows: out_idx[o] = XOR_t rows[o*k + t] * in_idx[t] over GF(2^8). out_idx,
 * in_idx and rows may each be NULL. This codec's shard r is f(r) for one polynomial f of degree
 * < k (the Vandermonde convention of cec_matrix), so a row is the Lagrange basis over the
 * survivors, rows[o*k + t] = prod_{u != t} (j ^ S_u) / prod_{u != t} (S_t ^ S_u) with j =
 * out_idx[o], S = in_idx: no matrix is inverted, and no coefficient is zero. The function runs the
 * planner kernel's own arithmetic (csrc/flag_solve.h) with loops in place of lanes. */
int cec_flag_solve(int k, int m, const uint8_t* held, const uint8_t* flags, int max_bad,
                   int* status, int* nout, uint8_t* out_idx, uint8_t* in_idx, uint8_t* rows);
/* cec_repair_flagged_ptrs with the rule of cec_flag_status_multi: shards, d_flags, d_status, nseg
 * and shard_len as there; every bad shard of a CEC_FLAG_REBUILT segment is recomputed and written
 * over the shard_len bytes at its address. Everything cec_repair_flagged_ptrs promises holds here:
 *  - Reads: d_flags (bytes of shards not held are not looked at), and for REBUILT segments only
 *    their survivors. No shard of any other segment is read. Writes: d_status, and the bad shards
 *    of each REBUILT segment; d_flags is not written and nothing of a segment that is not REBUILT
 *    is touched.
 *  - Survivors: the first k good shards in index order, for every code, RS(32,32) included (the
 *    survivor set cec_survivors prefers for RS(32,32) serves the FFT-domain decoders, which this
 *    call never runs; any k survivors give the same bytes). Held shards flagged good past the
 *    first k are not read.
 *  - Not waited for: neither synchronises hip_stream nor copies any flag to the host; the flags
 *    may still be in production by work queued earlier on that stream.
 *  - Validation: before anything is enqueued; on an error no byte is written. CEC_EINVAL: a NULL
 *    codec; max_bad outside [1, CEC_FLAG_MULTI_MAX]; with nseg > 0 a NULL shards, d_flags or
 *    d_status; the same non-NULL shard address twice anywhere in the call. CEC_ESHARDLEN:
 *    shard_len == 0. nseg == 0: CEC_OK.
 *  - Alignment: any; 16-byte columns when every held address is 16-byte aligned, otherwise the
 *    whole call runs byte-wise.
 *  - The device tables come from the codec's pool and are retired behind the launches
 *    (CEC_STAT_POOL_BYTES does not grow across repeated calls). Not capturable.
 * What differs: the decode rows are solved on the device, per segment, so no decode program is
 * prepared on the host and the LRU cache is neither read nor filled (CEC_STAT_DECODE_CACHED does
 * not change). The host uploads the nseg*n addresses and nothing else. A planner kernel (one wave
 * per segment) applies the rule, solves the rows and writes the segment's program chunk and its
 * row in the table of its bucket b = the count of its bad shards; then one launch of the
 * table-addressed product per bucket b <= min(max_bad, m) for which some held set of the call
 * holds k+b shards, each over all nseg rows, where a segment of another bucket costs one row of
 * workgroups that leave after one scalar load. Device footprint per segment, with e the widest
 * such bucket: 8n bytes of addresses, 8(k+1+b) per bucket b <= e of table rows and 4(772 + 8ke)
 * of program chunk; for RS(32,32) at max_bad 4 that is 512 + 1136 + 7184 bytes. The chunks are one
 * block, a pool block below 16 MiB and stream-ordered scratch on hip_stream from there on.
 * With m == 1 or max_bad == 1 the call is cec_repair_flagged_ptrs itself: same planners, same
 * products, same bytes. Not covered: more than CEC_FLAG_MULTI_MAX bad shards per segment
 * (CEC_FLAG_MANY, for cec_reconstruct_ptrs to take). */
int cec_repair_flagged_multi_ptrs(cec_codec* codec, uint8_t* const* shards, const uint8_t* d_flags,
                                  size_t nseg, size_t shard_len, int max_bad, uint8_t* d_status,
                                  void* hip_stream);
/* A degraded read decided from the same flags: the wanted data shards of every segment arrive,
 * verified, in the caller's own buffers (klauspost ReconstructData + Join); the good ones are
 * copied, the missing ones rebuilt into the destination. Nothing is healed: the shards are
 * read-only, and a shard that is absent can be read around. No status value is added; the four
 * codes mean, per segment: CLEAN every wanted shard copied, REBUILT good wanted shards copied and
 * the missing ones rebuilt, MANY and LOST no destination byte written.
 * Host only: the rule. held, flags: k+m bytes each, wanted: k bytes. good = held and flag != 0,
 * over all k+m shards (flags of shards not held are ignored). A wanted data shard is missing when
 * it is not good (not held, or held with flag 0); miss = their count. miss == 0: CEC_FLAG_CLEAN.
 * good < k: CEC_FLAG_LOST. miss <= max_bad: CEC_FLAG_REBUILT; *nmiss receives miss and
 * miss_idx[0 .. *nmiss) (CEC_FLAG_MULTI_MAX bytes, may be NULL) the missing shards, ascending.
 * Otherwise CEC_FLAG_MANY. *nmiss is 0 and miss_idx is not written for every status but REBUILT.
 * Bad or absent parity is simply not good; a data shard that is not wanted never counts as
 * missing. max_bad must be in [1, CEC_FLAG_MULTI_MAX] (CEC_EINVAL). */
int cec_read_status(int k, int m, const uint8_t* held, const uint8_t* flags, const uint8_t* wanted,
                    int max_bad, int* status, int* nmiss, uint8_t* miss_idx);
/* Host only: what the device computes for one segment. Status and *nout as above; for a REBUILT
 * segment out_idx (CEC_FLAG_MULTI_MAX bytes), in_idx (k bytes, the first k good shards in index
 * order) and rows (CEC_FLAG_MULTI_MAX * k bytes) are as in cec_flag_solve, the outputs being the
 * missing shards. copy_idx[0 .. *ncopy) (k bytes, may be NULL) are the data shards that are copied,
 * ascending: the wanted good ones of a CLEAN or REBUILT segment, none (*ncopy == 0) of a LOST or
 * MANY one. out_idx, in_idx and rows may each be NULL. The function runs the planner kernel's own
 * pieces (csrc/read_plan.h over csrc/flag_solve.h) with loops in place of lanes. */
int cec_read_solve(int k, int m, const uint8_t* held, const uint8_t* flags, const uint8_t* wanted,
                   int max_bad, int* status, int* nout, uint8_t* out_idx, uint8_t* in_idx,
                   uint8_t* rows, uint8_t* copy_idx, int* ncopy);
/* The read. shards, d_flags, d_status, nseg and shard_len as in cec_repair_flagged_multi_ptrs
 * (shards: HOST array of nseg*n DEVICE pointers, NULL = not held; d_flags: nseg*n DEVICE bytes at
 * any alignment; d_status: nseg DEVICE bytes), but shards is read-only here. dst is a HOST array
 * of nseg*k DEVICE pointers: dst[s*k+j] non-NULL = data shard j of segment s is wanted at that
 * address (shard_len bytes), NULL = not wanted: neither copied nor rebuilt, and never counted as
 * missing. d_status[s] follows cec_read_status. Parity is never an output.
 *  - Reads: d_flags (bytes of shards not held are not looked at); of a CLEAN segment its good
 *    wanted data shards; of a REBUILT segment its first k good shards in index order only (every
 *    good data shard is among them). Shards flagged bad, good shards past the first k, and every
 *    shard of a LOST or MANY segment are not read.
 *  - Writes: d_status, and shard_len bytes at each wanted dst of CLEAN and REBUILT segments.
 *    Nothing else: not shards, not d_flags, no dst of a LOST or MANY segment.
 *  - Not waited for: everything that depends on the flags is enqueued on hip_stream and the call
 *    returns; the flags may still be in production by work queued earlier on that stream. No
 *    stream synchronise, no device-to-host copy. (It waits for the codec's own upload stream, for
 *    its table, as the other _ptrs calls do.)
 *  - Validation: before anything is enqueued; on an error no byte is written. CEC_EINVAL: a NULL
 *    codec; max_bad outside [1, CEC_FLAG_MULTI_MAX]; with nseg > 0 a NULL shards, d_flags, dst or
 *    d_status; the same non-NULL dst address twice; a dst address equal to any shard address of
 *    the call (healing in place is the repair calls' job; equal addresses are what is checked).
 *    CEC_ESHARDLEN: shard_len == 0. nseg == 0: CEC_OK. A segment with no wanted shard is CLEAN and
 *    costs one idle row.
 *  - Alignment: any; 16-byte columns with a byte tail when every held address and every dst is
 *    16-byte aligned, otherwise the whole call runs byte-wise.
 *  - Memory: the tables (8n + 8k bytes of addresses, 16k of copy rows and 8(k+1+b) per bucket b of
 *    product rows per segment) come from the codec's pool and are retired behind the launches:
 *    CEC_STAT_POOL_BYTES does not grow across repeated calls. The program chunks, 4(772 + 8ke)
 *    bytes per segment with e the widest bucket, are one block as in the multi repair: a pool
 *    block below 16 MiB, stream-ordered scratch on hip_stream from there on. The decode cache is
 *    neither read nor filled (CEC_STAT_DECODE_CACHED does not change). Not capturable into a HIP
 *    graph, for the reasons given at cec_reconstruct_ptrs.
 * A planner kernel applies the rule, writes k copy rows {src, dst} per segment and, for a REBUILT
 * segment, solves its rows and writes its chunk and its product row; a gated copy kernel runs over
 * the nseg*k copy rows; then one launch of the table-addressed product per bucket b <= min(max_bad,
 * m, the most shards a segment wants), each over all nseg rows. An idle row costs one row of
 * workgroups that leave after one scalar load. RS(2,1) without CEC_OPT_FORCE_GENERIC takes its
 * closed forms and needs no chunk. In a REBUILT segment the good wanted data shards are read
 * twice, once by the copy and once by the product. */
int cec_read_flagged_ptrs(cec_codec* codec, const uint8_t* const* shards, const uint8_t* d_flags,
                          uint8_t* const* dst, size_t nseg, size_t shard_len, int max_bad,
                          uint8_t* d_status, void* hip_stream);
/* What a repair proved, per segment: the close of restoral_order_complete, which the chain accepts
 * only if the regenerated fragment hashes to its recorded fragment_hash. After the repairs above,
 * cec_hashq_add_check_where_ptrs (cess_ec.h below) re-hashes exactly the rebuilt fragments; this
 * folds its flags into one code per segment, which keeps "was bad, is healed" apart from "the
 * record itself is wrong" (such a fragment is rebuilt to the same bytes and fails again). */
#define CEC_CONFIRM_NONE 0    /* segment not CEC_FLAG_REBUILT: nothing to prove */
#define CEC_CONFIRM_PROVEN 1  /* every rebuilt fragment hashes to its record */
#define CEC_CONFIRM_REFUTED 2 /* some rebuilt fragment still does not: the record is wrong */
/* Host only: the rule for one segment. ok: its n bytes as the where-add leaves them (1 match, 0
 * mismatch, CEC_HASHQ_SKIPPED not hashed). status != CEC_FLAG_REBUILT: CEC_CONFIRM_NONE. Otherwise
 * REFUTED if any byte is 0, else PROVEN if any is 1, else NONE. CEC_EINVAL: n < 0, a NULL ok with
 * n > 0, a NULL confirm. */
int cec_confirm_rule(int n, int status, const uint8_t* ok, int* confirm);
/* The rule on the GPU: d_confirm[s] from d_status[s] and d_ok[s*n .. s*n+n), all DEVICE memory of
 * any alignment, nseg segments, one wave per segment. Enqueued on hip_stream on the current device,
 * as cec_xor_batch, and not waited for; d_status and d_ok may still be in production by work
 * queued earlier on that stream.
 *  - Reads: d_status, and d_ok of the CEC_FLAG_REBUILT segments only. Writes: d_confirm and nothing
 *    else; d_status keeps its four codes.
 *  - Validation: before anything is enqueued. CEC_EINVAL: n < 0; with nseg > 0 a NULL d_status or
 *    d_confirm, or a NULL d_ok with n > 0; nseg >= 2^33. nseg == 0: CEC_OK. */
int cec_confirm_flagged(const uint8_t* d_status, const uint8_t* d_ok, size_t nseg, int n,
                        uint8_t* d_confirm, void* hip_stream);
/* ---- the corrupt fragment found from parity alone ----------------------------------------------
 * The flags the calls above consume have had one source, a hash of every held fragment. For every
 * held set with two or more shards of redundancy the parity already names a single bad shard: in
 * this codec's convention shard i is f(i) for one polynomial f of degree < k, so the h held shards
 * of a segment, at the points H, satisfy at every byte offset
 *   S_a = XOR_{i in H} u_i * i^a * v_i = 0     a = 0 .. h-k-1
 *   u_i = 1 / prod_{i' in H, i' != i} (i ^ i')   (0^0 = 1)
 * and one bad shard j with error e gives S_a = u_j j^a e: S_1 = j S_0. With j known, T_a =
 * S_{a+1} ^ j S_a are the checks of the held set without j.
 * The rule, per segment, with r = min(nsyn, h - k) and nsyn in [1, CEC_LOCATE_SYN_MAX]: */
#define CEC_LOCATE_SYN_MAX 4
#define CEC_LOCATE_CLEAN 0     /* r >= 1 and S_0..S_{r-1} zero at every byte offset: held flags 1 */
#define CEC_LOCATE_FOUND 1     /* dirty, r >= 2, and: some byte offset has S_0 != 0; at the lowest
                                  such offset x exactly one j in H has S_1(x) = j S_0(x); T_0 ..
                                  T_{r-2} for that j are zero at every byte offset: held flags 1,
                                  shard j 0 */
#define CEC_LOCATE_AMBIGUOUS 2 /* dirty and not FOUND, every dirty segment with r = 1 included:
                                  held flags 0 */
#define CEC_LOCATE_UNCHECKED 3 /* h <= k: no redundancy is held, no shard byte is read: held
                                  flags 1 */
/* Flag bytes of shards that are not held are written 0; every reader ignores them. AMBIGUOUS marks
 * every held shard bad on purpose: the flagged repairs then report CEC_FLAG_LOST and write
 * nothing, cec_read_flagged_ptrs refuses the inconsistent segment, and
 * cec_hashq_add_check_where_ptrs with gate = CEC_LOCATE_AMBIGUOUS hashes exactly those fragments.
 * The guarantee and its limit: if exactly one held shard of a segment differs from the codeword of
 * the others, the segment is FOUND with that shard, for any r >= 2. If b held shards differ, 2 <=
 * b <= r - 1, the segment is never FOUND. With b >= r a wrong FOUND is possible (errors in several
 * shards at the same byte offsets can imitate one), which is what cec_confirm_flagged is for. The
 * rule is a statement about the mutual consistency of the held shards, not about their recorded
 * hashes.
 * Host only: the check rows of a held set. held: k+m bytes; *r receives min(nsyn, h - k) (0 for
 * h <= k); rows (CEC_LOCATE_SYN_MAX*(k+m) bytes, written whole): rows[a*(k+m) + i] = u_i * i^a for
 * held i and a < *r, and 0 elsewhere. CEC_EINVAL: a NULL pointer, nsyn out of range, k, m out of
 * the codec's range. */
int cec_locate_rows(int k, int m, const uint8_t* held, int nsyn, int* r, uint8_t* rows);
/* Host only: the rule on host memory, by the device code's own functions (csrc/locate_rule.h) with
 * loops in place of lanes. shards: k+m HOST pointers to shard_len bytes each, NULL = not held.
 * *status receives the CEC_LOCATE_* code, *found the shard of a FOUND segment, else -1. Refusals
 * as above. */
int cec_locate_host(int k, int m, const uint8_t* const* shards, size_t shard_len, int nsyn,
                    int* status, int* found);
/* The call. shards as in cec_repair_flagged_ptrs, read-only: a HOST array of nseg*n DEVICE
 * pointers (n = k+m), NULL = not held. d_flags: nseg*n DEVICE bytes at any alignment, written
 * whole, in the layout the repairs, the read and the where-add consume. d_status: nseg DEVICE
 * bytes, one CEC_LOCATE_* code per segment.
 *  - Reads: the held shards of segments with h > k, once; those of dirty segments with a
 *    candidate once more. Nothing of an UNCHECKED segment is read.
 *  - Writes: d_flags and d_status and nothing else. No shard is written.
 *  - Not waited for: everything is enqueued on hip_stream, nothing is copied to the host. (It
 *    waits for the codec's own upload stream, for its table, as the other _ptrs calls do.)
 *  - Validation: before anything is enqueued; an error writes no byte. CEC_EINVAL: a NULL codec;
 *    with nseg > 0 a NULL shards, d_flags or d_status; nsyn outside [1, CEC_LOCATE_SYN_MAX].
 *    CEC_ESHARDLEN: shard_len == 0. nseg == 0: CEC_OK. Shard addresses may alias: they are only
 *    read.
 *  - Alignment: any; 16-byte-aligned held addresses give vector columns with a byte tail,
 *    otherwise the whole call runs byte-wise.
 *  - Memory: one block from the codec's pool, retired behind the launches (CEC_STAT_POOL_BYTES
 *    does not grow across repeated calls): per segment a row of 8(most + 2) bytes, most being the
 *    largest held set, and 14 bytes of state; per distinct held set a planner table of 4n + 8
 *    bytes and one program chunk of 4(772 + 8hr) bytes. The decode cache is neither read nor
 *    filled (CEC_STAT_DECODE_CACHED does not change).
 *  - HIP graph capture: not capturable, for the reasons given at cec_reconstruct_ptrs (the
 *    kernels read a codec-owned table that is retired once the launches complete).
 * One grid of the syndrome product per value of r in the call, over all rows (a row of another r
 * or without redundancy is left after one or two scalar loads); a planner wave per segment reads
 * one byte of each held shard at the witness offset, the lowest offset with S_0 != 0 (a minimum,
 * so the result does not depend on the order in which waves ran); the confirm grids run where
 * there is a candidate; a last kernel writes status and flags. Not covered: two or more bad
 * shards per segment (they are AMBIGUOUS for up to r - 1 of them; cec_locate_multi_ptrs below
 * names two with four checks), shards in the batch layout. */
int cec_locate_ptrs(cec_codec* codec, const uint8_t* const* shards, size_t nseg, size_t shard_len,
                    int nsyn, uint8_t* d_flags, uint8_t* d_status, void* hip_stream);
/* ---- two corrupt fragments found from parity alone ----------------------------------------------
 * Bad shards B with errors e_i give S_a = XOR_{i in B} u_i i^a e_i: power sums with the shard
 * indices as locators, so 2t syndromes locate t shards. The widest syndrome product computes four,
 * which names two. The pair rule applies to a segment when max_bad >= 2 and r = min(nsyn, h - k) =
 * 4; every other segment gets steps 1-3 with its r and is AMBIGUOUS past them.
 *  1. Locate pass. dirty = some S_a != 0 somewhere; the witness x1 is the lowest byte offset at
 *     which ANY of S_0..S_{r-1} is non-zero (two bad shards can cancel S_0 at every offset).
 *  2. Column solve at x1. One index: S_0 != 0 and exactly one held j has S_{a+1} = j S_a for
 *     every a < r - 1; J = {j}. Two indices (r = 4, one index failed): det = S_1^2 ^ S_0 S_2 != 0,
 *     sigma1 = (S_1 S_2 ^ S_0 S_3) / det, sigma2 = (S_1 S_3 ^ S_2^2) / det, and exactly two held i
 *     satisfy i^2 ^ sigma1 i ^ sigma2 = 0; J = those two. Neither: AMBIGUOUS.
 *  3. Confirm with |J| = 1. T_a = S_{a+1} ^ j S_a (a < r - 1) zero everywhere: FOUND {j}.
 *     Otherwise, with the pair rule, x2 is the lowest offset at which any T_a is non-zero; there
 *     T_0 != 0 and exactly one held i != j must satisfy T_1 = i T_0 and T_2 = i T_1; J = {j, i},
 *     sigma1 = j ^ i, sigma2 = j i. Any other outcome: AMBIGUOUS.
 *  4. Confirm with |J| = 2. U_a = S_{a+2} ^ sigma1 S_{a+1} ^ sigma2 S_a (a = 0, 1) zero
 *     everywhere: FOUND J. Otherwise AMBIGUOUS.
 * Statuses are the four CEC_LOCATE_* codes; FOUND covers one or two shards. FOUND: the shards of J
 * have flag 0, the other held shards 1. AMBIGUOUS: every held flag 0. Not held: 0. nbad = |J| for
 * FOUND, else 0.
 * The guarantee and its limit: with r = 4 the four checks define a code of distance 5 on H. If the
 * held shards that differ from the codeword of the others are a set B with |B| <= 2, the result is
 * FOUND with exactly B: the column at x1 has error weight 1 or 2 inside B and decoding is unique
 * within radius 2; the held set without j has three checks and distance 4, which names the other
 * shard at x2; the pair confirm has two checks. A wrong FOUND needs an error of weight >= 3 outside
 * J at every offset where one exists, so it needs |B| >= 3: cec_confirm_flagged covers that case,
 * as it does for the single rule at |B| >= r. */
#define CEC_LOCATE_BAD_MAX (2)
/* Host only: the rule on host memory, by the device code's own functions
 * (csrc/locate_multi_rule.h) with loops in place of lanes. shards as in cec_locate_host. *status
 * receives the CEC_LOCATE_* code, *nfound |J| of a FOUND segment (else 0), found[0..2) its shards
 * ascending, unused entries -1. max_bad == 1 is cec_locate_host's rule, by its code. CEC_EINVAL: a
 * NULL pointer, nsyn or max_bad out of range, k, m out of the codec's range; nothing is written. */
int cec_locate_multi_host(int k, int m, const uint8_t* const* shards, size_t shard_len, int nsyn,
                          int max_bad, int* status, int* nfound, int found[2]);
/* The call. shards, d_flags and d_status as in cec_locate_ptrs. d_nbad: nseg DEVICE bytes, or NULL.
 * max_bad == 1 runs cec_locate_ptrs' own launches: d_flags and d_status are byte-equal to that
 * call's on every input.
 *  - Reads: the held shards of segments with h > k, once; those of a dirty segment with a
 *    candidate once more; those of a segment whose two bad shards do not meet at the first dirty
 *    offset a third time. Nothing of an UNCHECKED segment is read.
 *  - Writes: d_flags, d_status and, where given, d_nbad, and nothing else. No shard is written.
 *  - Not waited for: everything is enqueued on hip_stream, nothing is copied to the host. (It
 *    waits for the codec's own upload stream, for its table, as the other _ptrs calls do.)
 *  - Validation: before anything is enqueued; an error writes no byte. CEC_EINVAL: a NULL codec;
 *    with nseg > 0 a NULL shards, d_flags or d_status; nsyn outside [1, CEC_LOCATE_SYN_MAX];
 *    max_bad outside [1, CEC_LOCATE_BAD_MAX]. CEC_ESHARDLEN: shard_len == 0. nseg == 0: CEC_OK.
 *    Shard addresses may alias: they are only read.
 *  - Alignment: any; 16-byte-aligned held addresses give vector columns with a byte tail,
 *    otherwise the whole call runs byte-wise.
 *  - Memory: one block from the codec's pool, retired behind the launches (CEC_STAT_POOL_BYTES
 *    does not grow across repeated calls): per segment a row of 8(most + 2) bytes and 23 bytes of
 *    state (14 with max_bad == 1); per distinct held set a planner table of 6n + 8 bytes (4n + 8)
 *    and one program chunk of 4(772 + 8hr) bytes. The decode cache is neither read nor filled
 *    (CEC_STAT_DECODE_CACHED does not change).
 *  - HIP graph capture: not capturable, for the reasons given at cec_reconstruct_ptrs.
 * With max_bad == 2: one locate grid per value of r in the call; a planner wave per segment for
 * the column solve at x1; one T-confirm grid per r >= 2 for the rows with one candidate; with
 * r = 4 in the call a second planner launch (the second index at x2) and one U-confirm grid for
 * the rows with a pair; a last kernel writes status, flags and nbad. Every value between the
 * launches is a constant byte, a minimum or a word one wave writes. Not covered: more than two bad
 * shards or more than four syndromes, the pair rule for r < 4, shards in the batch layout. */
int cec_locate_multi_ptrs(cec_codec* codec, const uint8_t* const* shards, size_t nseg,
                          size_t shard_len, int nsyn, int max_bad, uint8_t* d_flags,
                          uint8_t* d_status, uint8_t* d_nbad, void* hip_stream);
/* ---- parity accumulated shard by shard (klauspost EncodeIdx and Update) -----------------------
 * Both are one primitive on the codec's encode matrix E (cec_matrix; row k+o is parity shard o):
 *   parity[o] ^= E[k+o][j] * x_j   for every o < m,
 * with x_j a data shard (EncodeIdx) or old_j ^ new_j of a changed data shard (Update).
 *  - EncodeIdx: feeding every data shard exactly once into zeroed parity, in any order, gives
 *    cec_encode_batch's parity; a subset gives the encode of the segment with the other data
 *    shards zero. No data shard is written.
 *  - Update: parity[o] ^= XOR over the changed shards j of E[k+o][j] * (old_j ^ new_j). Only the
 *    parity is written; the old data keeps its bytes and the caller swaps in the new ones.
 *  - Reads: the named shard (EncodeIdx) or the old and new bytes of the flagged slots (Update), and
 *    the parity (not read with accumulate == 0). Nothing else of the batch is touched.
 *  - Writes: the nseg * m * shard_len parity bytes, nothing else.
 *  - Validation happens before anything is enqueued; on any error no byte is written. CEC_EINVAL:
 *    codec or a needed pointer NULL, idx outside [0, k), nseg > 1 with shard_seg_stride <
 *    shard_len, bytes the call reads overlapping the parity range it writes, or shard_len >
 *    2^32 - 256 (the byte path's one launch per segment row: HIP takes fewer than 2^32 work items
 *    per grid dimension). CEC_ESHARDLEN: shard_len == 0. nseg == 0, or no flag set, is a no-op
 *    that returns CEC_OK.
 *  - Alignment: any alignment and any shard_len >= 1 is correct. When every base and stride is a
 *    16-byte multiple the kernels take 16-byte columns (a shard_len that is not gets a byte tail);
 *    otherwise the whole call runs byte-wise.
 *  - The batch calls enqueue on hip_stream and do not wait. Their coefficients travel in the
 *    kernel arguments: these calls read no codec-owned device memory, so there is no program to
 *    cache or to retire. They are not exercised under HIP graph capture in the tests. */
/* EncodeIdx on device buffers. Shard idx of segment s is at d_shard + s*shard_seg_stride
 * (stride k*shard_len for a batch in the library's layout with d_shard = d_data + idx*shard_len,
 * shard_len for shards packed alone). d_parity: [nseg][m][shard_len].
 * accumulate != 0: parity ^= E*x (klauspost). accumulate == 0: parity = E*x, the old parity not
 * read: the first shard of a segment then needs no zeroing pass. */
int cec_encode_idx_batch(cec_codec* codec, const uint8_t* d_shard, size_t shard_seg_stride, int idx,
                         uint8_t* d_parity, size_t nseg, size_t shard_len, int accumulate,
                         void* hip_stream);
/* Update on device buffers. d_old, d_new: [nseg][k][shard_len]. changed: HOST array of k flags,
 * one set for the whole call. Only flagged slots of d_old and d_new are read. d_parity
 * ([nseg][m][shard_len]) is updated in place. */
int cec_update_batch(cec_codec* codec, const uint8_t* d_old, const uint8_t* d_new, uint8_t* d_parity,
                     size_t nseg, size_t shard_len, const uint8_t* changed, void* hip_stream);
/* EncodeIdx and Update on scattered shards, in place: the two calls above without the batch.
 * data, old_data, new_data: HOST arrays of nseg*k DEVICE pointers; parity: a HOST array of nseg*m
 * DEVICE pointers, each shard_len bytes. Every segment has its own fed (or changed) set and its own
 * parity set, all in one call.
 *  - cec_encode_idx_ptrs: data[s*k+j] non-NULL = data shard j of segment s is fed in this call;
 *    parity[s*m+o] non-NULL = parity shard o of segment s is held here at that address (a NULL one
 *    is neither read nor written: under a placement that spreads a segment's parity over GPUs each
 *    names its own). Every named parity receives
 *      parity[o] ^= XOR over the fed j of E[k+o][j] * data_j.
 *    accumulate == 0: parity[o] = that sum, the old parity not read; a segment with a named parity
 *    and no fed shard gets that parity zero-filled (the encode of nothing, the neutral element, as
 *    in cec_reconstruct_partial_ptrs). accumulate != 0: such a segment is not touched.
 *  - cec_update_ptrs: a data slot with old_data[s*k+j] and new_data[s*k+j] both non-NULL is
 *    changed, both NULL unchanged. Every named parity receives
 *      parity[o] ^= XOR over the changed j of E[k+o][j] * (old_j ^ new_j).
 *    Only parity is written; the caller swaps in the new data. old == new for a slot is legal and
 *    contributes zero.
 *  - Reads: the fed or changed shards of segments that do work, and with accumulate (always for
 *    Update) their named parity. Writes: nothing but the shard_len bytes at each named parity of
 *    those segments. A segment without a fed or changed slot, or without a named parity, gets no
 *    workgroup and its pointers are not looked at further (but for the zero fill above).
 *  - Validation: everything is validated before anything is enqueued; on an error no byte is
 *    written. CEC_EINVAL: a NULL codec; a NULL array with nseg > 0; a slot with exactly one of its
 *    old and new entries (the arrays are out of step); the same parity address twice in the call
 *    (two rows would race on it); a parity address equal to any input address of the call. Equal
 *    addresses are what is checked: partial overlaps are the caller's duty, as in cec_xor_ptrs.
 *    Input addresses may repeat within and across segments: they are only read. CEC_ESHARDLEN:
 *    shard_len == 0; the shard_len bound of the batch forms applies. nseg == 0: CEC_OK.
 *  - Pointer arrays: they belong to the caller again on return. The device table comes from the
 *    codec's pool and is retired once the launches complete, as in cec_reconstruct_ptrs; the work
 *    is enqueued on hip_stream and not waited for.
 *  - Alignment: any alignment and any shard_len >= 1 is correct. When every address read or
 *    written is 16-byte aligned the kernels take 16-byte columns with a byte tail, otherwise the
 *    whole call runs byte-wise (the fallback is per call).
 *  - HIP graph capture: not capturable: the kernels read the codec-owned table.
 * No decode program is involved and nothing enters the LRU cache: segments are grouped by their
 * (input set, parity set), and every group runs one launch per chunk of 32 parities and 8 inputs,
 * its coefficients in the kernel arguments as in the batch forms. */
int cec_encode_idx_ptrs(cec_codec* codec, const uint8_t* const* data, uint8_t* const* parity,
                        size_t nseg, size_t shard_len, int accumulate, void* hip_stream);
int cec_update_ptrs(cec_codec* codec, const uint8_t* const* old_data,
                    const uint8_t* const* new_data, uint8_t* const* parity, size_t nseg,
                    size_t shard_len, void* hip_stream);
/* Host-buffer forms (klauspost-shaped, staged through HBM, synchronous). Only what is read is
 * staged: the shard and the m parity shards, or the old and new bytes of the changed shards and the
 * parity; the parity is copied back.
 * cec_encode_idx: parity holds m host pointers (none NULL); accumulates.
 * cec_update: shards holds k+m pointers, a NULL data entry = unchanged; new_data holds k, NULL =
 * unchanged. CEC_EINVAL where new_data[j] is set and shards[j] is NULL, or a parity pointer is
 * NULL. Nothing changed: CEC_OK, nothing done. */
int cec_encode_idx(cec_codec* codec, const uint8_t* data_shard, int idx, uint8_t* const* parity,
                   size_t shard_len);
int cec_update(cec_codec* codec, uint8_t* const* shards, const uint8_t* const* new_data,
               size_t shard_len);

/* SHA-256 of every shard of every segment in the batch layout, as 64 lowercase hex chars:
 * d_hex[(seg*(k+m) + shard)*64 ...]. d_parity may be NULL to hash the k data shards only, in
 * which case the index is seg*k + shard. */
int cec_sha256_batch(cec_codec* codec, const uint8_t* d_data, const uint8_t* d_parity,
                     size_t nseg, size_t shard_len, uint8_t* d_hex, void* hip_stream);

/* SHA-256 hex of n device buffers of `len` bytes: `d_bufs` is a host array of device pointers;
 * `hex` is host memory of n*64 bytes. Synchronous. */
int cec_sha256_hex(const uint8_t* const* d_bufs, size_t n, size_t len, uint8_t* hex,
                   void* hip_stream);

/* Host SHA-256 of n HOST buffers of `len` bytes (the records of a batch whose bytes are in host
 * memory): 64 lowercase hex chars per buffer to hex[i*64 ...]; with prefix_hex, also the hex of
 * each buffer's first prefix_len bytes (a nonzero multiple of 64, <= len; a segment's chain then
 * yields data fragment 0's hash, as cec_hashq_add_prefix does on the GPU). Runs on `threads`
 * threads of a process-wide pool (<= 1: the calling thread only); each core hashes several
 * equal-length chains at once (SHA-NI interleaved 2 or 4 ways, or AVX-512 16 lanes), because one
 * chain alone leaves most of a core's SHA throughput idle. Synchronous. Host only, no GPU. */
int cec_sha256_host(const uint8_t* const* bufs, size_t n, size_t len, uint8_t* hex,
                    size_t prefix_len, uint8_t* prefix_hex, int threads);
/* cec_sha256_host of buffers whose len is a multiple of 64 that also writes each chain's state
 * after those len bytes (8 words, before the padding) to state_out + 8 i: fragment 0's hash and
 * the state a segment chain resumes from on the GPU (cec_hashq_add_resume). */
int cec_sha256_host_state(const uint8_t* const* bufs, size_t n, size_t len, uint8_t* hex,
                          uint32_t* state_out, int threads);
/* Forms of the host hasher: which one runs is process-wide (cec_host_sha_set_form; -1 restores
 * the default: AVX-512 x16 where the CPU has it, else SHA-NI x2 where it has SHA-NI).
 * cec_host_sha_probe times one form on the calling thread over `chains` chains of
 * bytes_per_chain bytes and returns GB/s (< 0: the CPU lacks the form). */
#define CEC_HSHA_SCALAR 0
#define CEC_HSHA_NI1 1
#define CEC_HSHA_NI2 2
#define CEC_HSHA_NI4 3
#define CEC_HSHA_X16 4
int cec_host_sha_set_form(int form);
int cec_host_sha_form(void);
/* Worker threads of the process-wide host SHA-256 pool: grown to the largest `threads` a call
 * asked for, and to the sum of the host_threads of the live host / hybrid pipelines (several
 * pipelines, one per GPU, each bring their own CPU share). */
int cec_host_sha_pool_threads(void);
double cec_host_sha_probe(int form, size_t bytes_per_chain, int chains);

/* Hash queue: streaming SHA-256 of many long device buffers (fragment and segment hashes).
 * Chains keep their state in HBM between launches, so one tick advances every live chain of
 * every batch added so far; a producer that adds a batch per step and ticks once per step hashes
 * a window of batches at once (one chain per buffer is serial, so the GPU's hash rate is the
 * number of chains in flight times one wave's issue rate). All work is enqueued on the stream
 * given at creation; buffers and hex outputs must stay valid until their add is complete.
 * Completion is tracked on the host from the lengths alone (no read-back): an add is complete
 * once the ticks enqueued so far cover its blocks, i.e. when the stream reaches that tick. */
typedef struct cec_hashq cec_hashq;
/* capacity: maximum live chains, a power of two (128 B of HBM each). */
int cec_hashq_create(int device, size_t capacity, void* hip_stream, cec_hashq** out);
/* Frees the table in stream order on the queue's stream (after the launches queued there); does
 * not wait, and does not stall other streams. */
void cec_hashq_destroy(cec_hashq* q);
/* Append n chains: buffer i is d_base + (i / per) * outer_stride + (i % per) * inner_stride, len
 * bytes; its 64 lowercase hex chars go to d_hex + ((i / per) * hex_outer + i % per) * 64
 * (d_hex NULL: no output). E.g. the fragments of a batch [nseg][k][F]: per = k, outer = k*F,
 * inner = F; its segment hashes: per = 1, outer = inner = k*F, len = k*F. *ticket (optional)
 * names the add. CEC_ENOMEM when the ring would overflow (tick first). */
int cec_hashq_add(cec_hashq* q, const uint8_t* d_base, size_t n, size_t per, size_t outer_stride,
                  size_t inner_stride, size_t len, uint8_t* d_hex, size_t hex_outer,
                  uint64_t* ticket);
/* cec_hashq_add where chain i also emits the hex of its first prefix_len bytes (a nonzero
 * multiple of 64, <= len) to d_prefix_hex + ((i / per) * prefix_hex_outer + i % per) * 64.
 * The segment's chain thus yields data fragment 0's hash on the way (the split is contiguous,
 * fragment 0 = the segment's first F bytes): 32 instead of 40 MiB hashed per CESS segment.
 * Both outputs are final once the add is complete. d_prefix_hex NULL = cec_hashq_add. */
int cec_hashq_add_prefix(cec_hashq* q, const uint8_t* d_base, size_t n, size_t per,
                         size_t outer_stride, size_t inner_stride, size_t len, uint8_t* d_hex,
                         size_t hex_outer, size_t prefix_len, uint8_t* d_prefix_hex,
                         size_t prefix_hex_outer, uint64_t* ticket);
/* cec_hashq_add of chains that resume after their first start_len bytes (a multiple of 64 within
 * len's full blocks): chain i starts from the SHA-256 state d_states[8 i .. 8 i + 7] (memory
 * the device reads: device memory or pinned host memory, read by the add's kernel on the queue's
 * stream; the eight 32-bit words after start_len bytes, as cec_sha256_host_state gives them)
 * and hashes bytes start_len .. len of its buffer. A segment chain continued on the GPU after
 * the host hashed its fragment 0. */
int cec_hashq_add_resume(cec_hashq* q, const uint8_t* d_base, size_t n, size_t per,
                         size_t outer_stride, size_t inner_stride, size_t len, size_t start_len,
                         const uint32_t* d_states, uint8_t* d_hex, size_t hex_outer,
                         uint64_t* ticket);
/* cec_hashq_add of n buffers at arbitrary device addresses: d_bufs is a HOST array of n DEVICE
 * pointers of len bytes each (a rebuilt fragment in a caller-owned tensor, a miner's stored
 * fragments scrubbed against their recorded hashes). Chain i writes its hex to d_hex + 64 * i
 * (d_hex NULL: no output). The chains join the ring like those of cec_hashq_add: same ticks in
 * every tick mode, same ticket and status bookkeeping; one add is one length. The addresses travel
 * in kernel arguments (256 per launch), so there is no host->device copy, no table and no wait
 * for the ticks already queued: the array belongs to the caller again on return. Checked before
 * anything is enqueued (on an error the ring is unchanged): CEC_EINVAL for a NULL queue, a NULL
 * array with n > 0, a NULL entry or n > 2^32 - 1; CEC_ENOMEM when the ring would overflow (nothing
 * is added). n == 0: CEC_OK, ticket 0. */
int cec_hashq_add_ptrs(cec_hashq* q, const uint8_t* const* d_bufs, size_t n, size_t len,
                       uint8_t* d_hex, uint64_t* ticket);
/* cec_hashq_add_ptrs of chains that each run over several buffers back to back (a segment whose
 * data fragments lie in separate tensors, a file digest over scattered segments): d_parts is a
 * HOST array of n * parts DEVICE pointers, chain i hashes the concatenation of
 * d_parts[i * parts + 0 .. parts). Every part is part_len bytes (a nonzero multiple of 64, so no
 * SHA block straddles two parts) except that the last contributes len - (parts - 1) * part_len:
 * len is the chain's total length, (parts - 1) * part_len < len <= parts * part_len, 0 meaning
 * parts * part_len. Reads only those bytes, in place. Chain i writes its hex to d_hex + 64 * i
 * (NULL: no output) and, with d_prefix_hex, the hex of its first part (the prefix digest of
 * cec_hashq_add_prefix at part_len: data fragment 0's hash; needs len >= part_len) to
 * d_prefix_hex + 64 * i. The chains join the ring like those of any add: same ticket and status
 * bookkeeping, every tick mode; a tick that would carry such a chain from one part into the next
 * is issued as one launch up to the boundary, a small launch that moves the chain onto its next
 * part, and one launch for the rest, every live chain still advancing by min(max_blocks, blocks
 * left) per cec_hashq_tick. The array belongs to the caller again on return: the first parts'
 * addresses travel in kernel arguments (256 per launch), the queue keeps a host copy of the array
 * while the add is live. Checked before anything is enqueued (on an error the ring is unchanged):
 * CEC_EINVAL for a NULL queue, a NULL array with n > 0, a NULL entry, parts == 0, part_len zero or
 * not a multiple of 64, len outside its range or n > 2^32 - 1; CEC_ENOMEM when the ring would
 * overflow (nothing is added). n == 0: CEC_OK, ticket 0. parts == 1 is cec_hashq_add_ptrs. */
int cec_hashq_add_concat_ptrs(cec_hashq* q, const uint8_t* const* d_parts, size_t n, size_t parts,
                              size_t part_len, size_t len, uint8_t* d_hex, uint8_t* d_prefix_hex,
                              uint64_t* ticket);
/* cec_hashq_add whose chains are also checked: chain i compares its digest with the 64 lowercase hex
 * chars at d_expect + ((i / per) * expect_outer + i % per) * 64 and writes 1 (equal) or 0 to
 * d_ok[(i / per) * ok_outer + i % per]. d_hex may be NULL (flags only). The recorded-hash check of
 * a scrub, a repair gate or a retrieval, left in HBM on the queue's stream like the flags of
 * cec_verify_ptrs: no hex to copy out, nothing to wait for. d_expect is memory the device reads
 * (device memory or pinned host memory, as d_states of cec_hashq_add_resume), 4-byte aligned; it is
 * read by the tick launch that completes the chain, so it stays valid until the add is complete.
 * d_ok is device memory of any alignment. The 64 bytes are compared as bytes with the lowercase
 * hex the queue would have written; the queue does not parse them, so an upper-case or non-hex
 * expectation is a mismatch (flag 0), not an error. A flag is written exactly once, by the launch
 * that completes its chain: nothing is preset (unlike cec_verify_ptrs; a caller who wants one
 * flag per segment over several fragments ANDs them) and no other byte of d_ok is touched. The
 * chains join the ring like those of any add: same ticket and status bookkeeping, every tick
 * mode. Checked before anything is enqueued (on an error the ring is unchanged and no byte is
 * written): CEC_EINVAL for d_expect or d_ok NULL with n > 0 (a caller without expectations uses
 * cec_hashq_add), a d_expect that is not 4-byte aligned, and whatever cec_hashq_add refuses;
 * CEC_ENOMEM when the ring would overflow (nothing is added). n == 0: CEC_OK, ticket 0. */
int cec_hashq_add_check(cec_hashq* q, const uint8_t* d_base, size_t n, size_t per,
                        size_t outer_stride, size_t inner_stride, size_t len,
                        const uint8_t* d_expect, size_t expect_outer, uint8_t* d_ok, size_t ok_outer,
                        uint8_t* d_hex, size_t hex_outer, uint64_t* ticket);
/* cec_hashq_add_concat_ptrs (parts == 1: cec_hashq_add_ptrs) with the check: chain i against
 * d_expect + 64 * i, flag to d_ok + i. d_hex, d_prefix_hex as there, either may be NULL. A miner's
 * stored fragments scrubbed against their recorded hashes (parts == 1), a segment over its
 * scattered data fragments against its segment hash. d_expect, d_ok, the comparison and the flag
 * writes are those of cec_hashq_add_check; the prefix digest stays a hex output and is not
 * checked. With parts == 1 and no d_prefix_hex the call is cec_hashq_add_ptrs: part_len is not
 * used and len is every buffer's length as it is, 0 included. Checked before anything is
 * enqueued (on an error the ring is unchanged and no byte is written): CEC_EINVAL for d_expect or
 * d_ok NULL with n > 0, a d_expect that is not 4-byte aligned, and whatever the form it extends
 * refuses; CEC_ENOMEM when the ring would overflow. n == 0: CEC_OK, ticket 0. */
int cec_hashq_add_check_concat_ptrs(cec_hashq* q, const uint8_t* const* d_parts, size_t n,
                                    size_t parts, size_t part_len, size_t len,
                                    const uint8_t* d_expect, uint8_t* d_ok, uint8_t* d_hex,
                                    uint8_t* d_prefix_hex, uint64_t* ticket);
/* cec_hashq_add_check_concat_ptrs at parts == 1 whose chains the DEVICE admits: the proof of a
 * repair, which hashes only what was rebuilt, the list of which exists only in HBM. d_bufs: a HOST
 * array of n DEVICE pointers of len bytes each, NULL entries allowed. d_flags: n DEVICE bytes, any
 * alignment. d_gate: DEVICE bytes, one per `per` chains, or NULL. Chain i is admitted iff
 *   d_bufs[i] != NULL && d_flags[i] == 0 && (d_gate == NULL || d_gate[i / per] == gate).
 * With the d_flags of a scrub, per = k+m, d_gate = the d_status of cec_repair_flagged_ptrs and
 * gate = CEC_FLAG_REBUILT that is "the fragments the repair just rewrote".
 *  - Admitted chain: hashes its len bytes in place; the tick launch that completes it writes
 *    d_ok[i] = 1 or 0 against d_expect + 64 * i (as cec_hashq_add_check) and, with d_hex, its hex
 *    to d_hex + 64 * i.
 *  - Chain not admitted: the add's kernel writes d_ok[i] = CEC_HASHQ_SKIPPED; no byte at d_bufs[i]
 *    is read, its hex is not written, and it costs the ticks a record load. The flag and gate
 *    bytes of a NULL entry are not read.
 *  - Reads: d_flags and d_gate by the add's kernels, when the queue's stream gets there: they may
 *    still be in production by work queued earlier on that stream. Not waited for: nothing is
 *    synchronised or copied to the host; d_bufs belongs to the caller again on return (the
 *    addresses travel in kernel arguments, 256 per launch).
 *  - Packing: a tick wave costs the same with one live lane as with 64, so the admitted chains
 *    take the add's first slots in index order and the others are parked, complete, in its last;
 *    a group of 64 slots without an admitted chain leaves every tick after its record loads.
 *    The ok, expect and hex addresses travel with the chain, so the order is invisible outside.
 *  - Host bookkeeping: the host cannot know what the device admits. The add takes n ring slots
 *    and is tracked as n chains of len's blocks: cec_hashq_status reports it so, it is complete
 *    when such an add would be, and CEC_ENOMEM is returned when n slots do not fit.
 *  - Validation: before anything is enqueued; on an error the ring is unchanged and no byte is
 *    written. CEC_EINVAL: a NULL queue; with n > 0 a NULL d_bufs, d_expect, d_flags or d_ok;
 *    d_expect not 4-byte aligned; d_gate set with per == 0; gate outside 0..255; n > 2^32 - 1.
 *    n == 0: CEC_OK, ticket 0. */
#define CEC_HASHQ_SKIPPED 2 /* d_ok value of a chain the device did not admit */
int cec_hashq_add_check_where_ptrs(cec_hashq* q, const uint8_t* const* d_bufs, size_t n, size_t len,
                                   const uint8_t* d_expect, const uint8_t* d_flags, size_t per,
                                   const uint8_t* d_gate, int gate, uint8_t* d_ok, uint8_t* d_hex,
                                   uint64_t* ticket);
/* Host only: where the add above puts its chains. held[i] != 0 stands for d_bufs[i] != NULL; flags,
 * per, gate_bytes (may be NULL) and gate as there, in host memory. pos[i] (n words) receives chain
 * i's slot offset within the add, *nsel (may be NULL) the admitted count: the admitted chains hold
 * offsets [0, nsel) in index order, the others [nsel, n) descending. The function runs the admit
 * kernel's own arithmetic (csrc/hashq_where.h) with loops in place of lanes, in the kernel's
 * chunks of 256 and waves of 64. CEC_EINVAL: with n > 0 a NULL held, flags or pos; gate_bytes set
 * with per == 0; gate outside 0..255; n > 2^32 - 1. */
int cec_hashq_where_plan(const uint8_t* held, const uint8_t* flags, size_t n, size_t per,
                         const uint8_t* gate_bytes, int gate, uint32_t* pos, size_t* nsel);
/* Advance every live chain by at most max_blocks 64-byte blocks (0 = to completion). */
int cec_hashq_tick(cec_hashq* q, uint32_t max_blocks);
/* Tick until every chain added so far is complete (enqueued; synchronise the stream to wait). */
int cec_hashq_finish(cec_hashq* q);
/* Host-side status as of the ticks enqueued so far: *done = add `ticket` complete, *live_chains
 * = chains not yet complete, *blocks_left = most blocks any live chain still needs. Any output
 * pointer may be NULL. */
int cec_hashq_status(const cec_hashq* q, uint64_t ticket, int* done, size_t* live_chains,
                     uint64_t* blocks_left);
/* Queue options. CEC_HQOPT_TICK: tick kernel, 0 = auto by live chains, 1 or 2 = two waves
 * (schedule producer loading 1 or 2 blocks ahead + rounds consumer), 3 = one wave per 64 chains,
 * 4 = lane pairs (a producer wave + two consumer waves running each chain's rounds on two lanes:
 * the shortest chain latency, for few live chains). */
#define CEC_HQOPT_TICK 1
int cec_hashq_set_option(cec_hashq* q, int option, int value);

/* klauspost Split for one segment (host memory): shard i = seg[i*shard_len, (i+1)*shard_len),
 * zero-padded past seg_len. Requires k*shard_len >= seg_len > 0. */
int cec_split_segment(const uint8_t* seg, size_t seg_len, int k, uint8_t* const* shards,
                      size_t shard_len);

/* ---- host pipeline: files in host memory through the GPU ------------------------------------
 * The north_star's pinned hipMemcpyAsync multi-buffering behind the C ABI. A pipeline owns a
 * ring of `depth` pinned host batches and device slots for one codec; a run streams sources
 * through it batch by batch: read() fills a pinned batch (the file's next bytes; the last
 * segment is zero-padded, klauspost Split), H2D on a copy stream, cec_encode_batch on a compute
 * stream, parity D2H on a third stream, so reading batch i+1 overlaps the copies and kernels of
 * batch i and H2D overlaps D2H. The SegmentList hashes (segment hash and the k+m fragment
 * hashes, SHA-256 hex, c-pallets/file-bank/src/types.rs:13-16) are computed where `hash` says:
 *   CEC_PIPE_HASH_GPU     on the GPU by a hash queue that keeps `window` batches hashing at once
 *                         (device slots = window + 3);
 *   CEC_PIPE_HASH_HOST    on `host_threads` host threads (cec_sha256_host) from the pinned ring;
 *   CEC_PIPE_HASH_HYBRID  the segment chains (fragment 0's digest on the way) on the host, the
 *                         other fragments' chains on the GPU queue, except for the last batches
 *                         of the run's last source, which the host hashes wholly (`tail_batches`;
 *                         -1 = auto: the batches whose GPU chains would finish after the source's
 *                         remaining bytes have landed; needs the source's size). Below 12
 *                         host_threads (or with CEC_PIPELINE_RESUME=1; =0 turns it off) the host
 *                         hashes only fragment 0 and the GPU queue resumes the segment chain
 *                         from its state (cec_hashq_add_resume): half the host's bytes.
 * The pipeline is reusable: keep one for many files (its pinned ring is pinned once).
 *   read(user, dst, cap): write up to cap source bytes at dst; return the count, 0 at the end,
 *     < 0 to abort (CEC_ECALLBACK).
 *   on_fragments(user, seg, shards, shard_len): the k+m shards of segment `seg`, host memory
 *     valid during the call; in segment order, as soon as the batch's parity is back.
 *   on_record(user, seg, seg_hex, frag_hex): the segment's 64 hex chars and its k+m fragment
 *     hashes (k+m)*64 hex chars, fragment index order; in segment order.
 * Callbacks run on the calling thread and return 0 (nonzero aborts with CEC_ECALLBACK). */
#define CEC_PIPE_HASH_NONE 0
#define CEC_PIPE_HASH_GPU 1
#define CEC_PIPE_HASH_HOST 2
#define CEC_PIPE_HASH_HYBRID 3
typedef long long (*cec_read_fn)(void* user, uint8_t* dst, size_t cap);
typedef int (*cec_fragments_fn)(void* user, uint64_t seg, const uint8_t* const* shards,
                                size_t shard_len);
typedef int (*cec_record_fn)(void* user, uint64_t seg, const uint8_t* seg_hex,
                             const uint8_t* frag_hex);
typedef struct cec_pipeline_opts {
  size_t shard_len;      /* F: a segment is k * F bytes */
  size_t batch_segments; /* segments per full batch (0: 64); a run's first three batches are
                            1/8, 1/4, 1/2 of it and the last source's last ones halve down to
                            1/8 when its size is known (B >= 8; the records do not change) */
  int depth;             /* pinned host batches (0: 3, host / hybrid hashing 4; >= 2) */
  int hash;              /* CEC_PIPE_HASH_*: 0 none, 1 GPU, 2 host, 3 hybrid */
  int window;            /* batches hashing at once on the GPU queue (0: 32); the pipeline
                            holds window + 3 device batch slots (1.5 GiB each for CESS batches)
                            and shrinks the window to what free HBM holds */
  uint64_t max_segments; /* 0: no limit; else CEC_ESEGCOUNT when a source has more segments
                            (CEC_SEGMENT_COUNT: what one upload_declaration can carry) */
  int host_threads;      /* host SHA-256 threads for hash = 2 / 3 (0: 16) */
  int tail_batches;      /* hash = 3: batches at the end of the last source hashed wholly on
                            the host (-1: auto, 0: none) */
} cec_pipeline_opts;
typedef struct cec_pipeline_stats {
  uint64_t segments;   /* segments encoded */
  uint64_t bytes_in;   /* source bytes read */
  double seconds;      /* wall time of the run (per file: from its first read to its on_done) */
  double read_seconds; /* time inside read() */
  double wait_seconds; /* host time blocked on the GPU or the host hashers */
} cec_pipeline_stats;
typedef struct cec_pipeline cec_pipeline;
int cec_pipeline_create(cec_codec* codec, const cec_pipeline_opts* opts, cec_pipeline** out);
/* Waits for the pipeline's own streams and host hash jobs, then frees its pinned host ring and
 * device slots. The HIP runtime's hipHostFree / hipFree synchronise the whole device, so other
 * codecs' work on this GPU stalls until it is done: destroy a pipeline while the device is idle,
 * or keep it (a pipeline is reusable, one run per file or per list of files). */
void cec_pipeline_destroy(cec_pipeline* p);
/* The window the pipeline settled on (after fitting its slots into free HBM), its device batch
 * slots and pinned host batches. Any output may be NULL. */
int cec_pipeline_info(const cec_pipeline* p, int* window, int* device_slots, int* depth);
/* Stream one source through the pipeline (reusable: run again for the next file). */
int cec_pipeline_run(cec_pipeline* p, cec_read_fn read, cec_fragments_fn on_fragments,
                     cec_record_fn on_record, void* user, cec_pipeline_stats* stats);
/* Several sources (files) in one run, back to back: batches never mix files, segment numbers
 * count from 0 per file, each file's records come in segment order and its on_done once its
 * last record is out, in file order, while the next files already stream (the hashing of one
 * file's last batches overlaps the next file's copies). size: the source's bytes, 0 = unknown
 * (needed only for the hybrid placement of the last batches). stats: the whole run. */
typedef struct cec_source {
  cec_read_fn read;
  void* user; /* passed to read */
  uint64_t size;
} cec_source;
typedef int (*cec_file_fragments_fn)(void* user, size_t file, uint64_t seg,
                                     const uint8_t* const* shards, size_t shard_len);
typedef int (*cec_file_record_fn)(void* user, size_t file, uint64_t seg, const uint8_t* seg_hex,
                                  const uint8_t* frag_hex);
typedef int (*cec_file_done_fn)(void* user, size_t file, const cec_pipeline_stats* file_stats);
int cec_pipeline_run_files(cec_pipeline* p, const cec_source* sources, size_t nsources,
                           cec_file_fragments_fn on_fragments, cec_file_record_fn on_record,
                           cec_file_done_fn on_done, void* user, cec_pipeline_stats* stats);

/* ---- storage audit chunks ---------------------------------------------
 * A fragment is CHUNK_COUNT = 1024 chunks (primitives/common/src/lib.rs:62): 8 KiB chunks of an
 * 8 MiB fragment. A challenge names need = CHUNK_COUNT * 46 / 1000 = 47 distinct chunk indices
 * (NetSnapShot.random_index_list, c-pallets/audit/src/types.rs:21), drawn by
 * c-pallets/audit/src/lib.rs:955-964 from the chain's randomness: for seed = 1, 2, ...,
 * index = random_number(seed) % CHUNK_COUNT, repeats skipped. The PoDR2 tag arithmetic over the
 * chunks runs in the TEE and is not in the reference (unpinned, not provided). */
#define CEC_CHUNK_COUNT 1024
#define CEC_CHALLENGE_NEED (CEC_CHUNK_COUNT * 46 / 1000)
/* The selection loop over a given random stream: randoms[i] = random_number(seed i + 1) (the
 * chain's randomness, decoded as u64). Writes `need` indices; *used = randoms consumed.
 * CEC_EINVAL when the stream runs out first. Host only. */
int cec_challenge_indices(const uint64_t* randoms, size_t nrand, uint32_t chunk_count,
                          uint32_t need, uint32_t* out, size_t* used);
/* Gather chunks indices[0..nidx) of every fragment of an HBM batch ([nseg][k][shard_len] data,
 * [nseg][m][shard_len] parity; d_parity NULL: data fragments only) into d_chunks
 * [nfrag][nidx][chunk] (fragments in batch order, seg * (k+m) + shard), chunk = shard_len /
 * chunk_count, and/or the SHA-256 hex of each gathered chunk into d_hex [nfrag][nidx][64].
 * Either output may be NULL (not both). Enqueued on hip_stream. */
int cec_audit_chunks(cec_codec* codec, const uint8_t* d_data, const uint8_t* d_parity,
                     size_t nseg, size_t shard_len, uint32_t chunk_count,
                     const uint32_t* indices, uint32_t nidx, uint8_t* d_chunks, uint8_t* d_hex,
                     void* hip_stream);
/* The same audit of scattered fragments, in place: cec_audit_chunks without the batch. A miner that
 * answers a challenge holds one fragment of many unrelated segments, each in its own allocation.
 * frags: a HOST array of nfrag DEVICE pointers, each shard_len bytes. The outputs have the batch
 * form's shape with the position in `frags` as the fragment index: d_chunks [nfrag][nidx][chunk],
 * d_hex [nfrag][nidx][64], chunk = shard_len / chunk_count; either may be NULL (not both). The
 * codec's geometry plays no part: the codec supplies the device, the pool and the default stream.
 *  - Reads: only the nidx challenged chunks of each fragment. Fragments may alias each other:
 *    they are only read. Writes: nothing but the named output bytes.
 *  - Hashes: every chunk is hashed where it lies. With d_chunks NULL no chunk byte is copied and
 *    nothing is allocated whose size grows with nfrag * nidx * chunk: the call takes address tables
 *    only (8 bytes per fragment, 4 per index, 8 per chunk when d_hex is given). CEC_OPT_SHA_MODE
 *    and its automatic choice apply as in cec_audit_chunks.
 *  - Validation: everything is validated before anything is enqueued; on an error no byte is
 *    written. CEC_EINVAL: a NULL codec; both outputs NULL; with work to do, a NULL frags or
 *    indices, a NULL entry of frags, an index >= chunk_count, an output base equal to a fragment
 *    address, or nfrag * nidx >= 2^32. CEC_ESHARDLEN: shard_len == 0, chunk_count == 0 or
 *    shard_len % chunk_count != 0. nfrag == 0 or nidx == 0: CEC_OK, nothing done.
 *  - Arrays: both host arrays belong to the caller again on return. The device tables come from
 *    the codec's pool and are retired once the launches complete, as in cec_reconstruct_ptrs; the
 *    work is enqueued on hip_stream and not waited for.
 *  - Alignment: any alignment is correct. The gather takes 16-byte columns when every fragment
 *    address, d_chunks and chunk are 16-byte multiples, otherwise the whole call runs byte-wise
 *    (the fallback is per call).
 *  - HIP graph capture: not capturable: the kernels read the codec-owned tables. */
int cec_audit_chunks_ptrs(cec_codec* codec, const uint8_t* const* frags, size_t nfrag,
                          size_t shard_len, uint32_t chunk_count, const uint32_t* indices,
                          uint32_t nidx, uint8_t* d_chunks, uint8_t* d_hex, void* hip_stream);

/* ---- multi-GPU degraded read over RCCL ----------------------------------------
 * One process (or thread) per GPU, each with its own codec. Fragment f of segment s is stored on
 * rank (s + f) mod world, the GPU analogue of the chain's miner placement (random_assign_miner,
 * c-pallets/file-bank/src/functions.rs:187-283: a segment's fragments on distinct miners). A
 * degraded read brings the k survivors (cec_survivors) of every segment with lost fragments to
 * the rank that owns the segment's first lost fragment (repair restores a fragment where it
 * lives, restoral_order_complete, c-pallets/file-bank/src/lib.rs:1075-1122) by RCCL point-to-
 * point over xGMI, and rebuilds the lost fragments there. RCCL is loaded at run time; without it
 * these return CEC_ENCCL. This is the C form of cess_amd.distributed.degraded_read. */
#define CEC_DIST_ID_BYTES 128
typedef struct cec_dist cec_dist;
/* A fresh group id (on one rank; hand it to the others out of band, e.g. the host's control
 * plane). */
int cec_dist_unique_id(uint8_t* id /* CEC_DIST_ID_BYTES */);
/* Join the group as `rank` of `world` on the codec's device. Collective: every rank calls it
 * with the same id. The group keeps using `codec` until cec_dist_destroy. */
int cec_dist_create(cec_codec* codec, const uint8_t* id, int world, int rank, cec_dist** out);
/* Leave the group and free the handle. The handle's own teardown waits for its last degraded
 * read only, but RCCL's ncclCommDestroy, which it calls, drains the WHOLE device: every stream of
 * every codec on this GPU stalls until its queued work is done (measured: a 25 ms batch on an
 * unrelated stream finished inside the destroy, profiles/r04/destroy_report_c.log). Destroy dist
 * handles only when the device is idle (at shutdown, or between batches), never mid-traffic. */
void cec_dist_destroy(cec_dist* d);
/* One transfer of a plan. kind CEC_DIST_SURVIVOR: fragment `frag` of segment `seg` from rank src
 * to rank dst (src == dst: already local). kind CEC_DIST_PARTIAL: rank src's partial rebuild of
 * lost fragment `frag` (from the survivors src holds, cec_reconstruct_partial_batch) to the
 * decoder dst, which XORs the partials. */
#define CEC_DIST_SURVIVOR 0
#define CEC_DIST_PARTIAL 1
typedef struct cec_dist_move {
  uint64_t seg;
  int32_t frag, src, dst;
  int32_t kind;
} cec_dist_move;
/* Exchange of a degraded read (cec_dist_set_option CEC_DIST_OPT_EXCHANGE, cec_dist_plan_ex):
 * 0 = survivors (the k survivors travel to the decoder), 1 = partials (every other rank holding
 * survivors sends one partial per lost fragment), 2 = per segment whichever moves fewer
 * fragments, survivors on a tie (the default of a new group; RS(2,1) over >= 3 GPUs always ties;
 * a wide code spread over many GPUs with few erasures: RS(32,32) on 8 GPUs, one lost fragment,
 * 7 partials instead of 27-28 survivors). */
#define CEC_DIST_OPT_EXCHANGE 1
/* Test hook: value r >= 0 makes the next degraded reads fail inside round r's transfer group, as
 * an RCCL error there would (the group is ended and the communicator aborted, so peers get an
 * error instead of waiting; later calls on the handle return CEC_ENCCL). -1 = off (default). */
#define CEC_DIST_OPT_TEST_ABORT 2
/* At most `value` point-to-point transfers on any one rank per RCCL group (default 1024; 0 = one
 * group per round of 256 segments, up to ~7k transfers for RS(32,32)). A round is cut into groups
 * at the same plan positions on every rank, so every group holds both ends of its transfers; the
 * groups are enqueued back to back with no host synchronisation. */
#define CEC_DIST_OPT_GROUP_OPS 3
int cec_dist_set_option(cec_dist* d, int option, int value);
/* Transfer groups this handle has issued (diagnostic: the group split of CEC_DIST_OPT_GROUP_OPS). */
int cec_dist_groups(const cec_dist* d, uint64_t* groups);
/* Host only: the transfer groups a degraded read of the lost list issues with `group_ops`
 * (CEC_DIST_OPT_GROUP_OPS) and `exchange`: *ngroups of them, and the plan position (index of the
 * segment in ascending segment order) where each starts, written to starts (NULL: count only;
 * CEC_EINVAL if more than starts_cap). A round of 256 segments always starts a group. */
int cec_dist_plan_groups(int k, int m, int world, int exchange, int group_ops,
                         const uint64_t* lost_seg, const uint8_t* lost_frag, size_t nlost,
                         uint64_t* starts, size_t starts_cap, size_t* ngroups);
/* Host only: the plan a degraded read of the lost list runs. The list holds nlost (segment,
 * fragment) erasures, any order, duplicates allowed, at most m distinct per segment
 * (CEC_ETOOFEW otherwise; CEC_EINVAL for an index >= k+m). Writes the moves in issue order
 * (*nmoves of them; CEC_EINVAL if more than moves_cap, moves may be NULL to count) and, per lost
 * entry, the rank that rebuilds it (decoder, may be NULL). cec_dist_plan = exchange 0. */
int cec_dist_plan(int k, int m, int world, const uint64_t* lost_seg, const uint8_t* lost_frag,
                  size_t nlost, cec_dist_move* moves, size_t moves_cap, size_t* nmoves,
                  int32_t* decoder);
int cec_dist_plan_ex(int k, int m, int world, int exchange, const uint64_t* lost_seg,
                     const uint8_t* lost_frag, size_t nlost, cec_dist_move* moves,
                     size_t moves_cap, size_t* nmoves, int32_t* decoder);
/* Device address (shard_len bytes) of fragment (seg, frag) held by this rank, NULL if absent. */
typedef const uint8_t* (*cec_locate_fn)(void* user, uint64_t seg, int frag);
/* Degraded read. Collective: every rank passes the same lost list. Rank r sends the survivors
 * the placement puts on it (found through `locate`) and writes every lost fragment it rebuilds,
 * entry i, to d_out[i] (device, shard_len bytes; entries other ranks rebuild are not touched and
 * may be NULL; d_out may be NULL on a rank that rebuilds nothing). Before any byte moves the
 * ranks agree that each found its survivors: a NULL from `locate` fails the call on every rank
 * with CEC_EINVAL. Work runs on hip_stream; returns when the rebuilt fragments are in d_out.
 * *nrebuilt (optional) = fragments written on this rank. */
int cec_dist_degraded_read(cec_dist* d, const uint64_t* lost_seg, const uint8_t* lost_frag,
                           size_t nlost, size_t shard_len, cec_locate_fn locate, void* user,
                           uint8_t* const* d_out, void* hip_stream, size_t* nrebuilt);

/* ---- on-chain records (host only, no GPU) ---------------------------------------------------
 * SCALE bytes of what the codec's outputs become on chain:
 *   FileBank::upload_declaration(file_hash: Hash, deal_info: BoundedVec<SegmentList,
 *     SegmentCount>, user_brief: UserBrief)          c-pallets/file-bank/src/lib.rs:419-428
 *   SegmentList { hash: Hash, fragment_list: BoundedVec<Hash, FragmentCount> }   types.rs:13-16
 *   UserBrief { user: AccountId32, file_name, bucket_name: BoundedVec<u8, 63> }  types.rs:105-109
 *   Hash([u8; 64]) (a fixed array: 64 bytes, no length prefix)  primitives/common/src/lib.rs:16
 * Hashes are passed as 64 lowercase hex characters each. Every function writes at most out_cap
 * bytes to `out` and sets *out_len to the encoded size; out == NULL only sizes the encoding. */
#define CEC_SEGMENT_COUNT 1000 /* runtime/src/lib.rs:1026 (SegmentCount) */
#define CEC_FRAGMENT_COUNT 3   /* runtime/src/lib.rs:1027 (FragmentCount) */
#define CEC_NAME_MIN 3         /* runtime/src/lib.rs:1051 (NameMinLength) */
#define CEC_NAME_MAX 63        /* runtime/src/lib.rs:1041 (NameStrLimit) */
#define CEC_FILEBANK_PALLET 60 /* runtime/src/lib.rs:1532 */
#define CEC_CALL_UPLOAD_DECLARATION 0 /* c-pallets/file-bank/src/lib.rs:420 call_index(0) */
/* SCALE compact encoding of n. */
int cec_scale_compact(uint32_t n, uint8_t* out, size_t out_cap, size_t* out_len);
/* deal_info = compact(nseg) ++ per segment: hash ++ compact(nfrag) ++ nfrag hashes.
 * seg_hex: nseg * 64 bytes; frag_hex: nseg * nfrag * 64 (fragment index order).
 * CEC_ESEGCOUNT if nseg > CEC_SEGMENT_COUNT (the extrinsic would be rejected: split the file);
 * CEC_EINVAL if nfrag != CEC_FRAGMENT_COUNT (check_file_spec, c-pallets/file-bank/src/
 * functions.rs:4-11, rejects any other count with SpecError) or a hash is not lowercase hex. */
int cec_scale_deal_info(const uint8_t* seg_hex, const uint8_t* frag_hex, size_t nseg,
                        size_t nfrag, uint8_t* out, size_t out_cap, size_t* out_len);
/* Call data of upload_declaration: pallet index, call index, file_hash, deal_info, user_brief
 * (account: 32 bytes; names 3..63 bytes). */
int cec_scale_upload_declaration(const uint8_t* file_hash_hex, const uint8_t* seg_hex,
                                 const uint8_t* frag_hex, size_t nseg, size_t nfrag,
                                 const uint8_t* account, const uint8_t* file_name,
                                 size_t file_name_len, const uint8_t* bucket_name,
                                 size_t bucket_name_len, uint8_t* out, size_t out_cap,
                                 size_t* out_len);
/* Idle fillers: FileBank::upload_filler(tee_worker: AccountId, filler_list: Vec<FillerInfo>),
 * call_index(8) (c-pallets/file-bank/src/lib.rs:795-833); FillerInfo { block_num: u32,
 * miner_address: AccountId, filler_hash: Hash } (types.rs:82-86); at most UploadFillerLimit = 10
 * fillers per call (runtime/src/lib.rs:1033), each 8 MiB of idle space (lib.rs:821-825).
 * Call data for n fillers: block_num[n], miners n * 32 bytes, filler_hex n * 64 hex chars.
 * CEC_EINVAL past the limit (the chain's LengthExceedsLimit). */
#define CEC_CALL_UPLOAD_FILLER 8
#define CEC_UPLOAD_FILLER_LIMIT 10
#define CEC_FILLER_SIZE (8u << 20)
int cec_scale_upload_filler(const uint8_t* tee_worker, const uint32_t* block_num,
                            const uint8_t* miners, const uint8_t* filler_hex, size_t n,
                            uint8_t* out, size_t out_cap, size_t* out_len);
/* Restoral (repair) calls, c-pallets/file-bank/src/lib.rs:940-1122: a miner that lost a fragment
 * opens an order (13), another claims it (14; 15 for the fragments of an exiting miner,
 * RestoralTarget), rebuilds the fragment off chain and reports it (16). Hashes are 64 hex chars,
 * the miner an AccountId32. A repair service emits 16 only for a fragment whose rebuilt SHA-256
 * equals the recorded fragment hash. */
#define CEC_CALL_GENERATE_RESTORAL_ORDER 13
#define CEC_CALL_CLAIM_RESTORAL_ORDER 14
#define CEC_CALL_CLAIM_RESTORAL_EXIST_ORDER 15
#define CEC_CALL_RESTORAL_ORDER_COMPLETE 16
int cec_scale_generate_restoral_order(const uint8_t* file_hash_hex, const uint8_t* fragment_hex,
                                      uint8_t* out, size_t out_cap, size_t* out_len);
int cec_scale_claim_restoral_order(const uint8_t* fragment_hex, uint8_t* out, size_t out_cap,
                                   size_t* out_len);
int cec_scale_claim_restoral_exist_order(const uint8_t* miner, const uint8_t* file_hash_hex,
                                         const uint8_t* fragment_hex, uint8_t* out,
                                         size_t out_cap, size_t* out_len);
int cec_scale_restoral_order_complete(const uint8_t* fragment_hex, uint8_t* out, size_t out_cap,
                                      size_t* out_len);
/* Audit randomness inputs (c-pallets/audit/src/lib.rs:1067-1076): random_number(seed) asks the
 * chain's randomness for the subject (MyPalletId, seed).encode() = the 8 PalletId bytes ++ seed as
 * u32 LE (12 bytes; the audit pallet's id is SegbkPalletId = b"rewardpt", runtime/src/lib.rs:
 * 984,1004), and decodes the output's first 8 bytes as a little-endian u64. The randomness itself
 * (pallet_rrsc::ParentBlockRandomness) is chain state: a host holding it reproduces the inputs of
 * cec_challenge_indices with these two. */
#define CEC_AUDIT_PALLET_ID "rewardpt"
int cec_audit_random_subject(const uint8_t* pallet_id /* 8 bytes */, uint32_t seed,
                             uint8_t* out12);
int cec_audit_random_u64(const uint8_t* randomness, size_t len, uint64_t* out);
/* The challenge's random_list (NetSnapShot.random_list, c-pallets/audit/src/lib.rs:966-974): for
 * seed = now + 1, now + 2, ... (now = the block number), generate_challenge_random(seed)
 * (lib.rs:1079-1096) asks the randomness for the subject (MyPalletId, seed + 1) and keeps the first
 * 20 bytes of the H256 output; values already listed are skipped, until need = 47 values.
 * `randomness` holds nrand outputs of CEC_RANDOMNESS_BYTES each, output i being the chain's
 * randomness for cec_audit_random_subject(pallet, now + 2 + i) (a None output as 32 zero bytes,
 * the pallet's Default). Writes need * CEC_CHALLENGE_RANDOM_BYTES bytes to `out`; *used = outputs
 * consumed. CEC_EINVAL when the stream runs out first. Host only. */
#define CEC_RANDOMNESS_BYTES 32
#define CEC_CHALLENGE_RANDOM_BYTES 20
int cec_challenge_random_list(const uint8_t* randomness, size_t nrand, uint32_t need,
                              uint8_t* out, size_t* used);
/* 68-byte shard id = 64 hex chars ++ "-NNN" (index 0..999), the form Hash::from_shard_id reads
 * back (primitives/common/src/lib.rs:45-49; c-pallets/audit/src/tests.rs:267-269 builds
 * file_hash ++ "-001"). */
int cec_shard_id(const uint8_t* hash_hex, uint32_t index, uint8_t* out68);
/* Hash::from_shard_id: the first 64 bytes. */
int cec_hash_from_shard_id(const uint8_t* shard_id68, uint8_t* hash_hex_out);

/* Synthetic segments in HBM: little-endian 64-bit word w of segment s is
 * splitmix64(seed ^ ((seg0 + s) << 32) ^ w). seg_bytes must be a multiple of 8. */
int cec_fill_synthetic(uint8_t* d_out, size_t seg_bytes, size_t nseg, uint64_t seg0,
                       uint64_t seed, void* hip_stream);

/* Options, per codec (distinct codecs never affect each other). */
#define CEC_OPT_FORCE_GENERIC 1 /* 1: always use the run-time-coefficient kernel */
#define CEC_OPT_CT_VARIANT 2    /* compile-time kernel variant for tuning sweeps: -1 = default;
                                   other values need the tuning build (libcessec_tune.so) */
#define CEC_OPT_SHA_MODE 3      /* cec_sha256_batch kernel: 0 = auto, 1 = one wave per 64
                                   buffers, 2 = two waves (schedule producer + rounds consumer),
                                   3 = a producer + two consumer waves on lane pairs (the shortest
                                   chain latency; auto picks it for up to 341 x 64 buffers) */
#define CEC_OPT_RT_MODE 4       /* run-time-coefficient kernel: 0 = Horner over input groups
                                   with index-mode table XORs when 4 <= inputs <= 32, 1 = always
                                   the per-bit mask kernel, 2 = Horner with v_mov table reads */
#define CEC_OPT_DECODE_CACHE 6  /* capacity (>= 1) of the decode-program LRU cache, one entry
                                   per erasure pattern (default 4096) */
#define CEC_OPT_FFTDEC_MIN 7    /* RS(32,32): rebuilds of at least this many shards per segment
                                   may run the FFT-domain erasure decoder (0 = never; default 4) */
#define CEC_OPT_FFTDEC_MODE 8   /* RS(32,32), rebuilds past CEC_OPT_FFTDEC_MIN: 0 = the cheapest
                                   of the FFT-domain decoders (syndrome rows, formal derivative) and
                                   the run-time matrix kernel by the cost model (default), 1 = always
                                   the syndrome-row decoder, 2 = always the formal-derivative one.
                                   Both FFT-domain decoders address a coset's 32 shards with 32-bit
                                   buffer offsets, so they run only where shard_len is a multiple of
                                   1024, every base is 16-byte aligned and the shard stride
                                   (shard_len in the batch layout) is below 64 MiB (2^26); from
                                   64 MiB on, whatever CEC_OPT_FFTDEC_MIN and this option say, the
                                   run-time matrix kernels rebuild and the FFTDEC counters stay */
int cec_set_option(cec_codec* codec, int option, int value);
/* Counters (tests / monitoring). */
#define CEC_STAT_DECODE_CACHED 1   /* erasure patterns in the decode cache */
#define CEC_STAT_RETIRED_PENDING 2 /* device blocks retired but possibly still read by queued
                                      kernels (released once those complete) */
#define CEC_STAT_POOL_BYTES 3      /* HBM held by the codec's block pool (programs, plans, small
                                      scratch, the pointer tables of cec_reconstruct_ptrs: 8 bytes
                                      per address, reused call after call); batch-sized scratch is
                                      stream-ordered and is not held after the call's launches
                                      complete */
#define CEC_STAT_FFTDEC_SEGMENTS 4 /* segments rebuilt by the RS(32,32) FFT-domain decoders so far
                                      (the rest of a rebuild ran the run-time matrix kernels) */
#define CEC_STAT_FFTDEC_D_SEGMENTS 5 /* of those, segments rebuilt by the formal-derivative decoder */
int cec_get_stat(const cec_codec* codec, int stat, uint64_t* value);

#ifdef __cplusplus
}
#endif

#endif /* CESS_EC_H */
