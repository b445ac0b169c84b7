//! `ec-hip`: the CESS segment -> fragment Reed-Solomon codec on MI355X (gfx950), a thin Rust layer
//! over libcessec's C ABI (`include/cess_ec.h`).
//!
//! The API follows `reed-solomon-erasure` (`ReedSolomon::new(k, m)`, `encode`, `reconstruct`,
//! `reconstruct_data`, `verify`) so the uploader / miner tools that produce the chain's records
//! (`SegmentList { hash, fragment_list }`, c-pallets/file-bank/src/types.rs:13-16, submitted with
//! `upload_declaration`, c-pallets/file-bank/src/lib.rs:419-428) swap codecs without changing
//! their call sites. `Pipeline` streams whole files through the GPU (pinned multi-buffered copies,
//! encode, GPU SegmentList hashes); `deal_info` builds the SCALE bytes of the extrinsic argument.
#![allow(non_camel_case_types)]

use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_longlong, c_void};

#[repr(C)]
pub struct cec_codec {
    _p: [u8; 0],
}
#[repr(C)]
pub struct cec_pipeline {
    _p: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct cec_pipeline_opts {
    pub shard_len: usize,
    pub batch_segments: usize,
    pub depth: c_int,
    pub hash: c_int,
    pub window: c_int,
    pub max_segments: u64,
    /// host SHA-256 threads for hash = 2 (host) / 3 (hybrid); 0 = 16
    pub host_threads: c_int,
    /// hash = 3: batches at the end of the last source hashed wholly on the host (-1 = auto)
    pub tail_batches: c_int,
}

/// `cec_pipeline_opts.hash`: where the SegmentList hashes run.
pub const CEC_PIPE_HASH_NONE: c_int = 0;
pub const CEC_PIPE_HASH_GPU: c_int = 1;
pub const CEC_PIPE_HASH_HOST: c_int = 2;
pub const CEC_PIPE_HASH_HYBRID: c_int = 3;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct cec_pipeline_stats {
    pub segments: u64,
    pub bytes_in: u64,
    pub seconds: f64,
    pub read_seconds: f64,
    pub wait_seconds: f64,
}

pub type cec_read_fn = extern "C" fn(user: *mut c_void, dst: *mut u8, cap: usize) -> c_longlong;
pub type cec_fragments_fn =
    extern "C" fn(user: *mut c_void, seg: u64, shards: *const *const u8, shard_len: usize) -> c_int;
pub type cec_record_fn =
    extern "C" fn(user: *mut c_void, seg: u64, seg_hex: *const u8, frag_hex: *const u8) -> c_int;
pub type cec_file_fragments_fn = extern "C" fn(user: *mut c_void, file: usize, seg: u64,
                                               shards: *const *const u8, shard_len: usize)
                                               -> c_int;
pub type cec_file_record_fn = extern "C" fn(user: *mut c_void, file: usize, seg: u64,
                                            seg_hex: *const u8, frag_hex: *const u8) -> c_int;
pub type cec_file_done_fn =
    extern "C" fn(user: *mut c_void, file: usize, stats: *const cec_pipeline_stats) -> c_int;

/// One source of `cec_pipeline_run_files`: its read callback, that callback's user pointer and
/// the source's size in bytes (0 = unknown).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cec_source {
    pub read: cec_read_fn,
    pub user: *mut c_void,
    pub size: u64,
}

extern "C" {
    pub fn cec_strerror(code: c_int) -> *const c_char;
    pub fn cec_last_error() -> *const c_char;
    pub fn cec_create(k: c_int, m: c_int, device: c_int, out: *mut *mut cec_codec) -> c_int;
    pub fn cec_destroy(c: *mut cec_codec);
    pub fn cec_encode(c: *mut cec_codec, shards: *const *mut u8, shard_len: usize) -> c_int;
    pub fn cec_reconstruct(c: *mut cec_codec, shards: *const *mut u8, present: *const u8,
                           shard_len: usize, data_only: c_int) -> c_int;
    pub fn cec_verify(c: *mut cec_codec, shards: *const *mut u8, shard_len: usize,
                      ok: *mut c_int) -> c_int;
    pub fn cec_pipeline_create(c: *mut cec_codec, opts: *const cec_pipeline_opts,
                               out: *mut *mut cec_pipeline) -> c_int;
    pub fn cec_pipeline_destroy(p: *mut cec_pipeline);
    pub fn cec_pipeline_run(p: *mut cec_pipeline, read: cec_read_fn,
                            on_fragments: Option<cec_fragments_fn>,
                            on_record: Option<cec_record_fn>, user: *mut c_void,
                            stats: *mut cec_pipeline_stats) -> c_int;
    pub fn cec_pipeline_info(p: *const cec_pipeline, window: *mut c_int,
                             device_slots: *mut c_int, depth: *mut c_int) -> c_int;
    pub fn cec_pipeline_run_files(p: *mut cec_pipeline, sources: *const cec_source,
                                  nsources: usize, on_fragments: Option<cec_file_fragments_fn>,
                                  on_record: Option<cec_file_record_fn>,
                                  on_done: Option<cec_file_done_fn>, user: *mut c_void,
                                  stats: *mut cec_pipeline_stats) -> c_int;
    pub fn cec_sha256_host(bufs: *const *const u8, n: usize, len: usize, hex: *mut u8,
                           prefix_len: usize, prefix_hex: *mut u8, threads: c_int) -> c_int;
    pub fn cec_sha256_host_state(bufs: *const *const u8, n: usize, len: usize, hex: *mut u8,
                                 state_out: *mut u32, threads: c_int) -> c_int;
    pub fn cec_host_sha_set_form(form: c_int) -> c_int;
    pub fn cec_host_sha_form() -> c_int;
    pub fn cec_host_sha_pool_threads() -> c_int;
    pub fn cec_host_sha_probe(form: c_int, bytes_per_chain: usize, chains: c_int) -> f64;
    pub fn cec_scale_deal_info(seg_hex: *const u8, frag_hex: *const u8, nseg: usize,
                               nfrag: usize, out: *mut u8, out_cap: usize,
                               out_len: *mut usize) -> c_int;
}

/// The rest of `include/cess_ec.h`, declared one to one (HBM-resident batches, hash queue,
/// audit chunks, records, the multi-GPU degraded read). Device pointers are `*mut u8` /
/// `*const u8`; HIP streams are `*mut c_void` (null = the null stream).
pub mod sys {
    use super::{cec_codec, c_char, c_int, c_void};

    #[repr(C)]
    pub struct cec_hashq {
        _p: [u8; 0],
    }
    #[repr(C)]
    pub struct cec_dist {
        _p: [u8; 0],
    }
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default)]
    pub struct cec_dist_move {
        pub seg: u64,
        pub frag: i32,
        pub src: i32,
        pub dst: i32,
        pub kind: i32,
    }
    pub const CEC_DIST_ID_BYTES: usize = 128;
    pub const CEC_DIST_SURVIVOR: i32 = 0;
    pub const CEC_DIST_PARTIAL: i32 = 1;
    pub const CEC_DIST_OPT_EXCHANGE: c_int = 1;
    pub const CEC_DIST_OPT_GROUP_OPS: c_int = 3;
    pub type cec_locate_fn = extern "C" fn(user: *mut c_void, seg: u64, frag: c_int) -> *const u8;

    extern "C" {
        pub fn cec_version() -> *const c_char;
        pub fn cec_device_count() -> c_int;
        pub fn cec_codec_info(c: *const cec_codec, k: *mut c_int, m: *mut c_int,
                              device: *mut c_int) -> c_int;
        pub fn cec_matrix(c: *const cec_codec, out: *mut u8) -> c_int;
        pub fn cec_encode_batch(c: *mut cec_codec, d_data: *const u8, d_parity: *mut u8,
                                nseg: usize, shard_len: usize, stream: *mut c_void) -> c_int;
        pub fn cec_reconstruct_batch(c: *mut cec_codec, d_data: *mut u8, d_parity: *mut u8,
                                     nseg: usize, shard_len: usize, present: *const u8,
                                     per_segment: c_int, data_only: c_int,
                                     stream: *mut c_void) -> c_int;
        pub fn cec_decode_rows(k: c_int, m: c_int, present: *const u8, required: *const u8,
                               rows: *mut u8, out_idx: *mut u8, nreq: *mut c_int) -> c_int;
        pub fn cec_reconstruct_some_batch(c: *mut cec_codec, d_data: *mut u8, d_parity: *mut u8,
                                          nseg: usize, shard_len: usize, present: *const u8,
                                          required: *const u8, per_segment: c_int,
                                          stream: *mut c_void) -> c_int;
        pub fn cec_reconstruct_ptrs(c: *mut cec_codec, src: *const *const u8,
                                    dst: *const *mut u8, nseg: usize, shard_len: usize,
                                    stream: *mut c_void) -> c_int;
        pub fn cec_encode_ptrs(c: *mut cec_codec, d_data_ptrs: *const *const u8,
                               d_parity_ptrs: *const *mut u8, nseg: usize, shard_len: usize,
                               stream: *mut c_void) -> c_int;
        pub fn cec_reconstruct_partial_batch(c: *mut cec_codec, d_data: *mut u8,
                                             d_parity: *mut u8, nseg: usize, shard_len: usize,
                                             present: *const u8, held: *const u8,
                                             data_only: c_int, stream: *mut c_void) -> c_int;
        pub fn cec_verify_batch(c: *mut cec_codec, d_data: *const u8, d_parity: *const u8,
                                nseg: usize, shard_len: usize, d_ok: *mut u8,
                                stream: *mut c_void) -> c_int;
        pub fn cec_verify_ptrs(c: *mut cec_codec, src: *const *const u8,
                               expect: *const *const u8, nseg: usize, shard_len: usize,
                               d_ok: *mut u8, stream: *mut c_void) -> c_int;
        pub fn cec_xor_batch(d_dst: *mut u8, d_src: *const u8, nsrc: usize, src_stride: usize,
                             len: usize, stream: *mut c_void) -> c_int;
        pub fn cec_reconstruct_partial_ptrs(c: *mut cec_codec, src: *const *const u8,
                                            dst: *const *mut u8, present: *const u8,
                                            nseg: usize, shard_len: usize, accumulate: c_int,
                                            stream: *mut c_void) -> c_int;
        pub fn cec_xor_ptrs(c: *mut cec_codec, dst: *const *mut u8, src: *const *const u8,
                            nrows: usize, nsrc: usize, len: usize,
                            stream: *mut c_void) -> c_int;
        pub fn cec_flag_status(k: c_int, m: c_int, held: *const u8, flags: *const u8,
                               status: *mut c_int, lost: *mut c_int) -> c_int;
        pub fn cec_repair_flagged_ptrs(c: *mut cec_codec, shards: *const *mut u8,
                                       d_flags: *const u8, nseg: usize, shard_len: usize,
                                       d_status: *mut u8, stream: *mut c_void) -> c_int;
        pub fn cec_flag_status_multi(k: c_int, m: c_int, held: *const u8, flags: *const u8,
                                     max_bad: c_int, status: *mut c_int, nlost: *mut c_int,
                                     lost: *mut u8) -> c_int;
        pub fn cec_flag_solve(k: c_int, m: c_int, held: *const u8, flags: *const u8,
                              max_bad: c_int, status: *mut c_int, nout: *mut c_int,
                              out_idx: *mut u8, in_idx: *mut u8, rows: *mut u8) -> c_int;
        pub fn cec_repair_flagged_multi_ptrs(c: *mut cec_codec, shards: *const *mut u8,
                                             d_flags: *const u8, nseg: usize, shard_len: usize,
                                             max_bad: c_int, d_status: *mut u8,
                                             stream: *mut c_void) -> c_int;
        pub fn cec_read_status(k: c_int, m: c_int, held: *const u8, flags: *const u8,
                               wanted: *const u8, max_bad: c_int, status: *mut c_int,
                               nmiss: *mut c_int, miss_idx: *mut u8) -> c_int;
        pub fn cec_read_solve(k: c_int, m: c_int, held: *const u8, flags: *const u8,
                              wanted: *const u8, max_bad: c_int, status: *mut c_int,
                              nout: *mut c_int, out_idx: *mut u8, in_idx: *mut u8, rows: *mut u8,
                              copy_idx: *mut u8, ncopy: *mut c_int) -> c_int;
        pub fn cec_read_flagged_ptrs(c: *mut cec_codec, shards: *const *const u8,
                                     d_flags: *const u8, dst: *const *mut u8, nseg: usize,
                                     shard_len: usize, max_bad: c_int, d_status: *mut u8,
                                     stream: *mut c_void) -> c_int;
        pub fn cec_locate_rows(k: c_int, m: c_int, held: *const u8, nsyn: c_int, r: *mut c_int,
                               rows: *mut u8) -> c_int;
        pub fn cec_locate_host(k: c_int, m: c_int, shards: *const *const u8, shard_len: usize,
                               nsyn: c_int, status: *mut c_int, found: *mut c_int) -> c_int;
        pub fn cec_locate_ptrs(c: *mut cec_codec, shards: *const *const u8, nseg: usize,
                               shard_len: usize, nsyn: c_int, d_flags: *mut u8,
                               d_status: *mut u8, stream: *mut c_void) -> c_int;
        pub fn cec_locate_multi_host(k: c_int, m: c_int, shards: *const *const u8,
                                     shard_len: usize, nsyn: c_int, max_bad: c_int,
                                     status: *mut c_int, nfound: *mut c_int,
                                     found: *mut c_int) -> c_int;
        pub fn cec_locate_multi_ptrs(c: *mut cec_codec, shards: *const *const u8, nseg: usize,
                                     shard_len: usize, nsyn: c_int, max_bad: c_int,
                                     d_flags: *mut u8, d_status: *mut u8, d_nbad: *mut u8,
                                     stream: *mut c_void) -> c_int;
        pub fn cec_encode_idx_batch(c: *mut cec_codec, d_shard: *const u8,
                                    shard_seg_stride: usize, idx: c_int, d_parity: *mut u8,
                                    nseg: usize, shard_len: usize, accumulate: c_int,
                                    stream: *mut c_void) -> c_int;
        pub fn cec_update_batch(c: *mut cec_codec, d_old: *const u8, d_new: *const u8,
                                d_parity: *mut u8, nseg: usize, shard_len: usize,
                                changed: *const u8, stream: *mut c_void) -> c_int;
        pub fn cec_encode_idx_ptrs(c: *mut cec_codec, data: *const *const u8,
                                   parity: *const *mut u8, nseg: usize, shard_len: usize,
                                   accumulate: c_int, stream: *mut c_void) -> c_int;
        pub fn cec_update_ptrs(c: *mut cec_codec, old_data: *const *const u8,
                               new_data: *const *const u8, parity: *const *mut u8, nseg: usize,
                               shard_len: usize, stream: *mut c_void) -> c_int;
        pub fn cec_encode_idx(c: *mut cec_codec, data_shard: *const u8, idx: c_int,
                              parity: *const *mut u8, shard_len: usize) -> c_int;
        pub fn cec_update(c: *mut cec_codec, shards: *const *mut u8,
                          new_data: *const *const u8, shard_len: usize) -> c_int;
        pub fn cec_sha256_batch(c: *mut cec_codec, d_data: *const u8, d_parity: *const u8,
                                nseg: usize, shard_len: usize, d_hex: *mut u8,
                                stream: *mut c_void) -> c_int;
        pub fn cec_sha256_hex(d_bufs: *const *const u8, n: usize, len: usize, hex: *mut u8,
                              stream: *mut c_void) -> c_int;
        pub fn cec_hashq_create(device: c_int, capacity: usize, stream: *mut c_void,
                                out: *mut *mut cec_hashq) -> c_int;
        pub fn cec_hashq_destroy(q: *mut cec_hashq);
        pub fn cec_hashq_add(q: *mut cec_hashq, d_base: *const u8, n: usize, per: usize,
                             outer_stride: usize, inner_stride: usize, len: usize,
                             d_hex: *mut u8, hex_outer: usize, ticket: *mut u64) -> c_int;
        pub fn cec_hashq_add_resume(q: *mut cec_hashq, d_base: *const u8, n: usize, per: usize,
                                    outer_stride: usize, inner_stride: usize, len: usize,
                                    start_len: usize, d_states: *const u32, d_hex: *mut u8,
                                    hex_outer: usize, ticket: *mut u64) -> c_int;
        pub fn cec_hashq_add_prefix(q: *mut cec_hashq, d_base: *const u8, n: usize, per: usize,
                                    outer_stride: usize, inner_stride: usize, len: usize,
                                    d_hex: *mut u8, hex_outer: usize, prefix_len: usize,
                                    d_prefix_hex: *mut u8, prefix_hex_outer: usize,
                                    ticket: *mut u64) -> c_int;
        pub fn cec_hashq_add_ptrs(q: *mut cec_hashq, d_bufs: *const *const u8, n: usize,
                                  len: usize, d_hex: *mut u8, ticket: *mut u64) -> c_int;
        pub fn cec_hashq_add_concat_ptrs(q: *mut cec_hashq, d_parts: *const *const u8, n: usize,
                                         parts: usize, part_len: usize, len: usize,
                                         d_hex: *mut u8, d_prefix_hex: *mut u8,
                                         ticket: *mut u64) -> c_int;
        pub fn cec_hashq_add_check(q: *mut cec_hashq, d_base: *const u8, n: usize, per: usize,
                                   outer_stride: usize, inner_stride: usize, len: usize,
                                   d_expect: *const u8, expect_outer: usize, d_ok: *mut u8,
                                   ok_outer: usize, d_hex: *mut u8, hex_outer: usize,
                                   ticket: *mut u64) -> c_int;
        pub fn cec_hashq_add_check_concat_ptrs(q: *mut cec_hashq, d_parts: *const *const u8,
                                               n: usize, parts: usize, part_len: usize,
                                               len: usize, d_expect: *const u8, d_ok: *mut u8,
                                               d_hex: *mut u8, d_prefix_hex: *mut u8,
                                               ticket: *mut u64) -> c_int;
        pub fn cec_hashq_add_check_where_ptrs(q: *mut cec_hashq, d_bufs: *const *const u8,
                                              n: usize, len: usize, d_expect: *const u8,
                                              d_flags: *const u8, per: usize, d_gate: *const u8,
                                              gate: c_int, d_ok: *mut u8, d_hex: *mut u8,
                                              ticket: *mut u64) -> c_int;
        pub fn cec_hashq_where_plan(held: *const u8, flags: *const u8, n: usize, per: usize,
                                    gate_bytes: *const u8, gate: c_int, pos: *mut u32,
                                    nsel: *mut usize) -> c_int;
        pub fn cec_confirm_rule(n: c_int, status: c_int, ok: *const u8,
                                confirm: *mut c_int) -> c_int;
        pub fn cec_confirm_flagged(d_status: *const u8, d_ok: *const u8, nseg: usize, n: c_int,
                                   d_confirm: *mut u8, stream: *mut c_void) -> c_int;
        pub fn cec_hashq_tick(q: *mut cec_hashq, max_blocks: u32) -> c_int;
        pub fn cec_hashq_finish(q: *mut cec_hashq) -> c_int;
        pub fn cec_hashq_status(q: *const cec_hashq, ticket: u64, done: *mut c_int,
                                live_chains: *mut usize, blocks_left: *mut u64) -> c_int;
        pub fn cec_hashq_set_option(q: *mut cec_hashq, option: c_int, value: c_int) -> c_int;
        pub fn cec_split_segment(seg: *const u8, seg_len: usize, k: c_int,
                                 shards: *const *mut u8, shard_len: usize) -> c_int;
        pub fn cec_challenge_indices(randoms: *const u64, nrand: usize, chunk_count: u32,
                                     need: u32, out: *mut u32, used: *mut usize) -> c_int;
        pub fn cec_audit_chunks(c: *mut cec_codec, d_data: *const u8, d_parity: *const u8,
                                nseg: usize, shard_len: usize, chunk_count: u32,
                                indices: *const u32, nidx: u32, d_chunks: *mut u8,
                                d_hex: *mut u8, stream: *mut c_void) -> c_int;
        pub fn cec_audit_chunks_ptrs(c: *mut cec_codec, frags: *const *const u8, nfrag: usize,
                                     shard_len: usize, chunk_count: u32, indices: *const u32,
                                     nidx: u32, d_chunks: *mut u8, d_hex: *mut u8,
                                     stream: *mut c_void) -> c_int;
        pub fn cec_scale_compact(n: u32, out: *mut u8, out_cap: usize, out_len: *mut usize)
                                 -> c_int;
        pub fn cec_scale_upload_declaration(file_hash_hex: *const u8, seg_hex: *const u8,
                                            frag_hex: *const u8, nseg: usize, nfrag: usize,
                                            account: *const u8, file_name: *const u8,
                                            file_name_len: usize, bucket_name: *const u8,
                                            bucket_name_len: usize, out: *mut u8,
                                            out_cap: usize, out_len: *mut usize) -> c_int;
        pub fn cec_shard_id(hash_hex: *const u8, index: u32, out68: *mut u8) -> c_int;
        pub fn cec_hash_from_shard_id(shard_id68: *const u8, hash_hex_out: *mut u8) -> c_int;
        pub fn cec_scale_upload_filler(tee_worker: *const u8, block_num: *const u32,
                                       miners: *const u8, filler_hex: *const u8, n: usize,
                                       out: *mut u8, out_cap: usize, out_len: *mut usize)
                                       -> c_int;
        pub fn cec_scale_generate_restoral_order(file_hash_hex: *const u8,
                                                 fragment_hex: *const u8, out: *mut u8,
                                                 out_cap: usize, out_len: *mut usize) -> c_int;
        pub fn cec_scale_claim_restoral_order(fragment_hex: *const u8, out: *mut u8,
                                              out_cap: usize, out_len: *mut usize) -> c_int;
        pub fn cec_scale_claim_restoral_exist_order(miner: *const u8, file_hash_hex: *const u8,
                                                    fragment_hex: *const u8, out: *mut u8,
                                                    out_cap: usize, out_len: *mut usize)
                                                    -> c_int;
        pub fn cec_scale_restoral_order_complete(fragment_hex: *const u8, out: *mut u8,
                                                 out_cap: usize, out_len: *mut usize) -> c_int;
        pub fn cec_audit_random_subject(pallet_id: *const u8, seed: u32, out12: *mut u8)
                                        -> c_int;
        pub fn cec_audit_random_u64(randomness: *const u8, len: usize, out: *mut u64) -> c_int;
        pub fn cec_survivors(k: c_int, m: c_int, present: *const u8, survivors: *mut u8) -> c_int;
        pub fn cec_challenge_random_list(randomness: *const u8, nrand: usize, need: u32,
                                         out: *mut u8, used: *mut usize) -> c_int;
        pub fn cec_fill_synthetic(d_out: *mut u8, seg_bytes: usize, nseg: usize, seg0: u64,
                                  seed: u64, stream: *mut c_void) -> c_int;
        pub fn cec_set_option(c: *mut cec_codec, option: c_int, value: c_int) -> c_int;
        pub fn cec_get_stat(c: *const cec_codec, stat: c_int, value: *mut u64) -> c_int;
        pub fn cec_dist_unique_id(id: *mut u8) -> c_int;
        pub fn cec_dist_create(c: *mut cec_codec, id: *const u8, world: c_int, rank: c_int,
                               out: *mut *mut cec_dist) -> c_int;
        pub fn cec_dist_destroy(d: *mut cec_dist);
        pub fn cec_dist_plan(k: c_int, m: c_int, world: c_int, lost_seg: *const u64,
                             lost_frag: *const u8, nlost: usize, moves: *mut cec_dist_move,
                             moves_cap: usize, nmoves: *mut usize, decoder: *mut i32) -> c_int;
        pub fn cec_dist_plan_ex(k: c_int, m: c_int, world: c_int, exchange: c_int,
                                lost_seg: *const u64, lost_frag: *const u8, nlost: usize,
                                moves: *mut cec_dist_move, moves_cap: usize, nmoves: *mut usize,
                                decoder: *mut i32) -> c_int;
        pub fn cec_dist_set_option(d: *mut cec_dist, option: c_int, value: c_int) -> c_int;
        pub fn cec_dist_groups(d: *const cec_dist, groups: *mut u64) -> c_int;
        pub fn cec_dist_plan_groups(k: c_int, m: c_int, world: c_int, exchange: c_int,
                                    group_ops: c_int, lost_seg: *const u64, lost_frag: *const u8,
                                    nlost: usize, starts: *mut u64, starts_cap: usize,
                                    ngroups: *mut usize) -> c_int;
        pub fn cec_dist_degraded_read(d: *mut cec_dist, lost_seg: *const u64,
                                      lost_frag: *const u8, nlost: usize, shard_len: usize,
                                      locate: cec_locate_fn, user: *mut c_void,
                                      d_out: *const *mut u8, stream: *mut c_void,
                                      nrebuilt: *mut usize) -> c_int;
    }
}

/// One rank's share of the multi-GPU degraded read (libcessec's own RCCL group): fragment f of
/// segment s lives on rank (s + f) mod world (random_assign_miner's spread,
/// c-pallets/file-bank/src/functions.rs:187-283).
pub struct DistGroup<'c> {
    d: *mut sys::cec_dist,
    _codec: std::marker::PhantomData<&'c ReedSolomon>,
}

extern "C" fn locate_cb(user: *mut c_void, seg: u64, frag: c_int) -> *const u8 {
    let f = unsafe { &mut *(user as *mut &mut dyn FnMut(u64, usize) -> *const u8) };
    f(seg, frag as usize)
}

impl<'c> DistGroup<'c> {
    /// A fresh group id (on one rank; hand it to the others out of band).
    pub fn unique_id() -> Result<[u8; sys::CEC_DIST_ID_BYTES], Error> {
        let mut id = [0u8; sys::CEC_DIST_ID_BYTES];
        check(unsafe { sys::cec_dist_unique_id(id.as_mut_ptr()) })?;
        Ok(id)
    }

    /// Join as `rank` of `world` (collective over the ranks).
    pub fn join(codec: &'c ReedSolomon, id: &[u8; sys::CEC_DIST_ID_BYTES], world: i32,
                rank: i32) -> Result<Self, Error> {
        let mut d = std::ptr::null_mut();
        check(unsafe { sys::cec_dist_create(codec.c, id.as_ptr(), world, rank, &mut d) })?;
        Ok(DistGroup { d, _codec: std::marker::PhantomData })
    }

    /// Exchange of later degraded reads: 0 survivors, 1 partial products, 2 per segment
    /// whichever moves fewer fragments (the default of a new group; the same value on every
    /// rank).
    pub fn set_exchange(&mut self, exchange: i32) -> Result<(), Error> {
        check(unsafe { sys::cec_dist_set_option(self.d, sys::CEC_DIST_OPT_EXCHANGE, exchange) })
    }

    /// At most `ops` point-to-point transfers per rank in one RCCL group (default 1024; 0 = one
    /// group per round of 256 segments; the same value on every rank).
    pub fn set_group_ops(&mut self, ops: i32) -> Result<(), Error> {
        check(unsafe { sys::cec_dist_set_option(self.d, sys::CEC_DIST_OPT_GROUP_OPS, ops) })
    }

    /// Transfer groups this handle has issued so far.
    pub fn groups(&self) -> Result<u64, Error> {
        let mut g = 0u64;
        check(unsafe { sys::cec_dist_groups(self.d, &mut g) })?;
        Ok(g)
    }

    /// Rebuild the `lost` (segment, fragment) list, the same on every rank; `locate(seg, frag)`
    /// gives the device address of a fragment this rank holds (null if absent); `out[i]` receives
    /// lost entry i when this rank rebuilds it. Returns the number rebuilt here.
    pub fn degraded_read(&mut self, lost: &[(u64, u8)], shard_len: usize,
                         mut locate: impl FnMut(u64, usize) -> *const u8,
                         out: &[*mut u8]) -> Result<usize, Error> {
        let segs: Vec<u64> = lost.iter().map(|l| l.0).collect();
        let frags: Vec<u8> = lost.iter().map(|l| l.1).collect();
        let mut f: &mut dyn FnMut(u64, usize) -> *const u8 = &mut locate;
        let mut n = 0usize;
        check(unsafe {
            sys::cec_dist_degraded_read(self.d, segs.as_ptr(), frags.as_ptr(), lost.len(),
                                        shard_len, locate_cb,
                                        &mut f as *mut _ as *mut c_void,
                                        if out.is_empty() { std::ptr::null() } else { out.as_ptr() },
                                        std::ptr::null_mut(), &mut n)
        })?;
        Ok(n)
    }
}

impl Drop for DistGroup<'_> {
    fn drop(&mut self) {
        unsafe { sys::cec_dist_destroy(self.d) }
    }
}

pub const CEC_EINVAL: c_int = -1;
pub const CEC_ETOOFEW: c_int = -2;
pub const CEC_ESHARDLEN: c_int = -3;
pub const CEC_ESEGCOUNT: c_int = -9;
pub const CEC_FLAG_CLEAN: c_int = 0;
pub const CEC_FLAG_REBUILT: c_int = 1;
pub const CEC_FLAG_MANY: c_int = 2;
pub const CEC_FLAG_LOST: c_int = 3;
pub const CEC_FLAG_MULTI_MAX: c_int = 4;
pub const CEC_LOCATE_SYN_MAX: c_int = 4;
pub const CEC_LOCATE_CLEAN: c_int = 0;
pub const CEC_LOCATE_FOUND: c_int = 1;
pub const CEC_LOCATE_AMBIGUOUS: c_int = 2;
pub const CEC_LOCATE_UNCHECKED: c_int = 3;
pub const CEC_LOCATE_BAD_MAX: c_int = 2;
pub const CEC_CONFIRM_NONE: c_int = 0;
pub const CEC_CONFIRM_PROVEN: c_int = 1;
pub const CEC_CONFIRM_REFUTED: c_int = 2;
pub const CEC_HASHQ_SKIPPED: u8 = 2;
pub const SEGMENT_COUNT: usize = 1000; // runtime/src/lib.rs:1026
pub const FRAGMENT_COUNT: usize = 3; // runtime/src/lib.rs:1027

/// A libcessec error: the C code and its message.
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct Error {
    pub code: i32,
    pub message: String,
}

impl Error {
    fn from_code(code: c_int) -> Self {
        let msg = unsafe {
            let s = CStr::from_ptr(cec_strerror(code)).to_string_lossy().into_owned();
            let d = CStr::from_ptr(cec_last_error()).to_string_lossy().into_owned();
            if d.is_empty() { s } else { format!("{s} ({d})") }
        };
        Error { code, message: msg }
    }
}

impl std::fmt::Display for Error {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "libcessec error {}: {}", self.code, self.message)
    }
}

impl std::error::Error for Error {}

fn check(code: c_int) -> Result<(), Error> {
    if code == 0 { Ok(()) } else { Err(Error::from_code(code)) }
}

/// One codec bound to one GPU (`reed_solomon_erasure::ReedSolomon` shape).
pub struct ReedSolomon {
    c: *mut cec_codec,
    k: usize,
    m: usize,
}

unsafe impl Send for ReedSolomon {}

impl ReedSolomon {
    pub fn new(data_shards: usize, parity_shards: usize) -> Result<Self, Error> {
        Self::on_device(data_shards, parity_shards, 0)
    }

    pub fn on_device(data_shards: usize, parity_shards: usize, device: i32) -> Result<Self, Error> {
        let mut c = std::ptr::null_mut();
        check(unsafe { cec_create(data_shards as c_int, parity_shards as c_int, device, &mut c) })?;
        Ok(ReedSolomon { c, k: data_shards, m: parity_shards })
    }

    pub fn data_shard_count(&self) -> usize { self.k }
    pub fn parity_shard_count(&self) -> usize { self.m }
    pub fn total_shard_count(&self) -> usize { self.k + self.m }

    fn ptrs(shards: &mut [&mut [u8]]) -> Result<(Vec<*mut u8>, usize), Error> {
        let len = shards.first().map(|s| s.len()).unwrap_or(0);
        if len == 0 || shards.iter().any(|s| s.len() != len) {
            return Err(Error::from_code(CEC_ESHARDLEN));
        }
        Ok((shards.iter_mut().map(|s| s.as_mut_ptr()).collect(), len))
    }

    /// Parity shards `shards[k..]` from data shards `shards[..k]`, in place.
    pub fn encode(&self, shards: &mut [&mut [u8]]) -> Result<(), Error> {
        if shards.len() != self.k + self.m {
            return Err(Error::from_code(CEC_ETOOFEW));
        }
        let (p, len) = Self::ptrs(shards)?;
        check(unsafe { cec_encode(self.c, p.as_ptr(), len) })
    }

    pub fn verify(&self, shards: &mut [&mut [u8]]) -> Result<bool, Error> {
        let (p, len) = Self::ptrs(shards)?;
        let mut ok: c_int = 0;
        check(unsafe { cec_verify(self.c, p.as_ptr(), len, &mut ok) })?;
        Ok(ok != 0)
    }

    fn reconstruct_inner(&self, shards: &mut [Option<Vec<u8>>], data_only: bool) -> Result<(), Error> {
        let n = self.k + self.m;
        if shards.len() != n {
            return Err(Error::from_code(CEC_ETOOFEW));
        }
        let len = shards.iter().flatten().map(|s| s.len()).next().ok_or(Error::from_code(CEC_ETOOFEW))?;
        let present: Vec<u8> = shards.iter().map(|s| s.is_some() as u8).collect();
        for (i, s) in shards.iter_mut().enumerate() {
            if s.is_none() && (i < self.k || !data_only) {
                *s = Some(vec![0u8; len]);
            }
        }
        let mut scratch = vec![0u8; len];
        let p: Vec<*mut u8> = shards
            .iter_mut()
            .map(|s| match s { Some(v) => v.as_mut_ptr(), None => scratch.as_mut_ptr() })
            .collect();
        check(unsafe { cec_reconstruct(self.c, p.as_ptr(), present.as_ptr(), len, data_only as c_int) })
    }

    /// Recreate every missing (`None`) shard.
    pub fn reconstruct(&self, shards: &mut [Option<Vec<u8>>]) -> Result<(), Error> {
        self.reconstruct_inner(shards, false)
    }

    /// Recreate only the missing data shards.
    pub fn reconstruct_data(&self, shards: &mut [Option<Vec<u8>>]) -> Result<(), Error> {
        self.reconstruct_inner(shards, true)
    }

    /// `reed-solomon-erasure` `encode_single`: add data shard `i_data`'s contribution to the
    /// parity shards `shards[k..]` in place (`cec_encode_idx`: parity[o] ^= E[k+o][i] * shard).
    /// Feeding every data shard once into zeroed parity, in any order, gives `encode`'s parity.
    pub fn encode_single(&self, i_data: usize, shards: &mut [&mut [u8]]) -> Result<(), Error> {
        if shards.len() != self.k + self.m || i_data >= self.k {
            return Err(Error::from_code(CEC_EINVAL));
        }
        let (p, len) = Self::ptrs(shards)?;
        check(unsafe {
            sys::cec_encode_idx(self.c, p[i_data] as *const u8, i_data as c_int,
                                p[self.k..].as_ptr(), len)
        })
    }

    /// `encode_single_sep`: the same with the data shard and the m parity shards held apart.
    pub fn encode_single_sep(&self, i_data: usize, single_data: &[u8],
                             parity: &mut [&mut [u8]]) -> Result<(), Error> {
        if parity.len() != self.m || i_data >= self.k {
            return Err(Error::from_code(CEC_EINVAL));
        }
        let (p, len) = Self::ptrs(parity)?;
        if single_data.len() != len {
            return Err(Error::from_code(CEC_ESHARDLEN));
        }
        check(unsafe {
            sys::cec_encode_idx(self.c, single_data.as_ptr(), i_data as c_int, p.as_ptr(), len)
        })
    }

    /// klauspost `Update` (`cec_update`): `shards` is an encoded segment (k + m, `None` for a data
    /// shard that did not change), `new_data` the k data shards with `None` for unchanged ones.
    /// The parity shards are brought up to date in place from the old and new bytes of the changed
    /// shards only; the old data shards keep their bytes.
    pub fn update(&self, shards: &mut [Option<Vec<u8>>], new_data: &[Option<&[u8]>])
                  -> Result<(), Error> {
        if shards.len() != self.k + self.m || new_data.len() != self.k {
            return Err(Error::from_code(CEC_ETOOFEW));
        }
        let len = shards[self.k..].iter().flatten().map(|s| s.len()).next()
            .ok_or(Error::from_code(CEC_EINVAL))?;
        if shards.iter().flatten().any(|s| s.len() != len)
            || new_data.iter().flatten().any(|s| s.len() != len) {
            return Err(Error::from_code(CEC_ESHARDLEN));
        }
        let p: Vec<*mut u8> = shards
            .iter_mut()
            .map(|s| match s { Some(v) => v.as_mut_ptr(), None => std::ptr::null_mut() })
            .collect();
        let n: Vec<*const u8> = new_data
            .iter()
            .map(|s| match s { Some(v) => v.as_ptr(), None => std::ptr::null() })
            .collect();
        check(unsafe { sys::cec_update(self.c, p.as_ptr(), n.as_ptr(), len) })
    }

    /// Scattered device shards (`cec_reconstruct_ptrs`): `src` and `dst` hold `nseg * (k + m)`
    /// device addresses, segment by segment; a null `src` entry is an absent shard, a non-null
    /// `dst` entry of an absent shard asks for it there. Enqueued on `stream` (null: the HIP null
    /// stream) and not waited for; both slices may be reused as soon as the call returns.
    ///
    /// # Safety
    /// Every non-null address must be device memory of `shard_len` bytes on the codec's GPU that
    /// stays valid until the stream has passed the call's work.
    pub unsafe fn reconstruct_device(&self, src: &[*const u8], dst: &[*mut u8], shard_len: usize,
                                     stream: *mut c_void) -> Result<(), Error> {
        let n = self.k + self.m;
        if src.len() != dst.len() || src.len() % n != 0 {
            return Err(Error::from_code(CEC_EINVAL));
        }
        check(cec_reconstruct_ptrs(self.c, src.as_ptr(), dst.as_ptr(), src.len() / n, shard_len,
                                   stream))
    }

    /// Verify scattered device shards in place (`cec_verify_ptrs`): `src` and `expect` hold
    /// `nseg * (k + m)` device addresses, segment by segment. A non-null `expect` entry is
    /// recomputed from the segment's survivors among the non-null `src` entries and compared with
    /// the bytes there; an entry set in both slices is refused. `d_ok` (device, `nseg` bytes)
    /// receives 1 per segment whose expectations all matched (or that had none), else 0. Nothing
    /// else is written. Enqueued on `stream` and not waited for; both slices may be reused as
    /// soon as the call returns.
    ///
    /// # Safety
    /// Every non-null address must be device memory of `shard_len` bytes (`d_ok`: `nseg` bytes) on
    /// the codec's GPU that stays valid until the stream has passed the call's work.
    pub unsafe fn verify_device(&self, src: &[*const u8], expect: &[*const u8], shard_len: usize,
                                d_ok: *mut u8, stream: *mut c_void) -> Result<(), Error> {
        let n = self.k + self.m;
        if src.len() != expect.len() || src.len() % n != 0 {
            return Err(Error::from_code(CEC_EINVAL));
        }
        check(cec_verify_ptrs(self.c, src.as_ptr(), expect.as_ptr(), src.len() / n, shard_len,
                              d_ok, stream))
    }

    /// Partial rebuild of scattered device shards in place (`cec_reconstruct_partial_ptrs`):
    /// `src`, `dst` and `present` hold `nseg * (k + m)` entries, segment by segment. `present` is
    /// the erasure pattern every party knows; a non-null `src` entry is a shard this caller holds;
    /// a non-null `dst` entry of an absent shard receives XOR over the held survivors j of
    /// D[i][j] * shard_j (`accumulate`: is XORed with it, a read-modify-write). XOR-ing the
    /// partials over a partition of a segment's survivors gives the rebuilt shard (`xor_device`).
    /// Enqueued on `stream` and not waited for; the slices may be reused as soon as the call
    /// returns.
    ///
    /// # Safety
    /// Every non-null address must be device memory of `shard_len` bytes on the codec's GPU that
    /// stays valid until the stream has passed the call's work; wanted destinations must not
    /// overlap each other or a held survivor.
    pub unsafe fn reconstruct_partial_device(&self, src: &[*const u8], dst: &[*mut u8],
                                             present: &[u8], shard_len: usize, accumulate: bool,
                                             stream: *mut c_void) -> Result<(), Error> {
        let n = self.k + self.m;
        if src.len() != dst.len() || src.len() != present.len() || src.len() % n != 0 {
            return Err(Error::from_code(CEC_EINVAL));
        }
        check(cec_reconstruct_partial_ptrs(self.c, src.as_ptr(), dst.as_ptr(), present.as_ptr(),
                                           src.len() / n, shard_len, accumulate as c_int, stream))
    }

    /// GF(2^8) sum of scattered device buffers (`cec_xor_ptrs`): `dst[r] ^= XOR of the non-null
    /// entries of src[r * nsrc .. (r + 1) * nsrc]`, `len` bytes each. A null `dst[r]` or a row
    /// without a source is skipped. Enqueued on `stream` and not waited for; both slices may be
    /// reused as soon as the call returns.
    ///
    /// # Safety
    /// Every non-null address must be device memory of `len` bytes on the codec's GPU that stays
    /// valid until the stream has passed the call's work; no source may overlap a destination.
    pub unsafe fn xor_device(&self, dst: &[*mut u8], src: &[*const u8], nsrc: usize, len: usize,
                             stream: *mut c_void) -> Result<(), Error> {
        if src.len() != dst.len() * nsrc {
            return Err(Error::from_code(CEC_EINVAL));
        }
        check(cec_xor_ptrs(self.c, dst.as_ptr(), src.as_ptr(), dst.len(), nsrc, len, stream))
    }

    /// Heal flagged fragments in place (`cec_repair_flagged_ptrs`): `shards` holds `nseg * (k + m)`
    /// device addresses, segment by segment, null = not held. `d_flags` (device, one byte per
    /// entry of `shards`, 0 = that held shard is bad; what `hashq_add_check_concat_ptrs` writes for
    /// chains listed segment-major) is read on the GPU: a segment with exactly one bad shard and at
    /// least k good ones has that shard rebuilt over its address. `d_status` (device, `nseg` bytes)
    /// receives one `CEC_FLAG_*` code per segment (`flag_status` states the rule). Enqueued on
    /// `stream` and not waited for, and no flag is copied to the host: the flags may still be in
    /// production by work queued earlier on that stream. The slice may be reused as soon as the
    /// call returns.
    ///
    /// # Safety
    /// Every non-null address must be device memory of `shard_len` bytes on the codec's GPU
    /// (`d_flags`: one byte per entry, `d_status`: `nseg` bytes) that stays valid until the stream
    /// has passed the call's work; shards must not overlap each other.
    pub unsafe fn repair_flagged_ptrs(&self, shards: &[*mut u8], d_flags: *const u8,
                                      shard_len: usize, d_status: *mut u8,
                                      stream: *mut c_void) -> Result<(), Error> {
        let n = self.k + self.m;
        if shards.len() % n != 0 {
            return Err(Error::from_code(CEC_EINVAL));
        }
        check(cec_repair_flagged_ptrs(self.c, shards.as_ptr(), d_flags, shards.len() / n,
                                      shard_len, d_status, stream))
    }

    /// The rule `repair_flagged_ptrs` applies to one segment (`cec_flag_status`, host only):
    /// `held` and `flags` hold k + m bytes each. Returns the `CEC_FLAG_*` status and, for
    /// `CEC_FLAG_REBUILT`, the index of the shard that is rewritten.
    pub fn flag_status(&self, held: &[u8], flags: &[u8]) -> Result<(i32, Option<usize>), Error> {
        let n = self.k + self.m;
        if held.len() != n || flags.len() != n {
            return Err(Error::from_code(CEC_EINVAL));
        }
        let (mut status, mut lost): (c_int, c_int) = (0, -1);
        check(unsafe {
            cec_flag_status(self.k as c_int, self.m as c_int, held.as_ptr(), flags.as_ptr(),
                            &mut status, &mut lost)
        })?;
        Ok((status, if lost >= 0 { Some(lost as usize) } else { None }))
    }

    /// `repair_flagged_ptrs` for segments with several bad shards
    /// (`cec_repair_flagged_multi_ptrs`): a segment with 1 to `max_bad` bad shards (at most
    /// `CEC_FLAG_MULTI_MAX`) and at least k good ones has every bad shard rebuilt over its address,
    /// from the first k good shards in index order; the decode rows are solved per segment on the
    /// GPU. Arguments and stream behaviour as there (`flag_status_multi` states the rule).
    ///
    /// # Safety
    /// As for `repair_flagged_ptrs`.
    pub unsafe fn repair_flagged_multi_ptrs(&self, shards: &[*mut u8], d_flags: *const u8,
                                            shard_len: usize, max_bad: i32, d_status: *mut u8,
                                            stream: *mut c_void) -> Result<(), Error> {
        let n = self.k + self.m;
        if shards.len() % n != 0 {
            return Err(Error::from_code(CEC_EINVAL));
        }
        check(cec_repair_flagged_multi_ptrs(self.c, shards.as_ptr(), d_flags, shards.len() / n,
                                            shard_len, max_bad as c_int, d_status, stream))
    }

    /// The rule `repair_flagged_multi_ptrs` applies to one segment (`cec_flag_status_multi`, host
    /// only): returns the `CEC_FLAG_*` status and the ascending indices of the shards a
    /// `CEC_FLAG_REBUILT` segment rewrites (empty for every other status).
    pub fn flag_status_multi(&self, held: &[u8], flags: &[u8],
                             max_bad: i32) -> Result<(i32, Vec<usize>), Error> {
        let n = self.k + self.m;
        if held.len() != n || flags.len() != n {
            return Err(Error::from_code(CEC_EINVAL));
        }
        let (mut status, mut nlost): (c_int, c_int) = (0, 0);
        let mut lost = [0u8; CEC_FLAG_MULTI_MAX as usize];
        check(unsafe {
            cec_flag_status_multi(self.k as c_int, self.m as c_int, held.as_ptr(), flags.as_ptr(),
                                  max_bad as c_int, &mut status, &mut nlost, lost.as_mut_ptr())
        })?;
        Ok((status, lost[..nlost as usize].iter().map(|&i| i as usize).collect()))
    }

    /// A verified degraded read decided on the GPU (`cec_read_flagged_ptrs`): `shards` and
    /// `d_flags` as in `repair_flagged_multi_ptrs`, but the shards are only read. `dst` holds
    /// `nseg * k` device addresses, segment by segment: a non-null entry is where that data shard
    /// is wanted (`shard_len` bytes), null means not wanted. Per segment the good wanted data
    /// shards are copied and up to `max_bad` missing ones (not held, or flagged bad) rebuilt into
    /// their destinations from the first k good shards; `d_status` receives one `CEC_FLAG_*` code
    /// per segment (`read_status` states the rule), and no destination of a `CEC_FLAG_LOST` or
    /// `CEC_FLAG_MANY` segment is written. Enqueued on `stream` and not waited for; no flag is
    /// copied to the host.
    ///
    /// # Safety
    /// Every non-null entry of `shards` and `dst` must be valid device memory of `shard_len`
    /// bytes, `d_flags` of `shards.len()` bytes and `d_status` of one byte per segment, all until
    /// the work enqueued on `stream` has run; no destination may overlap a shard or another
    /// destination.
    pub unsafe fn read_flagged_ptrs(&self, shards: &[*const u8], d_flags: *const u8,
                                    dst: &[*mut u8], shard_len: usize, max_bad: i32,
                                    d_status: *mut u8, stream: *mut c_void) -> Result<(), Error> {
        let n = self.k + self.m;
        if shards.len() % n != 0 || dst.len() != shards.len() / n * self.k {
            return Err(Error::from_code(CEC_EINVAL));
        }
        check(cec_read_flagged_ptrs(self.c, shards.as_ptr(), d_flags, dst.as_ptr(),
                                    shards.len() / n, shard_len, max_bad as c_int, d_status,
                                    stream))
    }

    /// The rule `read_flagged_ptrs` applies to one segment (`cec_read_status`, host only):
    /// `wanted` names the k data shards to deliver. Returns the `CEC_FLAG_*` status and the
    /// ascending indices of the data shards a `CEC_FLAG_REBUILT` segment rebuilds into its
    /// destinations (empty for every other status).
    pub fn read_status(&self, held: &[u8], flags: &[u8], wanted: &[u8],
                       max_bad: i32) -> Result<(i32, Vec<usize>), Error> {
        let n = self.k + self.m;
        if held.len() != n || flags.len() != n || wanted.len() != self.k {
            return Err(Error::from_code(CEC_EINVAL));
        }
        let (mut status, mut nmiss): (c_int, c_int) = (0, 0);
        let mut miss = [0u8; CEC_FLAG_MULTI_MAX as usize];
        check(unsafe {
            cec_read_status(self.k as c_int, self.m as c_int, held.as_ptr(), flags.as_ptr(),
                            wanted.as_ptr(), max_bad as c_int, &mut status, &mut nmiss,
                            miss.as_mut_ptr())
        })?;
        Ok((status, miss[..nmiss as usize].iter().map(|&i| i as usize).collect()))
    }

    /// Find the corrupt shard of every segment from parity alone (`cec_locate_ptrs`): `shards`
    /// holds `nseg * (k + m)` device addresses, segment by segment, null = not held; they are only
    /// read. `d_status` receives one `CEC_LOCATE_*` code per segment and `d_flags` one byte per
    /// shard in the layout the flagged repairs and the flagged read consume: 1 for a held shard
    /// that is consistent, 0 for the one shard of a `CEC_LOCATE_FOUND` segment that disagrees with
    /// the others and for every shard of a `CEC_LOCATE_AMBIGUOUS` one (`locate_host` states the
    /// rule). `nsyn` in `1..=CEC_LOCATE_SYN_MAX` bounds the checks per byte. Enqueued on `stream`
    /// and not waited for; nothing is copied to the host.
    ///
    /// # Safety
    /// Every non-null entry of `shards` must be valid device memory of `shard_len` bytes,
    /// `d_flags` of `shards.len()` bytes and `d_status` of one byte per segment, all until the
    /// work enqueued on `stream` has run.
    pub unsafe fn locate_ptrs(&self, shards: &[*const u8], shard_len: usize, nsyn: i32,
                              d_flags: *mut u8, d_status: *mut u8,
                              stream: *mut c_void) -> Result<(), Error> {
        let n = self.k + self.m;
        if shards.len() % n != 0 {
            return Err(Error::from_code(CEC_EINVAL));
        }
        check(cec_locate_ptrs(self.c, shards.as_ptr(), shards.len() / n, shard_len,
                              nsyn as c_int, d_flags, d_status, stream))
    }

    /// The check rows of a held set (`cec_locate_rows`, host only): returns r = min(nsyn, h - k)
    /// and r rows of k + m coefficients, `rows[a][i]` = u_i * i^a for held i and 0 elsewhere; each
    /// row applied to the held shards of a consistent segment gives zero at every byte.
    pub fn locate_rows(&self, held: &[u8], nsyn: i32) -> Result<(usize, Vec<Vec<u8>>), Error> {
        let n = self.k + self.m;
        if held.len() != n {
            return Err(Error::from_code(CEC_EINVAL));
        }
        let mut r: c_int = 0;
        let mut rows = vec![0u8; CEC_LOCATE_SYN_MAX as usize * n];
        check(unsafe {
            cec_locate_rows(self.k as c_int, self.m as c_int, held.as_ptr(), nsyn as c_int,
                            &mut r, rows.as_mut_ptr())
        })?;
        Ok((r as usize, rows.chunks(n).take(r as usize).map(|c| c.to_vec()).collect()))
    }

    /// The rule `locate_ptrs` applies to one segment, on host memory (`cec_locate_host`):
    /// `shards` holds k + m entries of one length, `None` = not held. Returns the `CEC_LOCATE_*`
    /// status and the shard of a `CEC_LOCATE_FOUND` segment.
    pub fn locate_host(&self, shards: &[Option<&[u8]>],
                       nsyn: i32) -> Result<(i32, Option<usize>), Error> {
        let n = self.k + self.m;
        let len = shards.iter().flatten().map(|s| s.len()).next().unwrap_or(0);
        if shards.len() != n || shards.iter().flatten().any(|s| s.len() != len) {
            return Err(Error::from_code(CEC_EINVAL));
        }
        let ptrs: Vec<*const u8> =
            shards.iter().map(|s| s.map_or(std::ptr::null(), |b| b.as_ptr())).collect();
        let (mut status, mut found): (c_int, c_int) = (0, -1);
        check(unsafe {
            cec_locate_host(self.k as c_int, self.m as c_int, ptrs.as_ptr(), len, nsyn as c_int,
                            &mut status, &mut found)
        })?;
        Ok((status, if found >= 0 { Some(found as usize) } else { None }))
    }

    /// Find up to `max_bad` corrupt shards of every segment from parity alone
    /// (`cec_locate_multi_ptrs`): arguments as in `locate_ptrs`, plus `max_bad` in
    /// `1..=CEC_LOCATE_BAD_MAX` and `d_nbad`, one byte per segment or null, which receives the
    /// number of shards a `CEC_LOCATE_FOUND` segment names (0 for every other status). Two shards
    /// are named only where four checks are computed (`nsyn` = 4 and k + 4 or more shards held);
    /// `max_bad` = 1 is `locate_ptrs`. Enqueued on `stream` and not waited for.
    ///
    /// # Safety
    /// As for `locate_ptrs`; a non-null `d_nbad` must be device memory of one byte per segment.
    pub unsafe fn locate_multi_ptrs(&self, shards: &[*const u8], shard_len: usize, nsyn: i32,
                                    max_bad: i32, d_flags: *mut u8, d_status: *mut u8,
                                    d_nbad: *mut u8, stream: *mut c_void) -> Result<(), Error> {
        let n = self.k + self.m;
        if shards.len() % n != 0 {
            return Err(Error::from_code(CEC_EINVAL));
        }
        check(cec_locate_multi_ptrs(self.c, shards.as_ptr(), shards.len() / n, shard_len,
                                    nsyn as c_int, max_bad as c_int, d_flags, d_status, d_nbad,
                                    stream))
    }

    /// The rule `locate_multi_ptrs` applies to one segment, on host memory
    /// (`cec_locate_multi_host`): returns the `CEC_LOCATE_*` status and the shards of a
    /// `CEC_LOCATE_FOUND` segment, ascending (one or two).
    pub fn locate_multi_host(&self, shards: &[Option<&[u8]>], nsyn: i32,
                             max_bad: i32) -> Result<(i32, Vec<usize>), Error> {
        let n = self.k + self.m;
        let len = shards.iter().flatten().map(|s| s.len()).next().unwrap_or(0);
        if shards.len() != n || shards.iter().flatten().any(|s| s.len() != len) {
            return Err(Error::from_code(CEC_EINVAL));
        }
        let ptrs: Vec<*const u8> =
            shards.iter().map(|s| s.map_or(std::ptr::null(), |b| b.as_ptr())).collect();
        let (mut status, mut nfound): (c_int, c_int) = (0, 0);
        let mut found: [c_int; 2] = [-1, -1];
        check(unsafe {
            cec_locate_multi_host(self.k as c_int, self.m as c_int, ptrs.as_ptr(), len,
                                  nsyn as c_int, max_bad as c_int, &mut status, &mut nfound,
                                  found.as_mut_ptr())
        })?;
        Ok((status, found[..nfound as usize].iter().map(|&i| i as usize).collect()))
    }

    /// EncodeIdx on scattered device shards in place (`cec_encode_idx_ptrs`): `data` holds
    /// `nseg * k` entries and `parity` `nseg * m`, segment by segment. A non-null `data` entry is a
    /// data shard fed in this call, a non-null `parity` entry a parity shard held here; every
    /// named parity o of a segment receives XOR over its fed shards j of E[k+o][j] * data_j
    /// (`accumulate`: is XORed with it; otherwise overwritten, zero-filled where nothing is fed).
    /// Enqueued on `stream` and not waited for; the slices may be reused as soon as the call
    /// returns.
    ///
    /// # Safety
    /// Every non-null address must be device memory of `shard_len` bytes on the codec's GPU that
    /// stays valid until the stream has passed the call's work; parity shards must not overlap
    /// each other or a fed shard.
    pub unsafe fn encode_idx_device(&self, data: &[*const u8], parity: &[*mut u8],
                                    shard_len: usize, accumulate: bool,
                                    stream: *mut c_void) -> Result<(), Error> {
        if data.len() % self.k != 0 || parity.len() != data.len() / self.k * self.m {
            return Err(Error::from_code(CEC_EINVAL));
        }
        check(cec_encode_idx_ptrs(self.c, data.as_ptr(), parity.as_ptr(), data.len() / self.k,
                                  shard_len, accumulate as c_int, stream))
    }

    /// Update on scattered device shards in place (`cec_update_ptrs`): `old_data` and `new_data`
    /// hold `nseg * k` entries and `parity` `nseg * m`. A slot with both entries non-null is
    /// changed (both null: unchanged); every named parity o of a segment is XORed with the sum
    /// over its changed slots j of E[k+o][j] * (old_j ^ new_j). Only parity is written. Enqueued
    /// on `stream` and not waited for; the slices may be reused as soon as the call returns.
    ///
    /// # Safety
    /// As `encode_idx_device`, for the old and the new bytes alike.
    pub unsafe fn update_device(&self, old_data: &[*const u8], new_data: &[*const u8],
                                parity: &[*mut u8], shard_len: usize,
                                stream: *mut c_void) -> Result<(), Error> {
        if old_data.len() != new_data.len() || old_data.len() % self.k != 0
            || parity.len() != old_data.len() / self.k * self.m {
            return Err(Error::from_code(CEC_EINVAL));
        }
        check(cec_update_ptrs(self.c, old_data.as_ptr(), new_data.as_ptr(), parity.as_ptr(),
                              old_data.len() / self.k, shard_len, stream))
    }

    /// Storage-audit chunks of scattered device fragments in place (`cec_audit_chunks_ptrs`):
    /// `frags` holds the device addresses of fragments of `shard_len` bytes, each `chunk_count`
    /// chunks; chunk `indices[j]` of fragment f goes to `d_chunks[(f * nidx + j) * chunk ..]` and
    /// its SHA-256 hex to `d_hex[(f * nidx + j) * 64 ..]` (either output may be null, not both).
    /// With `d_chunks` null the chunks are hashed where they lie and no chunk byte is copied.
    /// Enqueued on `stream` and not waited for; both slices may be reused as soon as the call
    /// returns.
    ///
    /// # Safety
    /// Every fragment address must be device memory of `shard_len` bytes, `d_chunks` of
    /// `frags.len() * indices.len() * (shard_len / chunk_count)` and `d_hex` of
    /// `frags.len() * indices.len() * 64` bytes, on the codec's GPU and valid until the stream has
    /// passed the call's work; the outputs must not overlap a fragment.
    pub unsafe fn audit_chunks_device(&self, frags: &[*const u8], shard_len: usize,
                                      chunk_count: u32, indices: &[u32], d_chunks: *mut u8,
                                      d_hex: *mut u8, stream: *mut c_void) -> Result<(), Error> {
        if indices.len() > u32::MAX as usize {
            return Err(Error::from_code(CEC_EINVAL));
        }
        check(sys::cec_audit_chunks_ptrs(self.c, frags.as_ptr(), frags.len(), shard_len,
                                         chunk_count, indices.as_ptr(), indices.len() as u32,
                                         d_chunks, d_hex, stream))
    }

    /// The decode rows of the `required` lost shards of pattern `present` (`cec_decode_rows`):
    /// (shard indices ascending, one row of k coefficients over `cec_survivors` each).
    pub fn decode_rows(&self, present: &[u8], required: &[u8]) -> Result<(Vec<u8>, Vec<u8>), Error> {
        let n = self.k + self.m;
        if present.len() != n || required.len() != n {
            return Err(Error::from_code(CEC_EINVAL));
        }
        let mut rows = vec![0u8; n * self.k];
        let mut idx = vec![0u8; n];
        let mut nreq: c_int = 0;
        check(unsafe {
            cec_decode_rows(self.k as c_int, self.m as c_int, present.as_ptr(), required.as_ptr(),
                            rows.as_mut_ptr(), idx.as_mut_ptr(), &mut nreq)
        })?;
        idx.truncate(nreq as usize);
        rows.truncate(nreq as usize * self.k);
        Ok((idx, rows))
    }
}

impl Drop for ReedSolomon {
    fn drop(&mut self) {
        unsafe { cec_destroy(self.c) }
    }
}

/// Append scattered device buffers to a hash queue (`cec_hashq_add_ptrs`): chain i hashes the
/// `len` bytes at `d_bufs[i]` and writes its 64 hex chars to `d_hex + 64 * i` (null: no output).
/// Returns the add's ticket (0 for an empty slice). The addresses travel in kernel arguments:
/// nothing is copied or waited for, and the slice may be reused as soon as the call returns.
///
/// # Safety
/// `q` must be a live queue; every address must be device memory of `len` bytes (`d_hex`:
/// `64 * d_bufs.len()` bytes) on the queue's GPU that stays valid until the add is complete.
pub unsafe fn hashq_add_ptrs(q: *mut sys::cec_hashq, d_bufs: &[*const u8], len: usize,
                             d_hex: *mut u8) -> Result<u64, Error> {
    let mut ticket = 0u64;
    check(sys::cec_hashq_add_ptrs(q, d_bufs.as_ptr(), d_bufs.len(), len, d_hex, &mut ticket))?;
    Ok(ticket)
}

/// Append chains that each run over several scattered device buffers back to back
/// (`cec_hashq_add_concat_ptrs`): `d_parts` holds `parts` addresses per chain, chain-major; chain
/// i hashes its parts in order, `part_len` bytes each (a nonzero multiple of 64), the last one
/// only as far as the chain's total `len` (0: all of it). It writes its 64 hex chars to
/// `d_hex + 64 * i` and, unless `d_prefix_hex` is null, those of its first part to
/// `d_prefix_hex + 64 * i` (null: no output). Returns the add's ticket (0 for an empty slice).
/// Nothing is copied on the device; the queue keeps its own copy of the addresses, so the slice
/// may be reused as soon as the call returns.
///
/// # Safety
/// `q` must be a live queue; `d_parts.len()` must be a multiple of `parts`; every address must be
/// device memory of `part_len` bytes (`d_hex`, `d_prefix_hex`: 64 bytes per chain) on the queue's
/// GPU that stays valid until the add is complete.
pub unsafe fn hashq_add_concat_ptrs(q: *mut sys::cec_hashq, d_parts: &[*const u8], parts: usize,
                                    part_len: usize, len: usize, d_hex: *mut u8,
                                    d_prefix_hex: *mut u8) -> Result<u64, Error> {
    if parts == 0 || d_parts.len() % parts != 0 {
        return Err(Error::from_code(CEC_EINVAL));
    }
    let mut ticket = 0u64;
    check(sys::cec_hashq_add_concat_ptrs(q, d_parts.as_ptr(), d_parts.len() / parts, parts,
                                         part_len, len, d_hex, d_prefix_hex, &mut ticket))?;
    Ok(ticket)
}

/// `hashq_add_concat_ptrs` whose chains are checked against their recorded hashes on the GPU
/// (`cec_hashq_add_check_concat_ptrs`; `parts == 1`: one buffer per chain, a miner's scrub): chain
/// i compares its digest with the 64 lowercase hex chars at `d_expect + 64 * i` and writes 1
/// (equal) or 0 to `d_ok + i`, in the tick launch that completes it. `d_hex` and `d_prefix_hex`
/// may be null (flags only). Returns the add's ticket.
///
/// # Safety
/// As `hashq_add_concat_ptrs`; `d_expect` must be memory the device reads (64 bytes per chain,
/// 4-byte aligned) and `d_ok` device memory (one byte per chain), both valid until the add is
/// complete.
pub unsafe fn hashq_add_check_concat_ptrs(q: *mut sys::cec_hashq, d_parts: &[*const u8],
                                          parts: usize, part_len: usize, len: usize,
                                          d_expect: *const u8, d_ok: *mut u8, d_hex: *mut u8,
                                          d_prefix_hex: *mut u8) -> Result<u64, Error> {
    if parts == 0 || d_parts.len() % parts != 0 {
        return Err(Error::from_code(CEC_EINVAL));
    }
    let mut ticket = 0u64;
    check(sys::cec_hashq_add_check_concat_ptrs(q, d_parts.as_ptr(), d_parts.len() / parts, parts,
                                               part_len, len, d_expect, d_ok, d_hex,
                                               d_prefix_hex, &mut ticket))?;
    Ok(ticket)
}

/// `hashq_add_check_concat_ptrs` at `parts == 1` whose chains the GPU admits
/// (`cec_hashq_add_check_where_ptrs`): chain i runs iff `d_bufs[i]` is not null, `d_flags[i] == 0`
/// and (`d_gate` is null or `d_gate[i / per] == gate`), read from device memory when the queue's
/// stream gets there. An admitted chain writes 1 or 0 to `d_ok + i` against `d_expect + 64 * i`;
/// every other chain gets `CEC_HASHQ_SKIPPED` there and none of its bytes is read. With a scrub's
/// flags, `per = k + m`, `d_gate` the statuses of `repair_flagged_ptrs` and `gate =
/// CEC_FLAG_REBUILT`: the fragments the repair just rewrote. Returns the add's ticket.
///
/// # Safety
/// As `hashq_add_check_concat_ptrs`; `d_flags` (one byte per chain) and `d_gate` (one per `per`
/// chains, or null) must be device memory valid until the add's kernels have run.
pub unsafe fn hashq_add_check_where_ptrs(q: *mut sys::cec_hashq, d_bufs: &[*const u8], len: usize,
                                         d_expect: *const u8, d_flags: *const u8, per: usize,
                                         d_gate: *const u8, gate: u8, d_ok: *mut u8,
                                         d_hex: *mut u8) -> Result<u64, Error> {
    let mut ticket = 0u64;
    check(sys::cec_hashq_add_check_where_ptrs(q, d_bufs.as_ptr(), d_bufs.len(), len, d_expect,
                                              d_flags, per, d_gate, gate as c_int, d_ok, d_hex,
                                              &mut ticket))?;
    Ok(ticket)
}

/// What a repair proved, per segment, on the GPU (`cec_confirm_flagged`): `d_confirm[s]` becomes a
/// `CEC_CONFIRM_*` code from `d_status[s]` and the `n` bytes at `d_ok + s * n` that
/// `hashq_add_check_where_ptrs` left (`confirm_rule` states the rule). Enqueued on `stream`, not
/// waited for; only `d_confirm` is written.
///
/// # Safety
/// `d_status` and `d_confirm` must be device memory of `nseg` bytes, `d_ok` of `nseg * n`, valid
/// until the stream has run the kernel; `stream` a HIP stream of the current device or null.
pub unsafe fn confirm_flagged(d_status: *const u8, d_ok: *const u8, nseg: usize, n: usize,
                              d_confirm: *mut u8, stream: *mut c_void) -> Result<(), Error> {
    check(sys::cec_confirm_flagged(d_status, d_ok, nseg, n as c_int, d_confirm, stream))
}

/// The rule of `confirm_flagged` for one segment (`cec_confirm_rule`, host only): `CEC_CONFIRM_NONE`
/// unless `status` is `CEC_FLAG_REBUILT`; then `REFUTED` if any byte of `ok` is 0, else `PROVEN`
/// if any is 1, else `NONE`.
pub fn confirm_rule(status: c_int, ok: &[u8]) -> Result<c_int, Error> {
    let mut confirm: c_int = -1;
    check(unsafe {
        sys::cec_confirm_rule(ok.len() as c_int, status, ok.as_ptr(), &mut confirm)
    })?;
    Ok(confirm)
}

/// One segment's SegmentList hashes: 64 hex chars for the segment, k+m for its fragments.
#[derive(Clone, Debug, PartialEq, Eq)]
pub struct SegmentList {
    pub hash: [u8; 64],
    pub fragment_list: Vec<[u8; 64]>,
}

struct Ctx<'a, R: std::io::Read> {
    src: &'a mut R,
    n: usize,
    on_fragments: &'a mut dyn FnMut(u64, &[&[u8]]),
    records: Vec<SegmentList>,
    err: Option<std::io::Error>,
}

extern "C" fn read_cb<R: std::io::Read>(user: *mut c_void, dst: *mut u8, cap: usize) -> c_longlong {
    let ctx = unsafe { &mut *(user as *mut Ctx<R>) };
    let buf = unsafe { std::slice::from_raw_parts_mut(dst, cap) };
    match ctx.src.read(buf) {
        Ok(n) => n as c_longlong,
        Err(e) => {
            ctx.err = Some(e);
            -1
        }
    }
}

extern "C" fn frag_cb<R: std::io::Read>(user: *mut c_void, seg: u64, shards: *const *const u8,
                                        shard_len: usize) -> c_int {
    let ctx = unsafe { &mut *(user as *mut Ctx<R>) };
    let v: Vec<&[u8]> = (0..ctx.n)
        .map(|i| unsafe { std::slice::from_raw_parts(*shards.add(i), shard_len) })
        .collect();
    (ctx.on_fragments)(seg, &v);
    0
}

extern "C" fn rec_cb<R: std::io::Read>(user: *mut c_void, _seg: u64, seg_hex: *const u8,
                                       frag_hex: *const u8) -> c_int {
    let ctx = unsafe { &mut *(user as *mut Ctx<R>) };
    let mut hash = [0u8; 64];
    hash.copy_from_slice(unsafe { std::slice::from_raw_parts(seg_hex, 64) });
    let fh = unsafe { std::slice::from_raw_parts(frag_hex, 64 * ctx.n) };
    let fragment_list = fh.chunks(64).map(|c| { let mut h = [0u8; 64]; h.copy_from_slice(c); h }).collect();
    ctx.records.push(SegmentList { hash, fragment_list });
    0
}

/// libcessec's host pipeline (pinned multi-buffered H2D / encode / D2H, GPU hashes).
pub struct Pipeline<'c> {
    p: *mut cec_pipeline,
    n: usize,
    _codec: std::marker::PhantomData<&'c ReedSolomon>,
}

impl<'c> Pipeline<'c> {
    pub fn new(codec: &'c ReedSolomon, opts: cec_pipeline_opts) -> Result<Self, Error> {
        let mut p = std::ptr::null_mut();
        check(unsafe { cec_pipeline_create(codec.c, &opts, &mut p) })?;
        Ok(Pipeline { p, n: codec.k + codec.m, _codec: std::marker::PhantomData })
    }

    /// Stream a file through the GPU: `on_fragments(seg, shards)` sees each segment's k+m
    /// shards, the returned records are the file's SegmentLists in segment order.
    pub fn run<R: std::io::Read>(&mut self, src: &mut R,
                                 on_fragments: &mut dyn FnMut(u64, &[&[u8]]))
                                 -> Result<(Vec<SegmentList>, cec_pipeline_stats), Error> {
        let mut ctx = Ctx { src, n: self.n, on_fragments, records: Vec::new(), err: None };
        let mut st = cec_pipeline_stats::default();
        let rc = unsafe {
            cec_pipeline_run(self.p, read_cb::<R>, Some(frag_cb::<R>), Some(rec_cb::<R>),
                             &mut ctx as *mut Ctx<R> as *mut c_void, &mut st)
        };
        if let Some(e) = ctx.err.take() {
            return Err(Error { code: rc, message: e.to_string() });
        }
        check(rc)?;
        Ok((ctx.records, st))
    }
}

impl Drop for Pipeline<'_> {
    fn drop(&mut self) {
        unsafe { cec_pipeline_destroy(self.p) }
    }
}

/// SCALE bytes of `deal_info: BoundedVec<SegmentList, SegmentCount>` for upload_declaration.
pub fn deal_info(segments: &[SegmentList]) -> Result<Vec<u8>, Error> {
    let nfrag = segments.first().map(|s| s.fragment_list.len()).unwrap_or(FRAGMENT_COUNT);
    let seg: Vec<u8> = segments.iter().flat_map(|s| s.hash).collect();
    let frag: Vec<u8> = segments.iter().flat_map(|s| s.fragment_list.iter().flatten().copied()).collect();
    let mut len = 0usize;
    check(unsafe { cec_scale_deal_info(seg.as_ptr(), frag.as_ptr(), segments.len(), nfrag,
                                       std::ptr::null_mut(), 0, &mut len) })?;
    let mut out = vec![0u8; len];
    check(unsafe { cec_scale_deal_info(seg.as_ptr(), frag.as_ptr(), segments.len(), nfrag,
                                       out.as_mut_ptr(), len, &mut len) })?;
    Ok(out)
}

/// Size-query-then-fill of a libcessec SCALE encoder (`f(out, cap, &mut len)`).
fn scale_call(f: impl Fn(*mut u8, usize, *mut usize) -> c_int) -> Result<Vec<u8>, Error> {
    let mut len = 0usize;
    check(f(std::ptr::null_mut(), 0, &mut len))?;
    let mut out = vec![0u8; len];
    check(f(out.as_mut_ptr(), len, &mut len))?;
    Ok(out)
}

/// `FillerInfo` of c-pallets/file-bank/src/types.rs:82-86.
#[derive(Clone, Debug)]
pub struct FillerInfo {
    pub block_num: u32,
    pub miner_address: [u8; 32],
    pub filler_hash: [u8; 64],
}

/// Call data of `upload_filler(tee_worker, filler_list)` (call 8, at most 10 fillers).
pub fn upload_filler(tee_worker: &[u8; 32], fillers: &[FillerInfo]) -> Result<Vec<u8>, Error> {
    let blk: Vec<u32> = fillers.iter().map(|f| f.block_num).collect();
    let miners: Vec<u8> = fillers.iter().flat_map(|f| f.miner_address).collect();
    let hex: Vec<u8> = fillers.iter().flat_map(|f| f.filler_hash).collect();
    scale_call(|o, c, l| unsafe {
        sys::cec_scale_upload_filler(tee_worker.as_ptr(), blk.as_ptr(), miners.as_ptr(),
                                     hex.as_ptr(), fillers.len(), o, c, l)
    })
}

/// Call data of `restoral_order_complete(fragment_hash)` (call 16): emit it only after the
/// rebuilt fragment's SHA-256 hex equals `fragment_hash`.
pub fn restoral_order_complete(fragment_hash: &[u8; 64]) -> Result<Vec<u8>, Error> {
    scale_call(|o, c, l| unsafe { sys::cec_scale_restoral_order_complete(fragment_hash.as_ptr(), o, c, l) })
}

/// Call data of `claim_restoral_order(restoral_fragment)` (call 14).
pub fn claim_restoral_order(fragment_hash: &[u8; 64]) -> Result<Vec<u8>, Error> {
    scale_call(|o, c, l| unsafe { sys::cec_scale_claim_restoral_order(fragment_hash.as_ptr(), o, c, l) })
}
