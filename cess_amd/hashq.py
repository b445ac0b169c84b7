"""Streaming SHA-256 of fragments and segments on the GPU (libcessec hash queue,
include/cess_ec.h `cec_hashq_*`).

The records it produces are the `Hash` values of `SegmentList { hash, fragment_list }`
(c-pallets/file-bank/src/types.rs:13-16; `Hash([u8; 64])`, primitives/common/src/lib.rs:16):
64 lowercase hex chars of SHA-256 [ecosystem convention, SURVEY.md §8a a4].

Why a queue: a buffer's SHA-256 is one serial chain, and one GPU lane runs a chain at about one
wave's instruction issue rate, so hashing throughput is (chains in flight) x (per-chain rate).
One 1 GiB batch has 4096 fragment chains (RS(32,32)) or 192 (RS(2,1)): a few percent of the
chip. The queue keeps chain state in HBM, so each `tick` advances the chains of every batch
added so far; adding one batch per step and ticking once per step keeps a window of batches
hashing together. Completion is known on the host from lengths alone: `done(ticket)` turns true
once the ticks enqueued so far cover that add (the hex is in HBM when the stream gets there).
"""
from __future__ import annotations

from ctypes import byref, c_int, c_size_t, c_uint64, c_void_p
from typing import Optional

from . import _lib
from .reedsolomon import (CecError, ErrInvalidInput, ErrShardNoData, ErrShardSize, _dev_ptr,
                          _stream_handle, check)


def sha256_blocks(length: int) -> int:
    """64-byte compressions of one SHA-256 chain over `length` bytes, padding included."""
    return (length >> 6) + (2 if (length & 63) >= 56 else 1)


def _at(d, offset: int = 0):
    """The device address of `d` plus `offset` bytes; None stays None (a null pointer in C)."""
    return None if d is None else _dev_ptr(d) + offset


def _rows(rows, width: Optional[int] = None):
    """Rows of 1-D tensors as (rows as lists, their tensors in one list, the tensors' one size; 0
    without tensors). Rows that are not `width` long (None: as long as the first) or tensors of
    different sizes raise ErrShardSize, a None entry ErrInvalidInput."""
    rows = [list(row) for row in rows]
    if width is None and rows:
        width = len(rows[0])
    if any(len(row) != width for row in rows):
        raise ErrShardSize(ErrShardSize.__doc__)
    flat = [t for row in rows for t in row]
    if any(t is None for t in flat):
        raise ErrInvalidInput(ErrInvalidInput.__doc__)
    sizes = {t.numel() for t in flat}
    if len(sizes) > 1:
        raise ErrShardSize(ErrShardSize.__doc__)
    return rows, flat, sizes.pop() if sizes else 0


class HashQueue:
    """GPU hash queue bound to one device and one stream (all its work is ordered there)."""

    def __init__(self, capacity: int = 1 << 18, device: int = 0, stream=None):
        lib = _lib.load()
        h = c_void_p()
        self.stream = stream
        check(lib.cec_hashq_create(device, capacity, _stream_handle(stream), byref(h)),
              "HashQueue")
        self._h = h
        self.capacity = capacity
        self.device = device
        self._kept = []  # (ticket, uploaded expectations) of the checking adds still live

    def close(self) -> None:
        if getattr(self, "_h", None):
            if getattr(self, "_kept", None):
                self._release(everything=True)
            _lib.load().cec_hashq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def add(self, d_base, n: int, per: int, outer_stride: int, inner_stride: int, length: int,
            d_hex=None, hex_outer: int = 0, hex_offset: int = 0, prefix_len: int = 0,
            d_prefix_hex=None, prefix_hex_outer: int = 0, prefix_hex_offset: int = 0) -> int:
        """Append n chains (buffer i at base + (i // per) * outer + (i % per) * inner, `length`
        bytes; hex at d_hex + hex_offset + ((i // per) * hex_outer + i % per) * 64). With
        d_prefix_hex, chain i also writes the hex of its first prefix_len bytes (a multiple of 64)
        at d_prefix_hex + prefix_hex_offset + ((i // per) * prefix_hex_outer + i % per) * 64
        (cec_hashq_add_prefix). Returns the add's ticket."""
        t = c_uint64()
        hexp, prep = _at(d_hex, hex_offset), _at(d_prefix_hex, prefix_hex_offset)
        check(_lib.load().cec_hashq_add_prefix(self._h, _dev_ptr(d_base), n, per, outer_stride,
                                               inner_stride, length, hexp, hex_outer,
                                               prefix_len if prep else 0, prep,
                                               prefix_hex_outer, byref(t)),
              "HashQueue.add")
        return t.value

    def add_resume(self, d_base, n: int, per: int, outer_stride: int, inner_stride: int,
                   length: int, start_len: int, d_states, d_hex=None, hex_outer: int = 0,
                   hex_offset: int = 0) -> int:
        """`add` of n chains that resume after their first start_len bytes (a multiple of 64
        within length's full blocks; cec_hashq_add_resume): chain i starts from the eight 32-bit
        state words d_states[8 i .. 8 i + 7] (a device tensor, or the int address of memory the
        device reads, such as a pinned host tensor's data_ptr(); as cec_sha256_host_state gives
        them) and hashes bytes start_len .. length of its buffer. The states are read by the
        add's kernel on the queue's stream. Returns the add's ticket (0 for n == 0)."""
        t = c_uint64()
        check(_lib.load().cec_hashq_add_resume(self._h, _dev_ptr(d_base), n, per, outer_stride,
                                               inner_stride, length, start_len, _at(d_states),
                                               _at(d_hex, hex_offset), hex_outer, byref(t)),
              "HashQueue.add_resume")
        return t.value

    def add_ptrs(self, tensors, d_hex=None, hex_offset: int = 0) -> int:
        """Append one chain per tensor of `tensors`, 1-D uint8 device tensors of one length that
        lie wherever the caller has them (cec_hashq_add_ptrs); chain i writes its hex at
        d_hex + hex_offset + 64 * i (d_hex None: no output). The addresses travel in kernel
        arguments: nothing is copied or waited for. A None entry is refused by the library
        (CEC_EINVAL) with the ring unchanged; tensors of different lengths raise ErrShardSize.
        Returns the add's ticket (0 for an empty sequence)."""
        tensors = list(tensors)
        n = len(tensors)
        sizes = {t.numel() for t in tensors if t is not None}
        if len(sizes) > 1:
            raise ErrShardSize(ErrShardSize.__doc__)
        length = sizes.pop() if sizes else 0
        ptrs = (c_void_p * max(1, n))(*[_at(t) for t in tensors])
        t = c_uint64()
        check(_lib.load().cec_hashq_add_ptrs(self._h, ptrs, n, length, _at(d_hex, hex_offset),
                                             byref(t)),
              "HashQueue.add_ptrs")
        return t.value

    def add_concat_ptrs(self, chains, d_hex=None, hex_offset: int = 0, d_prefix_hex=None,
                        prefix_hex_offset: int = 0, length: Optional[int] = None) -> int:
        """Append one chain per row of `chains`: a row is a sequence of 1-D uint8 device tensors of
        one size (a multiple of 64) that lie wherever the caller has them, and its chain hashes
        them back to back, in place (cec_hashq_add_concat_ptrs). `length` is the chain's total
        byte count where the last tensor of a row counts only in part (None: all of it). Chain i
        writes its hex at d_hex + hex_offset + 64 * i and, with d_prefix_hex, the hex of its first
        tensor at d_prefix_hex + prefix_hex_offset + 64 * i. Rows of different lengths or tensors
        of different sizes raise ErrShardSize, a None entry ErrInvalidInput, empty tensors
        ErrShardNoData, before any C call; what the library refuses (a size that is no multiple
        of 64, a `length` that does not end in the last tensor) raises ErrInvalidInput with the
        ring unchanged. Returns the add's ticket (0 for an empty sequence, without a C call)."""
        chains, flat, part_len = _rows(chains)
        n = len(chains)
        if n == 0:
            return 0
        parts = len(chains[0])
        if part_len == 0:
            raise ErrShardNoData(ErrShardNoData.__doc__)
        ptrs = (c_void_p * len(flat))(*[_dev_ptr(t) for t in flat])
        t = c_uint64()
        hexp, prep = _at(d_hex, hex_offset), _at(d_prefix_hex, prefix_hex_offset)
        try:
            check(_lib.load().cec_hashq_add_concat_ptrs(self._h, ptrs, n, parts, part_len,
                                                        0 if length is None else length, hexp,
                                                        prep, byref(t)),
                  "HashQueue.add_concat_ptrs")
        except CecError as e:
            if e.code != _lib.CEC_EINVAL or isinstance(e, ErrInvalidInput):
                raise
            bad = ErrInvalidInput(str(e))
            bad.code = e.code
            raise bad from None
        return t.value

    def _expect(self, expect, n: int):
        """The recorded hashes of n chains as memory the device reads: a uint8 tensor [n][64]
        (device or pinned host) as it is, a list of n 64-byte `bytes` uploaded once. Returns
        (address, the uploaded tensor or None)."""
        import torch
        if isinstance(expect, torch.Tensor):
            if expect.dtype != torch.uint8 or expect.numel() != n * 64 or \
                    not expect.is_contiguous() or not (expect.is_cuda or expect.is_pinned()):
                raise ErrInvalidInput("expect must be a contiguous device or pinned uint8 [n][64]")
            return expect.data_ptr(), None
        rows = [bytes(h) for h in expect]
        if len(rows) != n or any(len(h) != 64 for h in rows):
            raise ErrInvalidInput("expect must hold one 64-byte hash per chain")
        host = torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.uint8)
        up = host.to(torch.device("cuda", self.device))
        return up.data_ptr(), up

    def _ok(self, d_ok, n: int):
        import torch
        if d_ok is None:
            d_ok = torch.empty(n, dtype=torch.uint8, device=torch.device("cuda", self.device))
        elif d_ok.numel() < n:
            raise ErrShardSize(ErrShardSize.__doc__)
        return d_ok

    def _release(self, everything: bool = False) -> None:
        """Drop the uploaded expectations of adds that are complete. A tensor is handed back to
        the allocator marked as in use on the queue's stream, so its memory is reused only once
        the ticks enqueued there have run."""
        if not self._kept:
            return
        import torch
        if self.stream is None:
            s = torch.cuda.default_stream(self.device)
        elif isinstance(self.stream, int):
            s = torch.cuda.ExternalStream(self.stream, device=self.device)
        else:
            s = self.stream
        live = []
        for ticket, up in self._kept:
            if everything or self.done(ticket):
                up.record_stream(s)
            else:
                live.append((ticket, up))
        self._kept = live

    def add_check(self, d_base, n: int, per: int, outer_stride: int, inner_stride: int,
                  length: int, d_expect, expect_outer: int, d_ok, ok_outer: int, d_hex=None,
                  hex_outer: int = 0, expect_offset: int = 0, ok_offset: int = 0,
                  hex_offset: int = 0) -> int:
        """`add` whose chains are also checked on the GPU (cec_hashq_add_check): chain i compares
        its digest with the 64 lowercase hex chars at
        d_expect + expect_offset + ((i // per) * expect_outer + i % per) * 64 (memory the device
        reads, 4-byte aligned: a device tensor, or the int address of e.g. a pinned host tensor)
        and writes 1 (equal) or 0 to d_ok + ok_offset + (i // per) * ok_outer + i % per, in the
        tick launch that completes it; nothing is preset. d_hex None: flags only. Returns the
        add's ticket."""
        t = c_uint64()
        check(_lib.load().cec_hashq_add_check(self._h, _dev_ptr(d_base), n, per, outer_stride,
                                              inner_stride, length, _at(d_expect, expect_offset),
                                              expect_outer, _at(d_ok, ok_offset), ok_outer,
                                              _at(d_hex, hex_offset), hex_outer, byref(t)),
              "HashQueue.add_check")
        return t.value

    def add_check_ptrs(self, tensors, expect, d_ok=None, d_hex=None):
        """`add_ptrs` with the check: one chain per tensor of `tensors` (1-D uint8 device tensors
        of one length, wherever they lie), chain i compared with expect[i], its flag (1 equal, 0
        not) written to d_ok[i] by the tick launch that completes it and its hex, with d_hex, to
        d_hex + 64 * i. `expect`: a device or pinned uint8 tensor [n][64], or a list of n 64-byte
        `bytes`, which is uploaded once and kept by the queue until the add is complete. d_ok
        None: a new uint8 device tensor [n]. Nothing waits. Returns (ticket, d_ok)."""
        return self.add_check_concat_ptrs([[t] for t in tensors], expect, d_ok, d_hex)

    def add_check_concat_ptrs(self, chains, expect, d_ok=None, d_hex=None, d_prefix_hex=None,
                              length: Optional[int] = None):
        """`add_concat_ptrs` with the check (cec_hashq_add_check_concat_ptrs): one chain per row
        of `chains` (a segment over its scattered data fragments), chain i compared with
        expect[i] and flagged in d_ok[i] as in `add_check_ptrs`; the prefix digest stays a hex
        output only. Rows of one tensor may be of any length. Returns (ticket, d_ok)."""
        chains, flat, part_len = _rows(chains)
        n = len(chains)
        d_ok = self._ok(d_ok, n)
        if n == 0:
            return 0, d_ok
        parts = len(chains[0])
        if parts > 1 and part_len == 0:
            raise ErrShardNoData(ErrShardNoData.__doc__)
        exp, up = self._expect(expect, n)
        ptrs = (c_void_p * max(1, len(flat)))(*[_dev_ptr(t) for t in flat])
        t = c_uint64()
        lib = _lib.load()
        if length is None:  # one buffer per chain: len is its length as it is, 0 included
            length = part_len if parts == 1 else 0
        try:
            check(lib.cec_hashq_add_check_concat_ptrs(self._h, ptrs, n, parts, part_len, length,
                                                      exp, _dev_ptr(d_ok), _at(d_hex),
                                                      _at(d_prefix_hex), byref(t)),
                  "HashQueue.add_check_concat_ptrs")
        except CecError as e:
            if e.code != _lib.CEC_EINVAL or isinstance(e, ErrInvalidInput):
                raise
            bad = ErrInvalidInput(str(e))
            bad.code = e.code
            raise bad from None
        if up is not None:
            self._kept.append((t.value, up))
        return t.value, d_ok

    def add_check_where_ptrs(self, tensors, expect, d_flags, per: int = 1, d_gate=None,
                             gate: int = 0, d_ok=None, d_hex=None):
        """`add_check_ptrs` whose chains the GPU admits (cec_hashq_add_check_where_ptrs): chain i
        runs iff tensors[i] is not None, d_flags[i] == 0 and (d_gate is None or
        d_gate[i // per] == gate), decided by the add's kernels from the uint8 device tensors
        d_flags [n] and d_gate when the queue's stream gets there, so both may still be in
        production on that stream (a scrub's flags and a repair's statuses: with per = k + m and
        gate = CEC_FLAG_REBUILT, the fragments the repair just rewrote). An admitted chain is
        compared with expect[i] and flagged 1 or 0 in d_ok[i] by the tick launch that completes
        it, its hex, with d_hex, at d_hex + 64 * i; every other chain gets d_ok[i] =
        CEC_HASHQ_SKIPPED from the add, no byte of its tensor is read and its hex is not written.
        `tensors` may hold None; the others are 1-D uint8 device tensors of one length (else
        ErrShardSize). `expect` as in `add_check_ptrs`: a list is uploaded once and kept until
        the add is complete. The add takes len(tensors) slots of the ring whatever is admitted.
        d_ok None: a new uint8 device tensor [n]. Nothing waits. Returns (ticket, d_ok)."""
        tensors = list(tensors)
        n = len(tensors)
        sizes = {t.numel() for t in tensors if t is not None}
        if len(sizes) > 1:
            raise ErrShardSize(ErrShardSize.__doc__)
        d_ok = self._ok(d_ok, n)
        if n == 0:
            return 0, d_ok
        if d_flags is None or d_flags.numel() < n or \
                (d_gate is not None and per > 0 and d_gate.numel() < (n + per - 1) // per):
            raise ErrShardSize(ErrShardSize.__doc__)
        exp, up = self._expect(expect, n)
        ptrs = (c_void_p * n)(*[_at(t) for t in tensors])
        t = c_uint64()
        check(_lib.load().cec_hashq_add_check_where_ptrs(
            self._h, ptrs, n, sizes.pop() if sizes else 0, exp, _dev_ptr(d_flags), per,
            _at(d_gate), gate, _dev_ptr(d_ok), _at(d_hex), byref(t)),
            "HashQueue.add_check_where_ptrs")
        if up is not None:
            self._kept.append((t.value, up))
        return t.value, d_ok

    def add_fragments(self, d_data, d_parity, nseg: int, k: int, m: int, shard_len: int,
                      d_hex, with_parity: bool = True) -> int:
        """Hash every fragment of a batch ([nseg][k][len] data, [nseg][m][len] parity) into
        d_hex[nseg][k+m][64] (fragment index order of SegmentList.fragment_list). Returns the
        ticket of the last add."""
        n_sh = k + m
        t = self.add(d_data, nseg * k, k, k * shard_len, shard_len, shard_len, d_hex,
                     n_sh, 0)
        if with_parity and m:
            t = self.add(d_parity, nseg * m, m, m * shard_len, shard_len, shard_len, d_hex,
                         n_sh, k * 64)
        return t

    def add_segments(self, d_data, nseg: int, seg_len: int, d_hex, seg_stride: Optional[int]
                     = None) -> int:
        """Hash nseg contiguous segments (SegmentList.hash) into d_hex[nseg][64]."""
        stride = seg_len if seg_stride is None else seg_stride
        return self.add(d_data, nseg, 1, stride, stride, seg_len, d_hex, 1, 0)

    def add_segment_lists(self, d_data, d_parity, nseg: int, k: int, m: int, shard_len: int,
                          d_seg_hex, d_frag_hex) -> int:
        """Every hash of a batch's SegmentLists ([nseg][k][len] data, [nseg][m][len] parity):
        segment hashes into d_seg_hex[nseg][64], fragment hashes into d_frag_hex[nseg][k+m][64].
        Data fragment 0's hash is the prefix digest of its segment's chain, so fragment 0 is
        hashed once (k*len + (k-1)*len + m*len bytes per segment instead of (2k+m)*len).
        Needs shard_len % 64 == 0 (else fragment 0 gets its own chain). Returns the ticket of
        the segment chains, the longest of the batch (the batch is done when they are)."""
        n_sh = k + m
        seg = k * shard_len
        if shard_len % 64 == 0:
            t = self.add(d_data, nseg, 1, seg, seg, seg, d_seg_hex, 1, 0, shard_len,
                         d_frag_hex, n_sh, 0)
            if k > 1:
                # data fragments 1..k-1: base shifted by one fragment, per = k - 1
                self.add(_dev_ptr(d_data) + shard_len, nseg * (k - 1), k - 1, seg, shard_len,
                         shard_len, d_frag_hex, n_sh, 64)
        else:
            t = self.add(d_data, nseg, 1, seg, seg, seg, d_seg_hex, 1, 0)
            self.add(d_data, nseg * k, k, seg, shard_len, shard_len, d_frag_hex, n_sh, 0)
        if m:
            self.add(d_parity, nseg * m, m, m * shard_len, shard_len, shard_len, d_frag_hex,
                     n_sh, k * 64)
        return t

    def add_segment_lists_device(self, segments, k: int, m: int, d_seg_hex, d_frag_hex) -> int:
        """add_segment_lists for shards that each lie in a tensor of their own, in place:
        segments[s] holds the k + m 1-D uint8 device tensors of segment s (data then parity, one
        size, a multiple of 64: else ErrShardSize). Segment hashes go into d_seg_hex[nseg][64],
        fragment hashes into d_frag_hex[nseg][k+m][64]. Per segment, a concat add runs the segment's
        chain over its k data shards and yields data fragment 0's hash as its prefix digest, and
        an add_ptrs hashes fragments 1..k+m-1. Nothing is copied. Returns the ticket of the last
        segment chain: the segment chains are the longest and complete in the same tick (0 for
        no segments)."""
        n_sh = k + m
        segments, _, size = _rows(segments, n_sh)
        if not segments:
            return 0
        if size % 64:
            raise ErrShardSize(ErrShardSize.__doc__)
        if size == 0:
            raise ErrShardNoData(ErrShardNoData.__doc__)
        # the C calls lay their hex out 64 bytes apart, a segment's fragment slots lie in its own
        # row of d_frag_hex: so one concat add and one pointer add per segment, a few small
        # launches each. The chains of all segments stand at the same block, so their part
        # boundaries cut a tick once, not once per segment.
        t = 0
        for s, seg in enumerate(segments):
            if n_sh > 1:
                self.add_ptrs(seg[1:], d_frag_hex, (s * n_sh + 1) * 64)
            t = self.add_concat_ptrs([seg[:k]], d_seg_hex, s * 64, d_frag_hex, s * n_sh * 64)
        return t

    def set_option(self, option: int, value: int) -> None:
        """cec_hashq_set_option (CEC_HQOPT_TICK: 0 auto, 1/2 two-wave prefetch depth, 3 one
        wave, 4 lane pairs: the shortest chain latency)."""
        check(_lib.load().cec_hashq_set_option(self._h, option, value), "HashQueue.set_option")

    def tick(self, max_blocks: int = 0) -> None:
        """Advance every live chain by at most max_blocks blocks (0: to completion)."""
        check(_lib.load().cec_hashq_tick(self._h, max_blocks), "HashQueue.tick")
        self._release()

    def finish(self) -> None:
        """Enqueue ticks until every chain added so far is complete."""
        check(_lib.load().cec_hashq_finish(self._h), "HashQueue.finish")
        self._release()

    def status(self, ticket: int = 0):
        done, live, left = c_int(), c_size_t(), c_uint64()
        check(_lib.load().cec_hashq_status(self._h, ticket, byref(done), byref(live),
                                           byref(left)), "HashQueue.status")
        return bool(done.value), live.value, left.value

    def done(self, ticket: int) -> bool:
        return self.status(ticket)[0]

    @property
    def live_chains(self) -> int:
        return self.status()[1]

    @property
    def blocks_left(self) -> int:
        return self.status()[2]
