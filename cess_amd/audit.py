"""Storage-audit chunks on HBM-resident fragment batches
(`audit_chunks`) and on fragments that are separate device tensors (`audit_chunks_device`).

Reference: a fragment is CHUNK_COUNT = 1024 chunks (primitives/common/src/lib.rs:62), so an 8 MiB
fragment is 1024 chunks of 8 KiB. A challenge (`generation_challenge`,
c-pallets/audit/src/lib.rs:901-988) names need = CHUNK_COUNT * 46 / 1000 = 47 distinct chunk
indices (`NetSnapShot.random_index_list`, types.rs:21): for seed = 1, 2, ..., index =
random_number(seed) % CHUNK_COUNT, repeats skipped (lib.rs:955-964), where random_number is the
chain's randomness decoded as u64 (lib.rs:1067-1076). Given that random stream, the selection
and the chunk bytes are byte-exact; the PoDR2 tags computed over the chunks live in the TEE and
are not in the reference (unpinned, not provided here).
"""
from __future__ import annotations

from ctypes import POINTER, byref, c_size_t, c_uint32, c_uint64, c_void_p
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .reedsolomon import (Encoder, ErrInvalidInput, _dev_ptr, _on_gpu, _stream_handle, check,
                          confirm_flagged)

CHUNK_COUNT = _lib.CEC_CHUNK_COUNT
CHALLENGE_NEED = CHUNK_COUNT * 46 // 1000  # 47


def challenge_indices(randoms: Sequence[int], chunk_count: int = CHUNK_COUNT,
                      need: int = CHALLENGE_NEED):
    """The reference's selection loop over random_number(1), random_number(2), ...:
    returns (indices, randoms consumed)."""
    r = np.ascontiguousarray(np.asarray(randoms, dtype=np.uint64))
    out = np.zeros(max(1, need), np.uint32)
    used = c_size_t()
    check(_lib.load().cec_challenge_indices(r.ctypes.data_as(POINTER(c_uint64)), r.size,
                                            chunk_count, need,
                                            out.ctypes.data_as(POINTER(c_uint32)), byref(used)),
          "challenge_indices")
    return out[:need].tolist(), used.value


RANDOM_BYTES = _lib.CEC_CHALLENGE_RANDOM_BYTES


def challenge_random_list(randomness: Sequence[bytes], need: int = CHALLENGE_NEED):
    """NetSnapShot.random_list (c-pallets/audit/src/lib.rs:966-974, generate_challenge_random
    :1079-1096): randomness[i] = the chain's 32-byte randomness output for the subject
    (MyPalletId, now + 2 + i) (records.audit_random_subject(now + 2 + i); None as 32 zero bytes).
    Returns (the `need` distinct 20-byte values in order, outputs consumed)."""
    buf = b"".join(bytes(r) if r is not None else bytes(32) for r in randomness)
    if any(r is not None and len(r) != 32 for r in randomness):
        raise ValueError("each randomness output is 32 bytes (an H256)")
    src = np.frombuffer(buf, np.uint8).copy() if buf else np.zeros(1, np.uint8)
    out = np.zeros(max(1, need) * RANDOM_BYTES, np.uint8)
    used = c_size_t()
    check(_lib.load().cec_challenge_random_list(src.ctypes.data, len(randomness), need,
                                                out.ctypes.data, byref(used)),
          "challenge_random_list")
    return [out[i * RANDOM_BYTES:(i + 1) * RANDOM_BYTES].tobytes() for i in range(need)], \
        used.value


def audit_chunks(enc: Encoder, d_data, d_parity, nseg: int, shard_len: int,
                 indices: Sequence[int], d_chunks=None, d_hex=None,
                 chunk_count: int = CHUNK_COUNT, stream=None) -> None:
    """Gather the challenged chunks of every fragment of a batch ([nseg][k][len] data and, if
    given, [nseg][m][len] parity) into d_chunks [nfrag][nidx][len / chunk_count] and/or their
    SHA-256 hex into d_hex [nfrag][nidx][64] (fragments in batch order)."""
    idx = np.ascontiguousarray(np.asarray(indices, dtype=np.uint32))
    check(enc._lib.cec_audit_chunks(
        enc._h, _dev_ptr(d_data), None if d_parity is None else _dev_ptr(d_parity), nseg,
        shard_len, chunk_count, idx.ctypes.data_as(POINTER(c_uint32)), idx.size,
        None if d_chunks is None else _dev_ptr(d_chunks),
        None if d_hex is None else _dev_ptr(d_hex), _stream_handle(stream)), "audit_chunks")


def audit_chunks_device(enc: Encoder, frags: Sequence, indices: Sequence[int], d_chunks=None,
                        d_hex=None, chunk_count: int = CHUNK_COUNT, stream=None) -> None:
    """audit_chunks for scattered fragments, in place (cec_audit_chunks_ptrs): `frags` is a
    sequence of 1-D uint8 device tensors of one length, each in its own allocation (a miner holds
    one fragment of many segments). Chunk indices[j] of frags[f] goes to d_chunks [nfrag][nidx]
    [len / chunk_count] and/or its SHA-256 hex to d_hex [nfrag][nidx][64]. With d_chunks None the
    chunks are hashed where they lie: no chunk byte is copied. An empty `frags` returns quietly;
    a None entry raises ErrInvalidInput, tensors of different lengths ErrShardSize, empty ones
    ErrShardNoData, before any C call. Enqueued on `stream` (default: torch's current stream) and
    not waited for."""
    frags = list(frags)
    if not frags:
        return
    if any(t is None for t in frags):
        raise ErrInvalidInput(ErrInvalidInput.__doc__)
    size = enc._check_device_shards(frags)
    import torch
    dev = torch.device("cuda", enc.device)
    ptrs = (c_void_p * len(frags))(*[_dev_ptr(_on_gpu(t, dev)) for t in frags])
    idx = np.ascontiguousarray(np.asarray(indices, dtype=np.uint32))
    check(enc._lib.cec_audit_chunks_ptrs(
        enc._h, ptrs, len(frags), size, chunk_count, idx.ctypes.data_as(POINTER(c_uint32)),
        idx.size, None if d_chunks is None else _dev_ptr(d_chunks),
        None if d_hex is None else _dev_ptr(d_hex), enc._device_stream(stream)),
        "audit_chunks_device")


def scrub_device(frags: Sequence, recorded, queue=None, d_ok=None):
    """A miner's scrub: does each stored fragment still hash to what the chain recorded for it
    (`FragmentInfo.hash`)? `frags` is a sequence of 1-D uint8 device tensors of one length, each
    wherever it lies; `recorded` their hashes, a list of 64-byte `bytes` or a device / pinned
    uint8 tensor [n][64]. Returns a uint8 device tensor (d_ok, or a new one): flag f is 1 where
    SHA-256(frags[f]) equals recorded[f], else 0, written on the GPU by the hash queue's ticks
    (HashQueue.add_check_ptrs). The chains are added and ticked to completion on `queue`'s stream
    and nothing is waited for: the flags are final when that stream gets there. queue None: a
    queue of the call's size on torch's current stream, owned and closed by the call (creating a
    queue waits once for its table's allocation; a service that scrubs again and again keeps
    one)."""
    import torch
    from .hashq import HashQueue
    frags = list(frags)
    if queue is not None:
        _, d_ok = queue.add_check_ptrs(frags, recorded, d_ok)
        queue.finish()
        return d_ok
    if not frags:
        return torch.empty(0, dtype=torch.uint8, device="cuda") if d_ok is None else d_ok
    if any(t is None for t in frags):
        raise ErrInvalidInput(ErrInvalidInput.__doc__)
    dev = frags[0].device
    cap = 1 << max(0, len(frags) - 1).bit_length()
    with HashQueue(capacity=cap, device=dev.index or 0,
                   stream=torch.cuda.current_stream(dev)) as q:
        _, d_ok = q.add_check_ptrs(frags, recorded, d_ok)
        q.finish()
    return d_ok


def scrub_repair_device(enc: Encoder, segments: Sequence, recorded, queue=None):
    """A miner's scrub that heals what it finds, without a host round trip: `segments` is a list
    of lists of k + m 1-D uint8 device tensors of one length (None = not held), `recorded` their
    hashes, per segment a list of k + m 64-byte `bytes` (anything at a shard not held), or one
    uint8 device / pinned tensor [nseg][k + m][64]. All on `queue`'s stream, nothing waited for:
    every held fragment gets a checked chain (HashQueue.add_check_ptrs, segment-major, the flag of
    fragment i of segment s at d_flags[s][i]; slots not held get no chain and their flag byte is
    whatever the buffer held, which the repair ignores), the queue is ticked to completion
    (finish()), and Encoder.RepairFlaggedDevice reads the flags where the ticks left them: a
    segment with exactly one fragment that no longer hashes to its record, and at least k that
    do, has that fragment rebuilt in place from the others. Returns (d_flags [nseg][k + m],
    d_status [nseg] of CEC_FLAG_* codes), both final when the stream gets there. The rebuild is
    not re-checked: a caller who wants proof scrubs again (a fragment whose *record* is wrong is
    rebuilt to the same bytes and flagged again). queue None: a queue of the call's size on
    torch's current stream, owned and closed by the call, as in scrub_device."""
    return _scrub_repair(enc, segments, recorded, queue, enc.RepairFlaggedDevice)


def scrub_repair_multi_device(enc: Encoder, segments: Sequence, recorded,
                              max_bad: int = _lib.CEC_FLAG_MULTI_MAX, queue=None):
    """scrub_repair_device for the wider codes, where several fragments of a segment may be gone
    at once: the same checked chains and ticks, then Encoder.RepairFlaggedMultiDevice reads the
    flags: a segment with 1 to `max_bad` fragments that no longer hash to their records, and at
    least k that do, has all of them rebuilt in place. Arguments and the returned (d_flags,
    d_status) as there."""
    def repair(segs, d_flags, stream):
        return enc.RepairFlaggedMultiDevice(segs, d_flags, max_bad=max_bad, stream=stream)
    return _scrub_repair(enc, segments, recorded, queue, repair)


def _scrub_table(enc, segments, recorded):
    """What the scrubs above hash: (segments as lists, their slots segment-major, the recorded
    hashes slot by slot, the runs [a, b) of held slots, d_flags [nseg][k + m])."""
    import torch
    segments = [list(seg) for seg in segments]
    nseg, n = len(segments), enc.Shards
    if any(len(seg) != n for seg in segments):
        raise ErrInvalidInput(ErrInvalidInput.__doc__)
    dev = torch.device("cuda", enc.device)
    slots = [t for seg in segments for t in seg]
    d_flags = torch.empty((nseg, n), dtype=torch.uint8, device=dev)
    if isinstance(recorded, torch.Tensor):
        if recorded.numel() != nseg * n * 64:
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        rec = recorded.view(nseg * n, 64)
    else:
        rec = [h for row in recorded for h in row]
        if len(rec) != nseg * n:
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
    # one add per run of held slots: its flags land at the run's place in d_flags
    runs, a = [], 0
    while a < len(slots):
        if slots[a] is None:
            a += 1
            continue
        b = a
        while b < len(slots) and slots[b] is not None:
            b += 1
        runs.append((a, b))
        a = b
    return segments, slots, rec, runs, d_flags


def _scrub_repair(enc, segments, recorded, queue, repair):
    """The scrub of the two calls above; repair(segments, d_flags, stream=...) ends it."""
    import torch
    from .hashq import HashQueue
    segments, slots, rec, runs, d_flags = _scrub_table(enc, segments, recorded)

    def go(q):
        flat = d_flags.view(-1)
        for a, b in runs:
            q.add_check_ptrs(slots[a:b], rec[a:b], flat[a:b])
        q.finish()
        stream = q.stream if q.stream is not None else 0  # a queue without one: the null stream
        return repair(segments, d_flags, stream=stream)

    if queue is not None:
        return d_flags, go(queue)
    held = sum(b - a for a, b in runs)
    cap = 1 << max(0, held - 1).bit_length()
    dev = torch.device("cuda", enc.device)
    with HashQueue(capacity=cap, device=enc.device, stream=torch.cuda.current_stream(dev)) as q:
        return d_flags, go(q)


def scrub_repair_confirm_device(enc: Encoder, segments: Sequence, recorded, max_bad: int = 1,
                                queue=None):
    """scrub_repair_device (max_bad == 1) or scrub_repair_multi_device (max_bad > 1) with the
    proof the chain asks of restoral_order_complete: after the repair, exactly the fragments it
    rewrote are hashed again and compared with their records, chosen on the GPU from d_flags and
    d_status (HashQueue.add_check_where_ptrs over the whole [nseg][k + m] table, None where a shard
    is not held, gated on CEC_FLAG_REBUILT), and confirm_flagged folds the result into one code
    per segment. Arguments as in scrub_repair_device. Returns (d_flags, d_status,
    d_ok [nseg][k + m], d_confirm [nseg]): d_ok is 1 where a rebuilt fragment now hashes to its record, 0 where it
    still does not, CEC_HASHQ_SKIPPED everywhere else; d_confirm is CEC_CONFIRM_PROVEN for a healed
    segment, CEC_CONFIRM_REFUTED where a record itself is wrong (the fragment is rebuilt to the
    same bytes and fails again), CEC_CONFIRM_NONE for a segment that was not rebuilt. All on the
    queue's stream, nothing waited for or copied out. A caller's queue, which has to be idle and
    hold at least k + m chains, may be smaller than the table: the scrub runs in adds that fit
    and the proof in slices of whole segments, each ticked to completion before the next. queue
    None: a queue of the table's size on torch's current stream, owned and closed by the call."""
    import torch
    from .hashq import HashQueue
    segments, slots, rec, runs, d_flags = _scrub_table(enc, segments, recorded)
    nseg, n = len(segments), enc.Shards
    dev = torch.device("cuda", enc.device)

    def go(q):
        stream = q.stream if q.stream is not None else 0  # a queue without one: the null stream
        flat = d_flags.view(-1)
        free = q.capacity
        for a, b in runs:
            while a < b:
                if free == 0:
                    q.finish()
                    free = q.capacity
                c = min(b, a + free)
                q.add_check_ptrs(slots[a:c], rec[a:c], flat[a:c])
                free -= c - a
                a = c
        q.finish()
        if max_bad == 1:
            d_status = enc.RepairFlaggedDevice(segments, d_flags, stream=stream)
        else:
            d_status = enc.RepairFlaggedMultiDevice(segments, d_flags, max_bad=max_bad,
                                                    stream=stream)
        d_ok = torch.empty((nseg, n), dtype=torch.uint8, device=dev)
        ok = d_ok.view(-1)
        step = max(1, q.capacity // n)  # whole segments per slice
        for s0 in range(0, nseg, step):
            s1 = min(nseg, s0 + step)
            a, b = s0 * n, s1 * n
            q.add_check_where_ptrs(slots[a:b], rec[a:b], flat[a:b], per=n, d_gate=d_status[s0:s1],
                                   gate=_lib.CEC_FLAG_REBUILT, d_ok=ok[a:b])
            q.finish()
        return d_flags, d_status, d_ok, confirm_flagged(d_status, d_ok, n, stream=stream)

    if queue is not None:
        return go(queue)
    cap = 1 << max(0, nseg * n - 1).bit_length()
    with HashQueue(capacity=cap, device=enc.device, stream=torch.cuda.current_stream(dev)) as q:
        return go(q)


def _queue_stream(q):
    """(the stream handle the C calls take, torch's view of the same stream) of a HashQueue."""
    import torch
    if q.stream is None:  # a queue without one: the null stream
        return 0, torch.cuda.default_stream(q.device)
    if isinstance(q.stream, int):
        return q.stream, torch.cuda.ExternalStream(q.stream, device=q.device)
    return q.stream, q.stream


def locate_repair_device(enc: Encoder, segments: Sequence, nsyn: int = _lib.CEC_LOCATE_SYN_MAX,
                         recorded=None, queue=None):
    """A scrub at the parity rate that heals what it finds: Encoder.LocateDevice names the one
    fragment of a segment that disagrees with the others, from parity alone, and
    Encoder.RepairFlaggedDevice reads those flags on the same stream and rebuilds it in place.
    `segments` as in scrub_repair_device. Without `recorded` nothing is hashed and the stream is
    torch's current one, or `queue`'s: returns (d_flags [nseg][k + m], d_locate [nseg] of
    CEC_LOCATE_* codes, d_status [nseg] of CEC_FLAG_* codes). With `recorded` (per segment k + m
    64-byte hashes, or one tensor [nseg][k + m][64]) the proof of scrub_repair_confirm_device
    follows: exactly the rebuilt fragments are hashed (HashQueue.add_check_where_ptrs gated on
    CEC_FLAG_REBUILT) and confirm_flagged folds the result: returns (d_flags, d_locate, d_status,
    d_ok [nseg][k + m], d_confirm [nseg]). A FOUND segment is REBUILT; an AMBIGUOUS one has every
    held flag 0, so the repair reports LOST and writes nothing. Nothing is waited for. queue None
    with `recorded`: a queue of the table's size on torch's current stream, owned and closed by
    the call."""
    import torch
    from .hashq import HashQueue
    segments = [list(seg) for seg in segments]
    nseg, n = len(segments), enc.Shards
    if any(len(seg) != n for seg in segments):
        raise ErrInvalidInput(ErrInvalidInput.__doc__)
    dev = torch.device("cuda", enc.device)

    def heal(stream):
        d_flags, d_locate = enc.LocateDevice(segments, nsyn=nsyn, stream=stream)
        return d_flags, d_locate, enc.RepairFlaggedDevice(segments, d_flags, stream=stream)

    if recorded is None:
        return heal(torch.cuda.current_stream(dev) if queue is None else _queue_stream(queue)[0])
    _, slots, rec, _, _ = _scrub_table(enc, segments, recorded)

    def go(q):
        stream = _queue_stream(q)[0]
        d_flags, d_locate, d_status = heal(stream)
        d_ok = torch.empty((nseg, n), dtype=torch.uint8, device=dev)
        flat, ok = d_flags.view(-1), d_ok.view(-1)
        step = max(1, q.capacity // n)  # whole segments per slice
        for s0 in range(0, nseg, step):
            s1 = min(nseg, s0 + step)
            a, b = s0 * n, s1 * n
            q.add_check_where_ptrs(slots[a:b], rec[a:b], flat[a:b], per=n, d_gate=d_status[s0:s1],
                                   gate=_lib.CEC_FLAG_REBUILT, d_ok=ok[a:b])
            q.finish()
        return d_flags, d_locate, d_status, d_ok, confirm_flagged(d_status, d_ok, n, stream=stream)

    if queue is not None:
        return go(queue)
    cap = 1 << max(0, nseg * n - 1).bit_length()
    with HashQueue(capacity=cap, device=enc.device, stream=torch.cuda.current_stream(dev)) as q:
        return go(q)


def locate_repair_multi_device(enc: Encoder, segments: Sequence,
                               max_bad: int = _lib.CEC_LOCATE_BAD_MAX,
                               nsyn: int = _lib.CEC_LOCATE_SYN_MAX, recorded=None, queue=None):
    """locate_repair_device for up to `max_bad` bad fragments per segment:
    Encoder.LocateMultiDevice names the one or two fragments of a segment that disagree with the
    others, from parity alone, and Encoder.RepairFlaggedMultiDevice(..., max_bad=max_bad) reads
    those flags on the same stream and rebuilds them in place. Arguments, streams and the proof
    with `recorded` as in locate_repair_device. Returns (d_flags, d_locate, d_status), or with
    `recorded` (d_flags, d_locate, d_status, d_ok, d_confirm). A FOUND segment is REBUILT; an
    AMBIGUOUS one (three bad fragments, say) has every held flag 0, so the repair reports LOST and
    writes nothing. Nothing is waited for."""
    import torch
    from .hashq import HashQueue
    segments = [list(seg) for seg in segments]
    nseg, n = len(segments), enc.Shards
    if any(len(seg) != n for seg in segments):
        raise ErrInvalidInput(ErrInvalidInput.__doc__)
    dev = torch.device("cuda", enc.device)

    def heal(stream):
        d_flags, d_locate, _ = enc.LocateMultiDevice(segments, nsyn=nsyn, max_bad=max_bad,
                                                     stream=stream)
        return d_flags, d_locate, enc.RepairFlaggedMultiDevice(segments, d_flags,
                                                               max_bad=max_bad, stream=stream)

    if recorded is None:
        return heal(torch.cuda.current_stream(dev) if queue is None else _queue_stream(queue)[0])
    _, slots, rec, _, _ = _scrub_table(enc, segments, recorded)

    def go(q):
        stream = _queue_stream(q)[0]
        d_flags, d_locate, d_status = heal(stream)
        d_ok = torch.empty((nseg, n), dtype=torch.uint8, device=dev)
        flat, ok = d_flags.view(-1), d_ok.view(-1)
        step = max(1, q.capacity // n)  # whole segments per slice
        for s0 in range(0, nseg, step):
            s1 = min(nseg, s0 + step)
            a, b = s0 * n, s1 * n
            q.add_check_where_ptrs(slots[a:b], rec[a:b], flat[a:b], per=n, d_gate=d_status[s0:s1],
                                   gate=_lib.CEC_FLAG_REBUILT, d_ok=ok[a:b])
            q.finish()
        return d_flags, d_locate, d_status, d_ok, confirm_flagged(d_status, d_ok, n, stream=stream)

    if queue is not None:
        return go(queue)
    cap = 1 << max(0, nseg * n - 1).bit_length()
    with HashQueue(capacity=cap, device=enc.device, stream=torch.cuda.current_stream(dev)) as q:
        return go(q)


def scrub_located_device(enc: Encoder, segments: Sequence, recorded,
                         nsyn: int = _lib.CEC_LOCATE_SYN_MAX, queue=None):
    """A scrub that hashes only what parity cannot settle, RS(2,1) included: Encoder.LocateDevice
    over the table, then HashQueue.add_check_where_ptrs over all of it with per = k + m, d_gate =
    the locate codes and gate = CEC_LOCATE_AMBIGUOUS, so exactly the held fragments of the
    inconsistent segments no single shard explains (with one parity shard: of every inconsistent
    segment) get a checked chain, ticked to completion; every other fragment is CEC_HASHQ_SKIPPED
    and no byte of it is hashed. The two are merged on the device: flags = where(d_ok == SKIPPED,
    located flags, d_ok). Arguments as in scrub_repair_device. Returns (d_flags [nseg][k + m],
    d_locate [nseg]): flags ready for the flagged repairs and the flagged read. Nothing is waited
    for. A caller's queue has to be idle and hold at least k + m chains."""
    import torch
    from .hashq import HashQueue
    segments, slots, rec, _, _ = _scrub_table(enc, segments, recorded)
    nseg, n = len(segments), enc.Shards
    dev = torch.device("cuda", enc.device)

    def go(q):
        stream, tstream = _queue_stream(q)
        d_flags, d_locate = enc.LocateDevice(segments, nsyn=nsyn, stream=stream)
        d_ok = torch.empty((nseg, n), dtype=torch.uint8, device=dev)
        flat, ok = d_flags.view(-1), d_ok.view(-1)
        step = max(1, q.capacity // n)  # whole segments per slice
        for s0 in range(0, nseg, step):
            s1 = min(nseg, s0 + step)
            a, b = s0 * n, s1 * n
            q.add_check_where_ptrs(slots[a:b], rec[a:b], flat[a:b], per=n,
                                   d_gate=d_locate[s0:s1], gate=_lib.CEC_LOCATE_AMBIGUOUS,
                                   d_ok=ok[a:b])
            q.finish()
        with torch.cuda.stream(tstream):
            merged = torch.where(d_ok == _lib.CEC_HASHQ_SKIPPED, d_flags, d_ok)
        return merged, d_locate

    if queue is not None:
        return go(queue)
    cap = 1 << max(0, nseg * n - 1).bit_length()
    with HashQueue(capacity=cap, device=enc.device, stream=torch.cuda.current_stream(dev)) as q:
        return go(q)
