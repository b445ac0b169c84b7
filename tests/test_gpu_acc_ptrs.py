"""Parity accumulated shard by shard on scattered device shards: cec_encode_idx_ptrs /
cec_update_ptrs and the Python methods over them (EncodeIdxDevice, EncodeIdxDeviceBatch,
UpdateDevice, UpdateDeviceBatch), bit-exact against the oracle (c_encode for full encodes,
build_matrix + mul_row_acc for single contributions).

Buffer setup as in test_gpu_acc.py: every parity shard is an allocation of its own between two
64-byte guard bands of 0xA5 that are checked afterwards (the equivalence test, which needs a batch
layout, and the row-slicing test, whose 65,537 shards are slices of one guarded allocation, are the
exceptions); every input is compared with its host copy afterwards; what a call must not read
holds garbage. Every pointer handed to the library points into a live allocation."""
from ctypes import c_void_p

import numpy as np
import pytest

from tests.test_gpu_acc import Dev, batch, oracle_parity, encoder

pytestmark = pytest.mark.gpu

LENS = [1, 15, 16, 17, 4096 + 16 + 3, 65536 + 16]
NARROW = [(2, 1), (4, 2), (10, 4)]
WIDE = [(32, 32), (3, 40), (128, 128)]
# the wide codes' shapes are those test_gpu_acc.py already has the oracle's parity for
WIDE_SHAPES = [(1, 3), (17, 1), (4096 + 16 + 3, 3), (65536 + 16, 1)]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    t.cuda.init()
    return t


@pytest.fixture(scope="module")
def cess(torch):
    import cess_amd
    return cess_amd


@pytest.fixture(scope="module")
def lib(cess):
    from cess_amd import _lib
    return _lib.load()


class Inputs:
    """Shards [nseg][k][ln] in one allocation, `off` bytes into it, every shard on a 16-byte
    multiple from its start with at least 16 bytes of 0xA5 behind it. t[s][j]: the shard's tensor."""

    def __init__(self, torch, arr, off=0):
        nseg, k, ln = arr.shape
        stride = (ln + 15) // 16 * 16 + 16
        host = np.full((nseg, k, stride), 0xA5, dtype=np.uint8)
        host[:, :, :ln] = arr
        self.d = Dev(torch, host, off=off)
        lo = self.d.lo
        self.t = [[self.d.dev[lo + (s * k + j) * stride:lo + (s * k + j) * stride + ln]
                   for j in range(k)] for s in range(nseg)]

    def check(self, what):
        self.d.check(what)


class Parity:
    """Parity shards [nseg][m][ln], each an allocation of its own between guard bands (`off`
    bytes into it). t[s][o]: the shard's tensor; check(what, want [nseg][m][ln])."""

    def __init__(self, torch, arr, off=0):
        nseg, m, ln = arr.shape
        self.d = [[Dev(torch, arr[s, o], off=off, guard=True) for o in range(m)]
                  for s in range(nseg)]
        self.t = [[d.dev[d.lo:d.lo + ln] for d in row] for row in self.d]

    def check(self, what, want=None):
        for s, row in enumerate(self.d):
            for o, d in enumerate(row):
                d.check((what, "segment", s, "parity", o), None if want is None else want[s][o])


def table(rows):
    flat = [None if t is None else t.data_ptr() for row in rows for t in row]
    return (c_void_p * len(flat))(*flat)


def stream_handle(stream):
    return None if stream is None else stream.cuda_stream


def encode_idx(lib, enc, data, parity, ln, accumulate=1, stream=None):
    """data[s]: k tensors or None, parity[s]: m tensors or None, as EncodeIdxDeviceBatch takes."""
    return lib.cec_encode_idx_ptrs(enc._h, table(data), table(parity), len(data), ln, accumulate,
                                   stream_handle(stream))


def update(lib, enc, old, new, parity, ln, stream=None):
    return lib.cec_update_ptrs(enc._h, table(old), table(new), table(parity), len(old), ln,
                               stream_handle(stream))


def garbage(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def contribution(orc, k, m, shards, fed):
    """[m][ln]: XOR over j in fed of E[k+o][j] * shards[j], from the oracle's matrix."""
    E = orc.build_matrix(k, k + m)
    out = np.zeros((m, shards.shape[1]), dtype=np.uint8)
    for j in fed:
        for o in range(m):
            orc.mul_row_acc(out[o], E[k + o][j], shards[j])
    return out


# ---- 1. feeding every data shard equals Encode ------------------------------------------------------

FULL_CASES = ([(k, m, ln, nseg) for k, m in NARROW for ln in LENS for nseg in (1, 3)] +
              [(k, m, ln, nseg) for k, m in WIDE for ln, nseg in WIDE_SHAPES])


@pytest.mark.parametrize("k,m,ln,nseg", FULL_CASES)
def test_every_shard_equals_encode(torch, cess, lib, corc, k, m, ln, nseg):
    """One shard per call in a shuffled order, and all of them in one call, into zeroed parity.
    (10,4) and wider cross the 8-input chunk, (3,40) and (128,128) the 32-output chunk."""
    data, par = batch(corc, k, m, ln, nseg)
    enc = encoder(cess, k, m)
    d_in = Inputs(torch, data)
    zeros = np.zeros((nseg, m, ln), dtype=np.uint8)
    one_by_one, at_once = Parity(torch, zeros), Parity(torch, zeros)
    for j in np.random.default_rng(k + 31 * m + ln).permutation(k):
        fed = [[row[i] if i == j else None for i in range(k)] for row in d_in.t]
        assert encode_idx(lib, enc, fed, one_by_one.t, ln) == 0
    assert encode_idx(lib, enc, d_in.t, at_once.t, ln) == 0
    torch.cuda.synchronize()
    one_by_one.check((k, m, ln, nseg, "one by one"), par)
    at_once.check((k, m, ln, nseg, "at once"), par)
    d_in.check((k, m, ln, nseg, "data"))


# ---- 2. mixed sets in one call ------------------------------------------------------------------------


def mixed_case(torch, corc, orc):
    """RS(4,2), five segments: one feeds one shard, one two, one nothing, one all four with p0
    not named, one has no parity named. -> (inputs, parity, fed rows, parity rows, want)."""
    k, m, ln, nseg = 4, 2, 4096 + 16 + 3, 5
    data, _ = batch(corc, k, m, ln, nseg)
    start = garbage(21, (nseg, m, ln))
    d_in, d_par = Inputs(torch, data), Parity(torch, start)
    fed_sets = [[2], [0, 3], [], [0, 1, 2, 3], [1]]
    named = [[0, 1], [0, 1], [0, 1], [1], []]
    fed = [[d_in.t[s][j] if j in fed_sets[s] else None for j in range(k)] for s in range(nseg)]
    par = [[d_par.t[s][o] if o in named[s] else None for o in range(m)] for s in range(nseg)]
    want = start.copy()
    for s in range(nseg):
        add = contribution(orc, k, m, data[s], fed_sets[s])
        for o in named[s]:
            want[s, o] ^= add[o]
    assert np.array_equal(want[2], start[2]) and np.array_equal(want[4], start[4])
    assert np.array_equal(want[3, 0], start[3, 0])
    return d_in, d_par, fed, par, want


def test_mixed_sets_in_one_call(torch, cess, lib, corc, orc):
    d_in, d_par, fed, par, want = mixed_case(torch, corc, orc)
    assert encode_idx(lib, encoder(cess, 4, 2), fed, par, want.shape[2]) == 0
    torch.cuda.synchronize()
    d_par.check("mixed sets", want)
    d_in.check("mixed sets data")


# ---- 3. overwrite ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("k,m", [(4, 2), (10, 4), (3, 40)])
@pytest.mark.parametrize("ln", [17, 4096 + 16 + 3])
def test_overwrite(torch, cess, lib, corc, orc, k, m, ln):
    """accumulate = 0 onto garbage: a segment that feeds everything gets its parity, one that feeds
    a subset the subset's product, one that names parity and feeds nothing zeros."""
    nseg = 3
    data, full = batch(corc, k, m, ln, nseg)
    enc = encoder(cess, k, m)
    d_in, d_par = Inputs(torch, data), Parity(torch, garbage(ln + k, (nseg, m, ln)))
    subset = [0, k - 1]
    fed = [d_in.t[0], [t if j in subset else None for j, t in enumerate(d_in.t[1])], [None] * k]
    want = np.stack([full[0], contribution(orc, k, m, data[1], subset),
                     np.zeros((m, ln), np.uint8)])
    assert encode_idx(lib, enc, fed, d_par.t, ln, 0) == 0
    torch.cuda.synchronize()
    d_par.check((k, m, ln, "overwrite"), want)
    d_in.check((k, m, ln, "overwrite data"))


# ---- 4. Update ------------------------------------------------------------------------------------------

UPDATE_SETS = {(4, 2): [[1], [0, 3], []],
               (10, 4): [list(range(10)), [2], [0, 9]],
               (32, 32): [list(range(5, 22)), [31], list(range(32))],
               (3, 40): [[0, 2], [1], [0, 1, 2]]}


def update_case(torch, corc, k, m):
    """Three segments of 4096 + 16 + 3 bytes, each with its own changed set. The caller's old and
    new copies hold different garbage in the unchanged slots, which are passed as NULL; slot
    `same` of segment 1 is passed with old == new at one address. -> (old inputs, new inputs,
    parity, old rows, new rows, the oracle's parity of the new data)."""
    ln, nseg = 4096 + 16 + 3, 3
    data, par = batch(corc, k, m, ln, nseg)
    sets = UPDATE_SETS[(k, m)]
    new = data.copy()
    old_buf = garbage(7 * k + m, data.shape)
    new_buf = old_buf ^ 0x5A
    for s, ch in enumerate(sets):
        new[s, ch] = garbage(100 * k + s, (len(ch), ln))
        old_buf[s, ch], new_buf[s, ch] = data[s, ch], new[s, ch]
    d_old, d_new, d_par = Inputs(torch, old_buf), Inputs(torch, new_buf), Parity(torch, par)
    old = [[d_old.t[s][j] if j in sets[s] else None for j in range(k)] for s in range(nseg)]
    nw = [[d_new.t[s][j] if j in sets[s] else None for j in range(k)] for s in range(nseg)]
    same = next(j for j in range(k) if j not in sets[1])
    old[1][same] = nw[1][same] = d_old.t[1][same]
    return d_old, d_new, d_par, old, nw, oracle_parity(corc, k, m, new)


@pytest.mark.parametrize("k,m", sorted(UPDATE_SETS))
def test_update(torch, cess, lib, corc, k, m):
    d_old, d_new, d_par, old, new, want = update_case(torch, corc, k, m)
    assert update(lib, encoder(cess, k, m), old, new, d_par.t, want.shape[2]) == 0
    torch.cuda.synchronize()
    d_par.check((k, m, "update"), want)
    d_old.check((k, m, "old"))
    d_new.check((k, m, "new"))


# ---- 5. parity subsets on Update ------------------------------------------------------------------------


def test_update_of_one_parity(torch, cess, lib, corc):
    k, m = 4, 2
    d_old, d_new, d_par, old, new, want = update_case(torch, corc, k, m)
    before = batch(corc, k, m, want.shape[2], 3)[1]
    only_p1 = [[None, row[1]] for row in d_par.t]
    assert update(lib, encoder(cess, k, m), old, new, only_p1, want.shape[2]) == 0
    torch.cuda.synchronize()
    expect = want.copy()
    expect[:, 0] = before[:, 0]  # p0 was not passed: untouched
    d_par.check("only p1", expect)
    d_old.check("only p1, old")
    d_new.check("only p1, new")


# ---- 6. alignment ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("ln", [1, 17, 4096 + 16 + 3])
def test_alignment(torch, cess, lib, corc, ln):
    """One input one byte off, then one parity three bytes off: the whole call runs byte-wise and
    gives the bytes of the aligned run."""
    k, m, nseg = 4, 2, 3
    data, par = batch(corc, k, m, ln, nseg)
    enc = encoder(cess, k, m)
    start = garbage(ln, (nseg, m, ln))
    d_in, aligned = Inputs(torch, data), Parity(torch, start)
    assert encode_idx(lib, enc, d_in.t, aligned.t, ln) == 0
    torch.cuda.synchronize()
    aligned.check((ln, "aligned"), par ^ start)
    got = np.stack([np.stack([t.cpu().numpy() for t in row]) for row in aligned.t])
    # one input of segment 1 at an odd address
    odd_in = Inputs(torch, data[1:2, 2:3], off=1)
    assert odd_in.t[0][0].data_ptr() % 16 == 1
    fed = [list(row) for row in d_in.t]
    fed[1][2] = odd_in.t[0][0]
    d_par = Parity(torch, start)
    assert encode_idx(lib, enc, fed, d_par.t, ln) == 0
    torch.cuda.synchronize()
    d_par.check((ln, "odd input"), got)
    odd_in.check((ln, "odd input data"))
    # one parity of segment 2 at an odd address
    odd_par = Parity(torch, start[2:3, 1:2], off=3)
    assert odd_par.t[0][0].data_ptr() % 16 == 3
    d_par = Parity(torch, start)
    named = [list(row) for row in d_par.t]
    named[2][1] = odd_par.t[0][0]
    assert encode_idx(lib, enc, d_in.t, named, ln) == 0
    torch.cuda.synchronize()
    expect = got.copy()
    expect[2, 1] = start[2, 1]  # its aligned stand-in was not passed
    d_par.check((ln, "odd parity, the others"), expect)
    odd_par.check((ln, "odd parity"), got[2:3, 1:2])
    d_in.check((ln, "data"))


# ---- 7. more rows than one grid slice -------------------------------------------------------------------


def test_row_slicing(torch, cess, lib, corc):
    """65,537 RS(2,1) segments of 16 bytes, every pointer a slice of one of three allocations."""
    k, m, ln, nseg = 2, 1, 16, 65535 + 2
    data, par = batch(corc, k, m, ln, nseg)
    enc = encoder(cess, k, m)
    d0 = Dev(torch, np.ascontiguousarray(data[:, 0]))
    d1 = Dev(torch, np.ascontiguousarray(data[:, 1]))
    d_par = Dev(torch, np.full(nseg * ln, 0x3C, np.uint8), guard=True)
    a = (c_void_p * (nseg * k))(*[d.ptr + s * ln for s in range(nseg) for d in (d0, d1)])
    p = (c_void_p * nseg)(*[d_par.ptr + s * ln for s in range(nseg)])
    assert lib.cec_encode_idx_ptrs(enc._h, a, p, nseg, ln, 0, None) == 0
    torch.cuda.synchronize()
    d_par.check("row slices", par)
    d0.check("row slices d0")
    d1.check("row slices d1")


# ---- 8. the batch calls' bytes --------------------------------------------------------------------------


@pytest.mark.parametrize("ln", [4096 + 16, 4096 + 16 + 3])
def test_equals_the_batch_calls(torch, cess, lib, corc, ln):
    """Pointers aimed into a batch layout: the same bytes as cec_encode_idx_batch and
    cec_update_batch give."""
    import ctypes
    k, m, nseg = 10, 4, 3
    data, _ = batch(corc, k, m, ln, nseg)
    enc = encoder(cess, k, m)
    start = garbage(ln + 1, nseg * m * ln)
    d_data = Dev(torch, data)
    new = data.copy()
    changed = [1, 4, 5, 9]
    new[:, changed] = garbage(ln + 2, (nseg, len(changed), ln))
    d_new = Dev(torch, new)
    by_batch, by_ptrs = Dev(torch, start, guard=True), Dev(torch, start, guard=True)
    p = (c_void_p * (nseg * m))(*[by_ptrs.ptr + i * ln for i in range(nseg * m)])
    for j in (3, 0, 9):
        assert lib.cec_encode_idx_batch(enc._h, d_data.ptr + j * ln, k * ln, j, by_batch.ptr, nseg,
                                        ln, 1, None) == 0
        a = (c_void_p * (nseg * k))()
        for s in range(nseg):
            a[s * k + j] = d_data.ptr + (s * k + j) * ln
        assert lib.cec_encode_idx_ptrs(enc._h, a, p, nseg, ln, 1, None) == 0
    torch.cuda.synchronize()
    want = by_batch.dev.cpu().numpy()[by_batch.lo:by_batch.lo + by_batch.n].copy()
    by_ptrs.check((ln, "encode_idx"), want)
    flags = (ctypes.c_uint8 * k)(*[1 if j in changed else 0 for j in range(k)])
    assert lib.cec_update_batch(enc._h, d_data.ptr, d_new.ptr, by_batch.ptr, nseg, ln, flags,
                                None) == 0
    a, b = (c_void_p * (nseg * k))(), (c_void_p * (nseg * k))()
    for s in range(nseg):
        for j in changed:
            a[s * k + j] = d_data.ptr + (s * k + j) * ln
            b[s * k + j] = d_new.ptr + (s * k + j) * ln
    assert lib.cec_update_ptrs(enc._h, a, b, p, nseg, ln, None) == 0
    torch.cuda.synchronize()
    want = by_batch.dev.cpu().numpy()[by_batch.lo:by_batch.lo + by_batch.n].copy()
    by_ptrs.check((ln, "update"), want)
    d_data.check((ln, "data"))
    d_new.check((ln, "new"))


# ---- 9. validation --------------------------------------------------------------------------------------


def test_refusals_write_nothing(torch, cess, lib, corc):
    from cess_amd import _lib
    k, m, ln, nseg = 2, 1, 1024, 2
    data, _ = batch(corc, k, m, ln, nseg)
    enc = encoder(cess, k, m)
    d_in, d_new = Inputs(torch, data), Inputs(torch, data ^ 0x33)
    d_par = Parity(torch, garbage(9, (nseg, m, ln)))
    ins, news, par = d_in.t, d_new.t, d_par.t

    def refused(rc, what, code=_lib.CEC_EINVAL):
        assert rc == code, what
        torch.cuda.synchronize()
        d_par.check(what)
        d_in.check(what)
        d_new.check(what)

    twice = [par[0], par[0]]
    refused(encode_idx(lib, enc, ins, twice, ln), "a parity address twice")
    refused(encode_idx(lib, enc, ins, twice, ln, 0), "a parity address twice, overwriting")
    refused(update(lib, enc, ins, news, twice, ln), "a parity address twice, update")
    refused(encode_idx(lib, enc, [ins[0], [par[0][0], None]], par, ln), "a parity is an input")
    refused(encode_idx(lib, enc, [[par[1][0], None], ins[1]], par, ln, 0),
            "a parity is another segment's input")
    refused(update(lib, enc, ins, [news[0], [par[0][0], news[1][1]]], par, ln),
            "a parity is a new shard")
    refused(update(lib, enc, ins, [news[0], [news[1][0], None]], par, ln), "old without new")
    refused(update(lib, enc, [[None, ins[0][1]], ins[1]], news, par, ln), "new without old")
    refused(encode_idx(lib, enc, ins, par, 0), "shard_len == 0", _lib.CEC_ESHARDLEN)
    refused(update(lib, enc, ins, news, par, 0), "shard_len == 0, update", _lib.CEC_ESHARDLEN)
    h = enc._h
    refused(lib.cec_encode_idx_ptrs(h, None, table(par), nseg, ln, 1, None), "NULL data")
    refused(lib.cec_encode_idx_ptrs(h, table(ins), None, nseg, ln, 1, None), "NULL parity")
    refused(lib.cec_update_ptrs(h, None, table(news), table(par), nseg, ln, None), "NULL old")
    refused(lib.cec_update_ptrs(h, table(ins), None, table(par), nseg, ln, None), "NULL new")
    refused(lib.cec_update_ptrs(h, table(ins), table(news), None, nseg, ln, None), "NULL parity")
    refused(lib.cec_encode_idx_ptrs(h, table(ins), table(par), 0, ln, 1, None), "nseg == 0",
            _lib.CEC_OK)
    refused(lib.cec_update_ptrs(h, table(ins), table(news), table(par), 0, ln, None),
            "nseg == 0, update", _lib.CEC_OK)
    refused(lib.cec_encode_idx_ptrs(h, None, None, 0, ln, 1, None), "nseg == 0, no arrays",
            _lib.CEC_OK)
    # what is allowed: inputs that repeat within and across segments
    rep = [[ins[0][0], ins[0][0]], [ins[0][0], ins[1][1]]]
    assert encode_idx(lib, enc, rep, par, ln) == _lib.CEC_OK
    torch.cuda.synchronize()
    d_in.check("repeated inputs")


# ---- 10. stream and pool --------------------------------------------------------------------------------


def test_stream_and_pool(torch, cess, lib, corc):
    from cess_amd import _lib
    k, m, ln, nseg = 10, 4, 4096 + 16, 3
    data, par = batch(corc, k, m, ln, nseg)
    enc = cess.New(k, m)
    d_in = Inputs(torch, data)
    d_par = Parity(torch, garbage(5, (nseg, m, ln)))
    cached = enc.stat(_lib.CEC_STAT_DECODE_CACHED)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert encode_idx(lib, enc, d_in.t, d_par.t, ln, 0, side) == 0
    side.synchronize()
    d_par.check("side stream", par)
    # Update there and back again on the same stream: the parity returns
    d_new = Inputs(torch, data ^ 0x0F)
    torch.cuda.synchronize()
    assert update(lib, enc, d_in.t, d_new.t, d_par.t, ln, side) == 0
    assert update(lib, enc, d_new.t, d_in.t, d_par.t, ln, side) == 0
    side.synchronize()
    d_par.check("side stream, update and back", par)

    def once():  # (synchronised: a table block retired by one call is free for the next)
        assert encode_idx(lib, enc, d_in.t, d_par.t, ln, 0) == 0
        torch.cuda.synchronize()

    once()
    pool_bytes = enc.stat(_lib.CEC_STAT_POOL_BYTES)
    for _ in range(20):
        once()
    assert enc.stat(_lib.CEC_STAT_POOL_BYTES) == pool_bytes
    assert enc.stat(_lib.CEC_STAT_DECODE_CACHED) == cached
    d_par.check("repeated", par)
    d_in.check("data")


# ---- 11. the Python methods -----------------------------------------------------------------------------


def test_python_encode_idx_device(torch, cess, corc, orc):
    d_in, d_par, fed, par, want = mixed_case(torch, corc, orc)
    enc = encoder(cess, 4, 2)
    enc.EncodeIdxDeviceBatch(fed, par)
    torch.cuda.synchronize()
    d_par.check("EncodeIdxDeviceBatch", want)
    # the same again one segment and one shard at a time: an XOR twice restores the start
    for row, prow in zip(fed, par):
        for j, t in enumerate(row):
            if t is not None:
                enc.EncodeIdxDevice(t, j, prow, stream=torch.cuda.current_stream())
    enc.EncodeIdxDeviceBatch([None] * 5, par)  # nothing fed
    torch.cuda.synchronize()
    start = np.stack([np.stack([d.host[d.lo:d.lo + d.n] for d in row]) for row in d_par.d])
    d_par.check("EncodeIdxDevice", start)
    # overwrite mode: what is fed replaces the parity, a segment that feeds nothing is zeroed
    enc.EncodeIdxDeviceBatch(fed, par, accumulate=False)
    torch.cuda.synchronize()
    over = want ^ start
    for s, prow in enumerate(par):
        for o, t in enumerate(prow):
            if t is None:
                over[s, o] = start[s, o]
    d_par.check("EncodeIdxDeviceBatch, overwrite", over)
    d_in.check("data")


def test_python_update_device(torch, cess, corc, monkeypatch):
    k, m = 4, 2
    d_old, d_new, d_par, old, new, want = update_case(torch, corc, k, m)
    enc = encoder(cess, k, m)
    enc.UpdateDeviceBatch(old, new, d_par.t)
    torch.cuda.synchronize()
    d_par.check("UpdateDeviceBatch", want)
    # back again one segment at a time, new -> old
    for s in range(3):
        enc.UpdateDevice(new[s] + d_par.t[s], old[s])
    torch.cuda.synchronize()
    d_par.check("UpdateDevice", batch(corc, k, m, want.shape[2], 3)[1])
    with pytest.raises(cess.ErrInvalidInput):
        enc.UpdateDevice([None] * k + d_par.t[0], new[1])
    # nothing changed: no C call (there is no library to call)
    monkeypatch.setattr(enc, "_lib", None)
    enc.UpdateDevice(d_old.t[0] + d_par.t[0], [None] * k)
    enc.UpdateDeviceBatch(old, [None] * 3, d_par.t)
    monkeypatch.undo()
    torch.cuda.synchronize()
    d_par.check("nothing changed", batch(corc, k, m, want.shape[2], 3)[1])
    d_old.check("old")
    d_new.check("new")
