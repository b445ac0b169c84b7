"""cec_reconstruct_partial_ptrs and cec_xor_ptrs with their Python forms (ReconstructPartialDevice,
ReconstructPartialDeviceBatch, XorDevice): the partial-product exchange in place, on one GPU.

Buffer setup (that of test_gpu_verify_ptrs.py): every shard and every destination is its own
allocation, made in shuffled order, and sits between two 64-byte guard bands of 0xA5. Held shards
that are survivors hold the C oracle's codeword; held shards that are not survivors hold random
garbage, and present shards a part does not hold are passed as NULL, so any read outside the held
survivors breaks a result. Every allocation is snapshotted before a call and compared after it:
only the payload bytes of the wanted destinations may change. Every comparison is bit-exact."""
import ctypes
from ctypes import c_uint8, c_void_p

import numpy as np
import pytest

from oracle.c_oracle import c_encode

pytestmark = pytest.mark.gpu

GUARD = 64
_CODEWORDS = {}
_EXPECT = {}
_MUL = []


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


def codewords(corc, k, m, ln, nseg):
    """nseg oracle codewords [nseg][n][ln], computed once per shape and never written."""
    key = (k, m, ln, nseg)
    if key not in _CODEWORDS:
        rng = np.random.default_rng(k * 1000003 + m * 1009 + ln + nseg)
        data = rng.integers(0, 256, (nseg, k, ln), dtype=np.uint8)
        par = np.stack([np.stack(c_encode(corc, k, m, list(data[s]))) for s in range(nseg)])
        _CODEWORDS[key] = np.concatenate([data, par], axis=1)
    return _CODEWORDS[key]


def erasures(k, m, nseg, rng, lose=None):
    n = k + m
    present = np.ones((nseg, n), np.uint8)
    for s in range(nseg):
        cnt = lose if lose else int(rng.integers(1, m + 1))
        present[s, rng.choice(n, size=cnt, replace=False)] = 0
    return present


def survivors(k, m, present_row):
    from cess_amd import _lib
    flags = np.ascontiguousarray(present_row, dtype=np.uint8)
    out = np.zeros(k, dtype=np.uint8)
    assert _lib.load().cec_survivors(k, m, flags.ctypes.data, out.ctypes.data) == 0
    return [int(i) for i in out]


def mul_table():
    """The Python oracle's gal_mul as a [256][256] table."""
    if not _MUL:
        from oracle.rs_oracle import gal_mul
        _MUL.append(np.array([[gal_mul(a, b) for b in range(256)] for a in range(256)],
                             dtype=np.uint8))
    return _MUL[0]


def cpu_partial(cess, k, m, full_s, present_row, held):
    """{lost shard: XOR over the survivors j in `held` of D[i][j] * shard_j}: the rows from
    cess_amd.decode_rows, the products by the Python oracle's table."""
    mul = mul_table()
    surv = survivors(k, m, present_row)
    idx, rows = cess.decode_rows(k, m, present_row, 1 - np.asarray(present_row, dtype=np.uint8))
    out = {}
    for o, f in enumerate(idx):
        acc = np.zeros(full_s.shape[1], dtype=np.uint8)
        for j, sv in enumerate(surv):
            if sv in held:
                acc ^= mul[rows[o][j]][full_s[sv]]
        out[int(f)] = acc
    return out


class Pool:
    """Guarded device allocations (see the module docstring) with a snapshot check."""

    def __init__(self, torch):
        self.torch = torch
        self.allocs, self.where = [], {}

    def add_many(self, specs, rng):
        """specs: [(key, payload, view offset)] -> {key: view}, allocated in shuffled order."""
        views = {}
        for j in rng.permutation(len(specs)):
            key, payload, off = specs[int(j)]
            lo, ln = GUARD + off, len(payload)
            host = np.full(lo + ln + GUARD, 0xA5, dtype=np.uint8)
            host[lo:lo + ln] = payload
            a = self.torch.from_numpy(host).cuda()
            v = a[lo:lo + ln]
            self.where[v.data_ptr()] = (len(self.allocs), lo)
            self.allocs.append(a)
            views[key] = v
        return views

    def snapshot(self):
        return self.torch.cat(self.allocs)

    def assert_only(self, before, writable, what=""):
        """Nothing but the payload bytes of the `writable` views differs from `before`."""
        after = self.torch.cat(self.allocs)
        offs = np.concatenate([[0], np.cumsum([a.numel() for a in self.allocs])])
        for v in writable:
            i, lo = self.where[v.data_ptr()]
            o = int(offs[i]) + lo
            before[o:o + v.numel()] = after[o:o + v.numel()]
        assert self.torch.equal(before, after), ("a byte outside the wanted outputs changed", what)


def partial_ptrs(torch, enc, pool, srcs, dsts, present, ln, acc, scribble=False):
    """cec_reconstruct_partial_ptrs over per-segment lists of n tensors or None -> return code.
    On success only the wanted destinations may have changed, on an error nothing."""
    from cess_amd import _lib
    nseg, n = len(srcs), enc.Shards
    flat = lambda rows: [None if t is None else t.data_ptr() for r in rows for t in r]  # noqa
    a = (c_void_p * max(1, nseg * n))(*flat(srcs))
    b = (c_void_p * max(1, nseg * n))(*flat(dsts))
    p = (c_uint8 * max(1, nseg * n))(*[int(x) for row in present for x in row])
    before = pool.snapshot()
    rc = _lib.load().cec_reconstruct_partial_ptrs(enc._h, a, b, p, nseg, ln, acc, None)
    if scribble:  # the arrays belong to the caller again
        for arr in (a, b, p):
            ctypes.memset(arr, 0xFF, ctypes.sizeof(arr))
    torch.cuda.synchronize()
    writable = [] if rc else [dsts[s][i] for s in range(nseg) for i in range(n)
                              if dsts[s][i] is not None and not present[s][i]]
    pool.assert_only(before, writable, rc)
    return rc


class World:
    """nseg segments spread over P parts: fragment f of segment s is held by part (s + f) mod P.
    src[r][s] is part r's list of n views or None, dst[r][s] its list of destinations (one per
    lost shard, pre-filled with the random R[r][s][f]). `shared_dst`: every part writes part 0's
    destinations. `off` shifts every view, `one_dst_off` only the first destination of part 0."""

    def __init__(self, torch, rng, k, m, full, present, P, off=0, one_dst_off=0,
                 shared_dst=False):
        nseg, n, ln = full.shape
        self.k, self.m, self.ln, self.P, self.nseg = k, m, ln, P, nseg
        self.full, self.present = full, present
        # (a segment below k present has no survivors: nothing of it can be wanted)
        self.surv = [survivors(k, m, present[s]) if present[s].sum() >= k else []
                     for s in range(nseg)]
        self.lost = [[f for f in range(n) if not present[s, f]] for s in range(nseg)]
        self.held = [[[f for f in range(n) if present[s, f] and (s + f) % P == r]
                      for s in range(nseg)] for r in range(P)]
        self.pool = Pool(torch)
        specs, self.R = [], {}
        first = True
        for r in range(P):
            for s in range(nseg):
                for f in self.held[r][s]:
                    body = full[s, f] if f in self.surv[s] else rng.integers(0, 256, ln,
                                                                             dtype=np.uint8)
                    specs.append((("src", r, s, f), body, off))
                if shared_dst and r:
                    continue
                for f in self.lost[s]:
                    self.R[r, s, f] = rng.integers(0, 256, ln, dtype=np.uint8)
                    specs.append((("dst", r, s, f), self.R[r, s, f],
                                  off + (one_dst_off if first else 0)))
                    first = False
        v = self.pool.add_many(specs, rng)
        self.src = [[[v.get(("src", r, s, f)) for f in range(n)] for s in range(nseg)]
                    for r in range(P)]
        self.dst = [[[v.get(("dst", 0 if shared_dst else r, s, f)) for f in range(n)]
                     for s in range(nseg)] for r in range(P)]

    def refill(self):
        for (r, s, f), body in self.R.items():
            self.dst[r][s][f].copy_(self.pool.torch.from_numpy(body))

    def expect(self, cess, r, s):
        return cpu_partial(cess, self.k, self.m, self.full[s], self.present[s],
                           set(self.held[r][s]))


def world_for(torch, cess, corc, k, m, ln, nseg, P, **kw):
    rng = np.random.default_rng(k * 7919 + m * 101 + ln * 31 + P)
    full = codewords(corc, k, m, ln, nseg)
    present = erasures(k, m, nseg, rng, lose=36 if (k, m) == (4, 40) else None)
    return World(torch, rng, k, m, full, present, P, **kw)


def expected_parts(cess, w, key):
    """[r][s] -> {lost shard: bytes}, computed once per shape (the worlds of one shape have the
    same pattern and placement whatever the kernels' mode)."""
    if key not in _EXPECT:
        _EXPECT[key] = [[w.expect(cess, r, s) for s in range(w.nseg)] for r in range(w.P)]
    return _EXPECT[key]


# ---- 1. partition identity, and each partial on its own -----------------------------------------

# the RS(4,40) case loses 36 shards: its outputs cross the 32-output program chunk
SHAPES = [(2, 1, 4096, 9, 2), (2, 1, 1, 3, 3), (4, 2, 1000, 7, 3), (10, 4, 4099, 6, 4),
          (32, 32, 4096, 5, 8), (32, 32, 65552, 3, 8), (4, 40, 272, 2, 3)]


@pytest.mark.parametrize("k,m,ln,nseg,P", SHAPES)
@pytest.mark.parametrize("rt_mode", [0, 1, 3])  # CEC_OPT_RT_MODE, as test_gpu_partial.py
def test_partials_and_their_xor(torch, cess, corc, k, m, ln, nseg, P, rt_mode):
    w = world_for(torch, cess, corc, k, m, ln, nseg, P)
    want = expected_parts(cess, w, (k, m, ln, nseg, P))
    enc = cess.New(k, m)
    enc.set_option(4, rt_mode)
    for r in range(P):
        assert partial_ptrs(torch, enc, w.pool, w.src[r], w.dst[r], w.present, ln, 0) == 0
        for s in range(nseg):
            for f in w.lost[s]:
                assert np.array_equal(w.dst[r][s][f].cpu().numpy(), want[r][s][f]), (r, s, f)
    # the XOR of the parts is the lost shard
    pairs = [(s, f) for s in range(nseg) for f in w.lost[s]]
    before = w.pool.snapshot()
    enc.XorDevice([w.dst[0][s][f] for s, f in pairs],
                  [[w.dst[r][s][f] for r in range(1, P)] for s, f in pairs])
    torch.cuda.synchronize()
    w.pool.assert_only(before, [w.dst[0][s][f] for s, f in pairs])
    for s, f in pairs:
        assert np.array_equal(w.dst[0][s][f].cpu().numpy(), w.full[s, f]), (s, f)


# ---- 2. accumulate -------------------------------------------------------------------------------


@pytest.mark.parametrize("k,m,ln,nseg,P", [(2, 1, 4099, 3, 2), (4, 2, 1000, 4, 3),
                                           (32, 32, 4096, 2, 8), (4, 40, 272, 1, 3)])
def test_accumulate(torch, cess, corc, k, m, ln, nseg, P):
    w = world_for(torch, cess, corc, k, m, ln, nseg, P, shared_dst=True)
    enc = cess.New(k, m)
    pairs = [(s, f) for s in range(nseg) for f in w.lost[s]]

    def got(s, f):
        return w.dst[0][s][f].cpu().numpy()

    # every part accumulates over the pre-fill R
    for r in range(P):
        assert partial_ptrs(torch, enc, w.pool, w.src[r], w.dst[r], w.present, ln, 1) == 0
    for s, f in pairs:
        assert np.array_equal(got(s, f), w.R[0, s, f] ^ w.full[s, f]), (s, f)
    # the first part stores over the same pre-fill, the others accumulate
    w.refill()
    for r in range(P):
        assert partial_ptrs(torch, enc, w.pool, w.src[r], w.dst[r], w.present, ln,
                            1 if r else 0) == 0
    for s, f in pairs:
        assert np.array_equal(got(s, f), w.full[s, f]), (s, f)
    # a part that holds no survivor: accumulate changes nothing, a store writes zeros
    none = [[None] * (k + m) for _ in range(nseg)]
    assert partial_ptrs(torch, enc, w.pool, none, w.dst[0], w.present, ln, 1) == 0
    for s, f in pairs:
        assert np.array_equal(got(s, f), w.full[s, f]), (s, f)
    assert partial_ptrs(torch, enc, w.pool, none, w.dst[0], w.present, ln, 0) == 0
    for s, f in pairs:
        assert not got(s, f).any(), (s, f)


# ---- 3. a subset of the outputs ------------------------------------------------------------------


def test_subset_of_outputs(torch, cess, corc):
    k, m, ln, nseg = 10, 4, 1000, 3
    n = k + m
    rng = np.random.default_rng(33)
    full = codewords(corc, k, m, ln, nseg)
    present = np.ones((nseg, n), np.uint8)
    present[0, [1, 7, 11]] = 0
    present[1, [0, 12, 13]] = 0
    present[2, [2, 3, 4, 5, 6]] = 0  # fewer than k present, and nothing wanted of it
    w = World(torch, rng, k, m, full, present, 1)
    dsts = [[None] * n for _ in range(nseg)]
    dsts[0][7] = w.dst[0][0][7]
    dsts[1][13] = w.dst[0][1][13]
    dsts[1][5] = w.dst[0][1][12]  # at a present shard: ignored
    enc = cess.New(k, m)
    assert partial_ptrs(torch, enc, w.pool, w.src[0], dsts, present, ln, 0) == 0
    assert np.array_equal(dsts[0][7].cpu().numpy(), full[0, 7])
    assert np.array_equal(dsts[1][13].cpu().numpy(), full[1, 13])
    # the Python form with `out`: only the named lost shard is an output
    out = {11: w.dst[0][0][11], 3: w.dst[0][0][1]}  # 3 is present: ignored
    before = w.pool.snapshot()
    got = enc.ReconstructPartialDevice(w.src[0][0], present[0], out=out)
    torch.cuda.synchronize()
    w.pool.assert_only(before, [out[11]])
    assert list(got) == [11] and got[11] is out[11]
    assert np.array_equal(out[11].cpu().numpy(), full[0, 11])
    # without `out` every lost shard is allocated
    got = enc.ReconstructPartialDevice(w.src[0][1], present[1])
    assert sorted(got) == [0, 12, 13]
    for f, t in got.items():
        assert np.array_equal(t.cpu().numpy(), full[1, f])
    with pytest.raises(cess.ErrInvalidInput):
        enc.ReconstructPartialDevice(w.src[0][0], present[0], accumulate=True)
    with pytest.raises(TypeError):  # a host tensor
        enc.ReconstructPartialDevice(w.src[0][0], present[0], out={11: out[11].cpu()})
    with pytest.raises(TypeError):  # a strided one
        wide = torch.zeros(2 * ln, dtype=torch.uint8, device="cuda")
        enc.ReconstructPartialDevice(w.src[0][0], present[0], out={11: wide[::2]})


# ---- 4. alignment --------------------------------------------------------------------------------


@pytest.mark.parametrize("ln", [15, 16, 17, 4096 + 16 + 3])
@pytest.mark.parametrize("k,m", [(4, 2), (32, 32)])
def test_alignment(torch, cess, corc, k, m, ln):
    nseg, P = 2, 2
    enc = cess.New(k, m)
    want = None
    # every view shifted by 0, 1 and 3 bytes, and one destination alone by 1
    for off, one in ((0, 0), (1, 0), (3, 0), (0, 1)):
        w = world_for(torch, cess, corc, k, m, ln, nseg, P, off=off, one_dst_off=one)
        want = want or expected_parts(cess, w, (k, m, ln, nseg, P))
        for acc in (0, 1):
            w.refill()
            for r in range(P):
                assert partial_ptrs(torch, enc, w.pool, w.src[r], w.dst[r], w.present, ln,
                                    acc) == 0
                for s in range(nseg):
                    for f in w.lost[s]:
                        exp = want[r][s][f] ^ w.R[r, s, f] if acc else want[r][s][f]
                        assert np.array_equal(w.dst[r][s][f].cpu().numpy(), exp), \
                            (off, one, acc, r, s, f)


# ---- 5. contract errors write nothing ------------------------------------------------------------


def test_contract_errors_write_nothing(torch, cess, corc):
    from cess_amd import _lib
    lib = _lib.load()
    k, m, ln, nseg = 4, 2, 1000, 3
    n = k + m
    rng = np.random.default_rng(55)
    full = codewords(corc, k, m, ln, nseg)
    present = np.ones((nseg, n), np.uint8)
    present[0, [1]] = 0
    present[1, [0, 5]] = 0
    present[2, [3]] = 0
    w = World(torch, rng, k, m, full, present, 1)
    src, dst = w.src[0], w.dst[0]
    enc = cess.New(k, m)

    def refused(srcs, dsts, flags, length, code, what):
        assert partial_ptrs(torch, enc, w.pool, srcs, dsts, flags, length, 0) == code, what
        assert partial_ptrs(torch, enc, w.pool, srcs, dsts, flags, length, 1) == code, what

    def edit(rows, s, i, t):
        rows = [list(r) for r in rows]
        rows[s][i] = t
        return rows

    # src non-NULL at a shard flagged absent
    refused(edit(src, 1, 5, src[1][4]), dst, present, ln, _lib.CEC_EINVAL, "held but absent")
    # a wanted dst that is a held survivor of its own segment
    refused(src, edit(dst, 1, 0, src[1][2]), present, ln, _lib.CEC_EINVAL, "dst is a survivor")
    # the same wanted dst twice, in two segments and in one
    refused(src, edit(dst, 2, 3, dst[0][1]), present, ln, _lib.CEC_EINVAL, "dst twice")
    refused(src, edit(dst, 1, 5, dst[1][0]), present, ln, _lib.CEC_EINVAL, "dst twice in one")
    # a wanted output and fewer than k shards flagged present
    few = present.copy()
    few[1, [1, 2]] = 0
    srcs = edit(edit(src, 1, 1, None), 1, 2, None)
    refused(srcs, dst, few, ln, _lib.CEC_ETOOFEW, "too few")
    # the same segment with nothing wanted is no error and nothing of it is written
    no_dst = [list(r) for r in dst]
    no_dst[1] = [None] * n
    assert partial_ptrs(torch, enc, w.pool, srcs, no_dst, few, ln, 0) == 0
    refused(src, dst, present, 0, _lib.CEC_ESHARDLEN, "shard_len 0")
    # NULL codec, NULL arrays, nseg == 0
    flat = lambda rows: [None if t is None else t.data_ptr() for r in rows for t in r]  # noqa
    a = (c_void_p * (nseg * n))(*flat(src))
    b = (c_void_p * (nseg * n))(*flat(dst))
    p = (c_uint8 * (nseg * n))(*[int(x) for x in present.reshape(-1)])
    before = w.pool.snapshot()
    for what, args, code in [("null codec", (None, a, b, p, nseg), _lib.CEC_EINVAL),
                             ("null src", (enc._h, None, b, p, nseg), _lib.CEC_EINVAL),
                             ("null dst", (enc._h, a, None, p, nseg), _lib.CEC_EINVAL),
                             ("null present", (enc._h, a, b, None, nseg), _lib.CEC_EINVAL),
                             ("nseg 0", (enc._h, a, b, p, 0), _lib.CEC_OK),
                             ("nseg 0, all null", (enc._h, None, None, None, 0), _lib.CEC_OK)]:
        for acc in (0, 1):
            assert lib.cec_reconstruct_partial_ptrs(*args, ln, acc, None) == code, what
    torch.cuda.synchronize()
    w.pool.assert_only(before, [])
    # and the arrays are fine: the call goes through, the arrays scribbled over before the
    # device has finished
    assert partial_ptrs(torch, enc, w.pool, src, dst, present, ln, 0, scribble=True) == 0
    for s in range(nseg):
        for f in w.lost[s]:
            assert np.array_equal(dst[s][f].cpu().numpy(), full[s, f]), (s, f)


# ---- 6. cache and pool ---------------------------------------------------------------------------


def test_cache_and_pool(torch, cess, corc):
    from cess_amd import _lib
    k, m, ln, nseg, P = 10, 4, 512, 4, 3
    n = k + m
    w = world_for(torch, cess, corc, k, m, ln, nseg, P)
    want = expected_parts(cess, w, (k, m, ln, nseg, P))
    enc = cess.New(k, m)
    # the batch form first, for part 1: same patterns, same held set, every lost shard
    held = np.zeros((nseg, n), np.uint8)
    for s in range(nseg):
        held[s, w.held[1][s]] = 1
    batch = np.zeros((nseg, n, ln), np.uint8)
    batch[held.astype(bool)] = w.full[held.astype(bool)]
    d_data = torch.from_numpy(batch[:, :k].copy()).cuda()
    d_par = torch.from_numpy(batch[:, k:].copy()).cuda()
    enc.ReconstructPartialBatch(d_data, d_par, nseg, ln, w.present, held)
    cached = enc.stat(_lib.CEC_STAT_DECODE_CACHED)
    assert partial_ptrs(torch, enc, w.pool, w.src[1], w.dst[1], w.present, ln, 0) == 0
    assert enc.stat(_lib.CEC_STAT_DECODE_CACHED) == cached, "the batch form's entries are shared"
    for s in range(nseg):
        for f in w.lost[s]:
            assert np.array_equal(w.dst[1][s][f].cpu().numpy(), want[1][s][f])
    # another part: new entries once, none the second time
    x_dst, x_src = [w.dst[0][0][w.lost[0][0]]], [[w.dst[1][0][w.lost[0][0]]]]

    def both():
        # (partial_ptrs synchronises: a table block retired by one call is free for the next. Calls
        # that are not waited for may hold several blocks at once, which is no leak either.)
        assert partial_ptrs(torch, enc, w.pool, w.src[2], w.dst[2], w.present, ln, 0) == 0
        enc.XorDevice(x_dst, x_src)
        torch.cuda.synchronize()

    both()
    cached = enc.stat(_lib.CEC_STAT_DECODE_CACHED)
    both()
    assert enc.stat(_lib.CEC_STAT_DECODE_CACHED) == cached
    pool_bytes = enc.stat(_lib.CEC_STAT_POOL_BYTES)
    for _ in range(20):
        both()
    assert enc.stat(_lib.CEC_STAT_POOL_BYTES) == pool_bytes
    assert enc.stat(_lib.CEC_STAT_DECODE_CACHED) == cached
    # the accumulate forms run the same programs
    assert partial_ptrs(torch, enc, w.pool, w.src[2], w.dst[2], w.present, ln, 1) == 0
    assert enc.stat(_lib.CEC_STAT_DECODE_CACHED) == cached


# ---- 7. rows past the grid-y limit ---------------------------------------------------------------


def test_rows_past_the_grid_limit(torch, cess, corc):
    """65,537 RS(2,1) segments of 16 bytes that share one codeword's tensors, one held survivor
    each; the destinations are distinct slices of one tensor, accumulated over a pre-fill."""
    from cess_amd import _lib
    k, m, ln, nseg = 2, 1, 16, 65537
    full = codewords(corc, k, m, ln, 1)[0]
    present = np.array([0, 1, 1], np.uint8)
    d1 = torch.from_numpy(full[1].copy()).cuda()
    rng = np.random.default_rng(77)
    fill = rng.integers(0, 256, (nseg + 2, ln), dtype=np.uint8)  # a guard slice at either end
    out = torch.from_numpy(fill).cuda()
    part = cpu_partial(cess, k, m, full, present, {1})[0]
    base = out.data_ptr() + ln
    src = [None, d1.data_ptr(), None] * nseg
    dst = [x for s in range(nseg) for x in (base + s * ln, None, None)]
    a, b = (c_void_p * len(src))(*src), (c_void_p * len(dst))(*dst)
    p = (c_uint8 * (3 * nseg))(*([0, 1, 1] * nseg))
    enc = cess.New(k, m)
    assert _lib.load().cec_reconstruct_partial_ptrs(enc._h, a, b, p, nseg, ln, 1, None) == 0
    torch.cuda.synchronize()
    want = fill.copy()
    want[1:-1] ^= part
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
    assert np.array_equal(d1.cpu().numpy(), full[1])


# ---- 8. cec_xor_ptrs -----------------------------------------------------------------------------


def xor_ptrs(torch, enc, pool, dsts, srcs, nsrc, ln):
    from cess_amd import _lib
    d = (c_void_p * max(1, len(dsts)))(*[None if t is None else t.data_ptr() for t in dsts])
    s = (c_void_p * max(1, len(dsts) * nsrc))(
        *[None if t is None else t.data_ptr() for row in srcs for t in row])
    before = pool.snapshot()
    rc = _lib.load().cec_xor_ptrs(enc._h, d, s, len(dsts), nsrc, ln, None)
    for arr in (d, s):
        ctypes.memset(arr, 0xFF, ctypes.sizeof(arr))
    torch.cuda.synchronize()
    writable = [] if rc else [t for t, row in zip(dsts, srcs)
                              if t is not None and any(x is not None for x in row)]
    pool.assert_only(before, writable, rc)
    return rc


@pytest.mark.parametrize("ln", [1, 15, 4096, (1 << 20) + 3])
@pytest.mark.parametrize("nsrc", [1, 2, 7])
def test_xor_ptrs(torch, cess, ln, nsrc):
    """Rows: every source; sources 0, 2, 4, ... NULL; a NULL dst; every source NULL; every
    source again. With `off` every view of the call is shifted (the byte-wise form)."""
    enc = cess.New(2, 1)
    rng = np.random.default_rng(ln * 13 + nsrc)
    nrows = 5
    for off in (0, 3):
        pool = Pool(torch)
        host = {(r, j): rng.integers(0, 256, ln, dtype=np.uint8)
                for r in range(nrows) for j in range(nsrc + 1)}
        v = pool.add_many([(key, body, off) for key, body in host.items()], rng)
        dsts = [v[r, 0] for r in range(nrows)]
        srcs = [[v[r, 1 + j] for j in range(nsrc)] for r in range(nrows)]
        srcs[1] = [None if j % 2 == 0 else t for j, t in enumerate(srcs[1])]
        dsts[2] = None
        srcs[3] = [None] * nsrc
        assert xor_ptrs(torch, enc, pool, dsts, srcs, nsrc, ln) == 0
        for r in range(nrows):
            want = host[r, 0].copy()
            if dsts[r] is not None:
                for j, t in enumerate(srcs[r]):
                    if t is not None:
                        want ^= host[r, 1 + j]
            assert np.array_equal(v[r, 0].cpu().numpy(), want), (off, r)
        # the Python form, rows of different lengths: applying the same sources again undoes it
        before = pool.snapshot()
        enc.XorDevice(dsts, [[t for t in row if t is not None] for row in srcs])
        torch.cuda.synchronize()
        pool.assert_only(before, [dsts[0], dsts[4]] + ([dsts[1]] if nsrc > 1 else []))
        for r in range(nrows):
            assert np.array_equal(v[r, 0].cpu().numpy(), host[r, 0]), (off, r)


def test_xor_ptrs_rows_past_the_grid_limit(torch, cess):
    from cess_amd import _lib
    nrows, ln = 65537, 16
    rng = np.random.default_rng(88)
    fill = rng.integers(0, 256, (nrows + 2, ln), dtype=np.uint8)
    parts = rng.integers(0, 256, (2, ln), dtype=np.uint8)
    out = torch.from_numpy(fill).cuda()
    srcs = torch.from_numpy(parts).cuda()
    base = out.data_ptr() + ln
    d = (c_void_p * nrows)(*[base + r * ln for r in range(nrows)])
    s = (c_void_p * (2 * nrows))(*([srcs[0].data_ptr(), srcs[1].data_ptr()] * nrows))
    enc = cess.New(2, 1)
    assert _lib.load().cec_xor_ptrs(enc._h, d, s, nrows, 2, ln, None) == 0
    torch.cuda.synchronize()
    want = fill.copy()
    want[1:-1] ^= parts[0] ^ parts[1]
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
    assert np.array_equal(srcs.cpu().numpy(), parts)


def test_xor_ptrs_validation_writes_nothing(torch, cess):
    from cess_amd import _lib
    lib = _lib.load()
    enc = cess.New(4, 2)
    rng = np.random.default_rng(99)
    ln, nrows, nsrc = 100, 3, 2
    pool = Pool(torch)
    v = pool.add_many([((r, j), rng.integers(0, 256, ln, dtype=np.uint8), 0)
                       for r in range(nrows) for j in range(nsrc + 1)], rng)
    dsts = [v[r, 0] for r in range(nrows)]
    srcs = [[v[r, 1], v[r, 2]] for r in range(nrows)]
    E = _lib.CEC_EINVAL
    assert xor_ptrs(torch, enc, pool, [dsts[0], dsts[1], dsts[0]], srcs, nsrc, ln) == E
    assert xor_ptrs(torch, enc, pool, dsts, [srcs[0], [v[1, 1], dsts[0]], srcs[2]], nsrc, ln) == E
    assert xor_ptrs(torch, enc, pool, dsts, [[dsts[0], None], srcs[1], srcs[2]], nsrc, ln) == E
    d = (c_void_p * nrows)(*[t.data_ptr() for t in dsts])
    s = (c_void_p * (nrows * nsrc))(*[t.data_ptr() for row in srcs for t in row])
    before = pool.snapshot()
    for what, args, code in [("null codec", (None, d, s, nrows, nsrc, ln), E),
                             ("null dst", (enc._h, None, s, nrows, nsrc, ln), E),
                             ("null src", (enc._h, d, None, nrows, nsrc, ln), E),
                             ("len 0", (enc._h, d, s, nrows, nsrc, 0), _lib.CEC_OK),
                             ("nsrc 0", (enc._h, d, s, nrows, 0, ln), _lib.CEC_OK),
                             ("nrows 0", (enc._h, d, s, 0, nsrc, ln), _lib.CEC_OK),
                             ("no work, null arrays", (enc._h, None, None, 0, 0, 0),
                              _lib.CEC_OK)]:
        assert lib.cec_xor_ptrs(*args, None) == code, what
    torch.cuda.synchronize()
    pool.assert_only(before, [])
    with pytest.raises(TypeError):
        enc.XorDevice([dsts[0]], [[srcs[0][0].cpu()]])
    with pytest.raises(cess.ErrShardSize):
        enc.XorDevice([dsts[0]], [[srcs[0][0][:-1]]])
    assert xor_ptrs(torch, enc, pool, dsts, srcs, nsrc, ln) == 0


# ---- 9. emulated ranks ---------------------------------------------------------------------------


def test_emulated_ranks(torch, cess, corc):
    """The partial exchange of the C protocol, in place on one GPU: RS(32,32) over 8 ranks."""
    from cess_amd.distributed import c_plan, fragment_owner
    k, m, ln, nseg, world = 32, 32, 4096, 12, 8
    n = k + m
    rng = np.random.default_rng(2026)
    full = codewords(corc, k, m, ln, nseg)
    lost = {s: sorted(int(f) for f in rng.choice(n, size=1 + s % 3, replace=False))
            for s in range(nseg)}
    present = np.ones((nseg, n), np.uint8)
    for s, fs in lost.items():
        present[s, fs] = 0
    moves, decoders = c_plan(lost, k, m, world, "partials")
    assert moves and all(kind == 1 for *_, kind in moves), "every move is a partial"
    pool = Pool(torch)
    frag = pool.add_many([((s, f), full[s, f], 0) for s in range(nseg) for f in range(n)
                          if present[s, f]], rng)
    wires = {(s, f, src): torch.full((ln,), 0x5A, dtype=torch.uint8, device="cuda")
             for s, f, src, _, _ in moves}
    outs = {(s, f): torch.full((ln,), 0x5A, dtype=torch.uint8, device="cuda")
            for s in lost for f in lost[s]}
    enc = cess.New(k, m)
    before = pool.snapshot()

    def placed(rank, s):
        return [frag[s, f] if present[s, f] and fragment_owner(s, f, world) == rank else None
                for f in range(n)]

    def run(rank, targets):
        """One partial call of `rank`: targets {seg: {frag: tensor}}."""
        segs = sorted(targets)
        enc.ReconstructPartialDeviceBatch([placed(rank, s) for s in segs],
                                          [present[s] for s in segs],
                                          [targets[s] for s in segs], accumulate=False)

    for rank in range(world):
        # the partials this rank sends, straight into the wire tensors
        send = {}
        for s, f, src, dst, _ in moves:
            assert dst == decoders[s, f] and src != dst
            if src == rank:
                send.setdefault(s, {})[f] = wires[s, f, src]
        if send:
            run(rank, send)
    for rank in range(world):
        # the decoder's own partial, straight into the caller's output tensors, then one XOR of
        # the received partials into them
        mine = {}
        for (s, f), dec in decoders.items():
            if dec == rank:
                mine.setdefault(s, {})[f] = outs[s, f]
        if not mine:
            continue
        run(rank, mine)
        pairs = [(s, f) for s in sorted(mine) for f in sorted(mine[s])]
        enc.XorDevice([outs[p] for p in pairs],
                      [[wires[s, f, src] for s2, f2, src, _, _ in moves if (s2, f2) == (s, f)]
                       for s, f in pairs])
    torch.cuda.synchronize()
    for (s, f), t in outs.items():
        assert np.array_equal(t.cpu().numpy(), full[s, f]), (s, f)
    pool.assert_only(before, [])
