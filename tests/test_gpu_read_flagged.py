"""cec_read_flagged_ptrs (Encoder.ReadFlaggedDevice, retrieve.read_segments_device): a verified
degraded read decided on the GPU from flags in device memory.

The buffers follow tests/test_gpu_repair_flagged.py (Case): truth from the C oracle; every held
shard and every destination a view into one allocation between bands of 0xA5; junk in the bad
shards and in the good shards past the first k; the flag tensor at an odd address; good flags 1 or
0xFF; random flag bytes at shards not held. The segments come from tests/read_flagged_cases.py.
After each call, bit-exact:
  - d_status equals cec_read_status of every segment, the bytes around d_status are intact;
  - the whole allocation equals its earlier image with the truth written at every wanted data
    shard of the CLEAN and REBUILT segments: nothing else changed, not the shards, not the guards,
    not the destinations nobody wants or those of LOST and MANY segments;
  - d_flags and the byte before it are unchanged;
  - the allocation equals a copy on which cec_reconstruct_ptrs (sources = the first k good shards)
    and plain copies produced the same shards."""
import hashlib
from ctypes import c_void_p

import numpy as np
import pytest

from tests import read_flagged_cases as rc
from tests.test_gpu_repair_flagged import CLEAN, GUARD, LOST, MANY, REBUILT, Case, truth

pytestmark = pytest.mark.gpu

MULTI_MAX = 4
EMPTY = 0x3C  # what a destination holds before the call


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
def encs(cess):
    made = {}

    def get(k, m, generic=False):
        from cess_amd import _lib
        if (k, m, generic) not in made:
            made[(k, m, generic)] = cess.New(k, m)
            if generic:
                made[(k, m, generic)].set_option(_lib.CEC_OPT_FORCE_GENERIC, 1)
        return made[(k, m, generic)]
    yield get
    for e in made.values():
        e.close()


class ReadCase(Case):
    """Case with destinations: behind the shards, in the same allocation, one slot per data shard
    of every segment (wanted or not), filled with EMPTY between the same guards and at the same
    offset from a 16-byte boundary as the shards."""

    def __init__(self, torch, k, m, full, case, off, seed, max_bad):
        held, bad, wanted = case
        super().__init__(torch, k, m, full, held, bad, off, seed)
        self.wanted = np.asarray(wanted, dtype=bool)
        self.max_bad = max_bad
        rng = np.random.default_rng(seed + 7919)
        self.good = self.held & (self.flags != 0)
        for s in range(self.nseg):  # junk in the good shards past the first k
            for i in np.nonzero(self.good[s])[0][k:]:
                o = self.hidx[s, i] * self.slot + self.lo
                self.image[o:o + self.ln] = rng.integers(0, 256, self.ln, dtype=np.uint8)
        self.src_bytes = self.image.size
        dimg = np.full((self.nseg * k, self.slot), 0xA5, dtype=np.uint8)
        dimg[:, self.lo:self.lo + self.ln] = EMPTY
        self.image = np.concatenate([self.image, dimg.ravel(), np.full(GUARD, 0xA5, np.uint8)])
        self.big = torch.from_numpy(self.image.copy()).cuda()
        self.want_status, self.want_miss = rc.read_statuses(k, m, self.held, None, self.wanted,
                                                            max_bad, flags=self.flags)

    def dst_off(self, s, j):
        return self.src_bytes + (s * self.k + j) * self.slot + self.lo

    def dst_addrs(self, base):
        d = np.zeros(self.wanted.shape, dtype=np.uint64)
        for s, j in zip(*np.nonzero(self.wanted)):
            d[s, j] = base + self.dst_off(s, j)
        return d

    def read(self):
        """The segments whose wanted shards arrive."""
        return np.nonzero((self.want_status == CLEAN) | (self.want_status == REBUILT))[0]

    def expected_image(self):
        img = self.image.copy()
        for s in self.read():
            for j in np.nonzero(self.wanted[s])[0]:
                o = self.dst_off(s, j)
                img[o:o + self.ln] = self.full[s, j]
        return img

    def call(self, enc, stream=None, d_flags=None, max_bad=None):
        from cess_amd import _lib
        a = self.addrs(self.big.data_ptr())
        d = self.dst_addrs(self.big.data_ptr())
        ptrs = (c_void_p * a.size)(*[int(x) for x in a.ravel()])
        dst = (c_void_p * d.size)(*[int(x) for x in d.ravel()])
        fl = self.d_flags if d_flags is None else d_flags
        return _lib.load().cec_read_flagged_ptrs(
            enc._h, ptrs, fl.data_ptr(), dst, self.nseg, self.ln,
            self.max_bad if max_bad is None else max_bad, self.d_status.data_ptr(),
            None if stream is None else stream.cuda_stream)

    def check_against_reconstruct(self, enc):
        """On a copy of the earlier image: cec_reconstruct_ptrs rebuilds the missing shards of the
        REBUILT segments into their destinations from exactly their first k good shards, and
        plain copies deliver the good wanted shards of the CLEAN and REBUILT ones."""
        from cess_amd import _lib
        torch = self.torch
        copy = torch.from_numpy(self.image.copy()).cuda()
        a, d = self.addrs(copy.data_ptr()), self.dst_addrs(copy.data_ptr())
        src, dst = np.zeros_like(a), np.zeros_like(a)
        rows = np.nonzero(self.want_status == REBUILT)[0]
        for s in rows:
            first = np.nonzero(self.good[s])[0][:self.k]
            src[s, first] = a[s, first]
            dst[s, self.want_miss[s]] = d[s, self.want_miss[s]]
        if rows.size:
            sp = (c_void_p * a.size)(*[int(x) for x in src.ravel()])
            dp = (c_void_p * a.size)(*[int(x) for x in dst.ravel()])
            assert _lib.load().cec_reconstruct_ptrs(enc._h, sp, dp, self.nseg, self.ln,
                                                    None) == 0
        for s in self.read():
            for j in np.nonzero(self.wanted[s] & self.good[s, :self.k])[0]:
                o, i = self.dst_off(s, j), self.hidx[s, j] * self.slot + self.lo
                copy[o:o + self.ln] = copy[i:i + self.ln]
        torch.cuda.synchronize()
        assert torch.equal(copy, self.big), "differs from cec_reconstruct_ptrs + copies on a copy"


def counts(c):
    """{(status, shards rebuilt): segments}"""
    out = {}
    for st, miss in zip(c.want_status, c.want_miss):
        out[(int(st), len(miss))] = out.get((int(st), len(miss)), 0) + 1
    return out


# ---- 1: RS(2,1), all 27 shard states x 4 wanted masks in one call -------------------------------

@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("ln", [1, 15, 16, 17, 4096, 4096 + 16 + 3, 3 * 4096 + 5, 65536])
def test_rs21_all_states(torch, cess, corc, encs, ln, off, generic):
    case = rc.rs21_all()
    c = ReadCase(torch, 2, 1, truth(corc, 2, 1, ln, 108), case, off, seed=ln * 2 + off, max_bad=1)
    assert set(counts(c)) == {(CLEAN, 0), (REBUILT, 1), (LOST, 0)}
    assert (c.flags[c.good] == 0xFF).any() and (c.flags[c.good] == 1).any()
    enc = encs(2, 1, generic)
    assert c.call(enc) == 0
    c.check(enc)


def test_rs21_bound_does_not_matter(torch, cess, corc, encs):
    """RS(2,1) can rebuild one shard: max_bad 4 gives max_bad 1's statuses and bytes."""
    case = rc.rs21_all()
    c = ReadCase(torch, 2, 1, truth(corc, 2, 1, 17, 108), case, 0, seed=21, max_bad=MULTI_MAX)
    assert set(counts(c)) == {(CLEAN, 0), (REBUILT, 1), (LOST, 0)}
    assert c.call(encs(2, 1)) == 0
    c.check(encs(2, 1))


# ---- 2: RS(4,2), all 3^6 states ------------------------------------------------------------------

@pytest.mark.parametrize("random_wanted", [False, True])
@pytest.mark.parametrize("max_bad", [1, 2])
def test_rs42_all_states(torch, cess, corc, encs, max_bad, random_wanted):
    ln = 4096 + 19
    case = rc.rs42_all(random_wanted)
    c = ReadCase(torch, 4, 2, truth(corc, 4, 2, ln, 729), case, 0, seed=42 + max_bad,
                 max_bad=max_bad)
    want = {(CLEAN, 0), (REBUILT, 1), (LOST, 0)} | ({(REBUILT, 2)} if max_bad == 2 else {(MANY, 0)})
    assert set(counts(c)) == want
    assert c.call(encs(4, 2)) == 0
    c.check(encs(4, 2))


# ---- 3: RS(10,4), 64 random segments, buckets 1 to 4 in one call --------------------------------

@pytest.mark.parametrize("max_bad", [1, 2, 3, 4])
def test_rs104_random(torch, cess, corc, encs, max_bad):
    ln = 8192 + 5
    c = ReadCase(torch, 10, 4, truth(corc, 10, 4, ln, 64), rc.rs104_random(), 0,
                 seed=104 + max_bad, max_bad=max_bad)
    got = set(counts(c))
    assert {(CLEAN, 0), (LOST, 0)} | {(REBUILT, e) for e in range(1, max_bad + 1)} <= got
    assert ((MANY, 0) in got) == (max_bad < 4)
    assert c.call(encs(10, 4)) == 0
    c.check(encs(10, 4))


# ---- 4: RS(32,32) -------------------------------------------------------------------------------

@pytest.mark.parametrize("max_bad", [4, 2])
def test_rs3232(torch, cess, corc, encs, max_bad):
    c = ReadCase(torch, 32, 32, truth(corc, 32, 32, 4096, 16), rc.rs3232_rows(), 0,
                 seed=3232 + max_bad, max_bad=max_bad)
    if max_bad == 4:
        assert set(counts(c)) == {(CLEAN, 0), (LOST, 0), (MANY, 0)} | {(REBUILT, e)
                                                                       for e in (1, 2, 3, 4)}
        assert c.want_status[9] == MANY and c.want_miss[10] == [0, 13, 31]
    else:
        assert c.want_status[10] == MANY
    assert c.held[8].sum() == 32 and c.want_status[8] == REBUILT  # exactly k shards held
    assert c.call(encs(32, 32)) == 0
    c.check(encs(32, 32))


# ---- 5: RS(200,56), the planner's lanes stride past 64 ------------------------------------------

@pytest.mark.parametrize("max_bad", [4, 2])
def test_rs20056(torch, cess, corc, encs, max_bad):
    c = ReadCase(torch, 200, 56, truth(corc, 200, 56, 256, 4), rc.rs20056_rows(), 0,
                 seed=20056 + max_bad, max_bad=max_bad)
    assert list(c.want_status) == ([CLEAN, REBUILT, REBUILT, LOST] if max_bad == 4
                                   else [CLEAN, MANY, MANY, LOST])
    assert c.call(encs(200, 56)) == 0
    c.check(encs(200, 56))


# ---- 6: flags produced on the stream -------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(2, 1), (10, 4)])
def test_flags_produced_on_the_stream(torch, cess, corc, encs, k, m):
    """The flags in device memory say "all good" and are synchronised; on stream S a kernel then
    writes the real flags, behind other work, and the call follows on S with no synchronise
    between: it acts on the flags the kernel wrote."""
    case = rc.rs21_all() if k == 2 else rc.rs104_random()
    ln = 4096 + 19
    c = ReadCase(torch, k, m, truth(corc, k, m, ln, len(case[0])), case, 0, seed=6 + k,
                 max_bad=min(m, MULTI_MAX))
    assert (REBUILT, 1) in counts(c) and (LOST, 0) in counts(c)
    new = torch.from_numpy(c.flags.copy()).cuda()
    zero = torch.zeros_like(new)
    work = torch.ones(1 << 22, dtype=torch.float32, device="cuda")
    c.d_flags.fill_(1)
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        for _ in range(8):
            work.mul_(1.0001)
        torch.bitwise_or(new, zero, out=c.d_flags)  # a kernel on S writes the flags
    assert c.call(encs(k, m), stream=S) == 0
    S.synchronize()
    c.check(encs(k, m))


# ---- 7: refusals with a live codec ----------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(2, 1), (4, 2)])
def test_refusals(torch, cess, corc, encs, k, m):
    from cess_amd import _lib
    lib = _lib.load()
    n, nseg, ln = k + m, 4, 64
    held = np.ones((nseg, n), dtype=bool)
    bad = np.zeros_like(held)
    bad[:, 0] = True
    c = ReadCase(torch, k, m, truth(corc, k, m, ln, nseg), (held, bad, np.ones((nseg, k), bool)),
                 0, seed=9, max_bad=1)
    enc = encs(k, m)
    a, d = c.addrs(c.big.data_ptr()), c.dst_addrs(c.big.data_ptr())

    def arr(x):
        return (c_void_p * x.size)(*[int(v) for v in x.ravel()])
    twice = d.copy()
    twice[3, k - 1] = twice[0, 1]      # the same destination in two segments
    inplace = d.copy()
    inplace[2, 0] = a[1, n - 1]        # a destination that is a shard of another segment
    own = d.copy()
    own[0, 0] = a[0, 0]                # ... and the segment's own bad shard: the repair's job
    ptrs, dst = arr(a), arr(d)
    fl, st = c.d_flags.data_ptr(), c.d_status.data_ptr()
    fn = lib.cec_read_flagged_ptrs
    assert fn(None, ptrs, fl, dst, nseg, ln, 1, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, None, fl, dst, nseg, ln, 1, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, None, dst, nseg, ln, 1, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, fl, None, nseg, ln, 1, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, fl, dst, nseg, ln, 1, None, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, fl, arr(twice), nseg, ln, 1, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, fl, arr(inplace), nseg, ln, 1, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, fl, arr(own), nseg, ln, 1, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, fl, dst, nseg, ln, 0, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, fl, dst, nseg, ln, 5, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, fl, dst, 0, ln, 5, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, fl, dst, nseg, 0, 1, st, None) == _lib.CEC_ESHARDLEN
    assert fn(enc._h, ptrs, fl, dst, 0, ln, 1, st, None) == _lib.CEC_OK
    assert fn(enc._h, None, None, None, 0, ln, 1, None, None) == _lib.CEC_OK
    torch.cuda.synchronize()
    assert (c.status_back.cpu().numpy() == 0xEE).all()   # d_status keeps every byte
    assert np.array_equal(c.big.cpu().numpy(), c.image)  # and no byte was written anywhere
    assert fn(enc._h, ptrs, fl, dst, nseg, ln, 1, st, None) == _lib.CEC_OK  # the arrays were fine
    c.check(enc)
    assert (c.want_status == REBUILT).all()


# ---- 8: the pool does not grow, the decode cache is not used ---------------------------------------

@pytest.mark.parametrize("k,m", [(2, 1), (10, 4)])
def test_pool_bytes_do_not_grow(torch, cess, corc, k, m):
    from cess_amd import _lib
    case = rc.rs21_all() if k == 2 else rc.rs104_random()
    ln = 256
    with cess.New(k, m) as enc:
        c = ReadCase(torch, k, m, truth(corc, k, m, ln, len(case[0])), case, 0, seed=10,
                     max_bad=min(m, MULTI_MAX))
        cached = enc.stat(_lib.CEC_STAT_DECODE_CACHED)
        seen = []
        for _ in range(10):
            assert c.call(enc) == 0
            torch.cuda.synchronize()
            seen.append(enc.stat(_lib.CEC_STAT_POOL_BYTES))
            assert enc.stat(_lib.CEC_STAT_DECODE_CACHED) == cached
        assert seen[1] == seen[9] and seen[1] > 0, seen
        c.check(enc, reference=False)  # the reference fills the decode cache
        assert enc.stat(_lib.CEC_STAT_DECODE_CACHED) == cached


# ---- 9: the Python forms ----------------------------------------------------------------------------

def test_python_forms(torch, cess, corc, encs):
    """Encoder.ReadFlaggedDevice with a joined tensor and a wanted mask, and with a list."""
    k, m, ln = 4, 2, 1000
    case = rc.rs42_all(True)
    pick = np.sort(np.random.default_rng(5).choice(729, 81, replace=False))
    case = tuple(x[pick] for x in case)
    nseg = len(pick)
    c = ReadCase(torch, k, m, truth(corc, k, m, ln, nseg), case, 0, seed=11, max_bad=2)
    assert {(CLEAN, 0), (REBUILT, 1), (LOST, 0)} <= set(counts(c))
    enc = encs(k, m)
    out = torch.full((nseg, k * ln), EMPTY, dtype=torch.uint8, device="cuda")
    st = enc.ReadFlaggedDevice(c.tensors(), c.d_flags, out, max_bad=2, wanted=c.wanted.tolist())
    outs = [torch.full((ln,), EMPTY, dtype=torch.uint8, device="cuda") if w else None
            for w in c.wanted.ravel()]
    st2 = enc.ReadFlaggedDevice(c.tensors(), c.d_flags, outs, max_bad=2)
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), c.want_status)
    assert np.array_equal(st2.cpu().numpy(), c.want_status)
    want = np.full((nseg, k, ln), EMPTY, dtype=np.uint8)
    for s in c.read():
        want[s, c.wanted[s]] = c.full[s, :k][c.wanted[s]]
    assert np.array_equal(out.cpu().numpy().reshape(nseg, k, ln), want)
    for i, t in enumerate(outs):
        if t is not None:
            assert np.array_equal(t.cpu().numpy(), want[i // k, i % k])
    assert np.array_equal(c.big.cpu().numpy(), c.image)  # the shards were only read
    with pytest.raises(cess.ErrInvalidInput):
        enc.ReadFlaggedDevice(c.tensors(), c.d_flags, out, max_bad=5)
    with pytest.raises(cess.ErrInvalidInput):  # a destination that is a shard of the call
        shard = next(t for seg in c.tensors() for t in seg if t is not None)
        enc.ReadFlaggedDevice(c.tensors(), c.d_flags, [shard] + [None] * (nseg * k - 1))


def test_read_segments_device(torch, cess, corc):
    """retrieve.read_segments_device on RS(2,1), F = 64 KiB, 8 segments: clean, each single
    fragment corrupted, one absent, two bad (LOST), and a wrong recorded segment hash."""
    from cess_amd import retrieve
    k, m, n, F, nseg = 2, 1, 3, 65536, 8
    full = truth(corc, k, m, F, nseg)

    def hexof(b):
        return hashlib.sha256(bytes(b)).hexdigest().encode()
    recorded = [[hexof(full[s, i]) for i in range(n)] for s in range(nseg)]
    seg_recorded = [hexof(full[s, :k].tobytes()) for s in range(nseg)]
    seg_recorded[6] = hexof(b"another segment")   # the record of segment 6 is wrong
    rng = np.random.default_rng(99)
    held = [[torch.from_numpy(full[s, i].copy()).cuda() for i in range(n)] for s in range(nseg)]
    for s, i in [(1, 0), (2, 1), (3, 2), (5, 0), (5, 2)]:   # corrupted: one byte differs
        held[s][i][int(rng.integers(0, F))] ^= 0x40
    held[4][1] = None                                       # absent
    recorded[4][1] = b"0" * 64
    before = [[None if t is None else t.clone() for t in seg] for seg in held]
    torch.cuda.synchronize()  # the fragments are final before another stream reads them
    S = torch.cuda.Stream()
    with cess.New(k, m) as enc, cess.HashQueue(capacity=32, stream=S) as q:
        with torch.cuda.stream(S):
            out = torch.full((nseg, k * F), EMPTY, dtype=torch.uint8, device="cuda")
            d_hex = torch.zeros((nseg, 64), dtype=torch.uint8, device="cuda")
        S.synchronize()
        got, d_flags, d_status, d_seg_ok = retrieve.read_segments_device(
            enc, held, recorded, seg_recorded=seg_recorded, out=out, max_bad=1, queue=q)
        assert got is out
        # the hex the queue computes over the rows of `out`, once more with the hex kept
        exp = torch.from_numpy(np.frombuffer(b"".join(seg_recorded), np.uint8).copy()).cuda()
        ok2 = torch.zeros(nseg, dtype=torch.uint8, device="cuda")
        q.add_check(out, nseg, 1, k * F, 0, k * F, exp, 1, ok2, 1, d_hex=d_hex, hex_outer=1)
        q.finish()
        S.synchronize()
    status = d_status.cpu().numpy()
    assert list(status) == [CLEAN, REBUILT, REBUILT, CLEAN, REBUILT, LOST, CLEAN, CLEAN]
    flags = d_flags.cpu().numpy()
    want_flags = np.ones((nseg, n), bool)
    for s, i in [(1, 0), (2, 1), (3, 2), (5, 0), (5, 2)]:
        want_flags[s, i] = False
    keep = np.ones((nseg, n), bool)
    keep[4, 1] = False  # no chain, the byte is whatever the buffer held
    assert np.array_equal((flags != 0)[keep], want_flags[keep])
    rows = out.cpu().numpy()
    for s in range(nseg):
        if s == 5:
            assert (rows[s] == EMPTY).all()  # LOST: not a byte written
        else:
            assert np.array_equal(rows[s], full[s, :k].ravel()), s
    ok = d_seg_ok.cpu().numpy()
    assert list(ok) == [1, 1, 1, 1, 1, 0, 0, 1]
    assert np.array_equal(ok2.cpu().numpy(), ok)
    hexes = d_hex.cpu().numpy()
    for s in range(nseg):
        assert bytes(hexes[s]) == hashlib.sha256(rows[s].tobytes()).hexdigest().encode(), s
    for seg, old in zip(held, before):   # the fragments were only read
        for t, o in zip(seg, old):
            assert t is None or torch.equal(t, o)
