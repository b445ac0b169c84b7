"""cec_repair_flagged_ptrs (Encoder.RepairFlaggedDevice): rebuilds decided on the GPU from flags in
device memory.

Truth is random data plus its parity from the C oracle (oracle/rs_oracle.c), never the code under
test. Every held shard is a view into one large allocation, between bands of 0xA5 (64 bytes and
the padding up to the next 16-byte boundary); a shard flagged bad holds random junk before the
call. The flag tensor starts at an odd address, a good flag is 1 or 0xFF, and the flag byte of a
shard that is not held is random (0 included). After each call:
  - d_status equals cec_flag_status of every segment, and the bytes around d_status are intact;
  - the whole allocation equals its image before the call with the rebuilt shards replaced by
    the truth: rebuilt shards are right and every other byte, guards included, is unchanged;
  - d_flags and the byte before it are unchanged;
  - the allocation equals a copy of the earlier image on which cec_reconstruct_ptrs rebuilt the
    same shards with the pattern read from the flags on the host.
Every comparison is bit-exact."""
import ctypes
from ctypes import c_void_p

import numpy as np
import pytest

from oracle.c_oracle import c_encode

pytestmark = pytest.mark.gpu

GUARD = 64
CLEAN, REBUILT, MANY, LOST = 0, 1, 2, 3
_TRUTH = {}


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
    """One codec per code for the module (their decode caches are shared by the cases)."""
    made = {}

    def get(k, m):
        if (k, m) not in made:
            made[(k, m)] = cess.New(k, m)
        return made[(k, m)]
    yield get
    for e in made.values():
        e.close()


def truth(corc, k, m, ln, nseg):
    """nseg oracle codewords [nseg][n][ln], computed once per shape and never written."""
    key = (k, m, ln, nseg)
    if key not in _TRUTH:
        rng = np.random.default_rng(k * 1000003 + m * 1009 + ln * 31 + nseg)
        data = rng.integers(0, 256, (k, nseg * ln), dtype=np.uint8)
        par = np.stack(c_encode(corc, k, m, list(data)))  # one call over every segment's bytes
        full = np.concatenate([data, par]).reshape(k + m, nseg, ln).transpose(1, 0, 2)
        _TRUTH[key] = np.ascontiguousarray(full)
        _TRUTH[key].setflags(write=False)
    return _TRUTH[key]


def statuses(k, m, held, flags):
    """cec_flag_status of every row -> (status [nseg], lost [nseg])."""
    from cess_amd import _lib
    lib = _lib.load()
    held = np.ascontiguousarray(held, dtype=np.uint8)
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    n = k + m
    st, lost = ctypes.c_int(), ctypes.c_int()
    u8p = ctypes.POINTER(ctypes.c_uint8)
    out = np.zeros((len(held), 2), np.int64)
    for s in range(len(held)):
        hp = ctypes.cast(c_void_p(held.ctypes.data + s * n), u8p)
        fp = ctypes.cast(c_void_p(flags.ctypes.data + s * n), u8p)
        assert lib.cec_flag_status(k, m, hp, fp, ctypes.byref(st), ctypes.byref(lost)) == 0
        out[s] = st.value, lost.value
    return out[:, 0], out[:, 1]


class Case:
    """One call's buffers: held [nseg][n] (0 / 1) and bad [nseg][n] (held shards whose flag is 0
    and whose bytes are junk) over the codewords `full`; every held shard at offset `off` from
    a 16-byte boundary of one allocation."""

    def __init__(self, torch, k, m, full, held, bad, off, seed):
        self.torch, self.k, self.m, self.n = torch, k, m, k + m
        self.full = full
        self.nseg, _, self.ln = full.shape
        self.held = np.asarray(held, dtype=bool)
        self.bad = np.asarray(bad, dtype=bool) & self.held
        rng = np.random.default_rng(seed)
        nheld = int(self.held.sum())
        self.slot = (GUARD + off + self.ln + 15) // 16 * 16
        self.lo = GUARD + off
        img = np.full((nheld, self.slot), 0xA5, dtype=np.uint8)
        payload = full[self.held]  # segment-major
        junk = self.bad[self.held]
        payload[junk] = rng.integers(0, 256, (int(junk.sum()), self.ln), dtype=np.uint8)
        img[:, self.lo:self.lo + self.ln] = payload
        self.image = np.concatenate([img.ravel(), np.full(GUARD, 0xA5, dtype=np.uint8)])
        self.hidx = np.full(self.held.shape, -1, dtype=np.int64)
        self.hidx[self.held] = np.arange(nheld)
        self.big = torch.from_numpy(self.image.copy()).cuda()
        # flags: good 1 or 0xFF, bad 0, not held anything; the tensor starts at an odd address
        fl = rng.choice(np.array([1, 0xFF], np.uint8), size=self.held.shape)
        fl[self.bad] = 0
        nh = ~self.held
        fl[nh] = rng.choice(np.array([0, 1, 0xFF, 7], np.uint8), size=int(nh.sum()))
        self.flags = fl
        self.flag_back = torch.from_numpy(
            np.concatenate([[0x5A], fl.ravel()]).astype(np.uint8)).cuda()
        self.d_flags = self.flag_back[1:].view(self.nseg, self.n)
        assert self.d_flags.data_ptr() % 2 == 1
        self.status_back = torch.full((self.nseg + 32,), 0xEE, dtype=torch.uint8, device="cuda")
        self.d_status = self.status_back[16:16 + self.nseg]
        self.want_status, self.want_lost = statuses(k, m, self.held, fl)

    def addrs(self, base):
        a = np.zeros(self.held.shape, dtype=np.uint64)
        a[self.held] = base + self.hidx[self.held].astype(np.uint64) * self.slot + self.lo
        return a

    def tensors(self):
        """Per segment the n shard views (None = not held), for the Python forms."""
        out = []
        for s in range(self.nseg):
            row = []
            for i in range(self.n):
                h = self.hidx[s, i]
                o = h * self.slot + self.lo
                row.append(None if h < 0 else self.big[o:o + self.ln])
            out.append(row)
        return out

    def expected_image(self):
        img = self.image.copy()
        for s in np.nonzero(self.want_status == REBUILT)[0]:
            j = self.want_lost[s]
            o = self.hidx[s, j] * self.slot + self.lo
            img[o:o + self.ln] = self.full[s, j]
        return img

    def call(self, enc, stream=None, d_flags=None):
        from cess_amd import _lib
        a = self.addrs(self.big.data_ptr())
        ptrs = (c_void_p * a.size)(*[int(x) for x in a.ravel()])
        fl = self.d_flags if d_flags is None else d_flags
        return _lib.load().cec_repair_flagged_ptrs(
            enc._h, ptrs, fl.data_ptr(), self.nseg, self.ln, self.d_status.data_ptr(),
            None if stream is None else stream.cuda_stream)

    def check(self, enc, reference=True):
        """Everything the module docstring lists, after a call that returned CEC_OK."""
        torch = self.torch
        torch.cuda.synchronize()
        sb = self.status_back.cpu().numpy()
        assert (sb[:16] == 0xEE).all() and (sb[16 + self.nseg:] == 0xEE).all()
        got = sb[16:16 + self.nseg]
        assert np.array_equal(got, self.want_status), np.nonzero(got != self.want_status)[0][:8]
        after = self.big.cpu().numpy()
        want = self.expected_image()
        diff = np.nonzero(after != want)[0]
        assert diff.size == 0, ("bytes differ from truth / a byte outside a rebuilt shard "
                                "changed", diff[:8], diff.size)
        fb = self.flag_back.cpu().numpy()
        assert fb[0] == 0x5A and np.array_equal(fb[1:], self.flags.ravel())
        if reference:
            self.check_against_reconstruct(enc)

    def check_against_reconstruct(self, enc):
        """cec_reconstruct_ptrs on a copy of the earlier image, the pattern read from the flags
        on the host: the rebuilt segments' bad shard is the destination, the other held shards
        the sources; segments that are not rebuilt name nothing."""
        from cess_amd import _lib
        torch = self.torch
        copy = torch.from_numpy(self.image.copy()).cuda()
        a = self.addrs(copy.data_ptr())
        src, dst = a.copy(), np.zeros_like(a)
        go = self.want_status == REBUILT
        src[~go] = 0
        rows = np.nonzero(go)[0]
        if rows.size:
            dst[rows, self.want_lost[rows]] = a[rows, self.want_lost[rows]]
            src[rows, self.want_lost[rows]] = 0
            sp = (c_void_p * a.size)(*[int(x) for x in src.ravel()])
            dp = (c_void_p * a.size)(*[int(x) for x in dst.ravel()])
            assert _lib.load().cec_reconstruct_ptrs(enc._h, sp, dp, self.nseg, self.ln,
                                                    None) == 0
        torch.cuda.synchronize()
        assert torch.equal(copy, self.big), "differs from cec_reconstruct_ptrs on a copy"


# ---- 1, 2: RS(2,1), compile-time rows and the general planner at its smallest n -----------------

def rs21_rows():
    """All 8 flag patterns with all three held, and every two-held set with its 4 patterns."""
    held, bad = [], []
    for h in [(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)]:
        idx = [i for i in range(3) if h[i]]
        for bits in range(1 << len(idx)):
            held.append(h)
            bad.append([int(i in idx and (bits >> idx.index(i)) & 1) for i in range(3)])
    return np.array(held), np.array(bad)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("ln", [1, 15, 16, 17, 4101, 4112])
def test_rs21_small(torch, cess, corc, encs, ln, off):
    held, bad = rs21_rows()
    assert len(held) == 20
    c = Case(torch, 2, 1, truth(corc, 2, 1, ln, len(held)), held, bad, off, seed=ln * 2 + off)
    assert set(c.want_status) == {CLEAN, REBUILT, LOST}
    assert (c.flags[c.held & ~c.bad] == 0xFF).any()  # 0xFF counts as good
    assert c.call(encs(2, 1)) == 0
    c.check(encs(2, 1))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("ln", [1, 17, 4101])
def test_rs21_force_generic(torch, cess, corc, ln, off):
    from cess_amd import _lib
    held, bad = rs21_rows()
    with cess.New(2, 1) as enc:
        enc.set_option(_lib.CEC_OPT_FORCE_GENERIC, 1)
        c = Case(torch, 2, 1, truth(corc, 2, 1, ln, len(held)), held, bad, off, seed=77 + ln + off)
        assert c.call(enc) == 0
        c.check(enc)


# ---- 3: wider codes ---------------------------------------------------------------------------

def wide_rows(k, m, rng):
    """One segment per bad index j (all held); then: clean; two bad (MANY); m not held and one bad
    (fewer than k good: LOST); one not held, nothing bad, its flag byte 0 (CLEAN); m - 1 not held
    and one bad (REBUILT from exactly k good)."""
    n = k + m
    held = np.ones((n + 5, n), dtype=bool)
    bad = np.zeros((n + 5, n), dtype=bool)
    bad[np.arange(n), np.arange(n)] = True
    bad[n + 1, rng.choice(n, size=2, replace=False)] = True
    gone = rng.choice(n, size=m + 1, replace=False)
    held[n + 2, gone[:m]] = False
    bad[n + 2, gone[m]] = True
    held[n + 3, gone[0]] = False
    held[n + 4, gone[:m - 1]] = False
    bad[n + 4, gone[m]] = True
    return held, bad, {"clean": n, "many": n + 1, "lost": n + 2, "ignored": n + 3,
                       "exactly_k": n + 4, "gone0": gone[0]}


@pytest.mark.parametrize("ln", [80, 4101])
@pytest.mark.parametrize("k,m", [(4, 2), (10, 4), (17, 3), (32, 32), (200, 56)])
def test_wider_codes(torch, cess, corc, encs, k, m, ln):
    rng = np.random.default_rng(k * 7 + m + ln)
    held, bad, at = wide_rows(k, m, rng)
    n = k + m
    c = Case(torch, k, m, truth(corc, k, m, ln, n + 5), held, bad, 0, seed=k + m + ln)
    c.flags[at["ignored"], at["gone0"]] = 0  # a shard that is not held: its flag is ignored
    c.flag_back[1 + at["ignored"] * n + at["gone0"]] = 0
    assert (c.want_status[:n] == REBUILT).all() and (c.want_lost[:n] == np.arange(n)).all()
    assert [c.want_status[at[x]] for x in ("clean", "many", "lost", "ignored", "exactly_k")] == \
        [CLEAN, MANY, LOST, CLEAN, REBUILT]
    assert c.call(encs(k, m)) == 0
    c.check(encs(k, m))


# ---- 4: several held sets in one call -----------------------------------------------------------

def test_several_held_sets(torch, cess, corc, encs):
    k, m, n, nseg, ln = 4, 2, 6, 40, 1000
    rng = np.random.default_rng(404)
    sets = [(1, 1, 1, 1, 1, 1), (0, 1, 1, 1, 1, 1), (1, 1, 1, 0, 1, 1), (1, 1, 1, 1, 1, 0),
            (1, 0, 1, 1, 0, 1)]
    which = rng.permutation(np.arange(nseg) % len(sets))
    held = np.array([sets[w] for w in which], dtype=bool)
    bad = np.zeros_like(held)
    for s in range(nseg):
        idx = np.nonzero(held[s])[0]
        bad[s, rng.choice(idx, size=int(rng.integers(0, 3)), replace=False)] = True
    c = Case(torch, k, m, truth(corc, k, m, ln, nseg), held, bad, 0, seed=4)
    assert set(c.want_status) == {CLEAN, REBUILT, MANY, LOST}
    assert c.call(encs(k, m)) == 0
    c.check(encs(k, m))


# ---- 5: decode cache of one entry ---------------------------------------------------------------

def test_cache_capacity_one(torch, cess, corc):
    from cess_amd import _lib
    k, m, n, ln = 4, 2, 6, 520
    with cess.New(k, m) as enc:
        enc.set_option(_lib.CEC_OPT_DECODE_CACHE, 1)
        held = np.ones((n, n), dtype=bool)
        c = Case(torch, k, m, truth(corc, k, m, ln, n), held, np.eye(n, dtype=bool), 0, seed=5)
        assert c.call(enc) == 0
        assert enc.stat(_lib.CEC_STAT_DECODE_CACHED) == 1
        c.check(enc)


# ---- 6: past one grid of rows -------------------------------------------------------------------

def test_65537_segments(torch, cess, corc, encs):
    """RS(2,1), 16-byte shards as views of three big tensors, bad shards only in segments 0,
    65,534, 65,535 and 65,536: the product launch is cut at 65,535 rows."""
    from cess_amd import _lib
    k, m, n, nseg, ln = 2, 1, 3, 65537, 16
    full = truth(corc, k, m, ln, nseg)
    badmap = {0: 0, 65534: 1, 65535: 2, 65536: 0}
    rng = np.random.default_rng(6)
    images = []
    for i in range(n):
        body = full[:, i, :].copy()
        for s, j in badmap.items():
            if j == i:
                body[s] = rng.integers(0, 256, ln, dtype=np.uint8)
        images.append(np.concatenate([np.full(GUARD, 0xA5, np.uint8), body.ravel(),
                                      np.full(GUARD, 0xA5, np.uint8)]))
    bigs = [torch.from_numpy(im.copy()).cuda() for im in images]
    flags = np.ones((nseg, n), np.uint8)
    for s, j in badmap.items():
        flags[s, j] = 0
    flag_back = torch.from_numpy(np.concatenate([[0x5A], flags.ravel()]).astype(np.uint8)).cuda()
    status_back = torch.full((nseg + 32,), 0xEE, dtype=torch.uint8, device="cuda")
    want, lost = statuses(k, m, np.ones((nseg, n), np.uint8), flags)
    assert (want == REBUILT).sum() == 4
    addr = np.stack([b.data_ptr() + GUARD + np.arange(nseg, dtype=np.uint64) * ln for b in bigs],
                    axis=1)
    ptrs = (c_void_p * addr.size)(*[int(x) for x in addr.ravel()])
    enc = encs(k, m)
    assert _lib.load().cec_repair_flagged_ptrs(enc._h, ptrs, flag_back.data_ptr() + 1, nseg, ln,
                                               status_back.data_ptr() + 16, None) == 0
    torch.cuda.synchronize()
    sb = status_back.cpu().numpy()
    assert (sb[:16] == 0xEE).all() and (sb[16 + nseg:] == 0xEE).all()
    assert np.array_equal(sb[16:16 + nseg], want)
    fb = flag_back.cpu().numpy()
    assert fb[0] == 0x5A and np.array_equal(fb[1:], flags.ravel())
    for i in range(n):  # healed: the three tensors hold the truth between their guards
        exp = np.concatenate([np.full(GUARD, 0xA5, np.uint8), full[:, i, :].ravel(),
                              np.full(GUARD, 0xA5, np.uint8)])
        assert np.array_equal(bigs[i].cpu().numpy(), exp), i
    # the same four rebuilds by cec_reconstruct_ptrs on copies
    copies = [torch.from_numpy(im.copy()).cuda() for im in images]
    segs = sorted(badmap)
    src = np.zeros((len(segs), n), np.uint64)
    dst = np.zeros((len(segs), n), np.uint64)
    for r, s in enumerate(segs):
        for i in range(n):
            a = copies[i].data_ptr() + GUARD + s * ln
            (dst if i == badmap[s] else src)[r, i] = a
    sp = (c_void_p * src.size)(*[int(x) for x in src.ravel()])
    dp = (c_void_p * dst.size)(*[int(x) for x in dst.ravel()])
    assert _lib.load().cec_reconstruct_ptrs(enc._h, sp, dp, len(segs), ln, None) == 0
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(copies[i], bigs[i]), i


# ---- 7: nothing to do ---------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(2, 1), (4, 2), (32, 32)])
def test_all_clean(torch, cess, corc, encs, k, m):
    """64 clean segments: the planner writes 64 idle rows (case 3, or all-zero rows) and the
    products leave every one of them alone."""
    nseg, ln = 64, 4101
    held = np.ones((nseg, k + m), dtype=bool)
    c = Case(torch, k, m, truth(corc, k, m, ln, nseg), held, np.zeros_like(held), 0, seed=7)
    assert (c.want_status == CLEAN).all()
    assert c.call(encs(k, m)) == 0
    c.check(encs(k, m), reference=False)
    assert np.array_equal(c.big.cpu().numpy(), c.image)


# ---- 8: stream order ----------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(2, 1), (4, 2)])
def test_flags_produced_on_the_stream(torch, cess, corc, encs, k, m):
    """The flags in device memory say "all good" and are synchronised; new flags are then copied
    in on stream S without waiting, and the call follows on S: it acts on the new flags."""
    n, nseg, ln = k + m, 24, 8192
    held = np.ones((nseg, n), dtype=bool)
    bad = np.zeros_like(held)
    even = np.arange(0, nseg, 2)
    bad[even, even % n] = True  # every other segment has one bad shard
    c = Case(torch, k, m, truth(corc, k, m, ln, nseg), held, bad, 0, seed=8)
    assert (c.want_status == REBUILT).sum() >= 2 and (c.want_status == CLEAN).sum() >= 1
    new = torch.from_numpy(c.flags.copy()).pin_memory()
    c.d_flags.fill_(1)
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        c.d_flags.copy_(new, non_blocking=True)
    assert c.call(encs(k, m), stream=S) == 0
    S.synchronize()
    c.check(encs(k, m))


def test_python_form_on_a_stream(torch, cess, corc, encs):
    k, m, n, nseg, ln = 4, 2, 6, 7, 300
    held = np.ones((nseg, n), dtype=bool)
    held[6, 2] = False
    bad = np.zeros_like(held)
    bad[np.arange(6), np.arange(6)] = True
    c = Case(torch, k, m, truth(corc, k, m, ln, nseg), held, bad, 0, seed=81)
    S = torch.cuda.Stream()
    torch.cuda.synchronize()
    out = encs(k, m).RepairFlaggedDevice(c.tensors(), c.d_flags, d_status=c.d_status, stream=S)
    assert out is c.d_status
    S.synchronize()
    c.check(encs(k, m))
    with pytest.raises(cess.ErrInvalidInput):
        encs(k, m).RepairFlaggedDevice(c.tensors(), c.d_flags[:-1])
    with pytest.raises(cess.ErrInvalidInput):
        encs(k, m).RepairFlaggedDevice(c.tensors(), c.d_flags, d_status=c.status_back)
    fresh = encs(k, m).RepairFlaggedDevice(c.tensors(), c.d_flags)
    torch.cuda.synchronize()
    assert np.array_equal(fresh.cpu().numpy(), c.want_status)


# ---- 9: validation ------------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(2, 1), (4, 2)])
def test_validation(torch, cess, corc, encs, k, m):
    from cess_amd import _lib
    lib = _lib.load()
    n, nseg, ln = k + m, 4, 64
    held = np.ones((nseg, n), dtype=bool)
    bad = np.zeros_like(held)
    bad[:, 0] = True
    c = Case(torch, k, m, truth(corc, k, m, ln, nseg), held, bad, 0, seed=9)
    enc = encs(k, m)
    a = c.addrs(c.big.data_ptr())
    ptrs = (c_void_p * a.size)(*[int(x) for x in a.ravel()])
    twice = a.copy()
    twice[3, n - 1] = twice[0, 1]  # the same address in two segments
    dup = (c_void_p * a.size)(*[int(x) for x in twice.ravel()])
    fl, st = c.d_flags.data_ptr(), c.d_status.data_ptr()
    fn = lib.cec_repair_flagged_ptrs
    assert fn(None, ptrs, fl, nseg, ln, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, None, fl, nseg, ln, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, None, nseg, ln, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, fl, nseg, ln, None, None) == _lib.CEC_EINVAL
    assert fn(enc._h, dup, fl, nseg, ln, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, fl, nseg, 0, st, None) == _lib.CEC_ESHARDLEN
    assert fn(enc._h, ptrs, fl, 0, ln, st, None) == _lib.CEC_OK
    assert fn(enc._h, None, None, 0, ln, None, None) == _lib.CEC_OK
    torch.cuda.synchronize()
    assert (c.status_back.cpu().numpy() == 0xEE).all()  # d_status keeps every byte
    assert np.array_equal(c.big.cpu().numpy(), c.image)  # and no shard byte was written
    assert fn(enc._h, ptrs, fl, nseg, ln, st, None) == _lib.CEC_OK  # the arrays were fine
    c.check(enc)


# ---- 10: the pool does not grow -----------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(2, 1), (10, 4)])
def test_pool_bytes_do_not_grow(torch, cess, corc, k, m):
    """Identical calls, each complete before the next (a block in flight cannot be reused): the
    tables of call n + 1 are the retired blocks of call n."""
    from cess_amd import _lib
    n, nseg, ln = k + m, 33, 256
    held = np.ones((nseg, n), dtype=bool)
    bad = np.zeros_like(held)
    bad[np.arange(nseg), np.arange(nseg) % n] = True
    with cess.New(k, m) as enc:
        c = Case(torch, k, m, truth(corc, k, m, ln, nseg), held, bad, 0, seed=10)
        seen = []
        for _ in range(4):
            assert c.call(enc) == 0
            torch.cuda.synchronize()
            seen.append(enc.stat(_lib.CEC_STAT_POOL_BYTES))
        assert seen[1] == seen[3] and seen[1] > 0, seen
        c.check(enc)
