"""cec_repair_flagged_multi_ptrs (Encoder.RepairFlaggedMultiDevice): up to four bad shards per
segment rebuilt from flags in device memory, the decode rows solved on the GPU.

The buffers are those of tests/test_gpu_repair_flagged.py (Case): truth from the C oracle, every
held shard a view into one allocation between bands of 0xA5, junk in the bad shards, the flag
tensor at an odd address, good flags 1 or 0xFF, random flag bytes at shards not held. After each
call, bit-exact:
  - d_status equals cec_flag_status_multi of every segment, the bytes around d_status are intact;
  - the whole allocation equals its earlier image with every bad shard of every REBUILT segment
    replaced by the truth, and nothing else changed, guards included;
  - d_flags and the byte before it are unchanged;
  - the allocation equals a copy on which cec_reconstruct_ptrs rebuilt the same shards, its
    sources being exactly the first k good shards of each segment."""
import ctypes
import hashlib
from ctypes import c_void_p

import numpy as np
import pytest

from oracle.c_oracle import c_encode
from tests.test_gpu_repair_flagged import CLEAN, GUARD, LOST, MANY, REBUILT, Case, truth

pytestmark = pytest.mark.gpu

MULTI_MAX = 4


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

    def get(k, m):
        if (k, m) not in made:
            made[(k, m)] = cess.New(k, m)
        return made[(k, m)]
    yield get
    for e in made.values():
        e.close()


def statuses_multi(k, m, held, flags, max_bad):
    """cec_flag_status_multi of every row -> (status [nseg], [lost...] per row)."""
    from cess_amd import _lib
    lib = _lib.load()
    held = np.ascontiguousarray(held, dtype=np.uint8)
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    n = k + m
    st, nl = ctypes.c_int(), ctypes.c_int()
    lost = (ctypes.c_uint8 * MULTI_MAX)()
    u8p = ctypes.POINTER(ctypes.c_uint8)
    status, losts = np.zeros(len(held), np.int64), []
    for s in range(len(held)):
        hp = ctypes.cast(c_void_p(held.ctypes.data + s * n), u8p)
        fp = ctypes.cast(c_void_p(flags.ctypes.data + s * n), u8p)
        assert lib.cec_flag_status_multi(k, m, hp, fp, max_bad, ctypes.byref(st),
                                         ctypes.byref(nl), lost) == 0
        status[s] = st.value
        losts.append([int(x) for x in lost[:nl.value]])
    return status, losts


class MultiCase(Case):
    """Case under the rule with a bound: want_lost is a list of shard indices per segment."""

    def __init__(self, torch, k, m, full, held, bad, off, seed, max_bad):
        super().__init__(torch, k, m, full, held, bad, off, seed)
        self.max_bad = max_bad
        self.want_status, self.want_lost = statuses_multi(k, m, self.held, self.flags, max_bad)

    def poke(self, s, i, payload):
        """Other bytes in held shard i of segment s, before the call."""
        o = self.hidx[s, i] * self.slot + self.lo
        self.image[o:o + self.ln] = payload
        self.big[o:o + self.ln] = self.torch.from_numpy(np.ascontiguousarray(payload)).cuda()

    def expected_image(self):
        img = self.image.copy()
        for s in np.nonzero(self.want_status == REBUILT)[0]:
            for j in self.want_lost[s]:
                o = self.hidx[s, j] * self.slot + self.lo
                img[o:o + self.ln] = self.full[s, j]
        return img

    def call(self, enc, stream=None, d_flags=None, max_bad=None):
        from cess_amd import _lib
        a = self.addrs(self.big.data_ptr())
        ptrs = (c_void_p * a.size)(*[int(x) for x in a.ravel()])
        fl = self.d_flags if d_flags is None else d_flags
        return _lib.load().cec_repair_flagged_multi_ptrs(
            enc._h, ptrs, fl.data_ptr(), self.nseg, self.ln,
            self.max_bad if max_bad is None else max_bad, self.d_status.data_ptr(),
            None if stream is None else stream.cuda_stream)

    def check_against_reconstruct(self, enc):
        """cec_reconstruct_ptrs on a copy of the earlier image: the bad shards of the rebuilt
        segments are the destinations, exactly their first k good shards the sources."""
        from cess_amd import _lib
        torch = self.torch
        copy = torch.from_numpy(self.image.copy()).cuda()
        a = self.addrs(copy.data_ptr())
        src, dst = np.zeros_like(a), np.zeros_like(a)
        rows = np.nonzero(self.want_status == REBUILT)[0]
        for s in rows:
            good = np.nonzero(self.held[s] & (self.flags[s] != 0))[0][:self.k]
            src[s, good] = a[s, good]
            dst[s, self.want_lost[s]] = a[s, self.want_lost[s]]
        if rows.size:
            sp = (c_void_p * a.size)(*[int(x) for x in src.ravel()])
            dp = (c_void_p * a.size)(*[int(x) for x in dst.ravel()])
            assert _lib.load().cec_reconstruct_ptrs(enc._h, sp, dp, self.nseg, self.ln,
                                                    None) == 0
        torch.cuda.synchronize()
        assert torch.equal(copy, self.big), "differs from cec_reconstruct_ptrs on a copy"


def counts(c):
    """{(status, bad shards rebuilt): segments}"""
    out = {}
    for st, lost in zip(c.want_status, c.want_lost):
        out[(int(st), len(lost))] = out.get((int(st), len(lost)), 0) + 1
    return out


# ---- 1: RS(4,2), all 64 flag patterns in one call ----------------------------------------------

def rs42_patterns():
    bad = np.array([[(p >> i) & 1 for i in range(6)] for p in range(64)], dtype=bool)
    return np.ones((64, 6), dtype=bool), bad


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("ln", [1, 17, 4101, 4112])
def test_rs42_all_patterns(torch, cess, corc, encs, ln, off):
    held, bad = rs42_patterns()
    full = truth(corc, 4, 2, ln, 64)
    c = MultiCase(torch, 4, 2, full, held, bad, off, seed=ln * 2 + off, max_bad=2)
    assert counts(c) == {(CLEAN, 0): 1, (REBUILT, 1): 6, (REBUILT, 2): 15, (LOST, 0): 42}
    assert c.call(encs(4, 2)) == 0
    c.check(encs(4, 2))
    # max_bad 1 is cec_repair_flagged_ptrs: same statuses, same image, the 15 MANY untouched
    one = MultiCase(torch, 4, 2, full, held, bad, off, seed=ln * 2 + off, max_bad=1)
    ref = Case(torch, 4, 2, full, held, bad, off, seed=ln * 2 + off)
    assert counts(one) == {(CLEAN, 0): 1, (REBUILT, 1): 6, (MANY, 0): 15, (LOST, 0): 42}
    assert np.array_equal(one.image, ref.image)
    assert one.call(encs(4, 2)) == 0
    assert ref.call(encs(4, 2)) == 0
    one.check(encs(4, 2))
    assert torch.equal(one.status_back, ref.status_back)
    assert torch.equal(one.big, ref.big)


# ---- 2: small k, the k_ptrt family --------------------------------------------------------------

def every_subset_bad(n, sizes):
    import itertools
    rows = [c for e in sizes for c in itertools.combinations(range(n), e)]
    bad = np.zeros((len(rows), n), dtype=bool)
    for r, c in enumerate(rows):
        bad[r, list(c)] = True
    return np.ones_like(bad), bad


@pytest.mark.parametrize("ln", [17, 4101])
@pytest.mark.parametrize("k,m,sizes", [(3, 2, (2,)), (2, 2, (2,)), (1, 3, (1, 2, 3))])
def test_small_k(torch, cess, corc, encs, k, m, sizes, ln):
    held, bad = every_subset_bad(k + m, sizes)
    c = MultiCase(torch, k, m, truth(corc, k, m, ln, len(held)), held, bad, 0, seed=k + ln,
                  max_bad=MULTI_MAX)
    assert (c.want_status == REBUILT).all()
    assert {len(x) for x in c.want_lost} == set(sizes)
    assert c.call(encs(k, m)) == 0
    c.check(encs(k, m))


# ---- 3: wider codes -----------------------------------------------------------------------------

def wide_case(torch, corc, k, m, ln, rows, max_bad, seed):
    """rows: (shards not held, bad shards) per segment, as counts drawn at random or index lists."""
    n = k + m
    rng = np.random.default_rng(seed)
    held = np.ones((len(rows), n), dtype=bool)
    bad = np.zeros_like(held)
    for s, (gone, lost) in enumerate(rows):
        if isinstance(gone, int):
            gone = rng.choice(n, size=gone, replace=False)
        held[s, list(gone)] = False
        if isinstance(lost, int):
            lost = rng.choice(np.nonzero(held[s])[0], size=lost, replace=False)
        bad[s, list(lost)] = True
    return MultiCase(torch, k, m, truth(corc, k, m, ln, len(rows)), held, bad, 0, seed=seed + 1,
                     max_bad=max_bad)


@pytest.mark.parametrize("ln", [80, 4101])
def test_rs104_buckets_1_to_4(torch, cess, corc, encs, ln):
    rows = [(0, 1), (0, 2), (0, 3), (0, 4), (0, 0), (1, 3), (2, 2), (3, 1), (1, 4), (0, [0, 1, 12, 13])]
    c = wide_case(torch, corc, 10, 4, ln, rows, MULTI_MAX, seed=104 + ln)
    assert [len(x) for x in c.want_lost] == [1, 2, 3, 4, 0, 3, 2, 1, 0, 4]
    assert c.want_status[4] == CLEAN and c.want_status[8] == LOST
    assert c.call(encs(10, 4)) == 0
    c.check(encs(10, 4))


@pytest.mark.parametrize("ln", [80, 4101])
def test_rs104_max_bad_2_leaves_three(torch, cess, corc, encs, ln):
    c = wide_case(torch, corc, 10, 4, ln, [(0, 3), (0, 2), (1, 1), (0, 0)], 2, seed=1042 + ln)
    assert list(c.want_status) == [MANY, REBUILT, REBUILT, CLEAN]
    assert c.call(encs(10, 4)) == 0
    c.check(encs(10, 4))


@pytest.mark.parametrize("ln", [80, 4101])
def test_rs173(torch, cess, corc, encs, ln):
    c = wide_case(torch, corc, 17, 3, ln, [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (0, [0, 19])],
                  MULTI_MAX, seed=173 + ln)
    assert list(c.want_status) == [REBUILT] * 4 + [LOST, REBUILT]
    assert c.call(encs(17, 3)) == 0
    c.check(encs(17, 3))


@pytest.mark.parametrize("ln", [80, 4101])
def test_rs3232(torch, cess, corc, encs, ln):
    k, m = 32, 32
    heavy_gone = [i for i in range(k) if i not in (5, 20)]  # 2 data held plus all 32 parity
    rows = [(0, 2), (0, 3), (0, 4), (0, 5), (heavy_gone, [5, 40]), (heavy_gone, [33, 63]),
            (m - 3, 3),   # exactly k + e held
            (m - 1, 2),   # k + 1 held, 2 bad: fewer than k good
            (7, 4), (0, 0)]
    c = wide_case(torch, corc, k, m, ln, rows, MULTI_MAX, seed=3232 + ln)
    assert list(c.want_status) == [REBUILT, REBUILT, REBUILT, MANY, REBUILT, REBUILT, REBUILT,
                                   LOST, REBUILT, CLEAN]
    assert c.held[6].sum() == k + 3 and len(c.want_lost[6]) == 3
    assert c.call(encs(k, m)) == 0
    c.check(encs(k, m))


@pytest.mark.parametrize("ln", [80, 4101])
def test_rs20056_past_64_lanes(torch, cess, corc, encs, ln):
    rows = [(0, 2), (0, 4), (30, 4), (0, [199, 255]), (0, 5)]
    c = wide_case(torch, corc, 200, 56, ln, rows, MULTI_MAX, seed=20056 + ln)
    assert list(c.want_status) == [REBUILT] * 4 + [MANY]
    assert c.call(encs(200, 56)) == 0
    c.check(encs(200, 56))


@pytest.mark.parametrize("ln", [80, 4101])
def test_rs104_rt_mode_1(torch, cess, corc, ln):
    """CEC_OPT_RT_MODE = 1: the per-bit mask product (k_ptrt) and its hb words."""
    from cess_amd import _lib
    with cess.New(10, 4) as enc:
        enc.set_option(_lib.CEC_OPT_RT_MODE, 1)
        c = wide_case(torch, corc, 10, 4, ln, [(0, 1), (0, 2), (0, 3), (0, 4), (0, 0), (2, 2)],
                      MULTI_MAX, seed=1041 + ln)
        assert [len(x) for x in c.want_lost] == [1, 2, 3, 4, 0, 2]
        assert c.call(enc) == 0
        c.check(enc)




# ---- 4: the read set ----------------------------------------------------------------------------

@pytest.mark.parametrize("k,m,bads,junk", [
    (4, 2, [[0], [2], [4]], [5]),
    (10, 4, [[0, 5], [3, 11], [10, 11]], [12, 13]),
    (32, 32, [[0, 33], [1, 2, 3], [4, 30, 31, 32]], [40, 63]),
])
def test_good_shards_past_the_first_k_are_not_read(torch, cess, corc, encs, k, m, bads, junk):
    """The shards in `junk` are held and flagged good but hold other bytes, and lie past the first
    k good shards of every segment: the rebuilt bytes are still the truth and the junk stays."""
    n, ln = k + m, 1000
    held = np.ones((len(bads), n), dtype=bool)
    bad = np.zeros_like(held)
    for s, b in enumerate(bads):
        bad[s, b] = True
    c = MultiCase(torch, k, m, truth(corc, k, m, ln, len(bads)), held, bad, 0, seed=k,
                  max_bad=MULTI_MAX)
    rng = np.random.default_rng(44)
    for s in range(len(bads)):
        first_k = np.nonzero(c.held[s] & (c.flags[s] != 0))[0][:k]
        assert not set(junk) & set(first_k)
        for i in junk:
            c.poke(s, i, rng.integers(0, 256, ln, dtype=np.uint8))
    assert (c.want_status == REBUILT).all()
    assert c.call(encs(k, m)) == 0
    c.check(encs(k, m))
    after = c.big.cpu().numpy()
    for s in range(len(bads)):
        for i in junk:
            o = c.hidx[s, i] * c.slot + c.lo
            assert not np.array_equal(after[o:o + ln], c.full[s, i])  # still the junk


# ---- 5: several held sets, mixed bad counts -----------------------------------------------------

def test_several_held_sets(torch, cess, corc, encs):
    k, m, n, nseg, ln = 4, 2, 6, 40, 1000
    rng = np.random.default_rng(505)
    sets = [(1, 1, 1, 1, 1, 1), (0, 1, 1, 1, 1, 1), (1, 1, 1, 0, 1, 1), (1, 1, 1, 1, 1, 0),
            (1, 0, 1, 1, 0, 1)]
    which = rng.permutation(np.arange(nseg) % len(sets))
    held = np.array([sets[w] for w in which], dtype=bool)
    bad = np.zeros_like(held)
    for s in range(nseg):
        idx = np.nonzero(held[s])[0]
        bad[s, rng.choice(idx, size=int(rng.integers(0, 4)), replace=False)] = True
    c = MultiCase(torch, k, m, truth(corc, k, m, ln, nseg), held, bad, 0, seed=5, max_bad=2)
    assert set(c.want_status) == {CLEAN, REBUILT, LOST}
    assert {len(x) for x in c.want_lost} == {0, 1, 2}
    assert c.call(encs(k, m)) == 0
    c.check(encs(k, m))
    # under max_bad 1 with the multi planner's codec, the same buffers show MANY as well
    d = MultiCase(torch, k, m, truth(corc, k, m, ln, nseg), held, bad, 0, seed=5, max_bad=1)
    assert set(d.want_status) == {CLEAN, REBUILT, MANY, LOST}
    assert d.call(encs(k, m)) == 0
    d.check(encs(k, m))


# ---- 6: past one grid of rows -------------------------------------------------------------------

def test_65537_segments(torch, cess, corc, encs):
    """RS(2,2), 16-byte shards as views of four big tensors; two bad shards only in segments 0,
    65,534, 65,535 and 65,536: the bucket-2 launch is cut at 65,535 rows, and the chunk block (3,216 bytes
    per segment, 211 MB) is stream-ordered scratch, its last chunks addressed 64 bits wide."""
    from cess_amd import _lib
    k, m, n, nseg, ln = 2, 2, 4, 65537, 16
    full = truth(corc, k, m, ln, nseg)
    badmap = {0: (0, 1), 65534: (1, 2), 65535: (2, 3), 65536: (0, 3)}
    rng = np.random.default_rng(6)
    images = []
    for i in range(n):
        body = full[:, i, :].copy()
        for s, js in badmap.items():
            if i in js:
                body[s] = rng.integers(0, 256, ln, dtype=np.uint8)
        images.append(np.concatenate([np.full(GUARD, 0xA5, np.uint8), body.ravel(),
                                      np.full(GUARD, 0xA5, np.uint8)]))
    bigs = [torch.from_numpy(im.copy()).cuda() for im in images]
    flags = np.ones((nseg, n), np.uint8)
    for s, js in badmap.items():
        flags[s, list(js)] = 0
    flag_back = torch.from_numpy(np.concatenate([[0x5A], flags.ravel()]).astype(np.uint8)).cuda()
    status_back = torch.full((nseg + 32,), 0xEE, dtype=torch.uint8, device="cuda")
    want = np.zeros(nseg, np.uint8)
    want[list(badmap)] = REBUILT
    some = [0, 1, 65533, 65534, 65535, 65536]
    st, lost = statuses_multi(k, m, np.ones((len(some), n), np.uint8), flags[some], 2)
    assert np.array_equal(st, want[some]) and lost[0] == [0, 1] and lost[5] == [0, 3]
    addr = np.stack([b.data_ptr() + GUARD + np.arange(nseg, dtype=np.uint64) * ln for b in bigs],
                    axis=1)
    ptrs = (c_void_p * addr.size)(*[int(x) for x in addr.ravel()])
    enc = encs(k, m)
    assert _lib.load().cec_repair_flagged_multi_ptrs(
        enc._h, ptrs, flag_back.data_ptr() + 1, nseg, ln, 2, status_back.data_ptr() + 16,
        None) == 0
    torch.cuda.synchronize()
    sb = status_back.cpu().numpy()
    assert (sb[:16] == 0xEE).all() and (sb[16 + nseg:] == 0xEE).all()
    assert np.array_equal(sb[16:16 + nseg], want)
    fb = flag_back.cpu().numpy()
    assert fb[0] == 0x5A and np.array_equal(fb[1:], flags.ravel())
    for i in range(n):  # healed: the four tensors hold the truth between their guards
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
            (dst if i in badmap[s] else src)[r, i] = a
    sp = (c_void_p * src.size)(*[int(x) for x in src.ravel()])
    dp = (c_void_p * dst.size)(*[int(x) for x in dst.ravel()])
    assert _lib.load().cec_reconstruct_ptrs(enc._h, sp, dp, len(segs), ln, None) == 0
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(copies[i], bigs[i]), i


# ---- 7: nothing to do ---------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(4, 2), (32, 32)])
def test_all_clean(torch, cess, corc, encs, k, m):
    nseg, ln = 64, 4101
    held = np.ones((nseg, k + m), dtype=bool)
    c = MultiCase(torch, k, m, truth(corc, k, m, ln, nseg), held, np.zeros_like(held), 0, seed=7,
                  max_bad=MULTI_MAX)
    assert (c.want_status == CLEAN).all()
    assert c.call(encs(k, m)) == 0
    c.check(encs(k, m), reference=False)
    assert np.array_equal(c.big.cpu().numpy(), c.image)


# ---- 8: stream order ----------------------------------------------------------------------------

def test_flags_produced_on_the_stream(torch, cess, corc, encs):
    """The flags in device memory say "all good" and are synchronised; new flags are then copied
    in on stream S without waiting, and the call follows on S: it acts on the new flags."""
    k, m, n, nseg, ln = 4, 2, 6, 24, 8192
    held = np.ones((nseg, n), dtype=bool)
    bad = np.zeros_like(held)
    even = np.arange(0, nseg, 2)
    bad[even, even % n] = True  # every other segment has two bad shards
    bad[even, (even + 3) % n] = True
    c = MultiCase(torch, k, m, truth(corc, k, m, ln, nseg), held, bad, 0, seed=8, max_bad=2)
    assert counts(c) == {(REBUILT, 2): nseg // 2, (CLEAN, 0): nseg // 2}
    new = torch.from_numpy(c.flags.copy()).pin_memory()
    c.d_flags.fill_(1)
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        c.d_flags.copy_(new, non_blocking=True)
    assert c.call(encs(k, m), stream=S) == 0
    S.synchronize()
    c.check(encs(k, m))


# ---- 9: validation ------------------------------------------------------------------------------

def test_validation(torch, cess, corc, encs):
    from cess_amd import _lib
    lib = _lib.load()
    k, m, n, nseg, ln = 4, 2, 6, 4, 64
    held = np.ones((nseg, n), dtype=bool)
    bad = np.zeros_like(held)
    bad[:, [0, 3]] = True
    c = MultiCase(torch, k, m, truth(corc, k, m, ln, nseg), held, bad, 0, seed=9, max_bad=2)
    enc = encs(k, m)
    a = c.addrs(c.big.data_ptr())
    ptrs = (c_void_p * a.size)(*[int(x) for x in a.ravel()])
    twice = a.copy()
    twice[3, n - 1] = twice[0, 1]  # the same address in two segments
    dup = (c_void_p * a.size)(*[int(x) for x in twice.ravel()])
    fl, st = c.d_flags.data_ptr(), c.d_status.data_ptr()
    fn = lib.cec_repair_flagged_multi_ptrs
    assert fn(None, ptrs, fl, nseg, ln, 2, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, None, fl, nseg, ln, 2, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, None, nseg, ln, 2, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, fl, nseg, ln, 2, None, None) == _lib.CEC_EINVAL
    assert fn(enc._h, dup, fl, nseg, ln, 2, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, fl, nseg, ln, 0, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, fl, nseg, ln, 5, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, fl, 0, ln, 5, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, fl, nseg, 0, 2, st, None) == _lib.CEC_ESHARDLEN
    assert fn(enc._h, ptrs, fl, 0, ln, 2, st, None) == _lib.CEC_OK
    assert fn(enc._h, None, None, 0, ln, 2, None, None) == _lib.CEC_OK
    torch.cuda.synchronize()
    assert (c.status_back.cpu().numpy() == 0xEE).all()  # d_status keeps every byte
    assert np.array_equal(c.big.cpu().numpy(), c.image)  # and no shard byte was written
    assert fn(enc._h, ptrs, fl, nseg, ln, 2, st, None) == _lib.CEC_OK  # the arrays were fine
    c.check(enc)


# ---- 10: the pool does not grow, the decode cache is not used ------------------------------------

@pytest.mark.parametrize("k,m", [(4, 2), (10, 4)])
def test_pool_bytes_do_not_grow(torch, cess, corc, k, m):
    from cess_amd import _lib
    n, nseg, ln = k + m, 33, 256
    held = np.ones((nseg, n), dtype=bool)
    bad = np.zeros_like(held)
    bad[np.arange(nseg), np.arange(nseg) % n] = True
    bad[np.arange(nseg), (np.arange(nseg) + 2) % n] = True
    with cess.New(k, m) as enc:
        c = MultiCase(torch, k, m, truth(corc, k, m, ln, nseg), held, bad, 0, seed=10,
                      max_bad=MULTI_MAX)
        cached = enc.stat(_lib.CEC_STAT_DECODE_CACHED)
        seen = []
        for _ in range(4):
            assert c.call(enc) == 0
            torch.cuda.synchronize()
            seen.append(enc.stat(_lib.CEC_STAT_POOL_BYTES))
            assert enc.stat(_lib.CEC_STAT_DECODE_CACHED) == cached
        assert seen[1] == seen[2] == seen[3] and seen[1] > 0, seen
        c.check(enc, reference=False)  # the reference fills the decode cache
        assert enc.stat(_lib.CEC_STAT_DECODE_CACHED) == cached


# ---- 11: the Python forms -------------------------------------------------------------------------

def test_python_form_on_a_stream(torch, cess, corc, encs):
    k, m, n, nseg, ln = 4, 2, 6, 7, 300
    held = np.ones((nseg, n), dtype=bool)
    held[6, 2] = False
    bad = np.zeros_like(held)
    bad[np.arange(6), np.arange(6)] = True
    bad[np.arange(3), np.arange(3) + 3] = True
    c = MultiCase(torch, k, m, truth(corc, k, m, ln, nseg), held, bad, 0, seed=81, max_bad=2)
    assert counts(c) == {(REBUILT, 2): 3, (REBUILT, 1): 3, (CLEAN, 0): 1}
    S = torch.cuda.Stream()
    torch.cuda.synchronize()
    out = encs(k, m).RepairFlaggedMultiDevice(c.tensors(), c.d_flags, max_bad=2,
                                              d_status=c.d_status, stream=S)
    assert out is c.d_status
    S.synchronize()
    c.check(encs(k, m))
    with pytest.raises(cess.ErrInvalidInput):
        encs(k, m).RepairFlaggedMultiDevice(c.tensors(), c.d_flags[:-1])
    with pytest.raises(cess.ErrInvalidInput):
        encs(k, m).RepairFlaggedMultiDevice(c.tensors(), c.d_flags, max_bad=5)
    with pytest.raises(cess.ErrInvalidInput):
        encs(k, m).RepairFlaggedMultiDevice(c.tensors(), c.d_flags, max_bad=0)
    fresh = encs(k, m).RepairFlaggedMultiDevice(c.tensors(), c.d_flags)
    torch.cuda.synchronize()
    assert np.array_equal(fresh.cpu().numpy(), np.where(c.want_status == REBUILT, REBUILT, CLEAN))


def test_scrub_repair_multi_device(torch, cess, corc):
    """RS(4,2), 3 segments of 4 KiB fragments, two fragments of segment 1 corrupted: the scrub
    flags them, the repair heals both, and a second scrub flags everything good."""
    k, m, n, nseg, F = 4, 2, 6, 3, 4096
    rng = np.random.default_rng(11)
    data = rng.integers(0, 256, (k, nseg * F), dtype=np.uint8)
    par = np.stack(c_encode(corc, k, m, list(data)))
    full = np.ascontiguousarray(np.concatenate([data, par]).reshape(n, nseg, F).transpose(1, 0, 2))
    recorded = [[hashlib.sha256(full[s, i].tobytes()).hexdigest().encode() for i in range(n)]
                for s in range(nseg)]
    now = full.copy()
    now[1, 2, 7] ^= 0x10
    now[1, 5, 4095] ^= 1
    segments = [[torch.from_numpy(now[s, i].copy()).cuda() for i in range(n)]
                for s in range(nseg)]
    with cess.New(k, m) as enc:
        d_flags, d_status = cess.audit.scrub_repair_multi_device(enc, segments, recorded)
        torch.cuda.synchronize()
        want_flags = np.ones((nseg, n), bool)
        want_flags[1, [2, 5]] = False
        assert np.array_equal(d_flags.cpu().numpy() != 0, want_flags)
        assert list(d_status.cpu().numpy()) == [CLEAN, REBUILT, CLEAN]
        for s in range(nseg):
            for i in range(n):
                assert np.array_equal(segments[s][i].cpu().numpy(), full[s, i]), (s, i)
        d_flags, d_status = cess.audit.scrub_repair_multi_device(enc, segments, recorded,
                                                                 max_bad=2)
        torch.cuda.synchronize()
        assert (d_flags.cpu().numpy() != 0).all()
        assert (d_status.cpu().numpy() == CLEAN).all()
