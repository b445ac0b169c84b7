"""cec_locate_multi_ptrs (Encoder.LocateMultiDevice): one or two corrupt fragments found from
parity alone, on the GPU.

Built on the LocCase of tests/test_gpu_locate.py: every held shard a view into one allocation
between bands of 0xA5, at an offset from a 16-byte boundary; the corruption is written into that
image on the host, and the expected status, flags and nbad of every segment are
cec_locate_multi_host on the same bytes. After a call the whole status and nbad vectors and the
whole flag tensor are compared, with the bytes around them (the flag tensor starts at an odd
address), and the allocation equals its image: the call writes no shard byte."""
import ctypes
import itertools
from ctypes import c_void_p

import numpy as np
import pytest

from tests.test_gpu_locate import (AMBIGUOUS, CLEAN, FOUND, UNCHECKED, WG, LocCase, mixed_case,
                                   recorded_of)
from tests.test_gpu_repair_flagged import cess, encs, torch, truth  # noqa: F401 (fixtures)
from tests.test_locate_rule import MUL_TABLE, div

pytestmark = pytest.mark.gpu


class MultiCase(LocCase):
    """A LocCase whose expectation is cec_locate_multi_host and whose call is
    cec_locate_multi_ptrs, with a guarded nbad vector."""

    def __init__(self, torch, k, m, full, held, off, seed, nsyn=4, max_bad=2):
        super().__init__(torch, k, m, full, held, off, seed, nsyn)
        self.max_bad = max_bad
        self.nbad_back = torch.full((self.nseg + 32,), 0xEE, dtype=torch.uint8, device="cuda")
        self.d_nbad = self.nbad_back[15:15 + self.nseg]

    def poke(self, s, i, x, value=None):
        """XOR a non-zero byte into shard i of segment s at offset x."""
        v = int(self.rng.integers(1, 256)) if value is None else value
        self.image[self.at(s, i) + x] ^= np.uint8(v)

    def cancel_pair(self, s, a, b):
        """e_b = (u_a / u_b) e_a at every offset of a random non-zero e_a: S_0 never shows."""
        import cess_amd
        u = cess_amd.locate_rows(self.k, self.m, self.held[s], 4)[1][0]
        e = self.rng.integers(0, 256, self.ln, dtype=np.uint8)
        e[int(self.rng.integers(0, self.ln))] |= 1
        oa, ob = self.at(s, a), self.at(s, b)
        self.image[oa:oa + self.ln] ^= e
        self.image[ob:ob + self.ln] ^= MUL_TABLE[div(int(u[a]), int(u[b]))][e]

    def expect(self, rows=None):
        """Status, found set, flags and nbad by cec_locate_multi_host on the image (for `rows`,
        default all; every other segment is expected clean)."""
        from cess_amd import _lib
        lib = _lib.load()
        a = self.addrs(self.image.ctypes.data)
        st, nf, found = ctypes.c_int(), ctypes.c_int(), (ctypes.c_int * 2)()
        self.want_locate = np.where(self.held.sum(1) > self.k, CLEAN, UNCHECKED).astype(np.uint8)
        self.want_nbad = np.zeros(self.nseg, np.uint8)
        self.want_found = [[] for _ in range(self.nseg)]
        self.want_flags = self.held.astype(np.uint8)
        for s in (range(self.nseg) if rows is None else rows):
            ptrs = (c_void_p * self.n)(*[int(x) or None for x in a[s]])
            assert lib.cec_locate_multi_host(self.k, self.m, ptrs, self.ln, self.nsyn,
                                             self.max_bad, ctypes.byref(st), ctypes.byref(nf),
                                             found) == 0
            self.want_locate[s] = st.value
            self.want_found[s] = list(found[:nf.value])
            if st.value == FOUND:
                self.want_nbad[s] = nf.value
                self.want_flags[s, self.want_found[s]] = 0
            elif st.value == AMBIGUOUS:
                self.want_flags[s] = 0

    def upload(self, rows=None):
        self.big = self.torch.from_numpy(self.image.copy()).cuda()
        self.expect(rows)

    def locate(self, enc, stream=None, flags=None, status=None, nbad=None, max_bad=None,
               no_nbad=False):
        from cess_amd import _lib
        a = self.addrs(self.big.data_ptr())
        ptrs = (c_void_p * a.size)(*[int(x) or None for x in a.ravel()])
        fl = self.d_loc_flags if flags is None else flags
        st = self.d_status if status is None else status
        nb = self.d_nbad if nbad is None else nbad
        return _lib.load().cec_locate_multi_ptrs(
            enc._h, ptrs, self.nseg, self.ln, self.nsyn,
            self.max_bad if max_bad is None else max_bad, fl.data_ptr(), st.data_ptr(),
            None if no_nbad else nb.data_ptr(), None if stream is None else stream.cuda_stream)

    def check_located(self, nbad=True):
        super().check_located()
        nb = self.nbad_back.cpu().numpy()
        if not nbad:
            assert (nb == 0xEE).all()
            return
        assert (nb[:15] == 0xEE).all() and (nb[15 + self.nseg:] == 0xEE).all()
        got = nb[15:15 + self.nseg]
        bad = np.flatnonzero(got != self.want_nbad)
        assert bad.size == 0, (bad[:8], got[bad[:8]], self.want_nbad[bad[:8]])


KINDS = ["clean", "one", "meet", "disjoint_low", "disjoint_high", "same", "zero", "cancel",
         "three"]
TWO_BAD = KINDS[2:8]


def corrupt(c, s, kind):
    """Corrupt segment s of MultiCase c in the given kind; returns the bad shards, ascending."""
    H = np.flatnonzero(c.held[s])
    ln = c.ln
    pick = sorted(int(v) for v in c.rng.choice(H, 3, replace=False))
    a, b = pick[0], pick[2]
    tail = ln - 1  # in the byte tail where the length has one
    low = (2 * ln) // 5 if ln > 1 else 0
    if kind == "clean":
        return []
    if kind == "one":
        c.corrupt(s, b, ["first", "last", "whole", "tail"][s % 4])
        return [b]
    if kind == "meet":
        c.replace(s, a)
        c.replace(s, b)
    elif kind == "disjoint_low":  # the lower index first, the higher in the tail
        c.poke(s, a, low)
        c.poke(s, b, tail)
    elif kind == "disjoint_high":  # the higher index first
        c.poke(s, b, 0)
        c.poke(s, a, tail)
    elif kind == "same":
        c.poke(s, a, low)
        c.poke(s, b, low)
    elif kind == "zero":  # the pair holds the first held shard (shard 0 where it is held)
        a = int(H[0])
        c.poke(s, a, tail)
        c.replace(s, b)
    elif kind == "cancel":
        c.cancel_pair(s, a, b)
    elif kind == "three":
        for j in pick:
            c.replace(s, j)
        return pick
    return [a, b]


def pair_held_sets(k, m, rng, null):
    """All shards (or all but `null`), k + 4 where the code can spare a shard, and k shards."""
    n, sets = k + m, []
    row = np.ones(n, bool)
    if null is not None:
        row[null] = False
    sets.append(row)
    if m > 4:
        row = np.zeros(n, bool)
        row[rng.choice(np.arange(1, n), k + 4, replace=False)] = True  # shard 0 not held
        sets.append(row)
    row = np.zeros(n, bool)
    row[rng.choice(n, k, replace=False)] = True
    sets.append(row)
    return sets


CODES = [
    ("rs4_4", 4, 4, None),          # the smallest pair-locating code
    ("rs10_4", 10, 4, None),
    ("rs10_4-null", 10, 4, 3),      # one shard not held: r = 3, the fallback
    ("rs4_2", 4, 2, None),          # r = 2, the fallback
    ("rs32_32", 32, 32, None),
    ("rs200_56", 200, 56, None),    # the planner's lanes stride past 64
]


@pytest.mark.parametrize("ln,off", [(1, 0), (15, 0), (16, 0), (WG, 0), (WG, 1)])
@pytest.mark.parametrize("id,k,m,null", CODES, ids=[c[0] for c in CODES])
def test_mixed_segments(torch, cess, corc, encs, id, k, m, null, ln, off):
    rng = np.random.default_rng(k * 137 + m * 19 + ln + off)
    sets = pair_held_sets(k, m, rng, null)
    held = np.array([row for row in sets for _ in KINDS])
    c = MultiCase(torch, k, m, truth(corc, k, m, ln, len(held)), held, off,
                  seed=k + m + ln + off + 2)
    bad = {}
    for s in range(c.nseg):
        if held[s].sum() > k:  # an unchecked set stays as it is: nothing of it is read
            bad[s] = corrupt(c, s, KINDS[s % len(KINDS)])
    c.upload()
    assert set(int(x) for x in c.want_locate) == {CLEAN, FOUND, AMBIGUOUS, UNCHECKED}
    for s, J in bad.items():
        r = min(4, int(held[s].sum()) - k)
        kind = KINDS[s % len(KINDS)]
        if kind == "one" and r >= 2:
            assert c.want_locate[s] == FOUND and c.want_found[s] == J, (s, kind)
        if kind in TWO_BAD and r == 4:
            assert c.want_locate[s] == FOUND and c.want_nbad[s] == 2, (s, kind)
            assert c.want_found[s] == J, (s, kind)
        if kind in TWO_BAD and r == 3:  # a code of distance 4: two errors never pass for one
            assert c.want_locate[s] == AMBIGUOUS, (s, kind)
    assert c.locate(encs(k, m)) == 0
    c.check_located()


def test_every_pair_of_flips_is_found(torch, cess, corc, encs):
    """Copies of one RS(4,4) codeword, each with one flipped bit in each of two shards: every
    shard pair, offsets in the 8-byte columns and in the tail, equal and in both orders, every
    bit. Each is FOUND with exactly its pair; the expectation is the plan itself."""
    k, m, ln = 4, 4, 37
    offsets = [(0, 0), (17, 17), (36, 36), (0, 36), (36, 0), (5, 6), (6, 5), (31, 32), (32, 31),
               (8, 24), (33, 35), (23, 2)]
    plan = [(a, b, xa, xb, bit, (bit * 3 + xa + 1) % 8)
            for a, b in itertools.combinations(range(k + m), 2)
            for xa, xb in offsets for bit in range(8)]
    nseg = len(plan)
    assert 2000 < nseg < 4000 and {p[4] for p in plan} == {p[5] for p in plan} == set(range(8))
    one = truth(corc, k, m, ln, 1)
    full = np.ascontiguousarray(np.broadcast_to(one, (nseg, k + m, ln)))
    c = MultiCase(torch, k, m, full, np.ones((nseg, k + m), bool), 0, seed=6)
    c.want_flags = np.ones((nseg, k + m), np.uint8)
    for s, (a, b, xa, xb, ba, bb) in enumerate(plan):
        c.flip(s, a, xa, ba)
        c.flip(s, b, xb, bb)
        c.want_flags[s, [a, b]] = 0
    c.big = torch.from_numpy(c.image.copy()).cuda()
    c.want_locate = np.full(nseg, FOUND, np.uint8)
    c.want_nbad = np.full(nseg, 2, np.uint8)
    assert c.locate(encs(k, m)) == 0
    c.check_located()


def test_rows_past_grid_y(torch, cess, corc, encs):
    k, m, ln, nseg = 4, 4, 16, 70000
    held = np.ones((nseg, k + m), bool)
    c = MultiCase(torch, k, m, truth(corc, k, m, ln, nseg), held, 0, seed=71)
    dirty = [0, 65535, 65536, 69999]
    want = {}
    for t, s in enumerate(dirty):
        want[s] = corrupt(c, s, ["meet", "disjoint_low", "disjoint_high", "cancel"][t])
    c.upload(rows=dirty)
    for s in dirty:
        assert c.want_locate[s] == FOUND and c.want_found[s] == want[s]
    assert int((c.want_locate == CLEAN).sum()) == nseg - 4
    assert c.locate(encs(k, m)) == 0
    c.check_located()


def mixed_pairs(torch, corc, k, m, ln):
    held = np.ones((len(KINDS) * 2, k + m), bool)
    c = MultiCase(torch, k, m, truth(corc, k, m, ln, len(held)), held, 0, seed=k + ln)
    for s in range(c.nseg):
        corrupt(c, s, KINDS[s % len(KINDS)])
    c.upload()
    return c


def test_repeats_are_equal_and_hold_nothing(torch, cess, corc, encs):
    from cess_amd import _lib
    k, m = 10, 4
    enc = encs(k, m)
    c = mixed_pairs(torch, corc, k, m, WG)
    cached = enc.stat(_lib.CEC_STAT_DECODE_CACHED)
    assert c.locate(enc) == 0
    c.check_located()
    f2 = torch.full_like(c.d_loc_flags, 0x33)
    s2 = torch.full_like(c.d_status, 0x33)
    n2 = torch.full_like(c.d_nbad, 0x33)
    side = torch.cuda.Stream()
    for _ in range(3):  # back to back on another stream, nothing waited for in between
        assert c.locate(enc, stream=side, flags=f2, status=s2, nbad=n2) == 0
    torch.cuda.synchronize()
    assert torch.equal(f2, c.d_loc_flags) and torch.equal(s2, c.d_status)
    assert torch.equal(n2, c.d_nbad)
    # with the stream drained between calls, the tables of call n + 1 are the retired blocks of
    # call n
    seen = []
    for _ in range(6):
        assert c.locate(enc, stream=side, flags=f2, status=s2, nbad=n2) == 0
        torch.cuda.synchronize()
        seen.append(enc.stat(_lib.CEC_STAT_POOL_BYTES))
        assert enc.stat(_lib.CEC_STAT_DECODE_CACHED) == cached
    assert seen[1] == seen[5] and seen[1] > 0, seen
    assert torch.equal(f2, c.d_loc_flags) and torch.equal(s2, c.d_status)
    assert torch.equal(n2, c.d_nbad)
    c.check_located()


@pytest.mark.parametrize("k,m,nsyn", [(10, 4, 4), (4, 2, 4), (10, 4, 3)])
def test_max_bad_1_is_locate_ptrs(torch, cess, corc, encs, k, m, nsyn):
    """Flags and status byte-equal to cec_locate_ptrs on the locate tests' mixed case, and nbad
    is 1 exactly where the status is FOUND."""
    from cess_amd import _lib
    enc = encs(k, m)
    c = mixed_case(torch, corc, k, m, WG, 1, nsyn)
    assert c.locate(enc) == 0  # cec_locate_ptrs
    c.check_located()
    a = c.addrs(c.big.data_ptr())
    ptrs = (c_void_p * a.size)(*[int(x) or None for x in a.ravel()])
    fl = torch.full_like(c.d_loc_flags, 0x44)
    st = torch.full_like(c.d_status, 0x44)
    nb = torch.full_like(c.d_status, 0x44)
    fn = _lib.load().cec_locate_multi_ptrs
    assert fn(enc._h, ptrs, c.nseg, c.ln, nsyn, 1, fl.data_ptr(), st.data_ptr(), nb.data_ptr(),
              None) == 0
    torch.cuda.synchronize()
    assert torch.equal(fl, c.d_loc_flags) and torch.equal(st, c.d_status)
    assert np.array_equal(nb.cpu().numpy(), (c.want_locate == FOUND).astype(np.uint8))
    # without an nbad vector: the same flags and status
    fl.fill_(0x55)
    st.fill_(0x55)
    assert fn(enc._h, ptrs, c.nseg, c.ln, nsyn, 1, fl.data_ptr(), st.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(fl, c.d_loc_flags) and torch.equal(st, c.d_status)


def test_refusals_write_nothing(torch, cess, corc, encs):
    from cess_amd import _lib
    lib = _lib.load()
    k, m = 4, 4
    enc = encs(k, m)
    c = mixed_pairs(torch, corc, k, m, 16)
    a = c.addrs(c.big.data_ptr())
    ptrs = (c_void_p * a.size)(*[int(x) or None for x in a.ravel()])
    fl, st, nb = c.d_loc_flags.data_ptr(), c.d_status.data_ptr(), c.d_nbad.data_ptr()
    fn = lib.cec_locate_multi_ptrs
    assert fn(enc._h, ptrs, c.nseg, c.ln, 0, 2, fl, st, nb, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, c.nseg, c.ln, 5, 2, fl, st, nb, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, c.nseg, c.ln, 4, 0, fl, st, nb, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, c.nseg, c.ln, 4, 3, fl, st, nb, None) == _lib.CEC_EINVAL
    assert fn(enc._h, None, c.nseg, c.ln, 4, 2, fl, st, nb, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, c.nseg, c.ln, 4, 2, None, st, nb, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, c.nseg, c.ln, 4, 2, fl, None, nb, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, c.nseg, 0, 4, 2, fl, st, nb, None) == _lib.CEC_ESHARDLEN
    assert fn(enc._h, None, 0, c.ln, 4, 2, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert (c.flag_out == 0xEE).all() and (c.status_back == 0xEE).all()
    assert (c.nbad_back == 0xEE).all()
    with pytest.raises(cess.ErrInvalidInput):
        enc.LocateMultiDevice(c.tensors(), nsyn=5)
    with pytest.raises(cess.ErrInvalidInput):
        enc.LocateMultiDevice(c.tensors(), max_bad=3)
    # a NULL d_nbad is legal: flags and status as with one, nbad untouched
    assert c.locate(enc, no_nbad=True) == 0
    c.check_located(nbad=False)
    d_flags, d_status, d_nbad = enc.LocateMultiDevice(c.tensors())  # its own outputs
    torch.cuda.synchronize()
    assert np.array_equal(d_flags.cpu().numpy(), c.want_flags)
    assert np.array_equal(d_status.cpu().numpy(), c.want_locate)
    assert np.array_equal(d_nbad.cpu().numpy(), c.want_nbad)


# ---- composition ----------------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(4, 4), (10, 4)])
def test_locate_repair_multi_restores_and_proves(torch, cess, corc, encs, k, m):
    from cess_amd import audit
    ln, nseg = WG, 8
    held = np.ones((nseg, k + m), bool)
    c = MultiCase(torch, k, m, truth(corc, k, m, ln, nseg), held, 0, seed=11 + k)
    clean_image = c.image.copy()
    kinds = {1: "meet", 2: "one", 3: "disjoint_high", 5: "three", 6: "cancel", 7: "zero"}
    bad = {s: corrupt(c, s, kind) for s, kind in kinds.items()}
    c.upload()
    want = np.zeros(nseg, np.uint8)
    want[list(bad)] = FOUND
    want[5] = AMBIGUOUS
    assert np.array_equal(c.want_locate, want), "three replaced shards are not AMBIGUOUS here"
    healed = clean_image.copy()  # the three-bad segment keeps its bytes
    for j in bad[5]:
        o = c.at(5, j)
        healed[o:o + ln] = c.image[o:o + ln]
    status = np.where(want == FOUND, cess.CEC_FLAG_REBUILT, cess.CEC_FLAG_CLEAN).astype(np.uint8)
    status[5] = cess.CEC_FLAG_LOST
    out = audit.locate_repair_multi_device(encs(k, m), c.tensors(),
                                           recorded=recorded_of(c.full, held))
    d_flags, d_locate, d_status, d_ok, d_confirm = out
    torch.cuda.synchronize()
    assert np.array_equal(d_locate.cpu().numpy(), want)
    assert np.array_equal(d_flags.cpu().numpy(), c.want_flags)
    assert np.array_equal(d_status.cpu().numpy(), status)
    assert np.array_equal(d_confirm.cpu().numpy(), (want == FOUND) * cess.CEC_CONFIRM_PROVEN)
    ok = d_ok.cpu().numpy()
    for s in range(nseg):
        for i in range(k + m):
            rebuilt = want[s] == FOUND and i in bad[s]
            assert ok[s, i] == (1 if rebuilt else cess.CEC_HASHQ_SKIPPED), (s, i)
    assert np.array_equal(c.big.cpu().numpy(), healed), "the original bytes are not back"
    # without records: the three tensors, the same repair
    c.upload()
    out = audit.locate_repair_multi_device(encs(k, m), c.tensors())
    torch.cuda.synchronize()
    assert len(out) == 3 and np.array_equal(out[1].cpu().numpy(), want)
    assert np.array_equal(out[2].cpu().numpy(), status)
    assert np.array_equal(c.big.cpu().numpy(), healed)
