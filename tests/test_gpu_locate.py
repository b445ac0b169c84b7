"""cec_locate_ptrs (Encoder.LocateDevice): the corrupt fragment found from parity alone, on the GPU.

Truth is random data plus its parity from the C oracle, laid out by the Case of
tests/test_gpu_repair_flagged.py: every held shard a view into one allocation between bands of
0xA5, at an offset from a 16-byte boundary. The corruption is written into that image on the host,
and the expected status and flags of every segment are cec_locate_host on the same bytes. After a
call the whole status vector and the whole flag tensor are compared, with the bytes around both
(the flag tensor starts at an odd address), and the allocation equals its image: the call writes
no shard byte."""
import ctypes
from ctypes import c_void_p

import numpy as np
import pytest

from oracle import rs_oracle
from tests import verify_flips
from tests.test_gpu_repair_flagged import Case, cess, encs, torch, truth  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

CLEAN, FOUND, AMBIGUOUS, UNCHECKED = 0, 1, 2, 3
WG = 256 * 8 + 16 + 5  # one workgroup's 8-byte columns, two more columns and a tail of 5 bytes
KINDS = ["clean", "first", "last", "clean", "whole", "two", "tail"]


class LocCase(Case):
    """A Case whose shards all hold the truth until corrupt_*() is called; upload() then copies
    the image to the GPU and computes what cec_locate_host says of every segment."""

    def __init__(self, torch, k, m, full, held, off, seed, nsyn):
        super().__init__(torch, k, m, full, held, np.zeros_like(np.asarray(held)), off, seed)
        self.nsyn = nsyn
        self.rng = np.random.default_rng(seed + 1)
        self.flag_out = torch.full((self.nseg * self.n + 48,), 0xEE, dtype=torch.uint8,
                                   device="cuda")
        self.d_loc_flags = self.flag_out[17:17 + self.nseg * self.n].view(self.nseg, self.n)
        assert self.d_loc_flags.data_ptr() % 2 == 1

    def at(self, s, i):
        assert self.held[s, i]
        return int(self.hidx[s, i]) * self.slot + self.lo

    def flip(self, s, i, x, bit=None):
        bit = int(self.rng.integers(0, 8)) if bit is None else bit
        self.image[self.at(s, i) + x] ^= np.uint8(1 << bit)

    def replace(self, s, i):
        o = self.at(s, i)
        self.image[o:o + self.ln] ^= self.rng.integers(1, 256, self.ln, dtype=np.uint8)

    def corrupt(self, s, i, kind):
        ln = self.ln
        if kind == "first":
            self.flip(s, i, 0)
        elif kind == "last":  # in the byte tail where the length has one
            self.flip(s, i, ln - 1)
        elif kind == "whole":
            self.replace(s, i)
        elif kind == "two":  # the witness is the lower of the two
            self.flip(s, i, (2 * ln) // 3)
            if ln >= 3:
                self.flip(s, i, ln // 3)
        elif kind == "tail":  # the first byte past the last whole 8-byte column
            self.flip(s, i, ln - (ln % 8 or 1))

    def upload(self):
        from cess_amd import _lib
        lib = _lib.load()
        self.big = self.torch.from_numpy(self.image.copy()).cuda()
        base = self.image.ctypes.data
        a = self.addrs(base)
        st, found = ctypes.c_int(), ctypes.c_int()
        self.want_locate = np.zeros(self.nseg, np.uint8)
        self.want_found = np.full(self.nseg, -1, np.int64)
        for s in range(self.nseg):
            ptrs = (c_void_p * self.n)(*[int(x) or None for x in a[s]])
            assert lib.cec_locate_host(self.k, self.m, ptrs, self.ln, self.nsyn,
                                       ctypes.byref(st), ctypes.byref(found)) == 0
            self.want_locate[s], self.want_found[s] = st.value, found.value
        fl = self.held.astype(np.uint8)
        fl[self.want_locate == AMBIGUOUS] = 0
        rows = np.flatnonzero(self.want_locate == FOUND)
        fl[rows, self.want_found[rows]] = 0
        self.want_flags = fl

    def locate(self, enc, stream=None, flags=None, status=None):
        from cess_amd import _lib
        a = self.addrs(self.big.data_ptr())
        ptrs = (c_void_p * a.size)(*[int(x) or None for x in a.ravel()])
        fl = self.d_loc_flags if flags is None else flags
        st = self.d_status if status is None else status
        return _lib.load().cec_locate_ptrs(enc._h, ptrs, self.nseg, self.ln, self.nsyn,
                                           fl.data_ptr(), st.data_ptr(),
                                           None if stream is None else stream.cuda_stream)

    def check_located(self):
        self.torch.cuda.synchronize()
        sb = self.status_back.cpu().numpy()
        assert (sb[:16] == 0xEE).all() and (sb[16 + self.nseg:] == 0xEE).all()
        got = sb[16:16 + self.nseg]
        bad = np.flatnonzero(got != self.want_locate)
        assert bad.size == 0, (bad[:8], got[bad[:8]], self.want_locate[bad[:8]])
        fo = self.flag_out.cpu().numpy()
        nf = self.nseg * self.n
        assert (fo[:17] == 0xEE).all() and (fo[17 + nf:] == 0xEE).all()
        gf = fo[17:17 + nf].reshape(self.nseg, self.n)
        bad = np.argwhere(gf != self.want_flags)
        assert bad.size == 0, bad[:8]
        assert np.array_equal(self.big.cpu().numpy(), self.image), "the call wrote a shard byte"


def held_sets(k, m, rng, null=None):
    """Held sets of the call: all (or all but the shards of `null`), k + 2, k + 1, k shards."""
    n, sets = k + m, []
    for h in (n, k + 2, k + 1, k):
        if h > n or any(int(s.sum()) == h for s in sets):
            continue
        row = np.zeros(n, bool)
        row[rng.choice(n, h, replace=False)] = True
        if h == n:
            row[:] = True
        sets.append(row)
    if null is not None:
        for row in sets:
            row[null] = False
    return sets


def mixed_case(torch, corc, k, m, ln, off, nsyn, null=None):
    rng = np.random.default_rng(k * 131 + m * 17 + ln + off)
    sets = held_sets(k, m, rng, null)
    held = np.array([row for row in sets for _ in KINDS])
    c = LocCase(torch, k, m, truth(corc, k, m, ln, len(held)), held, off,
                seed=k + m + ln + off, nsyn=nsyn)
    for s in range(c.nseg):
        H = np.flatnonzero(held[s])
        # shard 0, parity shards and the rest take their turn as the bad one
        j = H[0] if s % 5 == 0 else H[-1] if s % 5 == 1 else H[(s * 7) % len(H)]
        c.corrupt(s, j, KINDS[s % len(KINDS)])
    c.upload()
    return c


CODES = [
    ("rs4_2", 4, 2, 4, None),          # r = 2, the smallest locating code
    ("rs10_4", 10, 4, 4, None),        # r = 4
    ("rs10_4-nsyn2", 10, 4, 2, None),
    ("rs10_4-nsyn3", 10, 4, 3, None),
    ("rs32_32", 32, 32, 4, None),      # 64 inputs
    ("rs200_56", 200, 56, 4, None),    # the planner's lanes stride past 64
    ("rs2_1", 2, 1, 4, None),          # detect only
    ("rs2_2-null", 2, 2, 4, 1),        # r = 1 by the held set
]


@pytest.mark.parametrize("ln,off", [(1, 0), (15, 0), (16, 0), (WG, 0), (WG, 1)])
@pytest.mark.parametrize("id,k,m,nsyn,null", CODES, ids=[c[0] for c in CODES])
def test_mixed_segments(torch, cess, corc, encs, id, k, m, nsyn, null, ln, off):
    c = mixed_case(torch, corc, k, m, ln, off, nsyn, null)
    seen = set(int(x) for x in c.want_locate)
    if m == 1 or null is not None:
        assert seen == {CLEAN, AMBIGUOUS, UNCHECKED}
    else:
        assert seen == {CLEAN, FOUND, AMBIGUOUS, UNCHECKED}
        # a single bad shard with two or more checks is found, whatever was done to it
        full = np.flatnonzero((c.held.sum(1) >= k + 2) & (c.want_locate != CLEAN))
        assert full.size and (c.want_locate[full] == FOUND).all()
    assert c.locate(encs(k, m)) == 0
    c.check_located()


def test_rows_past_grid_y(torch, cess, corc, encs):
    k, m, ln, nseg = 4, 2, 16, 70000
    held = np.ones((nseg, k + m), bool)
    c = LocCase(torch, k, m, truth(corc, k, m, ln, nseg), held, 0, seed=70, nsyn=4)
    dirty = [0, 1, 65534, 65535, 65536, 69999]
    for t, s in enumerate(dirty):
        c.corrupt(s, t % (k + m), ["first", "last", "whole"][t % 3])
    c.upload()
    assert (c.want_locate[dirty] == FOUND).all() and int((c.want_locate == CLEAN).sum()) == nseg - 6
    assert c.locate(encs(k, m)) == 0
    c.check_located()


def test_every_bit_of_every_shard_is_found(torch, cess, corc, encs):
    """Thousands of copies of one codeword, each with one bit flipped, over every byte of every
    shard (tests/verify_flips.py's plan): every flipped segment is FOUND with its shard, every
    other one CLEAN. The expectation is the plan itself."""
    k, m, ln = 4, 2, 533
    pl = verify_flips.plan(k + m, ln, range(k + m), np.arange(ln))
    one = truth(corc, k, m, ln, 1)
    full = np.ascontiguousarray(np.broadcast_to(one, (pl.nseg, k + m, ln)))
    c = LocCase(torch, k, m, full, np.ones((pl.nseg, k + m), bool), 0, seed=5, nsyn=4)
    o = c.hidx[pl.segment, pl.shard] * c.slot + c.lo + pl.byte
    c.image[o] ^= pl.mask
    c.big = torch.from_numpy(c.image.copy()).cuda()
    c.want_locate = np.zeros(pl.nseg, np.uint8)
    c.want_locate[pl.segment] = FOUND
    c.want_flags = np.ones((pl.nseg, k + m), np.uint8)
    c.want_flags[pl.segment, pl.shard] = 0
    assert pl.nseg > 3000 and len(set(pl.mask)) == 8
    assert c.locate(encs(k, m)) == 0
    c.check_located()


def test_repeats_are_equal_and_hold_nothing(torch, cess, corc, encs):
    from cess_amd import _lib
    k, m = 10, 4
    enc = encs(k, m)
    c = mixed_case(torch, corc, k, m, WG, 0, 4)
    cached = enc.stat(_lib.CEC_STAT_DECODE_CACHED)
    assert c.locate(enc) == 0
    c.check_located()
    f2 = torch.full_like(c.d_loc_flags, 0x33)
    s2 = torch.full_like(c.d_status, 0x33)
    side = torch.cuda.Stream()
    for _ in range(3):  # back to back on another stream, nothing waited for in between
        assert c.locate(enc, stream=side, flags=f2, status=s2) == 0
    torch.cuda.synchronize()
    assert torch.equal(f2, c.d_loc_flags) and torch.equal(s2, c.d_status)
    # a retired block is reused once the launches before its retirement are complete: with the
    # stream drained between calls, the tables of call n + 1 are the retired blocks of call n
    seen = []
    for _ in range(6):
        assert c.locate(enc, stream=side, flags=f2, status=s2) == 0
        torch.cuda.synchronize()
        seen.append(enc.stat(_lib.CEC_STAT_POOL_BYTES))
        assert enc.stat(_lib.CEC_STAT_DECODE_CACHED) == cached
    assert seen[1] == seen[5] and seen[1] > 0, seen
    assert torch.equal(f2, c.d_loc_flags) and torch.equal(s2, c.d_status)
    c.check_located()


def test_refusals_write_nothing(torch, cess, corc, encs):
    from cess_amd import _lib
    lib = _lib.load()
    k, m = 4, 2
    enc = encs(k, m)
    c = mixed_case(torch, corc, k, m, 16, 0, 4)
    a = c.addrs(c.big.data_ptr())
    ptrs = (c_void_p * a.size)(*[int(x) or None for x in a.ravel()])
    fl, st = c.d_loc_flags.data_ptr(), c.d_status.data_ptr()
    fn = lib.cec_locate_ptrs
    assert fn(enc._h, ptrs, c.nseg, c.ln, 0, fl, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, c.nseg, c.ln, 5, fl, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, None, c.nseg, c.ln, 4, fl, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, c.nseg, c.ln, 4, None, st, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, c.nseg, c.ln, 4, fl, None, None) == _lib.CEC_EINVAL
    assert fn(enc._h, ptrs, c.nseg, 0, 4, fl, st, None) == _lib.CEC_ESHARDLEN
    assert fn(enc._h, None, 0, c.ln, 4, None, None, None) == 0
    torch.cuda.synchronize()
    assert (c.flag_out == 0xEE).all() and (c.status_back == 0xEE).all()
    with pytest.raises(cess.ErrInvalidInput):
        enc.LocateDevice(c.tensors(), nsyn=5)
    d_flags, d_status = enc.LocateDevice(c.tensors())  # the Python form, its own outputs
    torch.cuda.synchronize()
    assert np.array_equal(d_flags.cpu().numpy(), c.want_flags)
    assert np.array_equal(d_status.cpu().numpy(), c.want_locate)


# ---- composition ----------------------------------------------------------------------------------

def recorded_of(full, held):
    """Per segment the k + m recorded hashes of the truth (anything where a shard is not held)."""
    return [[rs_oracle.sha256_hex(full[s, i]) if held[s, i] else b"0" * 64
             for i in range(full.shape[1])] for s in range(full.shape[0])]


@pytest.mark.parametrize("k,m", [(4, 2), (10, 4)])
def test_locate_repair_restores_and_proves(torch, cess, corc, encs, k, m):
    from cess_amd import audit
    ln, nseg = WG, 7
    held = np.ones((nseg, k + m), bool)
    if m > 2:
        held[3, 1] = held[6, k] = False  # k + m - 1 held: still two or more checks
    c = LocCase(torch, k, m, truth(corc, k, m, ln, nseg), held, 0, seed=9 + k, nsyn=4)
    clean_image = c.image.copy()
    bad = {1: 0, 3: k + 1, 4: k - 1, 6: 2}
    for t, (s, j) in enumerate(bad.items()):
        c.corrupt(s, j, ["first", "whole", "tail", "two"][t])
    c.upload()
    out = audit.locate_repair_device(encs(k, m), c.tensors(), recorded=recorded_of(c.full, held))
    d_flags, d_locate, d_status, d_ok, d_confirm = out
    torch.cuda.synchronize()
    want = np.zeros(nseg, np.uint8)
    want[list(bad)] = FOUND
    assert np.array_equal(d_locate.cpu().numpy(), want)
    assert np.array_equal(d_flags.cpu().numpy(), c.want_flags)
    assert np.array_equal(d_status.cpu().numpy(), want * cess.CEC_FLAG_REBUILT)
    assert np.array_equal(d_confirm.cpu().numpy(), want * cess.CEC_CONFIRM_PROVEN)
    ok = d_ok.cpu().numpy()
    for s in range(nseg):
        for i in range(k + m):
            assert ok[s, i] == (1 if bad.get(s) == i else cess.CEC_HASHQ_SKIPPED)
    assert np.array_equal(c.big.cpu().numpy(), clean_image), "the original bytes are not back"
    # without records: the three tensors, the same repair
    c.upload()
    out = audit.locate_repair_device(encs(k, m), c.tensors())
    torch.cuda.synchronize()
    assert len(out) == 3 and np.array_equal(out[1].cpu().numpy(), want)
    assert np.array_equal(c.big.cpu().numpy(), clean_image)


def test_scrub_located_rs21_hashes_only_the_dirty(torch, cess, corc, encs):
    from cess_amd import audit
    from cess_amd.hashq import HashQueue
    k, m, ln, nseg = 2, 1, 4101, 8
    held = np.ones((nseg, 3), bool)
    held[6, 0] = False  # two held: unchecked, nothing of it is read or hashed
    c = LocCase(torch, k, m, truth(corc, k, m, ln, nseg), held, 0, seed=21, nsyn=4)
    c.corrupt(2, 1, "first")
    c.corrupt(5, 2, "whole")
    c.upload()
    rec = recorded_of(c.full, held)
    segs = c.tensors()
    seen = []
    with HashQueue(capacity=64, device=0, stream=torch.cuda.current_stream()) as q:
        add = q.add_check_where_ptrs

        def spy(*a, **kw):
            seen.append(kw["d_ok"])
            return add(*a, **kw)
        q.add_check_where_ptrs = spy
        d_flags, d_locate = audit.scrub_located_device(encs(k, m), segs, rec, queue=q)
        frags = [t for seg in segs for t in seg if t is not None]
        hashes = [h for s in range(nseg) for i, h in enumerate(rec[s]) if held[s, i]]
        d_scrub = audit.scrub_device(frags, hashes, queue=q)
        torch.cuda.synchronize()
    want = np.array([CLEAN, CLEAN, AMBIGUOUS, CLEAN, CLEAN, AMBIGUOUS, UNCHECKED, CLEAN], np.uint8)
    assert np.array_equal(d_locate.cpu().numpy(), want)
    scrub = np.zeros((nseg, 3), np.uint8)
    scrub[held] = d_scrub.cpu().numpy()
    flags, ok = d_flags.cpu().numpy(), seen[0].cpu().numpy().reshape(nseg, 3)
    assert len(seen) == 1
    for s in range(nseg):
        if want[s] == AMBIGUOUS:  # hashed: the flags of the hash scrub, which names the shard
            assert np.array_equal(flags[s], scrub[s]) and np.array_equal(ok[s], scrub[s])
            assert list(flags[s]) == [int(not (s == 2 and i == 1 or s == 5 and i == 2))
                                      for i in range(3)]
        else:  # good without a hash
            assert (ok[s] == cess.CEC_HASHQ_SKIPPED).all()
            assert np.array_equal(flags[s], held[s].astype(np.uint8))
            assert np.array_equal(scrub[s], held[s].astype(np.uint8))
    assert np.array_equal(c.big.cpu().numpy(), c.image)
