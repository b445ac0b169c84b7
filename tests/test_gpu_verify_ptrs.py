"""cec_verify_ptrs and its Python forms (VerifyDevice, VerifyDeviceBatch): scattered shards verified
in place by the compare forms of the pointer-table kernels.

Buffer setup of every case: every shard is its own tensor, allocated in shuffled order, and sits
between two 64-byte guard bands of 0xA5 inside its allocation. Survivors (cec_survivors of the
pattern of sources) and expectations hold the C oracle's codeword; sources beyond the k survivors
hold random garbage, so a kernel that read anything but the survivors reports a clean segment as
bad. Every allocation, guard bands included, is snapshotted before each call and compared after
it, so any write fails. d_ok sits between two guard bytes and is pre-filled with 0x5A."""
import ctypes
from ctypes import c_void_p

import numpy as np
import pytest

from oracle.c_oracle import c_encode

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0x5A
_CODEWORDS = {}


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
    """nseg oracle codewords of RS(k, m) with ln-byte shards, computed once per shape and never
    written afterwards."""
    key = (k, m, ln, nseg)
    if key not in _CODEWORDS:
        rng = np.random.default_rng(k * 1000003 + m * 1009 + ln + nseg)
        segs = []
        for _ in range(nseg):
            data = [rng.integers(0, 256, ln, dtype=np.uint8) for _ in range(k)]
            segs.append(data + c_encode(corc, k, m, data))
        _CODEWORDS[key] = segs
    return _CODEWORDS[key]


def survivors(k, m, sources):
    from cess_amd import _lib
    flags = np.zeros(k + m, dtype=np.uint8)
    flags[sorted(sources)] = 1
    out = np.zeros(k, dtype=np.uint8)
    assert _lib.load().cec_survivors(k, m, flags.ctypes.data, out.ctypes.data) == 0
    return [int(i) for i in out]


class Seg:
    """One segment as separate guarded device buffers (see the module docstring): shards in
    `sources` are sources, shards in `expects` expectations, the others do not exist. `off`
    shifts every view by that many bytes (0: 64-byte aligned or better)."""

    def __init__(self, torch, rng, k, m, full, sources, expects, off=0):
        n, ln = k + m, len(full[0])
        assert not set(sources) & set(expects)
        self.k, self.m, self.ln = k, m, ln
        self.sources, self.expects = sorted(sources), sorted(expects)
        # without an expectation nothing is read, and below k sources the call is refused: every
        # source then holds garbage
        self.surv = survivors(k, m, sources) if expects and len(sources) >= k else []
        self.alloc, self.view = {}, {}
        lo = GUARD + off
        for i in rng.permutation(n):
            i = int(i)
            if i not in sources and i not in expects:
                continue
            host = np.full(lo + ln + GUARD, 0xA5, dtype=np.uint8)
            host[lo:lo + ln] = (full[i] if i in expects or i in self.surv
                                else rng.integers(0, 256, ln, dtype=np.uint8))
            self.alloc[i] = torch.from_numpy(host).cuda()
            self.view[i] = self.alloc[i][lo:lo + ln]

    def ptrs(self):
        n = self.k + self.m
        s = [self.view[i].data_ptr() if i in self.sources else None for i in range(n)]
        e = [self.view[i].data_ptr() if i in self.expects else None for i in range(n)]
        return s, e

    def flip(self, shard, pos, mask):
        """XOR one byte of a shard on the device (call again to restore it)."""
        self.view[shard][pos] ^= mask

    def chunk_ends(self):
        """The first and the last expectation of each program chunk: the program's outputs are
        the expectations in ascending order, 32 to a chunk."""
        e = self.expects
        out = []
        for c in range(0, len(e), 32):
            for i in (e[c], e[min(c + 32, len(e)) - 1]):
                if i not in out:
                    out.append(i)
        return out


def verify(torch, enc, segs, ln, scribble=False):
    """cec_verify_ptrs over Seg objects -> (return code, the nseg bytes of d_ok as numpy). Checks
    that no buffer and no guard byte of d_ok changed."""
    from cess_amd import _lib
    src, exp, allocs = [], [], []
    for sg in segs:
        s, e = sg.ptrs()
        src += s
        exp += e
        allocs += list(sg.alloc.values())
    a = (c_void_p * max(1, len(src)))(*src)
    b = (c_void_p * max(1, len(exp)))(*exp)
    okbuf = torch.full((len(segs) + 2,), FILL, dtype=torch.uint8, device="cuda")
    before = torch.cat(allocs)
    rc = _lib.load().cec_verify_ptrs(enc._h, a, b, len(segs), ln, okbuf[1:].data_ptr(), None)
    if scribble:  # the arrays belong to the caller again
        ctypes.memset(a, 0xFF, ctypes.sizeof(a))
        ctypes.memset(b, 0xFF, ctypes.sizeof(b))
    torch.cuda.synchronize()
    assert torch.equal(before, torch.cat(allocs)), "a shard or a guard band was written"
    ok = okbuf.cpu().numpy()
    assert ok[0] == FILL and ok[-1] == FILL, "d_ok guard byte written"
    return rc, ok[1:-1]


def flip_positions(ln):
    """(byte, mask): one bit of byte 0, the last byte of the shard, and for each column width of
    the kernels (16, 8, 4 bytes) the last byte of the vector region and the first of the tail."""
    pos = [(0, 0x01)]
    for vb in (16, 8, 4):
        vec = ln - ln % vb
        for p in (vec - 1, vec):
            if 0 < p < ln and p not in [q for q, _ in pos]:
                pos.append((p, 0xFF))
    if ln - 1 not in [q for q, _ in pos]:
        pos.append((ln - 1, 0xFF))
    return pos


def segment_specs(k, m):
    """Five (sources, expectations) and the segments whose shards get flipped. RS(2,1): the
    encode and both closed forms of a lost data fragment in one call. Other codes: klauspost's
    Verify (every parity shard from the data shards: m expectations) three times, and data shard 0
    checked against all the others (one expectation; the sources beyond the k survivors hold
    garbage). Segment 2 has no expectation."""
    n = k + m
    if (k, m) == (2, 1):
        return [({0, 1}, {2}), ({1, 2}, {0}), ({0, 1, 2}, set()), ({0, 2}, {1}),
                ({0, 1}, {2})], [0, 1, 3]
    kp = (set(range(k)), set(range(k, n)))
    return [kp, kp, (set(range(n)), set()), kp, (set(range(1, n)), {0})], [1, 4]


# (k, m, CEC_OPT_FORCE_GENERIC): RS(2,1) the compile-time tile, cases 0 / 1 / 2; forced generic the
# mask kernel over 2 inputs; RS(4,2), RS(10,4) the bit-plane kernel, buckets 2 and 4, and bucket 1
# for the single expectation; RS(3,5) the mask kernel with 16-byte columns; RS(6,8) 8-byte
# columns; RS(9,11) bucket 12; RS(20,17) bucket 24, 4-byte columns; RS(32,32) bucket 32; RS(5,37)
# two program chunks of 32 + 5 outputs
CODES = [(2, 1, 0), (2, 1, 1), (4, 2, 0), (10, 4, 0), (3, 5, 0), (6, 8, 0), (9, 11, 0),
         (20, 17, 0), (32, 32, 0), (5, 37, 0)]
# (shard length, view offset): offset 3 takes the whole-call byte path
SHAPES = [(1, 0), (7, 0), (8, 0), (15, 0), (16, 0), (17, 0), (4096, 0), (4096 + 13, 0),
          (17, 3), (4096 + 13, 3)]


@pytest.mark.parametrize("ln,off", SHAPES)
@pytest.mark.parametrize("k,m,generic", CODES)
def test_clean_and_corrupt(torch, cess, corc, k, m, generic, ln, off):
    from cess_amd import _lib
    nseg = 5
    rng = np.random.default_rng(1000 * k + 10 * m + generic + ln + off)
    full = codewords(corc, k, m, ln, nseg)
    enc = cess.New(k, m)
    if generic:
        enc.set_option(_lib.CEC_OPT_FORCE_GENERIC, 1)
    specs, flip_segs = segment_specs(k, m)
    segs = [Seg(torch, rng, k, m, full[s], src, exp, off) for s, (src, exp) in enumerate(specs)]
    # clean codewords, the host arrays overwritten right after the return
    rc, ok = verify(torch, enc, segs, ln, scribble=True)
    assert rc == 0 and ok.tolist() == [1] * nseg, ("clean", rc, ok)
    # one flip per call: in the first and the last expectation of each chunk and in one survivor
    for s in flip_segs:
        sg = segs[s]
        for shard in sg.chunk_ends() + [sg.surv[len(sg.surv) // 2]]:
            for pos, mask in flip_positions(ln):
                sg.flip(shard, pos, mask)
                rc, ok = verify(torch, enc, segs, ln)
                sg.flip(shard, pos, mask)
                want = [0 if t == s else 1 for t in range(nseg)]
                assert rc == 0 and ok.tolist() == want, ("flip", s, shard, pos, rc, ok)
    # two corrupted segments in one call
    for s in (1, 3):
        segs[s].flip(segs[s].expects[0], ln - 1, 0xFF)
    rc, ok = verify(torch, enc, segs, ln)
    assert rc == 0 and ok.tolist() == [1, 0, 1, 0, 1], ("two corrupted", rc, ok)
    for s in (1, 3):
        segs[s].flip(segs[s].expects[0], ln - 1, 0xFF)
    rc, ok = verify(torch, enc, segs, ln)
    assert rc == 0 and ok.tolist() == [1] * nseg, ("restored", rc, ok)


def test_grid_chunking(torch, cess, corc):
    """65,540 RS(2,1) segments of 16 bytes, all aliasing the same three buffers, past the
    65,535-row split of a launch; only the last one expects a corrupted parity."""
    from cess_amd import _lib
    k, m, ln, nseg = 2, 1, 16, 65540
    full = codewords(corc, k, m, ln, 1)[0]
    d0, d1, p = [torch.from_numpy(full[i].copy()).cuda() for i in range(3)]
    bad = p.clone()
    bad[5] ^= 0x10
    bufs = [d0, d1, p, bad]
    src = [d0.data_ptr(), d1.data_ptr(), None] * nseg
    exp = [None, None, p.data_ptr()] * nseg
    exp[-1] = bad.data_ptr()
    a, b = (c_void_p * len(src))(*src), (c_void_p * len(exp))(*exp)
    okbuf = torch.full((nseg + 2,), FILL, dtype=torch.uint8, device="cuda")
    before = torch.cat(bufs)
    enc = cess.New(k, m)
    assert _lib.load().cec_verify_ptrs(enc._h, a, b, nseg, ln, okbuf[1:].data_ptr(), None) == 0
    torch.cuda.synchronize()
    ok = okbuf.cpu().numpy()
    assert ok[0] == FILL and ok[-1] == FILL
    assert (ok[1:-2] == 1).all() and ok[-2] == 0, np.flatnonzero(ok[1:-1] != 1)[:8]
    assert torch.equal(before, torch.cat(bufs))


@pytest.mark.parametrize("rt_mode", [None, 1])
def test_grid_chunking_run_time_rows(torch, cess, corc, rt_mode):
    """65,537 RS(4,2) segments of 16 bytes, all aliasing the same buffers, past the 65,535-row
    split of a launch: data shard 0 expected from the four survivors, by k_ptrb<1> and, with
    CEC_OPT_RT_MODE 1, by k_ptrt<1>; only the last segment expects a copy with one flipped bit."""
    from cess_amd import _lib
    k, m, ln, nseg = 4, 2, 16, 65537
    n = k + m
    full = codewords(corc, k, m, ln, 1)[0]
    surv = [torch.from_numpy(full[i].copy()).cuda() for i in range(1, k + 1)]
    good = torch.from_numpy(full[0].copy()).cuda()
    bad = good.clone()
    bad[5] ^= 0x10
    bufs = surv + [good, bad]
    src = ([None] + [t.data_ptr() for t in surv] + [None] * (m - 1)) * nseg
    exp = ([good.data_ptr()] + [None] * (n - 1)) * nseg
    exp[-n] = bad.data_ptr()
    a, b = (c_void_p * len(src))(*src), (c_void_p * len(exp))(*exp)
    okbuf = torch.full((nseg + 2,), FILL, dtype=torch.uint8, device="cuda")
    before = torch.cat(bufs)
    enc = cess.New(k, m)
    if rt_mode is not None:
        enc.set_option(_lib.CEC_OPT_RT_MODE, rt_mode)
    assert _lib.load().cec_verify_ptrs(enc._h, a, b, nseg, ln, okbuf[1:].data_ptr(), None) == 0
    torch.cuda.synchronize()
    ok = okbuf.cpu().numpy()
    assert ok[0] == FILL and ok[-1] == FILL
    assert (ok[1:-2] == 1).all() and ok[-2] == 0, np.flatnonzero(ok[1:-1] != 1)[:8]
    assert torch.equal(before, torch.cat(bufs))


@pytest.mark.parametrize("k,m", [(2, 1), (10, 4), (32, 32)])
def test_agrees_with_verify_batch(torch, cess, corc, k, m):
    """The addresses of a batch, some of its segments corrupt, handed to cec_verify_ptrs: d_ok
    equals cec_verify_batch's on the same batch."""
    from cess_amd import _lib
    n, nseg, ln = k + m, 6, 1024
    full = codewords(corc, k, m, ln, nseg)
    host = np.stack([np.stack(full[s]) for s in range(nseg)])
    host[1, k, 0] ^= 1  # first parity shard, first byte
    host[2, n - 1, ln - 1] ^= 0x80  # last parity shard, last byte
    host[4, k - 1, ln // 2] ^= 0xFF  # a data shard
    d_data = torch.from_numpy(host[:, :k].copy()).cuda()
    d_par = torch.from_numpy(host[:, k:].copy()).cuda()
    enc = cess.New(k, m)
    want = enc.VerifyBatch(d_data, d_par, nseg, ln)
    assert [bool(x) for x in want] == [True, False, False, True, False, True]
    src, exp = [], []
    for s in range(nseg):
        src += [d_data[s, i].data_ptr() for i in range(k)] + [None] * m
        exp += [None] * k + [d_par[s, o].data_ptr() for o in range(m)]
    a, b = (c_void_p * len(src))(*src), (c_void_p * len(exp))(*exp)
    d_ok = torch.full((nseg,), FILL, dtype=torch.uint8, device="cuda")
    snap = (d_data.clone(), d_par.clone())
    assert _lib.load().cec_verify_ptrs(enc._h, a, b, nseg, ln, d_ok.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert [bool(x) for x in d_ok.cpu().numpy()] == [bool(x) for x in want]
    assert torch.equal(d_data, snap[0]) and torch.equal(d_par, snap[1])


def test_validation_writes_nothing(torch, cess, corc):
    from cess_amd import _lib
    lib = _lib.load()
    k, m, nseg, ln = 4, 2, 3, 1000
    n = k + m
    rng = np.random.default_rng(4242)
    full = codewords(corc, k, m, ln, nseg)
    enc = cess.New(k, m)
    kp = (set(range(k)), set(range(k, n)))

    def refused(segs, length, code, what):
        rc, ok = verify(torch, enc, segs, length)
        assert rc == code, (what, rc)
        assert (ok == FILL).all(), (what, "d_ok written")

    segs = [Seg(torch, rng, k, m, full[s], *kp) for s in range(nseg)]
    # fewer than k sources with an expectation, in the middle segment
    few = list(segs)
    few[1] = Seg(torch, rng, k, m, full[1], {0, 1, 2}, {4, 5})
    refused(few, ln, _lib.CEC_ETOOFEW, "too few")
    # the same segment without an expectation is no error: flag 1, as a segment with no destination
    # in cec_reconstruct_ptrs
    few[1] = Seg(torch, rng, k, m, full[1], {0, 1, 2}, set())
    rc, ok = verify(torch, enc, few, ln)
    assert rc == 0 and ok.tolist() == [1, 1, 1]
    refused(segs, 0, _lib.CEC_ESHARDLEN, "shard_len 0")
    # a shard that is both a source and an expectation
    src, exp = [], []
    for sg in segs:
        s_, e_ = sg.ptrs()
        src += s_
        exp += e_
    both = list(src)
    both[2 * n + k] = exp[2 * n + k]
    d_ok = torch.full((nseg,), FILL, dtype=torch.uint8, device="cuda")
    a, b = (c_void_p * len(src))(*src), (c_void_p * len(exp))(*exp)
    ab = (c_void_p * len(both))(*both)
    calls = [("both", (ab, b, nseg, ln, d_ok.data_ptr()), _lib.CEC_EINVAL),
             ("null src", (None, b, nseg, ln, d_ok.data_ptr()), _lib.CEC_EINVAL),
             ("null expect", (a, None, nseg, ln, d_ok.data_ptr()), _lib.CEC_EINVAL),
             ("null d_ok", (a, b, nseg, ln, None), _lib.CEC_EINVAL),
             ("nseg 0", (a, b, 0, ln, d_ok.data_ptr()), _lib.CEC_OK),
             ("nseg 0, all null", (None, None, 0, ln, None), _lib.CEC_OK)]
    for what, args, code in calls:
        assert lib.cec_verify_ptrs(enc._h, *args, None) == code, what
        torch.cuda.synchronize()
        assert bool((d_ok == FILL).all()), (what, "d_ok written")
    # and the arrays are fine: the same call goes through
    assert lib.cec_verify_ptrs(enc._h, a, b, nseg, ln, d_ok.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [1, 1, 1]


def test_shares_the_decode_cache_with_the_rebuild(torch, cess, corc):
    """A rebuild and a verify of one pattern (required mask = expectation mask): one cache entry."""
    from cess_amd import _lib
    lib = _lib.load()
    k, m, ln = 10, 4, 256
    n = k + m
    full = codewords(corc, k, m, ln, 1)[0]
    enc = cess.New(k, m)
    dev = [torch.from_numpy(full[i].copy()).cuda() for i in range(n)]
    lost, wanted = [1, 11], 11
    src = [None if i in lost else dev[i].data_ptr() for i in range(n)]
    out = torch.zeros(ln, dtype=torch.uint8, device="cuda")
    dst = [out.data_ptr() if i == wanted else None for i in range(n)]
    exp = [dev[i].data_ptr() if i == wanted else None for i in range(n)]
    a = (c_void_p * n)(*src)
    before = enc.stat(_lib.CEC_STAT_DECODE_CACHED)
    assert lib.cec_reconstruct_ptrs(enc._h, a, (c_void_p * n)(*dst), 1, ln, None) == 0
    assert enc.stat(_lib.CEC_STAT_DECODE_CACHED) == before + 1
    d_ok = torch.full((1,), FILL, dtype=torch.uint8, device="cuda")
    assert lib.cec_verify_ptrs(enc._h, a, (c_void_p * n)(*exp), 1, ln, d_ok.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert enc.stat(_lib.CEC_STAT_DECODE_CACHED) == before + 1
    assert d_ok.cpu().tolist() == [1]
    assert np.array_equal(out.cpu().numpy(), full[wanted])


# ---- Python forms --------------------------------------------------------------------------------


@pytest.mark.parametrize("k,m", [(2, 1), (10, 4)])
def test_verify_device(torch, cess, corc, k, m):
    n, ln = k + m, 2049
    full = codewords(corc, k, m, ln, 1)[0]
    enc = cess.New(k, m)
    shards = [torch.from_numpy(full[i].copy()).cuda() for i in range(k)]
    shards += [torch.zeros(ln, dtype=torch.uint8, device="cuda") for _ in range(m)]
    enc.EncodeDevice(shards)
    assert enc.VerifyDevice(shards) is True
    for i in range(n):  # one byte of any shard
        pos = (37 * i + 5) % ln
        shards[i][pos] ^= 0x04
        assert enc.VerifyDevice(shards) is False, i
        shards[i][pos] ^= 0x04
    assert enc.VerifyDevice(shards) is True
    with pytest.raises(cess.ErrTooFewShards):
        enc.VerifyDevice(shards[:-1])
    with pytest.raises(cess.ErrShardNoData):
        enc.VerifyDevice(shards[:-1] + [None])
    with pytest.raises(cess.ErrShardNoData):
        enc.VerifyDevice(shards[:-1] + [torch.empty(0, dtype=torch.uint8, device="cuda")])
    with pytest.raises(cess.ErrShardSize):
        enc.VerifyDevice(shards[:-1] + [shards[-1][:-1]])


@pytest.mark.parametrize("handle", ["stream", "int"])
def test_verify_device_on_a_side_stream(torch, cess, corc, handle):
    """VerifyDevice enqueued on a stream that is not torch's current one, as a torch.cuda.Stream
    and as its raw handle, behind work that keeps that stream busy: the flag is read only after
    that stream has passed the verify, so a corrupted shard is never reported verified."""
    k, m, ln = 4, 2, 4096 + 13
    full = codewords(corc, k, m, ln, 1)[0]
    enc = cess.New(k, m)
    shards = [torch.from_numpy(full[i].copy()).cuda() for i in range(k + m)]
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    arg = side if handle == "stream" else side.cuda_stream
    busy = torch.ones(1 << 28, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the shards are in place before the side stream reads them
    for i, want in ((None, True), (k, False), (0, False), (None, True)):
        if i is not None:
            shards[i][ln - 1] ^= 0x20
            torch.cuda.synchronize()
        with torch.cuda.stream(side):  # some milliseconds of work ahead of the verify
            for _ in range(16):
                busy.add_(1)
        got = enc.VerifyDevice(shards, stream=arg)
        assert got is want, (handle, i, got)
        if i is not None:
            shards[i][ln - 1] ^= 0x20
            torch.cuda.synchronize()


def test_verify_device_batch_refuses_strided_and_foreign_tensors(torch, cess, corc):
    """d_ok must be nseg consecutive bytes on the codec's GPU, shards contiguous device tensors:
    the library writes and reads at their addresses."""
    k, m, ln, nseg = 2, 1, 64, 2
    full = codewords(corc, k, m, ln, nseg)
    enc = cess.New(k, m)
    segs = [[torch.from_numpy(full[s][i].copy()).cuda() for i in range(k + m)]
            for s in range(nseg)]
    buf = torch.full((2 * nseg,), FILL, dtype=torch.uint8, device="cuda")
    for bad in (buf[::2], torch.zeros(nseg, dtype=torch.uint8), buf[:nseg].view(1, nseg),
                torch.zeros(nseg, dtype=torch.int8, device="cuda"), buf[:nseg + 1]):
        with pytest.raises(cess.ErrInvalidInput):
            enc.VerifyDeviceBatch(segs, d_ok=bad)
    wide = torch.from_numpy(np.repeat(full[0][2], 2)).cuda()
    for bad in (wide[::2], torch.from_numpy(full[0][2].copy())):
        with pytest.raises(TypeError):
            enc.VerifyDeviceBatch([[segs[0][0], segs[0][1], bad], segs[1]], d_ok=buf[:nseg])
    torch.cuda.synchronize()
    assert bool((buf == FILL).all()), "a refused call wrote d_ok"
    assert enc.VerifyDeviceBatch(segs, d_ok=buf[:nseg]) is not None
    assert buf.cpu().tolist() == [1, 1, FILL, FILL]


def test_verify_device_batch_check_flags(torch, cess, corc):
    """The RS(4,2) example of the header: d1 lost, p1 checked against d0, d2, d3 and p0."""
    k, m, ln, nseg = 4, 2, 1500, 3
    full = codewords(corc, k, m, ln, nseg)
    enc = cess.New(k, m)
    segments = []
    for s in range(nseg):
        sh = [torch.from_numpy(full[s][i].copy()).cuda() for i in range(k + m)]
        sh[1] = None
        segments.append(sh)
    flags = [False, False, False, False, False, True]
    ok = enc.VerifyDeviceBatch(segments, check=[flags] * nseg)
    assert ok.cpu().tolist() == [1, 1, 1]
    segments[1][5][ln - 1] ^= 1  # the checked shard
    segments[2][4][0] ^= 1  # a survivor
    d_ok = torch.full((nseg,), FILL, dtype=torch.uint8, device="cuda")
    got = enc.VerifyDeviceBatch(segments, check=[flags] * nseg, d_ok=d_ok)
    assert got is d_ok
    assert d_ok.cpu().tolist() == [1, 0, 0]
    # check None for a segment: its present parity shards from its present data shards, which
    # are fewer than k here
    with pytest.raises(cess.ErrTooFewShards):
        enc.VerifyDeviceBatch(segments, check=[flags, flags, None])
    # whole segments without flags: klauspost's Verify per segment
    whole = [[torch.from_numpy(full[s][i].copy()).cuda() for i in range(k + m)]
             for s in range(nseg)]
    whole[2][0][7] ^= 0x40
    assert enc.VerifyDeviceBatch(whole).cpu().tolist() == [1, 1, 0]
    with pytest.raises(cess.ErrTooFewShards):
        enc.VerifyDeviceBatch([whole[0][:-1]])
    with pytest.raises(cess.ErrInvalidInput):
        enc.VerifyDeviceBatch(whole, check=[flags])
