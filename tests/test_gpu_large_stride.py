"""Kernels at their documented large-geometry limits: the RS(32,32) FFT-domain decoders at the
last shard stride they take (32-bit buffer offsets over a coset: 2^26 - 1024) and the matrix
fallback at 2^26, cec_xor_batch past 2^32 bytes on the 16-byte and on the byte path, and
cec_fill_synthetic past 2^32 bytes in total and inside one segment.

The decoder batches are column-periodic (tests/large_geom.py): a shard is a 7168-byte window tiled
along its length, the C oracle runs on the windows, and every byte in HBM is compared with the
tiled expectation. Outputs start as poison and every array lies between checked guard bands. At
most 19.3 GiB of HBM at once; a test skips only when mem_get_info reports less than its need. On
an MI355X every test takes under a second and the file about 10 s."""
import os

import numpy as np
import pytest

from tests import large_geom as lg

pytestmark = pytest.mark.gpu

MiB, GiB = 1 << 20, 1 << 30
JUNK = 0xA5


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


def need_hbm(torch, nbytes):
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"needs {nbytes / GiB:.1f} GiB of HBM, {free / GiB:.1f} GiB free")


def alloc_on(torch):
    return lambda n: torch.empty(n, dtype=torch.uint8, device="cuda")


# ---- D: the FFT-domain decoders at their stride limit --------------------------------------------

class Wide:
    """RS(32,32) segments of F-byte shards, column-periodic, a different window per segment."""
    k = m = 32

    def __init__(self, torch, corc, F, nseg):
        self.torch, self.F, self.nseg = torch, F, nseg
        win = np.random.default_rng(F % 251 + nseg).integers(0, 256, (nseg, 32, lg.W),
                                                             dtype=np.uint8)
        pwin = np.empty_like(win)
        corc.orc_encode_batch(32, 32, win.ctypes.data, pwin.ctypes.data, nseg, lg.W,
                              min(16, os.cpu_count() or 1), 1)
        self.win = torch.from_numpy(np.concatenate([win, pwin], axis=1)).cuda()  # [nseg][64][W]
        self.data = lg.Guarded(alloc_on(torch), nseg * 32 * F, fill=lg.POISON)
        self.par = lg.Guarded(alloc_on(torch), nseg * 32 * F, fill=lg.POISON)
        self.data3 = self.data.arr.view(nseg, 32, F)
        self.par3 = self.par.arr.view(nseg, 32, F)
        for s in range(nseg):
            for r in range(0, 32, 8):
                self.data3[s, r:r + 8] = lg.tile_columns(self.win[s, r:r + 8], F)

    def shard(self, s, j):
        return self.data3[s, j] if j < 32 else self.par3[s, j - 32]

    def erase(self, present):
        """present [nseg][64]: junk in every absent shard."""
        for s in range(self.nseg):
            for j in np.flatnonzero(present[s] == 0):
                self.shard(s, int(j))[:] = JUNK

    def check(self, what, data=True):
        self.torch.cuda.synchronize()
        assert self.data.guards_ok() and self.par.guards_ok(), (what, "a guard band was written")
        for s in range(self.nseg):
            if data:
                assert lg.column_mismatch(self.data3[s], self.win[s, :32]) == [], (what, "data", s)
            assert lg.column_mismatch(self.par3[s], self.win[s, 32:]) == [], (what, "parity", s)


@pytest.fixture(scope="module")
def wide(torch, corc):
    """One Wide batch at a time: (F, nseg) -> the batch, the previous one freed first."""
    held = {}

    def get(F, nseg):
        if (F, nseg) not in held:
            held.clear()
            # both arrays, a tiled 8-row piece and its comparison, the windows
            need_hbm(torch, 2 * nseg * 32 * F + 24 * F + 1 * GiB)
            held[(F, nseg)] = Wide(torch, corc, F, nseg)
        return held[(F, nseg)]
    yield get
    held.clear()
    torch.cuda.empty_cache()


F_LIMIT = (1 << 26) - 1024  # the last multiple of 1024 below the decoders' stride bound


def wide_erasures(ne, seed):
    """ne erasures: 8 on both sides at random, 32 split evenly (never a plain re-encode)."""
    rng = np.random.default_rng(seed)
    p = np.ones(64, np.uint8)
    if ne == 32:
        p[rng.choice(32, size=16, replace=False)] = 0
        p[32 + rng.choice(32, size=16, replace=False)] = 0
    else:
        p[rng.choice(64, size=ne, replace=False)] = 0
    return p


def test_d_geometry():
    # a coset of 32 shards spans 2^31 - 32 KiB; segment 2 starts 64 KiB below 2^32
    assert 32 * F_LIMIT == (1 << 31) - 32 * 1024 and 2 * 32 * F_LIMIT == (1 << 32) - 64 * 1024
    assert F_LIMIT % 1024 == 0 and F_LIMIT + 1024 == 1 << 26


def test_d_fft_encode_at_the_stride_limit(torch, cess, wide):
    b = wide(F_LIMIT, 3)
    enc = cess.New(32, 32)
    b.par.arr[:] = lg.POISON
    enc.EncodeBatch(b.data.arr, b.par.arr, b.nseg, b.F)
    b.check("encode")
    assert enc.VerifyBatch(b.data.arr, b.par.arr, b.nseg, b.F).all()


@pytest.mark.parametrize("ne", [8, 32])
@pytest.mark.parametrize("mode", [1, 2])
def test_d_fft_decoders_at_the_stride_limit(torch, cess, wide, mode, ne):
    """Syndrome rows (1) and formal derivative (2): 2 * 15 * stride + column + 512 comes within
    32 KiB of 2^31 in the 32-bit buffer offsets. One pattern for all segments, then one each."""
    b = wide(F_LIMIT, 3)
    enc = cess.New(32, 32)
    enc.EncodeBatch(b.data.arr, b.par.arr, b.nseg, b.F)  # the truth the rebuilds start from
    enc.set_option(8, mode)
    pats = np.stack([wide_erasures(ne, 100 * ne + s) for s in range(b.nseg)])
    for what, present in (("one pattern", pats[0]), ("per segment", pats)):
        b.erase(present if present.ndim == 2 else np.stack([present] * b.nseg))
        b4, b5 = enc.stat(4), enc.stat(5)
        enc.ReconstructBatch(b.data.arr, b.par.arr, b.nseg, b.F, present)
        b.check((what, mode, ne))
        assert enc.stat(4) - b4 == b.nseg, (what, "not on the FFT-domain decoders")
        assert enc.stat(5) - b5 == (b.nseg if mode == 2 else 0), what


@pytest.mark.parametrize("ne", [8, 32])
@pytest.mark.parametrize("mode", [1, 2])
def test_d_matrix_fallback_at_64_mib(torch, cess, wide, mode, ne):
    """shard_len = 2^26: the decoders' offsets would not fit, so the run-time matrix kernels
    rebuild whatever CEC_OPT_FFTDEC_MODE asks for, and the counters do not move."""
    b = wide(1 << 26, 1)
    enc = cess.New(32, 32)
    b.par.arr[:] = lg.POISON
    enc.EncodeBatch(b.data.arr, b.par.arr, b.nseg, b.F)
    b.check("encode")
    enc.set_option(8, mode)
    pats = np.stack([wide_erasures(ne, 100 * ne)])
    for what, present in (("one pattern", pats[0]), ("per segment", pats)):
        b.erase(pats)
        b4, b5 = enc.stat(4), enc.stat(5)
        enc.ReconstructBatch(b.data.arr, b.par.arr, b.nseg, b.F, present)
        b.check((what, mode, ne))
        assert (enc.stat(4), enc.stat(5)) == (b4, b5), what


# ---- E: cec_xor_batch past 2^32 ------------------------------------------------------------------

XOR_CHUNK = lg.W << 17  # 0.875 GiB, a whole number of windows


@pytest.mark.parametrize("length,nsrc,offset", [((1 << 32) + 4096, 2, 0), ((1 << 32) + 3, 1, 1)],
                         ids=["vec16", "bytes"])
def test_e_xor_batch_past_4_gib(torch, cess, length, nsrc, offset):
    """16-byte columns (everything aligned, two sources a stride of `length` apart), and the byte
    path (dst and src one byte off alignment): 2^24 + 1 blocks of 256 if launched as one grid,
    more work items than HIP takes in x, so the launcher caps the grid and the lanes stride."""
    need_hbm(torch, (1 + nsrc) * length + 4 * XOR_CHUNK + 1 * GiB)
    dst = lg.Guarded(alloc_on(torch), length, offset=offset)
    src = lg.Guarded(alloc_on(torch), nsrc * length, offset=offset)
    assert (dst.arr.data_ptr() % 16, src.arr.data_ptr() % 16) == (offset, offset)
    # dst starts column-periodic (a read 2^j bytes off is not the same bytes), sources random
    win = torch.from_numpy(np.random.default_rng(5).integers(0, 256, lg.W, dtype=np.uint8)).cuda()
    dst0 = lg.tile_columns(win, XOR_CHUNK)
    for c in range(0, length, XOR_CHUNK):
        n = min(XOR_CHUNK, length - c)
        dst.arr[c:c + n] = dst0[:n]
    src.arr.random_(0, 256)
    cess.xor_batch(dst.arr, src.arr, nsrc, length, length)
    torch.cuda.synchronize()
    assert dst.guards_ok() and src.guards_ok()
    for c in range(0, length, XOR_CHUNK):
        n = min(XOR_CHUNK, length - c)
        want = dst0[:n].clone()
        for j in range(nsrc):
            want.bitwise_xor_(src.arr[j * length + c:j * length + c + n])
        assert torch.equal(dst.arr[c:c + n], want), ("chunk at", c)


def test_e_acc_shard_len_bound(cess):
    """cec_encode_idx_batch / cec_update_batch launch their byte path as ceil(shard_len / 256)
    blocks of 256 in x, so they refuse a shard_len whose grid HIP would refuse: > 2^32 - 256."""
    from cess_amd import _lib
    from cess_amd.reedsolomon import CecError
    enc = cess.New(2, 1)
    enc.EncodeIdxBatch(0, 0, 0, 0, 0, (1 << 32) - 256)  # nseg = 0: validated, nothing to do
    enc.UpdateBatch(0, 0, 0, 0, (1 << 32) - 256, [1, 0])
    for call in (lambda: enc.EncodeIdxBatch(0, 0, 0, 0, 0, (1 << 32) - 255),
                 lambda: enc.UpdateBatch(0, 0, 0, 0, (1 << 32) - 255, [1, 0])):
        with pytest.raises(CecError) as e:
            call()
        assert e.value.code == _lib.CEC_EINVAL and "shard_len too large" in str(e.value)


# ---- F: cec_fill_synthetic -----------------------------------------------------------------------

SEED = 0xCE550009


def synthetic_bytes(orc, seg_bytes, seg0, lo, hi):
    """Bytes [lo, hi) (multiples of 8) of contiguous synthetic segments from seg0, by the numpy
    oracle: word w of segment s = splitmix64(seed ^ (s << 32) ^ w)."""
    i = np.arange(lo // 8, hi // 8, dtype=np.uint64)
    wps = np.uint64(seg_bytes // 8)
    s, w = i // wps + np.uint64(seg0), i % wps
    return orc.splitmix64(np.uint64(SEED) ^ (s << np.uint64(32)) ^ w).astype("<u8").view(np.uint8)


def check_windows(orc, g, seg_bytes, seg0, total):
    half = 4096
    for mid in (half, 1 << 31, 1 << 32, total - half):
        lo, hi = mid - half, mid + half
        got = g.arr[lo:hi].cpu().numpy()
        assert np.array_equal(got, synthetic_bytes(orc, seg_bytes, seg0, lo, hi)), ("window", mid)


def test_f_fill_synthetic_many_segments(torch, cess, orc):
    """520 segments of 16 MiB (8.125 GiB): windows against the oracle, and every byte against two
    half fills whose second half starts at seg0 + 260 and at byte 0 of its own launch."""
    seg_bytes, nseg, seg0 = 16 * MiB, 520, 5
    total = seg_bytes * nseg
    need_hbm(torch, 2 * total + 3 * GiB)
    a = lg.Guarded(alloc_on(torch), total, fill=lg.POISON)
    cess.fill_synthetic(a.arr, seg_bytes, nseg, seg0, SEED)
    torch.cuda.synchronize()
    assert a.guards_ok()
    check_windows(orc, a, seg_bytes, seg0, total)
    b = lg.Guarded(alloc_on(torch), total, fill=lg.POISON)
    cess.fill_synthetic(b.arr, seg_bytes, nseg // 2, seg0, SEED)
    cess.fill_synthetic(b.arr[total // 2:], seg_bytes, nseg // 2, seg0 + nseg // 2, SEED)
    torch.cuda.synchronize()
    assert b.guards_ok()
    for c in range(0, total, GiB):
        assert torch.equal(a.arr[c:c + GiB], b.arr[c:c + GiB]), ("GiB", c >> 30)


def torch_splitmix(torch, seg, w0, n):
    """splitmix64(SEED ^ (seg << 32) ^ w) for w in [w0, w0 + n) in wrapping int64 arithmetic (a
    logical right shift is an arithmetic one with the sign copies masked off)."""
    def s64(x):
        return x - (1 << 64) if x >= 1 << 63 else x

    def shr(z, b):
        return (z >> b) & ((1 << (64 - b)) - 1)
    w = torch.arange(w0, w0 + n, dtype=torch.int64, device="cuda")
    z = (w ^ s64(SEED ^ (seg << 32))) + s64(0x9E3779B97F4A7C15)
    z = (z ^ shr(z, 30)) * s64(0xBF58476D1CE4E5B9)
    z = (z ^ shr(z, 27)) * s64(0x94D049BB133111EB)
    return z ^ shr(z, 31)


def test_f_fill_synthetic_one_huge_segment(torch, cess, orc):
    """One segment of 2^32 + 4096 bytes (word indices past 2^29): windows against the numpy
    oracle, every word against splitmix64 re-derived in torch, and the halves differ."""
    seg_bytes, seg0 = (1 << 32) + 4096, 3
    need_hbm(torch, seg_bytes + 2 * GiB)
    a = lg.Guarded(alloc_on(torch), seg_bytes, fill=lg.POISON)
    cess.fill_synthetic(a.arr, seg_bytes, 1, seg0, SEED)
    torch.cuda.synchronize()
    assert a.guards_ok()
    check_windows(orc, a, seg_bytes, seg0, seg_bytes)
    # the re-derivation agrees with the numpy oracle where both are computed
    w0 = (1 << 29) - 8
    ref = synthetic_bytes(orc, seg_bytes, seg0, 8 * w0, 8 * (w0 + 16)).view("<i8")
    assert np.array_equal(torch_splitmix(torch, seg0, w0, 16).cpu().numpy(), ref)
    words = a.arr.view(torch.int64)
    step = 1 << 24
    for w in range(0, words.numel(), step):
        n = min(step, words.numel() - w)
        assert torch.equal(words[w:w + n], torch_splitmix(torch, seg0, w, n)), ("words from", w)
    half = words.numel() // 2
    differ = 0
    for w in range(0, half, step):
        n = min(step, half - w)
        differ += int((words[w:w + n] != words[half + w:half + w + n]).sum())
    # splitmix64 is a bijection of the counter: no two words of a segment are equal
    assert differ == half
