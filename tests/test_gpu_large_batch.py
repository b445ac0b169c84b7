"""In-layout batch kernels at byte offsets past 2^31 and 2^32 in both arrays.

Every in-layout kernel addresses base + seg * seg_stride + shard * shard_stride + col; the rest of
the suite stays below 1 GiB per array, where a 32-bit product or an `int` index cannot show. The
three batches here are the smallest that put both crossings inside the data and the parity array
at the geometry's real fragment sizes:

  A  RS(2,1),   F = 8 MiB,   520 segments: data 8.125 GiB (stride 2^24), parity 4.06 GiB (2^23)
  B  RS(32,32), F = 512 KiB, 264 segments: data and parity 4.125 GiB each (stride 2^24)
  C  RS(4,4),   F = 1 MiB,  1032 segments: data and parity 4.03 GiB each (stride 2^22)

The batches are segment-periodic (tests/large_geom.py): segment s holds base[s % 7], the C oracle
runs on the 7 base segments, and every byte of every array is compared on the GPU with the
7-segment expectation. The segments around the 2^31 / 2^32 offsets are also copied to the host and
given to the C oracle directly. Outputs start as poison, arrays lie between guard bands that are
checked after every call. One batch lives in HBM at a time (at most 22.3 GiB with a test's own
extra arrays); a test skips only when mem_get_info reports less than its need. On an MI355X every
test takes under a second and the file about 11 s."""
import hashlib
import os

import numpy as np
import pytest

from tests import large_geom as lg

pytestmark = pytest.mark.gpu

MiB, GiB = 1 << 20, 1 << 30
JUNK = 0xA5  # what an erased shard holds before its rebuild

GEOMS = {"A": (2, 1, 8 * MiB, 520, 0xA1), "B": (32, 32, 512 * 1024, 264, 0xB2),
         "C": (4, 4, 1 * MiB, 1032, 0xC3)}


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


def oracle_parity(corc, k, m, data):
    """The C oracle's parity [n][m][F] of data [n][k][F] (host arrays)."""
    data = np.ascontiguousarray(data)
    par = np.empty((data.shape[0], m, data.shape[2]), np.uint8)
    corc.orc_encode_batch(k, m, data.ctypes.data, par.ctypes.data, data.shape[0], data.shape[2],
                          min(16, os.cpu_count() or 1), 1)
    return par


class Batch:
    """One segment-periodic batch in HBM with its 7-segment truth."""

    def __init__(self, torch, corc, name):
        self.torch, self.corc, self.name = torch, corc, name
        self.k, self.m, self.F, self.nseg, seed = GEOMS[name]
        k, m, F, nseg = self.k, self.m, self.F, self.nseg
        self.n = k + m
        self.bytes = nseg * self.n * F
        self.base_h = np.random.default_rng(seed).integers(0, 256, (lg.P, k, F), dtype=np.uint8)
        self.pbase_h = oracle_parity(corc, k, m, self.base_h)
        self.base3 = torch.from_numpy(self.base_h).cuda()
        self.pbase3 = torch.from_numpy(self.pbase_h).cuda()
        self.data, self.data3 = self.new_array(k)
        self.par, self.par3 = self.new_array(m)
        self.segs = torch.arange(nseg, device="cuda")
        self.set_truth()

    def alloc(self, nbytes):
        return self.torch.empty(nbytes, dtype=self.torch.uint8, device="cuda")

    def new_array(self, shards):
        g = lg.Guarded(self.alloc, self.nseg * shards * self.F, fill=lg.POISON)
        return g, g.arr.view(self.nseg, shards, self.F)

    def rows(self, x3):
        return x3.view(self.nseg, -1)

    def set_truth(self, data3=None, par3=None):
        lg.tile_segments(self.rows(self.data3 if data3 is None else data3),
                         self.base3.view(lg.P, -1))
        lg.tile_segments(self.rows(self.par3 if par3 is None else par3),
                         self.pbase3.view(lg.P, -1))

    def poison_parity(self):
        self.par.arr[:] = lg.POISON

    def check(self, what, data=True, parity=True, arrays=None):
        """Guards intact, and every byte of the arrays equal to the periodic truth."""
        self.torch.cuda.synchronize()
        dg, d3, pg, p3 = arrays or (self.data, self.data3, self.par, self.par3)
        assert dg.guards_ok() and pg.guards_ok(), (what, "a guard band was written")
        if data:
            lg.assert_periodic(self.rows(d3), self.base3.view(lg.P, -1), (what, "data"))
        if parity:
            lg.assert_periodic(self.rows(p3), self.pbase3.view(lg.P, -1), (what, "parity"))

    def check_boundary_vs_oracle(self, what):
        """The segments around the 2^31 / 2^32 offsets of either array: the parity in HBM against
        the C oracle on the data in HBM, independent of the tiling."""
        segs = sorted(set(lg.boundary_segments(self.k * self.F, self.nseg)) |
                      set(lg.boundary_segments(self.m * self.F, self.nseg)))
        host = self.data3[segs].cpu().numpy()
        want = oracle_parity(self.corc, self.k, self.m, host)
        got = self.par3[segs].cpu().numpy()
        for i, s in enumerate(segs):
            assert np.array_equal(got[i], want[i]), (what, "segment", s)

    # a shard position over all segments, [nseg][F] (a strided view)
    def shard(self, j, arrays=None):
        d3, p3 = (arrays[1], arrays[3]) if arrays else (self.data3, self.par3)
        return d3[:, j] if j < self.k else p3[:, j - self.k]

    def heal(self, j, sl, arrays=None):
        """The test's own repair of junk it left: the truth back into shard j of segments sl."""
        base = self.base3[:, j] if j < self.k else self.pbase3[:, j - self.k]
        dst, segs = self.shard(j, arrays)[sl], self.segs[sl]
        step = max(1, 256 * MiB // self.F)
        for g in range(0, segs.numel(), step):
            dst[g:g + step] = base[segs[g:g + step] % lg.P]

    def erase_cycle(self, pats, arrays=None, value=JUNK):
        """Segment s loses the shards absent in pats[s % len(pats)]: junk there. Returns the
        per-segment presence flags [nseg][n]."""
        for i, p in enumerate(pats):
            for j in np.flatnonzero(np.asarray(p) == 0):
                self.shard(int(j), arrays)[i::len(pats)] = value
        return np.stack([pats[s % len(pats)] for s in range(self.nseg)]).astype(np.uint8)

    def boundary_offsets(self, shards):
        """Byte offsets of an array of `shards` shards per segment to flip: around 2^31 and 2^32,
        and the last byte of the last segment."""
        return list(lg.BOUNDARY_OFFSETS) + [self.nseg * shards * self.F - 1]


class Arena:
    """The module's HBM: one batch at a time, the previous one freed first."""

    def __init__(self, torch, corc):
        self.torch, self.corc, self.batch = torch, corc, None

    def drop(self):
        self.batch = None
        self.torch.cuda.empty_cache()

    def get(self, name, extra=0):
        """Batch `name`, built if it is not the current one; skips when the batch plus `extra`
        bytes of the test's own arrays (and library scratch) do not fit the free HBM."""
        k, m, F, nseg, _ = GEOMS[name]
        need = nseg * (k + m) * F + extra + 2 * GiB  # + truth, compare temporaries, guards
        if self.batch is not None and self.batch.name != name:
            self.drop()
        self.torch.cuda.empty_cache()
        free, _ = self.torch.cuda.mem_get_info()
        have = free + (self.batch.bytes if self.batch is not None else 0)
        if have < need:
            pytest.skip(f"needs {need / GiB:.1f} GiB of HBM, {have / GiB:.1f} GiB free")
        if self.batch is None:
            self.batch = Batch(self.torch, self.corc, name)
        return self.batch


@pytest.fixture(scope="module")
def arena(torch, corc):
    a = Arena(torch, corc)
    yield a
    a.drop()


def parity_bytes(name):
    """The batch-sized scratch of the generic VerifyBatch: a second parity array."""
    k, m, F, nseg, _ = GEOMS[name]
    return nseg * m * F


def one_pattern(n, lost):
    p = np.ones(n, np.uint8)
    p[list(lost)] = 0
    return p


def flip_protocol(torch, enc, b):
    """VerifyBatch on the clean batch, then one flipped bit at a time: exactly the segment that
    holds it is flagged, and the batch is clean again after the bit is put back."""
    k, m, F, nseg = b.k, b.m, b.F, b.nseg
    ok = enc.VerifyBatch(b.data.arr, b.par.arr, nseg, F)
    assert ok.shape == (nseg,) and ok.all(), np.flatnonzero(~ok)[:8]
    sites = [(b.data.arr, k * F, off) for off in b.boundary_offsets(k)] + \
            [(b.par.arr, m * F, off) for off in b.boundary_offsets(m)]
    for i, (arr, stride, off) in enumerate(sites):
        arr[off] ^= 1 << (i % 8)
        ok = enc.VerifyBatch(b.data.arr, b.par.arr, nseg, F)
        assert list(np.flatnonzero(~ok)) == [off // stride], (i, off, np.flatnonzero(~ok)[:8])
        arr[off] ^= 1 << (i % 8)
    assert enc.VerifyBatch(b.data.arr, b.par.arr, nseg, F).all()
    b.check("verify wrote nothing")


# ---- A: RS(2,1), F = 8 MiB, 520 segments ---------------------------------------------------------

@pytest.mark.parametrize("generic", [0, 1])
def test_a_encode(torch, cess, arena, generic):
    b = arena.get("A")
    enc = cess.New(b.k, b.m)
    enc.set_option(1, generic)
    b.poison_parity()
    enc.EncodeBatch(b.data.arr, b.par.arr, b.nseg, b.F)
    b.check(("encode", generic))
    b.check_boundary_vs_oracle(("encode", generic))


@pytest.mark.parametrize("generic", [0, 1])
def test_a_verify(torch, cess, arena, generic):
    # generic 0: k_verify21; 1: the parity recomputed into scratch (4.06 GiB), then k_cmp_segments
    b = arena.get("A", extra=generic * parity_bytes("A"))
    b.set_truth()
    enc = cess.New(b.k, b.m)
    enc.set_option(1, generic)
    flip_protocol(torch, enc, b)


@pytest.mark.parametrize("data_only", [False, True])
@pytest.mark.parametrize("generic", [0, 1])
def test_a_reconstruct(torch, cess, arena, generic, data_only):
    b = arena.get("A")
    b.set_truth()
    enc = cess.New(b.k, b.m)
    enc.set_option(1, generic)
    # per-segment patterns: segment s loses fragment s % 3
    pats = [one_pattern(3, [e]) for e in range(3)]
    present = b.erase_cycle(pats)
    enc.ReconstructBatch(b.data.arr, b.par.arr, b.nseg, b.F, present, data_only=data_only)
    torch.cuda.synchronize()
    if data_only:  # the lost parity fragments keep their junk, every byte
        assert lg.constant_mismatch(b.par3[2::3, 0], JUNK) == []
        b.heal(2, slice(2, None, 3))
    b.check(("per-segment", generic, data_only))
    # one pattern for every segment, each of the three erasures
    for e in range(3):
        b.shard(e)[:] = JUNK
        enc.ReconstructBatch(b.data.arr, b.par.arr, b.nseg, b.F, one_pattern(3, [e]),
                             data_only=data_only)
        torch.cuda.synchronize()
        if data_only and e == 2:
            assert lg.constant_mismatch(b.rows(b.par3), JUNK) == []
            b.set_truth()
        b.check(("one pattern", e, generic, data_only))


def test_a_encode_idx(torch, cess, arena):
    b = arena.get("A")
    b.set_truth()
    enc = cess.New(b.k, b.m)
    d0, d1 = b.data.arr.data_ptr(), b.data.arr.data_ptr() + b.F
    stride = b.k * b.F
    b.poison_parity()  # d0 overwrites without reading, d1 accumulates
    enc.EncodeIdxBatch(d0, stride, 0, b.par.arr, b.nseg, b.F, accumulate=False)
    enc.EncodeIdxBatch(d1, stride, 1, b.par.arr, b.nseg, b.F, accumulate=True)
    b.check("d0 overwrite, d1 accumulate")
    b.par.arr.zero_()  # the reverse feeding order into zeroed parity
    enc.EncodeIdxBatch(d1, stride, 1, b.par.arr, b.nseg, b.F, accumulate=True)
    enc.EncodeIdxBatch(d0, stride, 0, b.par.arr, b.nseg, b.F, accumulate=True)
    b.check("d1 then d0 into zeros")


def test_a_update(torch, cess, corc, arena):
    k, m, F, nseg, _ = GEOMS["A"]
    b = arena.get("A", extra=nseg * k * F)
    b.set_truth()
    enc = cess.New(k, m)
    # the new batch: d1 replaced by new periodic bytes; its d0 slot is never read (poison)
    new_h = b.base_h.copy()
    new_h[:, 1] = np.random.default_rng(0xA2).integers(0, 256, (lg.P, F), dtype=np.uint8)
    want = torch.from_numpy(oracle_parity(corc, k, m, new_h)).cuda()
    new_h[:, 0] = lg.POISON
    new, new3 = b.new_array(k)
    lg.tile_segments(b.rows(new3), torch.from_numpy(new_h).cuda().view(lg.P, -1))
    enc.UpdateBatch(b.data.arr, new.arr, b.par.arr, nseg, F, [0, 1])
    torch.cuda.synchronize()
    assert new.guards_ok()
    b.check("update reads only", parity=False)
    lg.assert_periodic(b.rows(b.par3), want.view(lg.P, -1), "updated parity")
    del new, new3
    b.set_truth()


def host_hashes(b):
    """hashlib over the 7 base segments: (segment hex [P][64], fragment hex [P][n][64]) uint8."""
    if not hasattr(b, "_hashes"):
        seg = np.zeros((lg.P, 64), np.uint8)
        frag = np.zeros((lg.P, b.n, 64), np.uint8)
        for r in range(lg.P):
            seg[r] = np.frombuffer(hashlib.sha256(b.base_h[r].tobytes()).hexdigest().encode(),
                                   np.uint8)
            for j in range(b.n):
                x = b.base_h[r, j] if j < b.k else b.pbase_h[r, j - b.k]
                frag[r, j] = np.frombuffer(hashlib.sha256(x.tobytes()).hexdigest().encode(),
                                           np.uint8)
        b._hashes = (seg, frag)
    return b._hashes


@pytest.mark.parametrize("sha_mode", [1, 2, 3])
def test_a_sha256_batch(torch, cess, arena, sha_mode):
    b = arena.get("A")
    b.set_truth()
    enc = cess.New(b.k, b.m)
    enc.set_option(3, sha_mode)
    hexes = lg.Guarded(b.alloc, b.nseg * b.n * 64, fill=lg.POISON)
    enc.Sha256Batch(b.data.arr, b.par.arr, b.nseg, b.F, hexes.arr)
    torch.cuda.synchronize()
    assert hexes.guards_ok()
    want = host_hashes(b)[1][np.arange(b.nseg) % lg.P]
    got = hexes.arr.cpu().numpy().reshape(b.nseg, b.n, 64)
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, bad[:8]


def test_a_hash_queue_segment_lists_and_check(torch, cess, arena):
    from cess_amd.hashq import HashQueue
    b = arena.get("A")
    b.set_truth()
    k, m, n, F, nseg = b.k, b.m, b.n, b.F, b.nseg
    seg_want = host_hashes(b)[0][np.arange(nseg) % lg.P]
    frag_want = host_hashes(b)[1][np.arange(nseg) % lg.P]
    seg_hex = lg.Guarded(b.alloc, nseg * 64, fill=lg.POISON)
    frag_hex = lg.Guarded(b.alloc, nseg * n * 64, fill=lg.POISON)
    with HashQueue() as q:
        # segment chains with fragment 0 as the prefix digest, fragment chains for the rest
        q.add_segment_lists(b.data.arr, b.par.arr, nseg, k, m, F, seg_hex.arr, frag_hex.arr)
        q.finish()
        torch.cuda.synchronize()
        assert seg_hex.guards_ok() and frag_hex.guards_ok()
        got = seg_hex.arr.cpu().numpy().reshape(nseg, 64)
        assert not (got != seg_want).any(), np.flatnonzero((got != seg_want).any(axis=1))[:8]
        got = frag_hex.arr.cpu().numpy().reshape(nseg, n, 64)
        assert not (got != frag_want).any(), np.argwhere((got != frag_want).any(axis=2))[:8]
        # the check pass: the recorded hashes are right except at the fragments that hold the
        # 2^31 / 2^32 offsets (and the last byte) of either array; flag 0 there and only there
        expect = frag_want.copy()
        wrong = set()
        for off in b.boundary_offsets(k):
            wrong.add((off // (k * F), off % (k * F) // F))
        for off in b.boundary_offsets(m):
            wrong.add((off // (m * F), k + off % (m * F) // F))
        for s, j in wrong:
            expect[s, j, 63] = ord("0") if expect[s, j, 63] != ord("0") else ord("1")
        d_expect = torch.from_numpy(expect).cuda()
        flags = lg.Guarded(b.alloc, nseg * n, fill=lg.POISON)
        q.add_check(b.data.arr, nseg * k, k, k * F, F, F, d_expect, n, flags.arr, n)
        q.add_check(b.par.arr, nseg * m, m, m * F, F, F, d_expect, n, flags.arr, n,
                    expect_offset=k * 64, ok_offset=k)
        q.finish()
        torch.cuda.synchronize()
        assert flags.guards_ok()
        got = flags.arr.cpu().numpy().reshape(nseg, n)
        want = np.ones((nseg, n), np.uint8)
        for s, j in wrong:
            want[s, j] = 0
        assert len(wrong) == 10
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    b.check("hashing wrote nothing")


@pytest.mark.parametrize("nidx", [47, 337])
def test_a_audit_chunks(torch, cess, arena, nidx):
    """47 challenged chunks, and 337, where the gathered chunks themselves (1560 fragments x 337 x
    8 KiB = 4.01 GiB) cross 2^32."""
    from cess_amd.audit import audit_chunks
    k, m, F, nseg, _ = GEOMS["A"]
    count, chunk = 1024, F // 1024
    out_bytes = nseg * (k + m) * nidx * chunk
    b = arena.get("A", extra=out_bytes + (512 * MiB if nidx > 47 else 0))
    b.set_truth()
    enc = cess.New(k, m)
    rng = np.random.default_rng(nidx)
    idx = np.concatenate([[0, 1023], 1 + rng.choice(1022, size=nidx - 2, replace=False)])
    idx = rng.permutation(idx).astype(np.uint32)
    assert (out_bytes > 1 << 32) == (nidx == 337)
    # expectation: gathered from the 7 base segments on the host, hex from hashlib
    frags = np.concatenate([b.base_h, b.pbase_h], axis=1).reshape(lg.P, b.n, count, chunk)
    want_h = np.ascontiguousarray(frags[:, :, idx])  # [P][n][nidx][chunk]
    want_hex = np.zeros((lg.P, b.n, nidx, 64), np.uint8)
    for r in range(lg.P):
        for j in range(b.n):
            for i in range(nidx):
                want_hex[r, j, i] = np.frombuffer(
                    hashlib.sha256(want_h[r, j, i].tobytes()).hexdigest().encode(), np.uint8)
    chunks = lg.Guarded(b.alloc, out_bytes, fill=lg.POISON)
    hexes = lg.Guarded(b.alloc, nseg * b.n * nidx * 64, fill=lg.POISON)
    audit_chunks(enc, b.data.arr, b.par.arr, nseg, F, idx, chunks.arr, hexes.arr, count)
    torch.cuda.synchronize()
    assert chunks.guards_ok() and hexes.guards_ok()
    lg.assert_periodic(chunks.arr.view(nseg, -1), torch.from_numpy(want_h).cuda().view(lg.P, -1),
                       "gathered chunks")
    lg.assert_periodic(hexes.arr.view(nseg, -1), torch.from_numpy(want_hex).cuda().view(lg.P, -1),
                       "chunk hashes")
    b.check("audit wrote nothing")


# ---- B: RS(32,32), F = 512 KiB, 264 segments -----------------------------------------------------

def wide_patterns(seed=70):
    """8 erasures on both sides, 6 on the data side, 6 on the parity side, 16, and 32 split evenly
    (all 32 on the parity side would be a re-encode)."""
    rng = np.random.default_rng(seed)
    pats = []
    for ne, lo, hi in ((8, 0, 64), (6, 0, 32), (6, 32, 64), (16, 0, 64)):
        pats.append(one_pattern(64, lo + rng.choice(hi - lo, size=ne, replace=False)))
    pats.append(one_pattern(64, list(rng.choice(32, size=16, replace=False)) +
                            list(32 + rng.choice(32, size=16, replace=False))))
    return pats


@pytest.mark.parametrize("path", ["fft", "rt0", "rt1", "rt2"])
def test_b_encode(torch, cess, arena, path):
    b = arena.get("B")
    enc = cess.New(b.k, b.m)
    if path != "fft":
        enc.set_option(1, 1)
        enc.set_option(4, int(path[2]))
    b.poison_parity()
    enc.EncodeBatch(b.data.arr, b.par.arr, b.nseg, b.F)
    b.check(("encode", path))
    b.check_boundary_vs_oracle(("encode", path))


@pytest.mark.parametrize("generic", [0, 1])
def test_b_verify(torch, cess, arena, generic):
    b = arena.get("B", extra=generic * parity_bytes("B"))
    b.set_truth()
    enc = cess.New(b.k, b.m)
    enc.set_option(1, generic)
    flip_protocol(torch, enc, b)


@pytest.mark.parametrize("mode", [1, 2])
def test_b_reconstruct_fft_decoders(torch, cess, arena, mode):
    """Per-segment patterns on the syndrome-row (1) and the formal-derivative (2) decoder: the
    counters prove which kernel rebuilt all 264 segments."""
    b = arena.get("B")
    b.set_truth()
    enc = cess.New(b.k, b.m)
    enc.set_option(8, mode)
    present = b.erase_cycle(wide_patterns())
    b4, b5 = enc.stat(4), enc.stat(5)
    enc.ReconstructBatch(b.data.arr, b.par.arr, b.nseg, b.F, present)
    b.check(("fftdec", mode))
    assert enc.stat(4) - b4 == b.nseg
    assert enc.stat(5) - b5 == (b.nseg if mode == 2 else 0)
    b.check_boundary_vs_oracle(("fftdec", mode))


def test_b_reconstruct_matrix_kernels(torch, cess, arena):
    """CEC_OPT_FFTDEC_MIN = 0: one to four erasures per segment (the bit-plane kernel k_rtb) and
    eight (Horner over input groups), a different pattern per segment; the counters stay."""
    b = arena.get("B")
    b.set_truth()
    enc = cess.New(b.k, b.m)
    enc.set_option(7, 0)
    rng = np.random.default_rng(71)
    pats = [one_pattern(64, rng.choice(64, size=ne, replace=False)) for ne in (1, 2, 3, 4, 8)]
    present = b.erase_cycle(pats)
    b4 = enc.stat(4)
    enc.ReconstructBatch(b.data.arr, b.par.arr, b.nseg, b.F, present)
    b.check("matrix kernels")
    assert enc.stat(4) == b4


def test_b_all_parity_lost_reencodes(torch, cess, arena):
    b = arena.get("B")
    b.set_truth()
    enc = cess.New(b.k, b.m)
    b.par.arr[:] = JUNK
    enc.ReconstructBatch(b.data.arr, b.par.arr, b.nseg, b.F, one_pattern(64, range(32, 64)))
    b.check("all parity lost")


def test_b_reconstruct_some(torch, cess, arena):
    """Four shards lost, one of them required (which one cycles with the segment): that shard is
    rebuilt, the other three keep their junk, every byte."""
    b = arena.get("B")
    b.set_truth()
    enc = cess.New(b.k, b.m)
    lost = [3, 17, 40, 63]
    present = b.erase_cycle([one_pattern(64, lost)])
    required = np.zeros_like(present)
    for s in range(b.nseg):
        required[s, lost[s % 4]] = 1
    enc.ReconstructSomeBatch(b.data.arr, b.par.arr, b.nseg, b.F, present, required)
    torch.cuda.synchronize()
    for r, j in enumerate(lost):
        for q in range(4):
            if q != r:  # segments q mod 4 did not ask for shard j
                assert bool((b.shard(j)[q::4] == JUNK).all()), (j, q)
                b.heal(j, slice(q, None, 4))
    b.check("required shards")


# ---- C: RS(4,4), F = 1 MiB, 1032 segments --------------------------------------------------------

def narrow_patterns(seed=72):
    """One to four erasures of RS(4,4), two patterns each."""
    rng = np.random.default_rng(seed)
    return [one_pattern(8, rng.choice(8, size=ne, replace=False))
            for ne in (1, 2, 3, 4) for _ in range(2)]


@pytest.mark.parametrize("rt_mode", [0, 1, 2, 3])
def test_c_run_time_kernels(torch, cess, arena, rt_mode):
    b = arena.get("C")
    b.set_truth()
    enc = cess.New(b.k, b.m)
    enc.set_option(4, rt_mode)
    b.poison_parity()
    enc.EncodeBatch(b.data.arr, b.par.arr, b.nseg, b.F)
    b.check(("encode", rt_mode))
    if rt_mode == 0:
        b.check_boundary_vs_oracle("encode")
    present = b.erase_cycle(narrow_patterns())
    enc.ReconstructBatch(b.data.arr, b.par.arr, b.nseg, b.F, present)
    b.check(("rebuild", rt_mode))


def test_c_partials_combined_by_xor(torch, cess, arena):
    """Two holders of the batch, each with every other survivor: their partial rebuilds XORed give
    the lost shards. A holder's other shards are junk (never read). cec_xor_batch adds one
    contiguous range, so the partials meet shard by shard, every range of the second copy past
    2^32 included."""
    k, m, F, nseg, _ = GEOMS["C"]
    b = arena.get("C", extra=nseg * (k + m) * F)
    b.set_truth()
    enc = cess.New(k, m)
    n = k + m
    dg2, d32 = b.new_array(k)
    pg2, p32 = b.new_array(m)
    two = (dg2, d32, pg2, p32)
    b.set_truth(d32, p32)
    pats = narrow_patterns(73)
    present = b.erase_cycle(pats)
    b.erase_cycle(pats, two)
    held = [np.zeros((nseg, n), np.uint8), np.zeros((nseg, n), np.uint8)]
    for s in range(nseg):
        surv = np.flatnonzero(present[s])[:k]  # cec_survivors: the first k present
        held[0][s, surv[(s % 2)::2]] = 1
        held[1][s, surv[1 - (s % 2)::2]] = 1
    # a present shard a holder does not hold is junk in its copy (per pattern and segment parity)
    npat = len(pats)
    for h, arrays in ((0, None), (1, two)):
        for c in range(2 * npat):
            for j in range(n):
                if present[c, j] and not held[h][c, j]:
                    b.shard(j, arrays)[c::2 * npat] = JUNK
    enc.ReconstructPartialBatch(b.data.arr, b.par.arr, nseg, F, present, held[0])
    enc.ReconstructPartialBatch(dg2.arr, pg2.arr, nseg, F, present, held[1])
    from cess_amd import xor_batch
    seg_stride = {True: k * F, False: m * F}
    for s in range(nseg):
        for j in np.flatnonzero(present[s] == 0):
            isd = bool(j < k)
            off = s * seg_stride[isd] + int(j if isd else j - k) * F
            dst = (b.data if isd else b.par).arr.data_ptr() + off
            src = (dg2 if isd else pg2).arr.data_ptr() + off
            xor_batch(dst, src, 1, seg_stride[isd], F)
    torch.cuda.synchronize()
    assert dg2.guards_ok() and pg2.guards_ok()
    # the first copy's junk (its unheld survivors) back to truth, then every byte of it
    for c in range(2 * npat):
        for j in range(n):
            if present[c, j] and not held[0][c, j]:
                assert bool((b.shard(j)[c::2 * npat] == JUNK).all()), (c, j)
                b.heal(j, slice(c, None, 2 * npat))
    b.check("partials combined")
    del two, dg2, d32, pg2, p32


def test_c_xor_sources_a_segment_stride_apart(torch, cess, arena):
    """cec_xor_batch with src_stride = the segment stride and one source per segment: source j
    lies at j * 2^22, past 2^32 from segment 1024 on. The sum of shard 1 over all segments."""
    from cess_amd import xor_batch
    b = arena.get("C")
    b.set_truth()
    k, F, nseg = b.k, b.F, b.nseg
    acc = lg.Guarded(b.alloc, F, fill=0)
    xor_batch(acc.arr, b.data.arr.data_ptr() + F, nseg, k * F, F)
    torch.cuda.synchronize()
    assert acc.guards_ok()
    want = np.zeros(F, np.uint8)
    for s in range(nseg):
        want ^= b.base_h[s % lg.P, 1]
    assert np.array_equal(acc.arr.cpu().numpy(), want)
    b.check("xor read only")
