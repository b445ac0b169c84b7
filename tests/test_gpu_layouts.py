"""In-layout kernels where the launchers' dispatch on the low bits of the Layout had never run:
bit-exact against the C oracle (c_encode), no tolerances.

A. The host-buffer API stages one segment at shard stride pad256(len) on a 256-byte-aligned base,
   so a length that is no multiple of the column width runs a vector body and then a byte tail in
   the last workgroup. The lengths put that tail behind more than one workgroup of every column
   width (256 lanes of 16 / 8 / 4 bytes: tiles of 4096 / 2048 / 1024 bytes):

       len    16-byte columns             8-byte columns          4-byte columns
       9      tail only                   1 + tail 1              2 + tail 1
       2051   128 + tail 3                one tile + tail 3       two tiles + tail 3
       4099   one tile + tail 3           two tiles + tail 3      four tiles + tail 3
       4112   one tile + 1, no tail       -                       -
       8195   two tiles + tail 3          four tiles + tail 3     eight tiles + tail 3
       8285   2 tiles + 5 + tail 13       4 tiles + 11 + tail 5   8 tiles + 23 + tail 1

   (8195 is the one length at which 16-byte columns fill whole workgroups, more than one, before
   a tail: at 4099 their grid is a single workgroup.) None is a multiple of 1024, so RS(32,32)
   stays on the matrix kernels. Before every call the stage is filled with other bytes
   (junk_calls), so a byte the call under test does not write differs from the expected one.

B. The batch API with d_data and d_parity at GUARD + off inside larger tensors, between 64-byte
   bands of 0xA5: bases that are 16-, 8-, 4-aligned or odd take the dispatch arms the aligned
   tensors of the other modules never reach. After every call the whole of both buffers is compared
   with the expected bytes (outputs from the oracle, everything else from before the call) and
   the four bands with 0xA5.

The comment above each row names the kernel that the dispatch in cess_ec.cpp (launch_chunk,
do_encode, do_decode) and kernels.hip (run_ct, run_hg, run_rt, run_rtb, run_rth) picks for it."""
import hashlib

import numpy as np
import pytest

from oracle.c_oracle import c_encode

pytestmark = pytest.mark.gpu

GUARD = 64
OPT_GENERIC, OPT_VARIANT, OPT_RT_MODE, OPT_FFTDEC_MIN, OPT_FFTDEC_MODE = 1, 2, 4, 7, 8
STAT_FFTDEC_SEGMENTS = 4
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


def codewords(corc, k, m, ln, nseg=1):
    """Oracle codewords [nseg][k + m][ln] of random data: one c_encode over the whole batch (the
    arithmetic is per byte), computed once per shape and read-only afterwards."""
    key = (k, m, ln, nseg)
    if key not in _CODEWORDS:
        rng = np.random.default_rng(k * 1000003 + m * 1009 + ln * 7 + nseg)
        data = rng.integers(0, 256, (nseg, k, ln), dtype=np.uint8)
        cols = [np.ascontiguousarray(data[:, j, :]).reshape(-1) for j in range(k)]
        par = np.stack([p.reshape(nseg, ln) for p in c_encode(corc, k, m, cols)], axis=1)
        full = np.concatenate([data, par], axis=1)
        full.setflags(write=False)
        _CODEWORDS[key] = full
    return _CODEWORDS[key]


def same(got, want, what):
    bad = np.flatnonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))
    assert bad.size == 0, (what, "wrong bytes", int(bad.size), "first at", int(bad[0]))


# ==== A. host-buffer API: vector body plus tail, past one workgroup ================================

LENS_A = [9, 2051, 4099, 4112, 8195, 8285]


def junk_calls(enc, rng, ln):
    """Other bytes into every slot of the codec's stage, as a previous call leaves them: an encode
    of junk shards (the data slots by copy, the parity slots by the kernels), then a rebuild of the
    first m data shards of another junk set (the other data slots and every parity slot by copy).
    No byte of any slot is then left from an earlier call on the same bytes, even where a kernel
    skipped it."""
    k, m = enc.DataShards, enc.ParityShards
    enc.Encode([rng.integers(0, 256, ln, dtype=np.uint8) for _ in range(k + m)])
    sh = [rng.integers(0, 256, ln, dtype=np.uint8) for _ in range(k + m)]
    for i in range(min(m, k)):
        sh[i] = None
    enc.ReconstructData(sh)


def host_encode_verify(enc, full, rng, what):
    """Encode against the oracle; Verify true, then false with the last byte of the last parity
    shard flipped, then with the first byte of data shard 0 flipped."""
    n, ln = full.shape
    k = enc.DataShards
    junk_calls(enc, rng, ln)
    shards = [full[i].copy() for i in range(k)] + [np.full(ln, 0x5A, np.uint8) for _ in range(k, n)]
    enc.Encode(shards)
    for i in range(n):
        same(shards[i], full[i], (what, "encode", i))
    junk_calls(enc, rng, ln)
    assert enc.Verify([s.copy() for s in full]), (what, "verify")
    for i, at in ((n - 1, ln - 1), (0, 0)):
        bad = [s.copy() for s in full]
        bad[i][at] ^= 0x40
        junk_calls(enc, rng, ln)
        assert not enc.Verify(bad), (what, "verify with a flipped byte", i, at)


def host_rebuild(enc, full, erased, rng, what):
    """Reconstruct and ReconstructData of one erasure pattern against the oracle's codeword."""
    n, ln = full.shape
    k = enc.DataShards
    for data_only in (False, True):
        junk_calls(enc, rng, ln)
        shards = [None if i in erased else full[i].copy() for i in range(n)]
        (enc.ReconstructData if data_only else enc.Reconstruct)(shards)
        for i in range(n):
            if data_only and i >= k and i in erased:
                assert shards[i] is None, (what, data_only, i)
            else:
                same(shards[i], full[i], (what, "data_only", data_only, "shard", i))


def host_rebuild_some(enc, full, erased, rng, what):
    """ReconstructSome of one lost shard of the pattern: the others stay None."""
    n, ln = full.shape
    one = sorted(erased)[len(erased) // 2]
    junk_calls(enc, rng, ln)
    shards = [None if i in erased else full[i].copy() for i in range(n)]
    enc.ReconstructSome(shards, [i == one for i in range(n)])
    for i in range(n):
        if i in erased and i != one:
            assert shards[i] is None, (what, "some", i)
        else:
            same(shards[i], full[i], (what, "some", i))


@pytest.mark.parametrize("ln", LENS_A)
@pytest.mark.parametrize("generic", [0, 1])
def test_host_rs21(cess, corc, ln, generic):
    """RS(2,1), one segment through the host-buffer API: the compile-time tile, body closed form
    and tail generic column, and the per-bit mask kernel."""
    full = codewords(corc, 2, 1, ln)[0]
    rng = np.random.default_rng(21 + ln + generic)
    with cess.New(2, 1) as enc:
        enc.set_option(OPT_GENERIC, generic)
        # generic 0: encode = k_ct<EncCT<2,1>, 1, NT, u32x4> (run_ct_variant's default), body
        #   ct_column_horner, tail ct_tail<EncCT<2,1>, 16>
        # generic 1: two inputs are below the Horner kernels' four, one output: k_rt<1, 1, u32x4>
        #   (bucket 1; RS(2,1) never has two outputs, so bucket 2 is RS(32,32)'s below)
        host_encode_verify(enc, full, rng, (ln, generic))
        # generic 0: lost 0 / 1 = k_ct<Dec1CT<2,1,0 / 1>>, body ct_column_rs21 (closed forms), tail
        #   the generic Horner column; lost 2 = k_ct<EncCT<2,1>> again (launch_decode_ct)
        # generic 1: k_rt<1, 1, u32x4> with the pattern's decode row
        for lost in range(3):
            host_rebuild(enc, full, {lost}, rng, (ln, generic, lost))
        host_rebuild_some(enc, full, {0}, rng, (ln, generic))


@pytest.mark.parametrize("ln", LENS_A)
@pytest.mark.parametrize("generic,rt_mode", [(0, 0), (1, 0), (1, 1), (1, 2), (1, 3)])
def test_host_rs3232_encode(cess, corc, ln, generic, rt_mode):
    """RS(32,32) encode and verify at lengths the FFT refuses (len % 1024 != 0)."""
    full = codewords(corc, 32, 32, ln)[0]
    rng = np.random.default_rng(3232 + ln + 8 * generic + rt_mode)
    with cess.New(32, 32) as enc:
        enc.set_option(OPT_GENERIC, generic)
        enc.set_option(OPT_RT_MODE, rt_mode)
        # generic 0: run_wide_variant -> launch_fft_rs3232 refuses -> run_hg<EncCT<32,32>, 4, 0>:
        #   k_hg (4-byte columns) and ct_tail<P, 4>
        # generic 1, one chunk of 32 outputs from 32 inputs (bucket 32):
        #   rt_mode 0: k_rthx<8>    rt_mode 1: k_rt<32, 1, uint32_t>    rt_mode 2: k_rth<8>
        #   rt_mode 3: k_rtb has no bucket past four and a chunk holds up to 32 outputs (no split
        #   into fours), so launch_matvec_rtb declines and k_rth<8> runs, as under rt_mode 2
        host_encode_verify(enc, full, rng, (ln, generic, rt_mode))


RT_COUNTS = [1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 24, 32]   # every rt_dispatch bucket
REBUILDS_3232 = ([(1, ne) for ne in RT_COUNTS] +
                 [(mode, ne) for mode in (0, 2) for ne in (1, 2, 3, 4, 6, 16, 32)])


@pytest.mark.parametrize("ln", LENS_A)
@pytest.mark.parametrize("rt_mode,ne", REBUILDS_3232)
def test_host_rs3232_rebuild(cess, corc, ln, rt_mode, ne):
    """RS(32,32) rebuilds of `ne` shards (patterns from a fixed seed) on the run-time matrix
    kernels (CEC_OPT_FFTDEC_MIN = 0), 32 inputs, one chunk of `ne` outputs."""
    full = codewords(corc, 32, 32, ln)[0]
    rng = np.random.default_rng(1000 * rt_mode + 10 * ne + ln)
    erased = set(rng.choice(64, size=ne, replace=False).tolist())
    with cess.New(32, 32) as enc:
        enc.set_option(OPT_RT_MODE, rt_mode)
        enc.set_option(OPT_FFTDEC_MIN, 0)
        # rt_mode 1: k_rt<bucket, 1, TV>: u32x4 for 1..6 outputs, u32x2 for 7, 8, 12, uint32_t
        #   for 16, 24, 32
        # rt_mode 0: 1..4 outputs k_rtb<1..3, u32x2, 4> / k_rtb<4, u32x2, 8>; above, k_rthx<8>
        # rt_mode 2: k_rth<8> for every count (k_rtb is rt_mode 0's and 3's)
        # (ReconstructData of a pattern with lost parity has fewer outputs: a smaller bucket of
        # the same kernel family)
        host_rebuild(enc, full, erased, rng, (ln, rt_mode, ne))
        if ne in (1, 6):
            host_rebuild_some(enc, full, erased, rng, (ln, rt_mode, ne))


# (k, m): inputs -> Horner group count of run_rth, encode outputs -> bucket
#   RS(4,2)   NG 1 (four inputs, the fewest the Horner kernels take), bucket 2
#   RS(5,5)   NG 2, bucket 5              RS(10,4)  NG 3, bucket 4
#   RS(17,3)  5 groups: NG 6, bucket 3    RS(20,10) 5 groups: NG 6, bucket 12
#   RS(33,3)  33 inputs: no Horner form, bucket 3
OTHER_CODES = [(4, 2), (5, 5), (10, 4), (17, 3), (20, 10), (33, 3)]


@pytest.mark.parametrize("ln", LENS_A)
@pytest.mark.parametrize("rt_mode", [0, 1, 2, 3])
@pytest.mark.parametrize("k,m", OTHER_CODES)
def test_host_other_codes(cess, corc, k, m, ln, rt_mode):
    """Codes without a compile-time kernel: encode, verify and rebuilds of m shards and of one."""
    full = codewords(corc, k, m, ln)[0]
    rng = np.random.default_rng(k * 131 + m * 17 + ln + rt_mode)
    with cess.New(k, m) as enc:
        enc.set_option(OPT_GENERIC, 1)  # RS(5,5) generic; none of these has a built-in kernel
        enc.set_option(OPT_RT_MODE, rt_mode)
        # rt_mode 0 encode: RS(4,2) k_rtb<2>, RS(10,4) k_rtb<4, u32x2, 8>, RS(17,3) and RS(33,3)
        #   k_rtb<3, u32x2, 4> (at most four outputs from at least four inputs), RS(5,5)
        #   k_rthx<2>, RS(20,10) k_rthx<6>
        # rt_mode 1: k_rt<bucket>, u32x4 up to six outputs, RS(20,10) k_rt<12, 1, u32x2>
        # rt_mode 2: k_rth<NG> with NG as listed above; RS(33,3) k_rt<3> (over kRthMaxIn inputs)
        # rt_mode 3: k_rtb<bucket> up to four outputs; RS(5,5) and RS(20,10) fall to k_rth<NG>
        host_encode_verify(enc, full, rng, (k, m, ln, rt_mode))
        # rebuilds: k inputs again; m outputs = the encode's bucket, one output = bucket 1
        # (rt_mode 0 / 3: k_rtb<1>, rt_mode 1: k_rt<1>, rt_mode 2: k_rth<NG> or RS(33,3) k_rt<1>)
        many = set(rng.choice(k + m, size=m, replace=False).tolist())
        host_rebuild(enc, full, many, rng, (k, m, ln, rt_mode, "m lost"))
        host_rebuild(enc, full, {int(rng.integers(0, k + m))}, rng, (k, m, ln, rt_mode, "one lost"))
        host_rebuild_some(enc, full, many, rng, (k, m, ln, rt_mode))


@pytest.mark.parametrize("ln", [4099, 8285])
@pytest.mark.parametrize("k,m,variants", [(2, 1, range(0, 9)), (32, 32, range(0, 22))])
def test_host_tuning_variants(cess, corc, k, m, variants, ln):
    """The tuning library's encode variants (CEC_OPT_CT_VARIANT), each equal to the oracle:
    RS(2,1) 0-8 = k_ct with U = 1, 2, 4 columns per lane (cached, then nontemporal) and block
      sizes 512, 128, 1024: ct_tile's partial tiles (U = 2: tiles of 8192 bytes, U = 4: 16384) and
      its tail in the last of several workgroups;
    RS(32,32) 0-10 = k_ct streaming / nibble-window columns of 16, 8 and 4 bytes with their
      ct_tail<P, 16 / 8 / 4>, 11-21 = k_hg with three- and four-input groups, its flag forms and
      block sizes 128 and 512."""
    full = codewords(corc, k, m, ln)[0]
    rng = np.random.default_rng(k + ln)
    with cess.New(k, m, tuning=True) as enc:
        for v in variants:
            enc.set_option(OPT_VARIANT, v)
            junk_calls(enc, rng, ln)
            shards = [full[i].copy() for i in range(k)] + [np.full(ln, 0x5A, np.uint8)
                                                           for _ in range(m)]
            enc.Encode(shards)
            for i in range(k + m):
                same(shards[i], full[i], (k, m, ln, "variant", v, "shard", i))


# ==== B. batch API: offset bases between guard bands ===============================================

OFFS = [(0, 0), (16, 48), (8, 8), (4, 12), (0, 4), (1, 0), (0, 1), (3, 5)]
NSEG = 3


class Off:
    """Bytes on the device at GUARD + off inside a larger uint8 tensor whose other bytes are 0xA5
    (64-byte bands on both sides at least). `t` is the contiguous slice the library is given;
    get() checks the bands and returns the bytes."""

    def __init__(self, torch, body, off=0):
        body = np.ascontiguousarray(body, dtype=np.uint8).reshape(-1)
        self.torch, self.lo, self.n = torch, GUARD + off, body.size
        host = np.full(self.lo + self.n + GUARD, 0xA5, dtype=np.uint8)
        host[self.lo:self.lo + self.n] = body
        self.whole = torch.from_numpy(host).cuda()
        assert self.whole.data_ptr() % 256 == 0  # the offsets below are the bases' low bits
        self.t = self.whole[self.lo:self.lo + self.n]
        assert self.t.is_contiguous() and self.t.data_ptr() == self.whole.data_ptr() + self.lo

    def put(self, body):
        body = np.ascontiguousarray(body, dtype=np.uint8).reshape(-1)
        assert body.size == self.n
        self.t.copy_(self.torch.from_numpy(body))

    def get(self, what):
        self.torch.cuda.synchronize()
        got = self.whole.cpu().numpy()
        assert (got[:self.lo] == 0xA5).all(), (what, "low guard band written")
        assert (got[self.lo + self.n:] == 0xA5).all(), (what, "high guard band written")
        return got[self.lo:self.lo + self.n]


class Batch:
    """d_data [nseg][k][ln] and d_parity [nseg][m][ln] at offs = (data, parity) between bands."""

    def __init__(self, torch, state, k, offs):
        self.k = k
        self.d = Off(torch, state[:, :k], offs[0])
        self.p = Off(torch, state[:, k:], offs[1])

    def put(self, state):
        self.d.put(state[:, :self.k])
        self.p.put(state[:, self.k:])

    def get(self, what):
        nseg = NSEG
        d = self.d.get((what, "data")).reshape(nseg, self.k, -1)
        p = self.p.get((what, "parity")).reshape(nseg, -1, d.shape[2])
        return np.concatenate([d, p], axis=1)

    def check(self, what, want):
        """Every byte of both buffers equals `want` [nseg][k + m][ln]; the four bands are intact."""
        got = self.get(what)
        for s in range(got.shape[0]):
            for i in range(got.shape[1]):
                same(got[s, i], want[s, i], (what, "segment", s, "shard", i))


def patterns(k, m, rng):
    """A different erasure pattern per segment. RS(2,1): shard s mod 3 (the mixed kernel's case);
    else one lost shard, m lost shards, and a random count of them."""
    n = k + m
    present = np.ones((NSEG, n), np.uint8)
    if (k, m) == (2, 1):
        present[np.arange(NSEG), np.arange(NSEG) % 3] = 0
        return present
    for s, ne in enumerate((1, m, int(rng.integers(1, m + 1)))):
        present[s, rng.choice(n, size=ne, replace=False)] = 0
    return present


# (k, m, CEC_OPT_FORCE_GENERIC, CEC_OPT_RT_MODE); the last row puts k_rth, which only rt_mode 2
# and 3 select, on the offset bases too
BATCH_CODES = [(2, 1, 0, 0), (32, 32, 0, 0), (10, 4, 0, 0), (5, 5, 1, 0), (10, 4, 0, 2)]
BATCH_CASES = [(k, m, g, r, ln) for k, m, g, r in BATCH_CODES
               for ln in ((48, 1024, 4112, 8192) if k == 32 else (48, 4112, 8192))]


@pytest.mark.parametrize("offs", OFFS, ids=lambda o: "d%d_p%d" % o)
@pytest.mark.parametrize("k,m,generic,rt_mode,ln", BATCH_CASES)
def test_batch_offset_bases(torch, cess, corc, k, m, generic, rt_mode, ln, offs):
    """Every in-layout batch call on bases at offs. What the low bits of the bases select:
    RS(2,1): both 16-aligned k_ct / k_ct_dec1_mixed21 / k_verify21; else k_ct_bytes, the mixed
      launch refused (one k_ct_bytes launch per pattern) and the verify recomputed into aligned
      scratch and compared by k_cmp_segments (bytes when the stored parity is unaligned).
    RS(32,32): both 16-aligned and len % 1024 == 0 the FFT encode, verify and (by the cost model)
      decoders; 4-aligned k_hg and, for the rebuilds, k_rtb / k_rthx with vec_ok on bases that are
      no multiple of 16, while k_rt and k_rtb (16- and 8-byte columns) run byte-wise there; an
      odd base: run_hg hands over to run_ct, whose own check picks k_ct_bytes, and every run-time
      kernel runs with vec_ok == 0.
    RS(10,4), RS(5,5) generic: k_rtb (8-byte columns when 16-aligned, else bytes) and k_rthx<2>
      (4-byte columns from 4-aligned bases on); RS(10,4) under rt_mode 2: k_rth<3>, as k_rthx.
    Partials always take the run-time kernels; xor_batch XORs part 1 into part 0 at the offset
    base (k_xor_reduce<false> unless both bases are 16-aligned)."""
    n = k + m
    full = codewords(corc, k, m, ln, NSEG)
    rng = np.random.default_rng(k * 7 + rt_mode + ln + 16 * offs[0] + offs[1])
    junk = rng.integers(0, 256, full.shape, dtype=np.uint8)  # what lost slots hold before a call
    what = (k, m, rt_mode, ln, offs)
    enc = cess.New(k, m)
    enc.set_option(OPT_GENERIC, generic)
    enc.set_option(OPT_RT_MODE, rt_mode)

    # EncodeBatch: all data unchanged, parity from the oracle
    b = Batch(torch, np.concatenate([full[:, :k], junk[:, k:]], axis=1), k, offs)
    enc.EncodeBatch(b.d.t, b.p.t, NSEG, ln)
    b.check((what, "encode"), full)

    # ReconstructBatch, a different pattern per segment, both data_only settings
    present = patterns(k, m, rng)
    lost = present == 0
    start = np.where(lost[:, :, None], junk, full)
    for data_only in (False, True):
        b.put(start)
        enc.ReconstructBatch(b.d.t, b.p.t, NSEG, ln, present, data_only=data_only)
        want = full.copy()
        if data_only:
            want[:, k:] = start[:, k:]
        b.check((what, "reconstruct", data_only), want)

    # ReconstructSomeBatch: one lost shard per segment required, the other lost ones left alone
    required = np.zeros_like(present)
    for s in range(NSEG):
        ls = np.flatnonzero(lost[s])
        required[s, ls[len(ls) // 2]] = 1
    b.put(start)
    enc.ReconstructSomeBatch(b.d.t, b.p.t, NSEG, ln, present, required)
    b.check((what, "some"), np.where(required[:, :, None] == 1, full, start))

    # ReconstructPartialBatch over two parts (shard f of segment s held by part (s + f) % 2), each
    # on its own offset buffers, then part 1 XORed into part 0
    parts, starts = [b, Batch(torch, junk, k, offs)], []
    for r in range(2):
        held = present & (((np.arange(NSEG)[:, None] + np.arange(n)[None, :]) % 2) == r)
        st = rng.integers(0, 256, full.shape, dtype=np.uint8)
        st = np.where(held[:, :, None] == 1, full, st)
        parts[r].put(st)
        enc.ReconstructPartialBatch(parts[r].d.t, parts[r].p.t, NSEG, ln, present,
                                    held.astype(np.uint8))
        got = parts[r].get((what, "partial", r))
        same(got[~lost], st[~lost], (what, "partial", r, "a present shard was written"))
        starts.append(got)
    for src, dst in ((parts[1].d, parts[0].d), (parts[1].p, parts[0].p)):
        cess.xor_batch(dst.t, src.t, 1, dst.n, dst.n)
    got = parts[0].get((what, "xor"))
    same(got, starts[0] ^ starts[1], (what, "xor of the two parts"))
    same(got[lost], full[lost], (what, "XOR of the partials is the rebuilt shard"))
    parts[1].check((what, "xor source"), starts[1])

    # VerifyBatch: good; last parity byte of the last segment flipped; first data byte of segment 0
    ok = Off(torch, np.full(NSEG, 0x77, np.uint8), 1)
    for flip, flags in ((None, [1, 1, 1]), ((NSEG - 1, n - 1, ln - 1), [1, 1, 0]),
                        ((0, 0, 0), [0, 1, 1])):
        state = full.copy()
        if flip:
            state[flip] ^= 0x5A
        b.put(state)
        ok.put(np.full(NSEG, 0x77, np.uint8))
        enc.VerifyBatch(b.d.t, b.p.t, NSEG, ln, d_ok=ok.t)
        assert ok.get((what, "verify flags", flip)).tolist() == flags, (what, "verify", flip)
        b.check((what, "verify", flip), state)
    enc.close()


@pytest.mark.parametrize("offs", OFFS, ids=lambda o: "d%d_p%d" % o)
@pytest.mark.parametrize("ln", [1024, 8192])
def test_batch_fftdec_refused_off_16(torch, cess, corc, ln, offs):
    """RS(32,32) rebuilds of at least four shards at FFT-eligible lengths: the FFT-domain decoders
    take every segment (CEC_STAT_FFTDEC_SEGMENTS advances by nseg) when both bases are 16-byte
    aligned, and none otherwise (fftdec_layout_ok for the per-segment plan, launch_fftdec /
    launch_fftdec_d for the single pattern: the run-time matrix kernels rebuild instead); the bytes
    are the oracle's either way. The decoder is forced per count (CEC_OPT_FFTDEC_MODE 1 syndrome
    rows, 2 formal derivative): the default cost model sends some patterns of four to twelve
    outputs to the matrix kernel on any layout, which would hide a refusal."""
    k = m = 32
    full = codewords(corc, k, m, ln, NSEG)
    rng = np.random.default_rng(ln + 16 * offs[0] + offs[1])
    junk = rng.integers(0, 256, full.shape, dtype=np.uint8)
    aligned = offs[0] % 16 == 0 and offs[1] % 16 == 0
    assert aligned == (offs in ((0, 0), (16, 48)))
    enc = cess.New(k, m)
    b = Batch(torch, junk, k, offs)
    for ne, mode in ((4, 1), (8, 2), (16, 1), (32, 2)):
        enc.set_option(OPT_FFTDEC_MODE, mode)
        present = np.ones((NSEG, 2 * k), np.uint8)
        for s in range(NSEG):
            present[s, rng.choice(2 * k, size=ne, replace=False)] = 0
        for pat in (present, present[1]):  # per-segment patterns, then one for the whole batch
            lost = np.broadcast_to(pat == 0, (NSEG, 2 * k))
            b.put(np.where(lost[:, :, None], junk, full))
            before = enc.stat(STAT_FFTDEC_SEGMENTS)
            enc.ReconstructBatch(b.d.t, b.p.t, NSEG, ln, pat)
            b.check((ln, offs, ne, mode, pat.ndim), full)
            assert enc.stat(STAT_FFTDEC_SEGMENTS) - before == (NSEG if aligned else 0), \
                (ln, offs, ne, mode, pat.ndim)
    enc.close()


def test_batch_sha256_offset_bases(torch, cess, corc):
    """Sha256Batch of data and parity at every offset pair, the hex output between bands too,
    against hashlib."""
    k, m, ln = 2, 1, 4112
    full = codewords(corc, k, m, ln, NSEG)
    enc = cess.New(k, m)
    for offs in OFFS:
        b = Batch(torch, full, k, offs)
        hexes = Off(torch, np.zeros(NSEG * (k + m) * 64, np.uint8))
        enc.Sha256Batch(b.d.t, b.p.t, NSEG, ln, hexes.t)
        hx = hexes.get((offs, "hex")).reshape(NSEG, k + m, 64)
        for s in range(NSEG):
            for i in range(k + m):
                assert hx[s, i].tobytes().decode() == \
                    hashlib.sha256(full[s, i].tobytes()).hexdigest(), (offs, s, i)
        b.check((offs, "sha256 reads only"), full)
    enc.close()


def test_batch_audit_chunks_offset_bases(torch, cess, corc):
    """audit.audit_chunks (the gathered chunks and their hex hashes) at every offset pair against
    a numpy gather: 8192-byte fragments of 1024 chunks, the first and the last chunk among the
    four named; k_chunk_gather<false> (8-byte chunks, and bases off 16)."""
    from cess_amd import audit
    k, m, ln, cc = 2, 1, 8192, 1024
    idx = [0, 511, 700, 1023]
    chunk = ln // cc
    full = codewords(corc, k, m, ln, NSEG)
    want = np.stack([full[:, :, j * chunk:(j + 1) * chunk] for j in idx], axis=2)  # [s][i][j][8]
    enc = cess.New(k, m)
    for offs in OFFS:
        b = Batch(torch, full, k, offs)
        chunks = Off(torch, np.zeros(want.size, np.uint8), offs[0])
        hexes = Off(torch, np.zeros(NSEG * (k + m) * len(idx) * 64, np.uint8))
        audit.audit_chunks(enc, b.d.t, b.p.t, NSEG, ln, idx, d_chunks=chunks.t, d_hex=hexes.t,
                           chunk_count=cc)
        same(chunks.get((offs, "chunks")), want, (offs, "chunks"))
        hx = hexes.get((offs, "hex")).reshape(NSEG, k + m, len(idx), 64)
        for s in range(NSEG):
            for i in range(k + m):
                for j in range(len(idx)):
                    assert hx[s, i, j].tobytes().decode() == \
                        hashlib.sha256(want[s, i, j].tobytes()).hexdigest(), (offs, s, i, j)
        b.check((offs, "audit reads only"), full)
    enc.close()
