"""Scattered shards and required subsets on the GPU: cec_reconstruct_ptrs / cec_encode_ptrs (every
shard its own device buffer, addressed through a pointer table), cec_reconstruct_some_batch (only
the required lost shards of the batch layout) and their Python forms, bit-exact against the C
oracle.

Buffer setup of every pointer-table case: every shard is its own tensor, allocated in shuffled
order; every destination sits inside a larger tensor between two 64-byte guard bands of 0xA5 that
are checked afterwards; present shards beyond the k survivors cec_survivors names, and every
destination before the call, hold random garbage (so a kernel that read anything but the named
survivors, or skipped an output, cannot pass). Every pointer handed to the library is a live
allocation of sufficient size."""
import ctypes
from ctypes import c_void_p

import numpy as np
import pytest

from oracle.c_oracle import c_encode

pytestmark = pytest.mark.gpu

GUARD = 64
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
    written afterwards (tests copy out of them)."""
    key = (k, m, ln, nseg)
    if key not in _CODEWORDS:
        rng = np.random.default_rng(k * 1000003 + m * 1009 + ln + nseg)
        segs = []
        for _ in range(nseg):
            data = [rng.integers(0, 256, ln, dtype=np.uint8) for _ in range(k)]
            segs.append(data + c_encode(corc, k, m, data))
        _CODEWORDS[key] = segs
    return _CODEWORDS[key]


def survivors(cess, k, m, present):
    from cess_amd import _lib
    flags = np.asarray(present, dtype=np.uint8)
    out = np.zeros(k, dtype=np.uint8)
    assert _lib.load().cec_survivors(k, m, flags.ctypes.data, out.ctypes.data) == 0
    return [int(i) for i in out]


class Scattered:
    """One segment as separate device buffers (see the module docstring). `want` lists the lost
    shards that get a destination; `off` shifts every source and destination view by that many
    bytes from its allocation (0: 64-byte aligned or better)."""

    def __init__(self, torch, cess, rng, k, m, full, present, want, off=0):
        n, ln = k + m, len(full[0])
        self.full, self.want, self.ln, self.off = full, list(want), ln, off
        # below k present the call is refused; every present shard then counts as a survivor
        surv = (set(survivors(cess, k, m, present)) if int(np.sum(present != 0)) >= k
                else set(np.flatnonzero(present).tolist()))
        self.src, self.dst, self.big = [None] * n, [None] * n, {}
        for i in rng.permutation(n):
            i = int(i)
            if present[i]:
                body = full[i] if i in surv else rng.integers(0, 256, ln, dtype=np.uint8)
                t = torch.empty(ln + off, dtype=torch.uint8, device="cuda")
                t[off:].copy_(torch.from_numpy(body))
                self.src[i] = t[off:]
            else:
                host = np.full(ln + 2 * GUARD + off, 0xA5, dtype=np.uint8)
                host[GUARD + off:GUARD + off + ln] = rng.integers(0, 256, ln, dtype=np.uint8)
                self.big[i] = (torch.from_numpy(host).cuda(), host)
                if i in self.want:
                    self.dst[i] = self.big[i][0][GUARD + off:GUARD + off + ln]

    def ptrs(self):
        s = [None if t is None else t.data_ptr() for t in self.src]
        d = [None if t is None else t.data_ptr() for t in self.dst]
        return s, d

    def check(self, what):
        """Wanted shards equal the oracle's, guard bands are intact, and lost shards that were
        not asked for still hold what they held."""
        lo = GUARD + self.off
        for i, (dev, before) in self.big.items():
            got = dev.cpu().numpy()
            assert (got[:lo] == before[:lo]).all(), (what, i, "low guard band written")
            assert (got[lo + self.ln:] == 0xA5).all(), (what, i, "high guard band written")
            if i in self.want:
                bad = np.flatnonzero(got[lo:lo + self.ln] != self.full[i])
                assert bad.size == 0, (what, i, "first wrong byte", int(bad[0]) if bad.size else -1)
            else:
                assert np.array_equal(got, before), (what, i, "an unwanted shard was written")


def call_ptrs(enc, segs, ln, scribble=False):
    """cec_reconstruct_ptrs over a list of Scattered segments; returns the C return code. With
    `scribble` the host pointer arrays are overwritten as soon as the call has returned."""
    from cess_amd import _lib
    n = enc.Shards
    src, dst = [], []
    for sg in segs:
        s, d = sg.ptrs()
        src += s
        dst += d
    a = (c_void_p * max(1, len(src)))(*src)
    b = (c_void_p * max(1, len(dst)))(*dst)
    rc = _lib.load().cec_reconstruct_ptrs(enc._h, a, b, len(segs), ln, None)
    if scribble:
        ctypes.memset(a, 0xFF, ctypes.sizeof(a))
        ctypes.memset(b, 0xFF, ctypes.sizeof(b))
    assert len(src) == len(segs) * n
    return rc


def random_pattern(rng, n, nlost):
    present = np.ones(n, dtype=np.uint8)
    lost = sorted(rng.choice(n, size=nlost, replace=False).tolist())
    present[lost] = 0
    return present, lost


# ---- RS(2,1): the product geometry, compile-time kernel ---------------------------------------

RS21_LENS = [1, 15, 16, 4096 + 16 + 3, 65536]


@pytest.mark.parametrize("ln", RS21_LENS)
def test_rs21_mixed_cases_one_call(torch, cess, corc, ln):
    """7 segments in one call: lost d0, lost d1, lost parity, and a segment with nothing wanted
    (once intact, once with a lost shard nobody asked for). The host pointer arrays are
    overwritten right after the call returns, before the stream is synchronised."""
    k, m, nseg = 2, 1, 7
    rng = np.random.default_rng(21 + ln)
    full = codewords(corc, k, m, ln, nseg)
    enc = cess.New(k, m)
    segs = []
    for s in range(nseg):
        present = np.ones(3, dtype=np.uint8)
        want = []
        if s == 3:
            pass  # intact: nothing to do
        elif s == 6:
            present[1] = 0  # lost, not wanted
        else:
            present[s % 3] = 0
            want = [s % 3]
        segs.append(Scattered(torch, cess, rng, k, m, full[s], present, want))
    assert call_ptrs(enc, segs, ln, scribble=True) == 0
    torch.cuda.synchronize()
    for s, sg in enumerate(segs):
        sg.check(("rs21", ln, s))


@pytest.mark.parametrize("ln", RS21_LENS)
def test_rs21_encode_ptrs(torch, cess, corc, ln):
    from cess_amd import _lib
    k, m, nseg = 2, 1, 7
    rng = np.random.default_rng(210 + ln)
    full = codewords(corc, k, m, ln, nseg)
    enc = cess.New(k, m)
    present = np.array([1, 1, 0], dtype=np.uint8)
    segs = [Scattered(torch, cess, rng, k, m, full[s], present, [2]) for s in range(nseg)]
    data = (c_void_p * (nseg * k))(*[sg.src[i].data_ptr() for sg in segs for i in range(k)])
    par = (c_void_p * (nseg * m))(*[sg.dst[2].data_ptr() for sg in segs])
    assert _lib.load().cec_encode_ptrs(enc._h, data, par, nseg, ln, None) == 0
    torch.cuda.synchronize()
    for s, sg in enumerate(segs):
        sg.check(("rs21 encode", ln, s))
    # the klauspost-shaped form: one segment, a list of k + m tensors
    sh = [segs[0].src[0], segs[0].src[1], torch.zeros(ln, dtype=torch.uint8, device="cuda")]
    enc.EncodeDevice(sh)
    torch.cuda.synchronize()
    assert np.array_equal(sh[2].cpu().numpy(), full[0][2])


@pytest.mark.parametrize("off", [1, 8])
def test_rs21_unaligned_views(torch, cess, corc, off):
    """Sources and destinations `off` bytes into their allocations: the byte path."""
    k, m, nseg, ln = 2, 1, 7, 4096 + 16 + 3
    rng = np.random.default_rng(2100 + off)
    full = codewords(corc, k, m, ln, nseg)
    enc = cess.New(k, m)
    segs = []
    for s in range(nseg):
        present = np.ones(3, dtype=np.uint8)
        present[s % 3] = 0
        segs.append(Scattered(torch, cess, rng, k, m, full[s], present, [s % 3], off=off))
    assert call_ptrs(enc, segs, ln) == 0
    torch.cuda.synchronize()
    for s, sg in enumerate(segs):
        sg.check(("rs21 unaligned", off, s))


# ---- narrow run-time codes --------------------------------------------------------------------


@pytest.mark.parametrize("k,m", [(4, 2), (10, 4)])
@pytest.mark.parametrize("subset", ["one", "all"])
def test_narrow_codes_random_erasures(torch, cess, corc, k, m, subset):
    nseg, ln = 6, 4099
    rng = np.random.default_rng(k * 10 + m + len(subset))
    full = codewords(corc, k, m, ln, nseg)
    enc = cess.New(k, m)
    segs = []
    for s in range(nseg):
        present, lost = random_pattern(rng, k + m, 1 + s % m)
        want = [int(rng.choice(lost))] if subset == "one" else lost
        segs.append(Scattered(torch, cess, rng, k, m, full[s], present, want))
    assert call_ptrs(enc, segs, ln) == 0
    torch.cuda.synchronize()
    for s, sg in enumerate(segs):
        sg.check((k, m, subset, s))


# ---- RS(32,32) ------------------------------------------------------------------------------

WIDE_LENS = [4096, (1 << 16) + 16]
WIDE_MISSING = [1, 4, 8, 32]


def wide_subsets(rng, lost):
    """Required subsets of 1, 3 and all of the lost shards (as far as there are that many), and
    one of just over half: a proper subset wide enough for the FFT-domain decoders."""
    out = []
    for size in (1, 3, len(lost) // 2 + 1, len(lost)):
        size = min(size, len(lost))
        sub = sorted(rng.choice(lost, size=size, replace=False).tolist())
        if sub not in out:
            out.append(sub)
    return out


@pytest.mark.parametrize("ln", WIDE_LENS)
@pytest.mark.parametrize("missing", WIDE_MISSING)
def test_wide_reconstruct_device(torch, cess, corc, ln, missing):
    """ReconstructDevice on lists of 64 tensors: one to four required shards run the bit-plane
    kernel, more the general one (8: one bucket; 32: the widest)."""
    k = m = 32
    nseg = 4
    rng = np.random.default_rng(3200 + ln + missing)
    full = codewords(corc, k, m, ln, nseg)
    enc = cess.New(k, m)
    for s in range(nseg):
        present, lost = random_pattern(rng, k + m, missing)
        for sub in wide_subsets(rng, lost):
            sg = Scattered(torch, cess, rng, k, m, full[s], present, sub)
            shards = list(sg.src)
            required = [i in sub for i in range(k + m)]
            enc.ReconstructDevice(shards, required, out={i: sg.dst[i] for i in sub})
            torch.cuda.synchronize()
            sg.check(("wide", ln, missing, s, sub))
            for i in range(k + m):
                if i in sub:
                    assert shards[i].data_ptr() == sg.dst[i].data_ptr()
                elif not present[i]:
                    assert shards[i] is None
    # required=None, out=None: every lost shard, freshly allocated
    present, lost = random_pattern(rng, k + m, missing)
    sg = Scattered(torch, cess, rng, k, m, full[0], present, [])
    shards = list(sg.src)
    enc.ReconstructDevice(shards)
    torch.cuda.synchronize()
    for i in lost:
        assert np.array_equal(shards[i].cpu().numpy(), full[0][i]), (ln, missing, i)


@pytest.mark.parametrize("ln", WIDE_LENS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_wide_some_batch(torch, cess, corc, ln, mode):
    """cec_reconstruct_some_batch on the batch layout, through the cost model (mode 0) and each
    FFT-domain decoder forced (1: syndrome rows, 2: formal derivative; they take the layouts they
    fit, the run-time kernels the rest). Lost shards that were not required are pre-filled with a
    pattern and must come back unchanged; present shards beyond the survivors hold garbage."""
    from cess_amd import _lib
    k = m = 32
    n, nseg = k + m, 4
    rng = np.random.default_rng(6400 + ln + mode)
    full = codewords(corc, k, m, ln, nseg)
    enc = cess.New(k, m)
    enc.set_option(_lib.CEC_OPT_FFTDEC_MODE, mode)
    for missing in WIDE_MISSING:
        base_present, base_lost = random_pattern(rng, n, missing)
        for sub in wide_subsets(rng, base_lost):
            for per_segment in (0, 1):
                presents, requireds = [], []
                host = np.empty((nseg, n, ln), dtype=np.uint8)
                for s in range(nseg):
                    if per_segment and s:
                        present, lost = random_pattern(rng, n, missing)
                        req = sorted(rng.choice(lost, size=len(sub), replace=False).tolist())
                    else:
                        present, lost, req = base_present, base_lost, sub
                    surv = set(survivors(cess, k, m, present))
                    required = np.zeros(n, dtype=np.uint8)
                    required[req] = 1
                    required[int(np.flatnonzero(present)[0])] = 1  # ignored: the shard is there
                    for i in range(n):
                        if i in surv:
                            host[s, i] = full[s][i]
                        elif present[i]:
                            host[s, i] = rng.integers(0, 256, ln, dtype=np.uint8)
                        else:
                            host[s, i] = 0x5C
                    presents.append(present)
                    requireds.append(required)
                d_data = torch.from_numpy(host[:, :k].copy()).cuda()
                d_par = torch.from_numpy(host[:, k:].copy()).cuda()
                if per_segment:
                    enc.ReconstructSomeBatch(d_data, d_par, nseg, ln, np.stack(presents),
                                             np.stack(requireds))
                else:
                    enc.ReconstructSomeBatch(d_data, d_par, nseg, ln, presents[0], requireds[0])
                torch.cuda.synchronize()
                got = np.concatenate([d_data.cpu().numpy(), d_par.cpu().numpy()], axis=1)
                for s in range(nseg):
                    for i in range(n):
                        asked = requireds[s][i] and not presents[s][i]
                        want = full[s][i] if asked else host[s, i]
                        assert np.array_equal(got[s, i], want), (ln, mode, missing, sub,
                                                                 per_segment, s, i, bool(asked))
    if mode and ln % 1024 == 0:  # the forced decoder did run (subsets of four outputs and more)
        assert enc.stat(_lib.CEC_STAT_FFTDEC_SEGMENTS) > 0
        assert (enc.stat(_lib.CEC_STAT_FFTDEC_D_SEGMENTS) > 0) == (mode == 2)


# ---- the table kernels against the in-layout kernels, bucket by bucket ---------------------------

# (CEC_OPT_RT_MODE, lost fragments): mode 1 runs the per-bit mask product (k_rt / k_ptrt) in every
# output bucket 1..8, 12, 16, 24, 32; mode 3 the bit-plane product (k_rtb / k_ptrb) in its four
BUCKET_CASES = ([(1, c) for c in (1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 17, 25)] +
                [(3, c) for c in (1, 2, 3, 4)])
# (shard length, view offset): 4117 = vector blocks and a tail that is not empty for 16-, 8- and
# 4-byte columns (separate aligned buffers; the batch layout's shard stride is the odd length
# itself, so there the same bytes come from the byte path); 333 bytes one byte into every
# allocation = the byte path everywhere
BUCKET_SHAPES = [(4117, 0), (333, 1)]


def guarded_batch(torch, host, off):
    """`host` ([nseg][shards][len]) on the device between two guard bands, `off` more bytes into
    its allocation; returns (the whole allocation, the view)."""
    flat = np.full(host.size + 2 * GUARD + off, 0xA5, dtype=np.uint8)
    flat[GUARD + off:GUARD + off + host.size] = host.reshape(-1)
    big = torch.from_numpy(flat).cuda()
    return big, big[GUARD + off:GUARD + off + host.size].view(*host.shape)


def batch_result(big, host, off):
    """The batch back on the host after its guard bands were checked."""
    got = big.cpu().numpy()
    lo = GUARD + off
    assert (got[:lo] == 0xA5).all() and (got[lo + host.size:] == 0xA5).all(), "guard band written"
    return got[lo:lo + host.size].reshape(host.shape)


@pytest.mark.parametrize("ln,off", BUCKET_SHAPES)
@pytest.mark.parametrize("mode,nlost", BUCKET_CASES)
def test_table_and_layout_kernels_agree(torch, cess, corc, mode, nlost, ln, off):
    """RS(32,32) without the FFT-domain decoders, three segments with a different lost set each,
    every lost shard rebuilt three ways: one per-segment ReconstructSomeBatch (the in-layout
    kernel, a chunk per workgroup row), one uniform ReconstructBatch on segment 0's pattern (the
    in-layout kernel, one chunk for the launch) and ReconstructDevice on separate buffers (the
    table kernel). All agree with the C oracle bit for bit; nothing else is written."""
    from cess_amd import _lib
    k = m = 32
    n, nseg = k + m, 3
    rng = np.random.default_rng(70000 + 1000 * mode + 10 * nlost + off)
    full = codewords(corc, k, m, ln, nseg)
    enc = cess.New(k, m)
    enc.set_option(_lib.CEC_OPT_FFTDEC_MIN, 0)
    enc.set_option(_lib.CEC_OPT_RT_MODE, mode)
    patterns = [random_pattern(rng, n, nlost) for _ in range(nseg)]

    def batch_host(pats):
        """Survivors from the codewords, garbage in every other shard."""
        host = rng.integers(0, 256, (nseg, n, ln), dtype=np.uint8)
        for s, (present, _) in enumerate(pats):
            for i in survivors(cess, k, m, present):
                host[s, i] = full[s][i]
        return host

    def run_batch(pats, call):
        host = batch_host(pats)
        dbig, d_data = guarded_batch(torch, host[:, :k].copy(), off)
        pbig, d_par = guarded_batch(torch, host[:, k:].copy(), off)
        call(d_data, d_par)
        torch.cuda.synchronize()
        got = np.concatenate([batch_result(dbig, host[:, :k], off),
                              batch_result(pbig, host[:, k:], off)], axis=1)
        for s, (_, lost) in enumerate(pats):
            for i in range(n):
                want = full[s][i] if i in lost else host[s, i]
                assert np.array_equal(got[s, i], want), (s, i, "lost" if i in lost else "kept")
        return got

    presents = np.stack([p for p, _ in patterns])
    per_seg = run_batch(patterns, lambda d, p: enc.ReconstructSomeBatch(
        d, p, nseg, ln, presents, 1 - presents))
    uniform = run_batch([patterns[0]] * nseg, lambda d, p: enc.ReconstructBatch(
        d, p, nseg, ln, patterns[0][0]))

    for s, (present, lost) in enumerate(patterns):
        sg = Scattered(torch, cess, rng, k, m, full[s], present, lost, off=off)
        before = {i: t.cpu().numpy() for i, t in enumerate(sg.src) if t is not None}
        shards = list(sg.src)
        enc.ReconstructDevice(shards, out={i: sg.dst[i] for i in lost})
        torch.cuda.synchronize()
        sg.check(("table", mode, nlost, ln, s))
        for i, b in before.items():
            assert np.array_equal(sg.src[i].cpu().numpy(), b), (s, i, "a source was written")
        for i in lost:
            table = sg.dst[i].cpu().numpy()
            assert np.array_equal(table, per_seg[s, i]), (s, i, "table != per-segment")
            if s == 0:
                assert np.array_equal(table, uniform[0, i]), (i, "table != uniform")


# ---- rows past the grid-y limit -------------------------------------------------------------------


@pytest.mark.parametrize("k,m,rt_mode", [(2, 1, None), (4, 2, None), (4, 2, 1)])
def test_rows_past_the_grid_limit(torch, cess, corc, k, m, rt_mode):
    """65,537 segments of 16 bytes, past the 65,535-row split of a launch, that share one
    codeword's tensors as sources; data shard 0 is lost and only it is wanted, into distinct slices
    of one tensor with a guard slice at either end. RS(2,1): k_ptr21; RS(4,2): k_ptrb<1> (four
    inputs, one output), and with CEC_OPT_RT_MODE 1 k_ptrt<1>."""
    from cess_amd import _lib
    n, ln, nseg = k + m, 16, 65537
    full = codewords(corc, k, m, ln, 1)[0]
    present = np.ones(n, dtype=np.uint8)
    present[0] = 0
    surv = survivors(cess, k, m, present)
    rng = np.random.default_rng(4100 + 10 * k + (rt_mode or 0))
    held = {i: (full[i].copy() if i in surv else rng.integers(0, 256, ln, dtype=np.uint8))
            for i in range(1, n)}
    dev = {i: torch.from_numpy(h).cuda() for i, h in held.items()}
    fill = rng.integers(0, 256, (nseg + 2, ln), dtype=np.uint8)
    out = torch.from_numpy(fill).cuda()
    base = out.data_ptr() + ln
    src = ([None] + [dev[i].data_ptr() for i in range(1, n)]) * nseg
    dst = [x for s in range(nseg) for x in [base + s * ln] + [None] * (n - 1)]
    a, b = (c_void_p * len(src))(*src), (c_void_p * len(dst))(*dst)
    enc = cess.New(k, m)
    if rt_mode is not None:
        enc.set_option(_lib.CEC_OPT_RT_MODE, rt_mode)
    assert _lib.load().cec_reconstruct_ptrs(enc._h, a, b, nseg, ln, None) == 0
    torch.cuda.synchronize()
    want = fill.copy()
    want[1:-1] = full[0]
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
    for i, h in held.items():
        assert np.array_equal(dev[i].cpu().numpy(), h), (i, "a source was written")


# ---- past kRtMaxOut outputs, and the widest geometry ---------------------------------------------


def test_rs100_100_forty_of_hundred(torch, cess, corc):
    """100 lost, 40 required: two chunks of the program (32 + 8 outputs)."""
    k = m = 100
    nseg, ln = 2, 1024
    rng = np.random.default_rng(100100)
    full = codewords(corc, k, m, ln, nseg)
    enc = cess.New(k, m)
    segs = []
    for s in range(nseg):
        present, lost = random_pattern(rng, k + m, 100)
        want = sorted(rng.choice(lost, size=40, replace=False).tolist())
        segs.append(Scattered(torch, cess, rng, k, m, full[s], present, want))
    assert call_ptrs(enc, segs, ln) == 0
    torch.cuda.synchronize()
    for s, sg in enumerate(segs):
        sg.check(("rs100", s))


def test_rs128_128_five_required(torch, cess, corc):
    k = m = 128
    nseg, ln = 2, 1024
    rng = np.random.default_rng(128128)
    full = codewords(corc, k, m, ln, nseg)
    enc = cess.New(k, m)
    segs = []
    for s in range(nseg):
        present, lost = random_pattern(rng, k + m, 60)
        want = sorted(rng.choice(lost, size=5, replace=False).tolist())
        segs.append(Scattered(torch, cess, rng, k, m, full[s], present, want))
    assert call_ptrs(enc, segs, ln) == 0
    torch.cuda.synchronize()
    for s, sg in enumerate(segs):
        sg.check(("rs128", s))


# ---- the contract -----------------------------------------------------------------------------


def test_contract_errors_write_nothing(torch, cess, corc):
    from cess_amd import _lib
    lib = _lib.load()
    k, m, nseg, ln = 4, 2, 3, 1000
    n = k + m
    rng = np.random.default_rng(42)
    full = codewords(corc, k, m, ln, nseg)
    enc = cess.New(k, m)

    def fresh(bad_seg=None, bad_wants=True):
        segs = []
        for s in range(nseg):
            present = np.ones(n, dtype=np.uint8)
            lost = [0, 5] if s != bad_seg else [0, 2, 5]  # k - 1 present in the bad segment
            present[lost] = 0
            want = lost[:2] if s != bad_seg or bad_wants else []
            segs.append(Scattered(torch, cess, rng, k, m, full[s], present, want))
        return segs

    def untouched(segs, what):
        torch.cuda.synchronize()
        for sg in segs:
            for i, (dev, before) in sg.big.items():
                assert np.array_equal(dev.cpu().numpy(), before), (what, i)

    # k - 1 present in the middle segment of a multi-segment call
    segs = fresh(bad_seg=1)
    assert call_ptrs(enc, segs, ln) == _lib.CEC_ETOOFEW
    untouched(segs, "too few")
    # the same segment asking for nothing is no work and no error (klauspost: nothing required
    # returns before the shards are counted); its neighbours are rebuilt
    segs = fresh(bad_seg=1, bad_wants=False)
    assert call_ptrs(enc, segs, ln) == _lib.CEC_OK
    torch.cuda.synchronize()
    for s, sg in enumerate(segs):
        sg.check(("nothing wanted of too few", s))
    # a destination that is a survivor of its own segment
    segs = fresh()
    src, dst = [], []
    for sg in segs:
        s_, d_ = sg.ptrs()
        src += s_
        dst += d_
    dst[2 * n + 0] = src[2 * n + 1]
    a, b = (c_void_p * len(src))(*src), (c_void_p * len(dst))(*dst)
    assert lib.cec_reconstruct_ptrs(enc._h, a, b, nseg, ln, None) == _lib.CEC_EINVAL
    untouched(segs, "dst is a survivor")
    # shard_len 0, NULL arrays, nseg 0
    segs = fresh()
    assert call_ptrs(enc, segs, 0) == _lib.CEC_ESHARDLEN
    assert lib.cec_reconstruct_ptrs(enc._h, None, b, nseg, ln, None) == _lib.CEC_EINVAL
    assert lib.cec_reconstruct_ptrs(enc._h, a, None, nseg, ln, None) == _lib.CEC_EINVAL
    assert lib.cec_encode_ptrs(enc._h, None, b, nseg, ln, None) == _lib.CEC_EINVAL
    assert lib.cec_reconstruct_ptrs(enc._h, a, b, 0, ln, None) == _lib.CEC_OK
    assert lib.cec_encode_ptrs(enc._h, a, b, 0, ln, None) == _lib.CEC_OK
    untouched(segs, "no-op calls")
    # dst entries of present shards are ignored: a guarded buffer offered for one stays as it was
    segs = fresh()
    src, dst = [], []
    for sg in segs:
        s_, d_ = sg.ptrs()
        src += s_
        dst += d_
    spare = torch.full((ln + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    dst[1] = spare[GUARD:].data_ptr()  # shard 1 of segment 0 is present
    a, b = (c_void_p * len(src))(*src), (c_void_p * len(dst))(*dst)
    assert lib.cec_reconstruct_ptrs(enc._h, a, b, nseg, ln, None) == _lib.CEC_OK
    torch.cuda.synchronize()
    assert bool((spare == 0xA5).all())
    for s, sg in enumerate(segs):
        sg.check(("after the refused calls", s))


# ---- Python forms --------------------------------------------------------------------------------


@pytest.mark.parametrize("k,m", [(2, 1), (10, 4), (32, 32)])
def test_reconstruct_some_host_arrays(cess, corc, k, m):
    """klauspost ReconstructSome on host arrays: `required` of Shards or DataShards flags; shards
    nobody asked for stay None, flags on present shards are ignored."""
    n, ln = k + m, 2049
    rng = np.random.default_rng(9 * k + m)
    full = codewords(corc, k, m, ln, 1)[0]
    enc = cess.New(k, m)
    nlost = min(m, 8)
    present, lost = random_pattern(rng, n, nlost)
    if not any(i < k for i in lost):  # make sure a data shard is among the lost
        lost = sorted(set(lost[1:]) | {0})
    for req_len in (n, k):
        pool = [i for i in lost if i < req_len]
        ask = sorted(rng.choice(pool, size=max(1, len(pool) // 2), replace=False).tolist())
        shards = [None if i in lost else full[i].copy() for i in range(n)]
        required = [i in ask for i in range(req_len)]
        required[next(i for i in range(req_len) if i not in lost)] = True  # present: ignored
        enc.ReconstructSome(shards, required)
        for i in range(n):
            if i in ask:
                assert np.array_equal(shards[i], full[i]), (k, m, req_len, i)
            elif i in lost:
                assert shards[i] is None, (k, m, req_len, i)
            else:
                assert np.array_equal(shards[i], full[i])
    with pytest.raises(cess.ErrInvalidInput):
        enc.ReconstructSome([None if i in lost else full[i] for i in range(n)], [True] * (n + 1))
    with pytest.raises(cess.ErrTooFewShards):
        enc.ReconstructSome([full[i] if i < k - 1 else None for i in range(n)], [True] * n)


def test_repair_fragment_one_parity_of_wide_segment(cess, corc):
    """repair_fragment of one parity fragment of an RS(32,32) segment that lost 8."""
    from cess_amd.repair import repair_fragment
    k = m = 32
    ln = 8192
    rng = np.random.default_rng(88)
    full = codewords(corc, k, m, ln, 1)[0]
    enc = cess.New(k, m)
    index = k + 7
    others = rng.choice([i for i in range(k + m) if i != index], size=7, replace=False)
    lost = sorted(others.tolist() + [index])
    surv = {i: full[i] for i in range(k + m) if i not in lost}
    got = repair_fragment(enc, surv, index)
    assert np.array_equal(got, full[index])
