"""Parity accumulated shard by shard on the GPU: cec_encode_idx_batch / cec_update_batch, their host
forms and the Python methods (EncodeIdx, Update, EncodeIdxBatch, UpdateBatch), bit-exact against
the oracle (c_encode for full encodes, build_matrix + mul_row_acc for single contributions, run
over a whole batch as one long array: the arithmetic is per byte).

Buffer setup of every device case: the parity batch sits between two 64-byte guard bands of 0xA5
that are checked afterwards; source buffers are compared with their host copies afterwards; slots a
call must not read hold garbage that differs between the old and the new buffer."""
import ctypes
from ctypes import c_void_p

import numpy as np
import pytest

from oracle.c_oracle import c_encode

pytestmark = pytest.mark.gpu

GUARD = 64
CODES = [(2, 1), (1, 1), (4, 2), (10, 4), (17, 3), (32, 32), (3, 40), (128, 128)]
NARROW = [c for c in CODES if c[0] + c[1] <= 20]
WIDE = [c for c in CODES if c[0] + c[1] > 20]
LENS = [1, 15, 16, 17, 4096 + 16 + 3, 65536 + 16]
_BATCHES = {}
_ENCODERS = {}


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
def lib(cess):
    from cess_amd import _lib
    return _lib.load()


def encoder(cess, k, m):
    if (k, m) not in _ENCODERS:
        _ENCODERS[(k, m)] = cess.New(k, m)
    return _ENCODERS[(k, m)]


def oracle_parity(corc, k, m, data):
    """Oracle parity [nseg][m][ln] of data [nseg][k][ln]: one c_encode over the whole batch."""
    nseg, _, ln = data.shape
    cols = [np.ascontiguousarray(data[:, j, :]).reshape(-1) for j in range(k)]
    par = c_encode(corc, k, m, cols)
    return np.stack([p.reshape(nseg, ln) for p in par], axis=1)


def batch(corc, k, m, ln, nseg):
    """(data [nseg][k][ln], oracle parity [nseg][m][ln]), computed once per shape and never written
    afterwards (tests copy out of them)."""
    key = (k, m, ln, nseg)
    if key not in _BATCHES:
        rng = np.random.default_rng(k * 1000003 + m * 1009 + ln * 7 + nseg)
        data = rng.integers(0, 256, (nseg, k, ln), dtype=np.uint8)
        _BATCHES[key] = (data, oracle_parity(corc, k, m, data))
    return _BATCHES[key]


class Dev:
    """A host array on the device, `off` bytes into its allocation (0: 64-byte aligned or better),
    between guard bands when `guard`. check(want) compares the body with `want` (default: the
    bytes it was created with) and the guard bands with 0xA5."""

    def __init__(self, torch, body, off=0, guard=False):
        body = np.ascontiguousarray(body, dtype=np.uint8).reshape(-1)
        g = GUARD if guard else 0
        self.lo, self.n = off + g, body.size
        self.host = np.full(off + 2 * g + body.size, 0xA5, dtype=np.uint8)
        self.host[self.lo:self.lo + self.n] = body
        self.dev = torch.from_numpy(self.host).cuda()
        self.ptr = self.dev.data_ptr() + self.lo

    def check(self, what, want=None):
        got = self.dev.cpu().numpy()
        lo, hi = self.lo, self.lo + self.n
        assert (got[:lo] == self.host[:lo]).all(), (what, "low guard band written")
        assert (got[hi:] == self.host[hi:]).all(), (what, "high guard band written")
        want = self.host[lo:hi] if want is None else np.ascontiguousarray(want).reshape(-1)
        bad = np.flatnonzero(got[lo:hi] != want)
        assert bad.size == 0, (what, "first wrong byte", int(bad[0]) if bad.size else -1)


def encode_idx(lib, enc, shard_ptr, stride, idx, par_ptr, nseg, ln, accumulate=1):
    return lib.cec_encode_idx_batch(enc._h, shard_ptr, stride, idx, par_ptr, nseg, ln, accumulate,
                                    None)


def update(lib, enc, old_ptr, new_ptr, par_ptr, nseg, ln, changed):
    flags = (ctypes.c_uint8 * len(changed))(*changed)
    return lib.cec_update_batch(enc._h, old_ptr, new_ptr, par_ptr, nseg, ln, flags, None)


# ---- 1. EncodeIdx of every shard equals Encode ---------------------------------------------------

# narrow codes: every length with one and three segments; wide codes: every length, the segment
# count alternating (the kernels differ between codes only in the output bucket and the chunking)
FULL_CASES = ([(k, m, ln, nseg) for k, m in NARROW for ln in LENS for nseg in (1, 3)] +
              [(k, m, ln, 3 if i % 2 == 0 else 1) for k, m in WIDE for i, ln in enumerate(LENS)])


@pytest.mark.parametrize("k,m,ln,nseg", FULL_CASES)
def test_encode_idx_every_shard_equals_encode(torch, cess, lib, corc, k, m, ln, nseg):
    data, par = batch(corc, k, m, ln, nseg)
    enc = encoder(cess, k, m)
    d_data = Dev(torch, data)
    d_par = Dev(torch, np.zeros(nseg * m * ln, np.uint8), guard=True)
    order = np.random.default_rng(k + 31 * m + ln).permutation(k)
    for j in order:
        assert encode_idx(lib, enc, d_data.ptr + int(j) * ln, k * ln, int(j), d_par.ptr, nseg,
                          ln) == 0
    torch.cuda.synchronize()
    d_par.check((k, m, ln, nseg), par)
    d_data.check((k, m, ln, nseg, "data"))


# ---- 2. a subset gives the encode with the other shards zeroed -------------------------------------


@pytest.mark.parametrize("k,m", [(10, 4), (32, 32)])
def test_encode_idx_subset(torch, cess, lib, corc, orc, k, m):
    nseg, ln = 3, 4096 + 16
    data, _ = batch(corc, k, m, ln, nseg)
    enc = encoder(cess, k, m)
    rng = np.random.default_rng(5 * k + m)
    subset = sorted(rng.choice(k, size=k // 2, replace=False).tolist())
    # the oracle's matrix, a column at a time: a row / column mix-up shows here
    E = orc.build_matrix(k, k + m)
    want = np.zeros((m, nseg * ln), dtype=np.uint8)
    for j in subset:
        col = np.ascontiguousarray(data[:, j, :]).reshape(-1)
        for o in range(m):
            orc.mul_row_acc(want[o], E[k + o][j], col)
    want = np.stack([w.reshape(nseg, ln) for w in want], axis=1)
    zeroed = data.copy()
    zeroed[:, [j for j in range(k) if j not in subset], :] = 0
    assert np.array_equal(want, oracle_parity(corc, k, m, zeroed))
    d_data = Dev(torch, data)
    d_par = Dev(torch, np.zeros(nseg * m * ln, np.uint8), guard=True)
    for j in rng.permutation(subset):
        assert encode_idx(lib, enc, d_data.ptr + int(j) * ln, k * ln, int(j), d_par.ptr, nseg,
                          ln) == 0
    torch.cuda.synchronize()
    d_par.check((k, m, "subset"), want)
    d_data.check((k, m, "subset data"))


# ---- 3. overwrite -------------------------------------------------------------------------------


@pytest.mark.parametrize("k,m,ln,nseg", [(2, 1, 4096 + 16, 3), (2, 1, 4096 + 16 + 3, 1),
                                         (10, 4, 17, 3), (3, 40, 4096 + 16, 3)])
def test_overwrite_first_shard(torch, cess, lib, corc, k, m, ln, nseg):
    """accumulate = 0 onto garbage parity gives the bytes of accumulate = 1 onto zeros; the rest
    of the shards then accumulate to the full encode."""
    data, par = batch(corc, k, m, ln, nseg)
    enc = encoder(cess, k, m)
    rng = np.random.default_rng(ln + k)
    d_data = Dev(torch, data)
    d_zero = Dev(torch, np.zeros(nseg * m * ln, np.uint8), guard=True)
    d_garb = Dev(torch, rng.integers(0, 256, nseg * m * ln, dtype=np.uint8), guard=True)
    first = k - 1
    assert encode_idx(lib, enc, d_data.ptr + first * ln, k * ln, first, d_zero.ptr, nseg, ln, 1) == 0
    assert encode_idx(lib, enc, d_data.ptr + first * ln, k * ln, first, d_garb.ptr, nseg, ln, 0) == 0
    torch.cuda.synchronize()
    one = d_zero.dev.cpu().numpy()[GUARD:GUARD + nseg * m * ln]
    d_garb.check((k, m, ln, "overwrite"), one)
    d_zero.check((k, m, ln, "accumulate onto zeros"), one)
    for j in range(k - 1):
        assert encode_idx(lib, enc, d_data.ptr + j * ln, k * ln, j, d_garb.ptr, nseg, ln, 1) == 0
    torch.cuda.synchronize()
    d_garb.check((k, m, ln, "overwrite then accumulate"), par)
    d_data.check((k, m, ln, "data"))


# ---- 4. strides ---------------------------------------------------------------------------------


@pytest.mark.parametrize("ln,pad", [(4096 + 16, 48), (4096 + 16 + 3, 5)])
def test_strides(torch, cess, lib, corc, orc, ln, pad):
    """The same shard from the batch layout (stride k * len), packed alone (stride len) and with a
    padded stride gives the same parity."""
    k, m, nseg, idx = 10, 4, 3, 3
    data, _ = batch(corc, k, m, ln, nseg)
    enc = encoder(cess, k, m)
    rng = np.random.default_rng(ln)
    shard = np.ascontiguousarray(data[:, idx, :])
    E = orc.build_matrix(k, k + m)
    want = np.zeros((nseg, m, ln), dtype=np.uint8)
    for o in range(m):
        acc = np.zeros(nseg * ln, dtype=np.uint8)
        orc.mul_row_acc(acc, E[k + o][idx], shard.reshape(-1))
        want[:, o, :] = acc.reshape(nseg, ln)
    padded = rng.integers(0, 256, (nseg, ln + pad), dtype=np.uint8)  # garbage between the shards
    padded[:, :ln] = shard
    sources = [(Dev(torch, data), idx * ln, k * ln), (Dev(torch, shard), 0, ln),
               (Dev(torch, padded), 0, ln + pad)]
    for src, first, stride in sources:
        d_par = Dev(torch, rng.integers(0, 256, nseg * m * ln, dtype=np.uint8), guard=True)
        assert encode_idx(lib, enc, src.ptr + first, stride, idx, d_par.ptr, nseg, ln, 0) == 0
        torch.cuda.synchronize()
        d_par.check((ln, "stride", stride), want)
        src.check((ln, "source of stride", stride))


# ---- 5. alignment -------------------------------------------------------------------------------


@pytest.mark.parametrize("k,m,nseg", [(2, 1, 1), (10, 4, 3)])
@pytest.mark.parametrize("off,ln", [(1, 4096 + 16 + 3), (8, 4096 + 16 + 3), (1, 4096 + 16),
                                    (0, 4096 + 3)])
def test_alignment(torch, cess, lib, corc, k, m, nseg, off, ln):
    """Every buffer `off` bytes into its allocation (the byte path), and an aligned base with a
    length that is no multiple of 16 (RS(2,1), one segment: 16-byte columns plus a byte tail)."""
    data, par = batch(corc, k, m, ln, nseg)
    enc = encoder(cess, k, m)
    rng = np.random.default_rng(off * 100 + ln + k)
    d_data = Dev(torch, data, off=off)
    d_par = Dev(torch, rng.integers(0, 256, nseg * m * ln, dtype=np.uint8), off=off, guard=True)
    for j in range(k):
        assert encode_idx(lib, enc, d_data.ptr + j * ln, k * ln, j, d_par.ptr, nseg, ln,
                          0 if j == 0 else 1) == 0
    torch.cuda.synchronize()
    d_par.check((k, m, off, ln, "encode_idx"), par)
    d_data.check((k, m, off, ln, "data"))
    # Update of shard k - 1 in the same placement
    new = data.copy()
    new[:, k - 1, :] = rng.integers(0, 256, (nseg, ln), dtype=np.uint8)
    d_new = Dev(torch, new, off=off)
    assert update(lib, enc, d_data.ptr, d_new.ptr, d_par.ptr, nseg, ln,
                  [0] * (k - 1) + [1]) == 0
    torch.cuda.synchronize()
    d_par.check((k, m, off, ln, "update"), oracle_parity(corc, k, m, new))
    d_new.check((k, m, off, ln, "new"))


# ---- 6. more segments than one grid slice ----------------------------------------------------------


@pytest.mark.parametrize("ln", [16, 1])
def test_grid_slicing(torch, cess, lib, corc, ln):
    k, m, nseg = 2, 1, 65537
    data, par = batch(corc, k, m, ln, nseg)
    enc = encoder(cess, k, m)
    d_data = Dev(torch, data)
    d_par = Dev(torch, np.full(nseg * m * ln, 0x3C, np.uint8), guard=True)
    assert encode_idx(lib, enc, d_data.ptr + ln, k * ln, 1, d_par.ptr, nseg, ln, 0) == 0
    assert encode_idx(lib, enc, d_data.ptr, k * ln, 0, d_par.ptr, nseg, ln, 1) == 0
    torch.cuda.synchronize()
    d_par.check(("slices", ln), par)
    d_data.check(("slices data", ln))


# ---- 7. Update ------------------------------------------------------------------------------------


def update_masks(k, m):
    masks = {"one": [k // 2], "all": list(range(k))}
    if (k, m) == (17, 3):
        masks["all17"] = list(range(17))  # three input chunks
    if (k, m) == (32, 32):
        masks["twenty"] = list(range(3, 23))
    if (k, m) == (3, 40):
        masks["two"] = [0, 2]  # two output chunks
    return masks


UPDATE_CASES = [(k, m, ln, nseg) for k, m in CODES
                for ln, nseg in ((1, 3), (4096 + 16, 3), (4096 + 16 + 3, 1))]


@pytest.mark.parametrize("k,m,ln,nseg", UPDATE_CASES)
def test_update(torch, cess, lib, corc, k, m, ln, nseg):
    data, par = batch(corc, k, m, ln, nseg)
    enc = encoder(cess, k, m)
    rng = np.random.default_rng(7 * k + m + ln)
    for name, mask in update_masks(k, m).items():
        flags = [1 if j in mask else 0 for j in range(k)]
        new = data.copy()
        new[:, mask, :] = rng.integers(0, 256, (nseg, len(mask), ln), dtype=np.uint8)
        want = oracle_parity(corc, k, m, new)
        # slots the call must not read: garbage that differs between old and new
        old_buf, new_buf = data.copy(), new.copy()
        rest = [j for j in range(k) if j not in mask]
        old_buf[:, rest, :] = rng.integers(0, 256, (nseg, len(rest), ln), dtype=np.uint8)
        new_buf[:, rest, :] = old_buf[:, rest, :] ^ 0x5A
        d_old, d_new = Dev(torch, old_buf), Dev(torch, new_buf)
        d_par = Dev(torch, par, guard=True)
        assert update(lib, enc, d_old.ptr, d_new.ptr, d_par.ptr, nseg, ln, flags) == 0
        torch.cuda.synchronize()
        d_par.check((k, m, ln, name), want)
        d_old.check((k, m, ln, name, "old"))
        d_new.check((k, m, ln, name, "new"))
        # the Python form, back again: new -> old on the same flags restores the old parity
        enc.UpdateBatch(d_new.dev[d_new.lo:], d_old.dev[d_old.lo:], d_par.dev[d_par.lo:], nseg, ln,
                        flags)
        torch.cuda.synchronize()
        d_par.check((k, m, ln, name, "back"), par)
        # an empty mask, and new == old on the flagged shards, leave the parity as it is
        assert update(lib, enc, d_old.ptr, d_new.ptr, d_par.ptr, nseg, ln, [0] * k) == 0
        assert update(lib, enc, d_old.ptr, d_old.ptr, d_par.ptr, nseg, ln, flags) == 0
        torch.cuda.synchronize()
        d_par.check((k, m, ln, name, "no-ops"), par)


# ---- 8. host forms ---------------------------------------------------------------------------------


@pytest.mark.parametrize("k,m", [(2, 1), (10, 4), (32, 32)])
def test_host_forms(cess, corc, k, m):
    ln = 2049
    data, par = batch(corc, k, m, ln, 1)
    data, par = data[0], par[0]
    enc = encoder(cess, k, m)
    rng = np.random.default_rng(k + m)
    parity = [np.zeros(ln, dtype=np.uint8) for _ in range(m)]
    for j in rng.permutation(k):
        src = data[j].copy()
        enc.EncodeIdx(src, int(j), parity)
        assert np.array_equal(src, data[j])
    for o in range(m):
        assert np.array_equal(parity[o], par[o]), (k, m, o)
    # Update: a few shards change, the unchanged old shards are None
    changed = sorted(rng.choice(k, size=max(1, k // 3), replace=False).tolist())
    new = data.copy()
    new[changed] = rng.integers(0, 256, (len(changed), ln), dtype=np.uint8)
    want = oracle_parity(corc, k, m, new[None])[0]
    shards = [data[j].copy() if j in changed else None for j in range(k)] + parity
    newd = [new[j].copy() if j in changed else None for j in range(k)]
    enc.Update(shards, newd)
    for j in changed:
        assert np.array_equal(shards[j], data[j]), "an old data shard was written"
        assert np.array_equal(newd[j], new[j])
    for o in range(m):
        assert np.array_equal(shards[k + o], want[o]), (k, m, o)
    # nothing changed: nothing happens
    enc.Update(shards, [None] * k)
    for o in range(m):
        assert np.array_equal(shards[k + o], want[o])


def test_host_form_errors_write_nothing(cess, corc):
    k, m, ln = 4, 2, 100
    data, par = batch(corc, k, m, ln, 1)
    data, par = data[0], par[0]
    enc = encoder(cess, k, m)

    def parity():
        return [p.copy() for p in par]

    def intact(p):
        assert all(np.array_equal(a, b) for a, b in zip(p, par))

    for bad_idx in (-1, k):
        p = parity()
        with pytest.raises(cess.ErrInvShardNum):
            enc.EncodeIdx(data[0], bad_idx, p)
        intact(p)
    p = parity()
    with pytest.raises(cess.ErrTooFewShards):
        enc.EncodeIdx(data[0], 0, p[:1])
    with pytest.raises(cess.ErrShardSize):
        enc.EncodeIdx(data[0][:50], 0, p)
    with pytest.raises(cess.ErrShardSize):
        enc.EncodeIdx(data[0], 0, [p[0], p[1][:50]])
    with pytest.raises(cess.ErrShardNoData):
        enc.EncodeIdx(np.zeros(0, np.uint8), 0, p)
    with pytest.raises(cess.ErrInvalidInput):
        enc.EncodeIdx(data[0], 0, [p[0], None])
    intact(p)
    shards = [d.copy() for d in data] + p
    new0 = [data[1].copy()] + [None] * (k - 1)
    with pytest.raises(cess.ErrTooFewShards):
        enc.Update(shards[:-1], new0)
    with pytest.raises(cess.ErrTooFewShards):
        enc.Update(shards, new0[:-1])
    with pytest.raises(cess.ErrShardSize):
        enc.Update(shards, [data[1][:50].copy()] + [None] * (k - 1))
    with pytest.raises(cess.ErrShardNoData):
        enc.Update([None] * (k + m), [None] * k)
    with pytest.raises(cess.ErrInvalidInput):
        enc.Update([None] + shards[1:], new0)
    with pytest.raises(cess.ErrInvalidInput):
        enc.Update(shards[:-1] + [None], new0)
    intact(p)
    assert all(np.array_equal(a, b) for a, b in zip(shards[:k], data))


# ---- 9. refusals at the C level ---------------------------------------------------------------------


def test_refusals_write_nothing(torch, cess, lib):
    from cess_amd import _lib
    k, m, ln, nseg = 2, 1, 1024, 3
    enc = encoder(cess, k, m)
    rng = np.random.default_rng(99)
    arena = Dev(torch, rng.integers(0, 256, 16384, dtype=np.uint8), guard=True)
    a = arena.ptr

    def refused(rc, what):
        assert rc == _lib.CEC_EINVAL, what
        torch.cuda.synchronize()
        arena.check(what)

    # shards at a + s * 4096: [0, 1024), [4096, 5120), [8192, 9216); the parity takes 3072 bytes
    refused(encode_idx(lib, enc, a, 4096, 0, a + 1025, nseg, ln), "parity meets the second shard")
    refused(encode_idx(lib, enc, a, 4096, 0, a + 1023, nseg, ln), "parity meets the first shard")
    refused(encode_idx(lib, enc, a, 4096, 0, a + 9000, nseg, ln), "parity meets the last shard")
    refused(encode_idx(lib, enc, a + 512, 4096, 0, a, nseg, ln, 0), "overwrite mode, overlapping")
    refused(encode_idx(lib, enc, a, ln - 1, 0, a + 12288, nseg, ln), "stride below the length")
    refused(encode_idx(lib, enc, a, 4096, k, a + 12288, nseg, ln), "idx == k")
    refused(encode_idx(lib, enc, a, 4096, -1, a + 12288, nseg, ln), "idx < 0")
    refused(encode_idx(lib, enc, None, 4096, 0, a + 12288, nseg, ln), "NULL shard")
    refused(encode_idx(lib, enc, a, 4096, 0, None, nseg, ln), "NULL parity")
    assert encode_idx(lib, enc, a, 4096, 0, a + 12288, nseg, 0) == _lib.CEC_ESHARDLEN
    assert encode_idx(lib, enc, a, 4096, 0, a + 12288, 0, ln) == _lib.CEC_OK
    # Update: old [3][2][1024] at a, new at a + 6144; parity inside a flagged slot of either
    flags = (ctypes.c_uint8 * 2)(1, 0)
    refused(lib.cec_update_batch(enc._h, a, a + 6144, a + 4000, nseg, ln, flags, None),
            "parity meets an old shard")
    refused(lib.cec_update_batch(enc._h, a, a + 6144, a + 12288 - 3072 + 1, nseg, ln, flags, None),
            "parity meets a new shard")
    refused(lib.cec_update_batch(enc._h, a, a + 6144, a + 12288, nseg, ln, None, None),
            "NULL flags")
    refused(lib.cec_update_batch(enc._h, a, None, a + 12288, nseg, ln, flags, None), "NULL new")
    assert lib.cec_update_batch(enc._h, a, a + 6144, a + 12288, nseg, 0, flags,
                                None) == _lib.CEC_ESHARDLEN
    assert lib.cec_update_batch(enc._h, a, a + 6144, a + 12288, 0, ln, flags, None) == _lib.CEC_OK
    torch.cuda.synchronize()
    arena.check("no-op calls")
    # what is allowed: the parity exactly in the gap between two shards, one segment's parity on
    # an unflagged slot, a stride below the length with one segment
    before = arena.host[arena.lo:arena.lo + arena.n].copy()
    assert encode_idx(lib, enc, a, 4096, 0, a + 1024, nseg, ln, 0) == _lib.CEC_OK
    assert lib.cec_update_batch(enc._h, a + 8192, a + 12288, a + 8192 + 1024, 1, ln, flags,
                                None) == _lib.CEC_OK
    assert encode_idx(lib, enc, a + 4096, 0, 0, a + 5120, 1, ln, 0) == _lib.CEC_OK
    torch.cuda.synchronize()
    got = arena.dev.cpu().numpy()[arena.lo:arena.lo + arena.n]
    for lo, hi in ((0, 1024), (4096, 5120), (8192, 9216), (12288, 16384)):
        assert np.array_equal(got[lo:hi], before[lo:hi]), ("a source was written", lo)
    torch.cuda.synchronize()
