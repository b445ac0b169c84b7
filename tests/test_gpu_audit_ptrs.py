"""cec_audit_chunks_ptrs on the GPU: the challenged chunks of fragments that lie in separate
allocations, gathered and hashed in place. References: numpy slicing and hashlib.sha256, and the
batch form (cec_audit_chunks) on the same bytes packed as a batch. Every comparison is exact."""
import ctypes
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
OPT_SHA_MODE = 3
STAT_POOL_BYTES = 3
EINVAL, ESHARDLEN = -1, -3
_DATA = {}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    t.cuda.init()
    return t


@pytest.fixture(scope="module")
def enc(torch):
    import cess_amd
    e = cess_amd.New(2, 1, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def enc11(torch):
    """RS(1,1): its data-only batch [nfrag][1][len] is a plain array of fragments."""
    import cess_amd
    e = cess_amd.New(1, 1, device=0)
    yield e
    e.close()


def fragments(nfrag, ln):
    """Random fragments [nfrag][ln], made once per shape and read-only afterwards."""
    key = (nfrag, ln)
    if key not in _DATA:
        a = np.random.default_rng(nfrag * 1000003 + ln).integers(0, 256, (nfrag, ln),
                                                                   dtype=np.uint8)
        a.setflags(write=False)
        _DATA[key] = a
    return _DATA[key]


def expected(frs, idx, cc):
    """(chunks [nfrag][nidx][chunk], hex [nfrag][nidx][64] as bytes) of fragments `frs`. Aliased
    pointers are expected by indexing the result of the distinct fragments."""
    chunk = frs[0].size // cc
    want = np.stack([f.reshape(cc, chunk)[idx] for f in frs])
    hexes = np.zeros((len(frs), len(idx), 64), np.uint8)
    for f in range(len(frs)):
        for j in range(len(idx)):
            hexes[f, j] = np.frombuffer(
                hashlib.sha256(want[f, j].tobytes()).hexdigest().encode(), np.uint8)
    return want, hexes


def device_views(torch, frs, offs):
    """Each fragment in its own allocation, `offs[i]` bytes into it."""
    out = []
    for a, off in zip(frs, offs):
        base = torch.empty(a.size + 32, dtype=torch.uint8, device="cuda")
        v = base[off:off + a.size]
        v.copy_(torch.from_numpy(a.copy()))
        out.append(v)
    return out


class Guarded:
    """n output bytes `off` past a 64-byte band, another band behind, all preset to 0xA5."""

    def __init__(self, torch, n, off=0):
        self.n, self.lo = n, GUARD + off
        self.buf = torch.full((GUARD + off + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.t = self.buf[self.lo:self.lo + n]

    def get(self, what):
        a = self.buf.cpu().numpy()
        assert (a[:self.lo] == 0xA5).all(), (what, "bytes before the output")
        assert (a[self.lo + self.n:] == 0xA5).all(), (what, "bytes behind the output")
        return a[self.lo:self.lo + self.n]

    def untouched(self, what):
        assert (self.buf.cpu().numpy() == 0xA5).all(), what


def run_and_check(torch, enc, frs, offs, idx, cc, chunks_off, what, hash_only_too=True):
    from cess_amd import audit
    nfrag, ln = len(frs), frs[0].size
    chunk = ln // cc
    want, want_hex = expected(frs, idx, cc)
    views = device_views(torch, frs, offs)
    clones = [v.clone() for v in views]
    chunks = Guarded(torch, nfrag * len(idx) * chunk, chunks_off)
    hexes = Guarded(torch, nfrag * len(idx) * 64)
    audit.audit_chunks_device(enc, views, idx, d_chunks=chunks.t, d_hex=hexes.t, chunk_count=cc)
    torch.cuda.synchronize()
    assert np.array_equal(chunks.get((what, "chunks")).reshape(want.shape), want), (what, "chunks")
    assert np.array_equal(hexes.get((what, "hex")).reshape(want_hex.shape), want_hex), (what, "hex")
    only = Guarded(torch, nfrag * len(idx) * chunk, chunks_off)
    audit.audit_chunks_device(enc, views, idx, d_chunks=only.t, chunk_count=cc)
    torch.cuda.synchronize()
    assert np.array_equal(only.get((what, "chunks only")).reshape(want.shape), want), what
    if hash_only_too:
        hx = Guarded(torch, nfrag * len(idx) * 64)
        audit.audit_chunks_device(enc, views, idx, d_hex=hx.t, chunk_count=cc)
        torch.cuda.synchronize()
        assert np.array_equal(hx.get((what, "hash only")).reshape(want_hex.shape), want_hex), \
            (what, "hash only")
    for v, c in zip(views, clones):
        assert torch.equal(v, c), (what, "a fragment was written")
    return want, want_hex


CESS_IDX = [0, 1023] + list(range(7, 1000, 22))[:45]  # 47 distinct indices, both ends among them

SHAPES = [
    # shard_len, chunk_count, nfrag, indices
    (16 << 10, 1024, 5, [0, 511, 700, 1023]),        # chunk 16: one vector lane
    (1024 * 48, 1024, 5, [1023, 0, 511, 5]),         # chunk 48
    (5120, 1024, 5, [0, 511, 700, 1023]),            # chunk 5: byte path
    (8 << 20, 1024, 3, CESS_IDX),                    # CESS shape: 8 KiB chunks, two vector tiles
    (4 * 4112, 4, 5, [3, 0, 2]),                     # chunk 4112: one tile plus a one-lane tail
    (4 * 261, 4, 5, [3, 0, 2]),                      # chunk 261: byte path, two tiles, tail of 5
]


@pytest.mark.parametrize("ln,cc,nfrag,idx", SHAPES, ids=[f"{s[0]}x{s[1]}" for s in SHAPES])
def test_gather_and_hash_equal_numpy_hashlib_and_the_batch_form(torch, enc, enc11, ln, cc, nfrag,
                                                                idx):
    from cess_amd import audit
    assert len(set(idx)) == len(idx)
    data = fragments(nfrag, ln)
    order = np.random.default_rng(ln + cc).permutation(nfrag)
    frs = [data[i] for i in order]  # separate tensors, handed over in shuffled order
    want, want_hex = run_and_check(torch, enc, frs, [0] * nfrag, idx, cc, 0, (ln, cc))
    # the batch form on the same bytes packed as a batch, in the same order
    chunk = ln // cc
    d = torch.from_numpy(np.stack(frs)).cuda()
    bc = torch.zeros(nfrag * len(idx) * chunk, dtype=torch.uint8, device="cuda")
    bh = torch.zeros(nfrag * len(idx) * 64, dtype=torch.uint8, device="cuda")
    audit.audit_chunks(enc11, d, None, nfrag, ln, idx, d_chunks=bc, d_hex=bh, chunk_count=cc)
    torch.cuda.synchronize()
    assert np.array_equal(bc.cpu().numpy().reshape(want.shape), want)
    assert np.array_equal(bh.cpu().numpy().reshape(want_hex.shape), want_hex)


@pytest.mark.parametrize("ln,cc", [(4 * 4112, 4), (4 * 261, 4), (16 << 10, 1024)])
@pytest.mark.parametrize("case", ["frags+16", "frags+1 chunks+1", "one fragment +1"])
def test_offset_bases(torch, enc, ln, cc, case):
    """Views off their allocations' bases; outputs inside larger buffers of 0xA5 whose other
    bytes stay; fragments unchanged."""
    nfrag, idx = 5, [cc - 1, 0, 2]
    data = fragments(nfrag, ln)
    offs, chunks_off = {"frags+16": ([16] * nfrag, 0),
                        "frags+1 chunks+1": ([1] * nfrag, 1),
                        "one fragment +1": ([0, 0, 1, 0, 0], 0)}[case]
    run_and_check(torch, enc, [data[i] for i in (4, 2, 0, 3, 1)], offs, idx, cc, chunks_off,
                  (ln, cc, case))


def test_more_fragments_than_one_grid_is_high(torch, enc):
    """65,537 pointers (one past a grid's 65,535 rows and one more) aliasing 64 fragments: every
    row of both outputs."""
    from cess_amd import audit
    nfrag, ln, cc, idx, ndist = 65537, 32, 2, [1, 0], 64
    data = fragments(ndist, ln)
    base = torch.from_numpy(data.copy()).cuda()
    sel = np.random.default_rng(9).integers(0, ndist, nfrag)
    sel[[0, 65534, 65535, 65536]] = [63, 1, 62, 2]
    views = [base[s] for s in sel.tolist()]
    w64, h64 = expected(list(data), idx, cc)
    chunks = Guarded(torch, nfrag * 2 * 16)
    hexes = Guarded(torch, nfrag * 2 * 64)
    audit.audit_chunks_device(enc, views, idx, d_chunks=chunks.t, d_hex=hexes.t, chunk_count=cc)
    torch.cuda.synchronize()
    assert np.array_equal(chunks.get("chunks").reshape(nfrag, 2, 16), w64[sel])
    assert np.array_equal(hexes.get("hex").reshape(nfrag, 2, 64), h64[sel])
    assert np.array_equal(base.cpu().numpy(), data)


def test_hash_only_allocates_address_tables_only(torch):
    """48 pointers aliasing 3 fragments of 8 MiB, 47 indices: 18 MB of chunks are hashed where
    they lie. The codec's pool may grow by the address tables (about 20 KiB, rounded to pool
    blocks), not by anything chunk-sized: less than 1 MiB is the condition."""
    import cess_amd
    from cess_amd import audit
    ln, cc, idx = 8 << 20, 1024, CESS_IDX
    data = fragments(3, ln)
    base = device_views(torch, list(data), [0, 0, 0])
    sel = [i % 3 for i in range(48)]
    w3, h3 = expected(list(data), idx, cc)
    e = cess_amd.New(2, 1, device=0)
    hx = Guarded(torch, 48 * len(idx) * 64)
    before = e.stat(STAT_POOL_BYTES)
    audit.audit_chunks_device(e, [base[s] for s in sel], idx, d_hex=hx.t, chunk_count=cc)
    after = e.stat(STAT_POOL_BYTES)
    torch.cuda.synchronize()
    assert 48 * len(idx) * (ln // cc) > 17 << 20  # the chunk bytes a gather would have staged
    assert after - before < 1 << 20, (before, after)
    assert np.array_equal(hx.get("hex").reshape(48, len(idx), 64), h3[sel])
    e.close()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_padding_edges_of_the_in_place_hash(torch, mode, off):
    """Chunk lengths around SHA-256's padding boundaries, 140 chains over three groups of 64, in
    every one-shot kernel form; chunk 1 of a fragment starts wherever chunk 0 ends."""
    import cess_amd
    from cess_amd import audit
    e = cess_amd.New(2, 1, device=0)
    e.set_option(OPT_SHA_MODE, mode)
    nfrag, cc, idx = 70, 2, [1, 0]
    for chunk in (55, 56, 63, 64, 119, 120, 128):
        data = fragments(nfrag, cc * chunk)
        frs = list(data)
        views = device_views(torch, frs, [off] * nfrag)
        want, want_hex = expected(frs, idx, cc)
        hx = Guarded(torch, nfrag * 2 * 64)
        audit.audit_chunks_device(e, views, idx, d_hex=hx.t, chunk_count=cc)
        torch.cuda.synchronize()
        assert np.array_equal(hx.get((mode, off, chunk)).reshape(want_hex.shape), want_hex), \
            (mode, off, chunk)
    e.close()


def raw_call(enc, ptrs, nfrag, ln, cc, idx, nidx, d_chunks, d_hex):
    return enc._lib.cec_audit_chunks_ptrs(
        enc._h, ptrs, nfrag, ln, cc,
        None if idx is None else idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), nidx,
        None if d_chunks is None else d_chunks.data_ptr(),
        None if d_hex is None else d_hex.data_ptr(), None)


def test_arrays_belong_to_the_caller_on_return(torch, enc):
    """Both host arrays are overwritten right after the call returns, before any wait."""
    nfrag, ln, cc = 300, 1024 * 48, 1024
    data = fragments(5, ln)
    base = device_views(torch, list(data), [0] * 5)
    sel = [i % 5 for i in range(nfrag)]
    idx = np.array([1023, 0, 77, 512], np.uint32)
    w5, h5 = expected(list(data), idx.tolist(), cc)
    chunks = Guarded(torch, nfrag * 4 * 48)
    hexes = Guarded(torch, nfrag * 4 * 64)
    ptrs = (ctypes.c_void_p * nfrag)(*[base[s].data_ptr() for s in sel])
    rc = raw_call(enc, ptrs, nfrag, ln, cc, idx, 4, chunks.t, hexes.t)
    for i in range(nfrag):
        ptrs[i] = 0xDEAD0000
    idx[:] = 0xFFFFFFFF
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(chunks.get("chunks").reshape(nfrag, 4, 48), w5[sel])
    assert np.array_equal(hexes.get("hex").reshape(nfrag, 4, 64), h5[sel])


def test_refusals_write_nothing(torch, enc):
    nfrag, ln, cc = 4, 4096, 4
    data = fragments(nfrag, ln)
    base = device_views(torch, list(data), [0] * nfrag)
    chunks = Guarded(torch, nfrag * 2 * (ln // cc))
    hexes = Guarded(torch, nfrag * 2 * 64)
    good = [b.data_ptr() for b in base]
    idx = np.array([0, 3], np.uint32)

    def call(ptr_list=good, ln_=ln, idx_=idx, dc=chunks.t, dh=hexes.t, nfrag_=nfrag, nidx_=2):
        ptrs = (ctypes.c_void_p * len(ptr_list))(*ptr_list)
        rc = raw_call(enc, ptrs, nfrag_, ln_, cc, idx_, nidx_, dc, dh)
        torch.cuda.synchronize()
        return rc

    assert call(idx_=np.array([0, cc], np.uint32)) == EINVAL      # an index == chunk_count
    assert call(ptr_list=good[:2] + [None] + good[3:]) == EINVAL  # a NULL entry
    assert call(ln_=ln - 1) == ESHARDLEN                          # shard_len % chunk_count != 0
    assert call(dc=None, dh=None) == EINVAL                       # both outputs NULL
    assert call(ptr_list=good[:3] + [chunks.t.data_ptr()]) == EINVAL  # d_chunks is a fragment
    assert call(ptr_list=[hexes.t.data_ptr()] + good[1:]) == EINVAL   # d_hex is a fragment
    assert call(dc=base[1], dh=None) == EINVAL                    # the same, named as an output
    chunks.untouched("chunks")
    hexes.untouched("hex")
    # nothing to do: CEC_OK, nothing written
    assert call(nfrag_=0) == 0
    assert call(nidx_=0) == 0
    chunks.untouched("chunks")
    hexes.untouched("hex")
    for v, a in zip(base, data):
        assert np.array_equal(v.cpu().numpy(), a)
    # and the same call, valid, works
    assert call() == 0
    want, want_hex = expected(list(data), [0, 3], cc)
    assert np.array_equal(chunks.get("chunks").reshape(want.shape), want)
    assert np.array_equal(hexes.get("hex").reshape(want_hex.shape), want_hex)
