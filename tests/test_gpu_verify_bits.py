"""Single-bit sensitivity of the verify kernels (cec_verify_batch, cec_verify_ptrs): their whole
output is one byte per segment, so a kernel that never looks at part of its input passes any test
that flips elsewhere. Here one call verifies thousands of copies of one C-oracle codeword, each
but the clean ones with one flipped bit at a planned place (tests/verify_flips.py: every byte of
every shard, the bit by a fixed rule that covers every (byte of a column, bit) and for the
bit-sliced RS(32,32) kernel every (half, byte, plane); every bit of each shard's last byte), and
the whole flag vector is asserted: 0 for every flipped segment, 1 for every clean one.

Setup of every case: the codeword is encoded on the host once, uploaded once, replicated on the
device with expand().contiguous(), and the flips are applied by one indexed XOR per tensor with
unique indices. d_ok sits between two guard bytes, pre-filled. Verify writes nothing: after the
call the same indexed XOR takes the flips out again and every byte of the buffers, gaps between
shards included, must equal the replicated codeword, which holds exactly when the call left every
byte as it was."""
from ctypes import POINTER, c_void_p

import numpy as np
import pytest

from oracle.c_oracle import c_encode
from tests import verify_flips as vf

pytestmark = pytest.mark.gpu

FILL = 0x5A
GAP = 0xA5


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


def codeword(corc, k, m, ln):
    rng = np.random.default_rng(k * 1000003 + m * 1009 + ln)
    data = [rng.integers(0, 256, ln, dtype=np.uint8) for _ in range(k)]
    return np.stack(data + c_encode(corc, k, m, data))


def xor_at(torch, flat, idx, mask):
    """flat[idx] ^= mask on the device, idx unique."""
    assert len(np.unique(idx)) == len(idx)
    assert idx.min() >= 0 and idx.max() < flat.numel()
    i = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).cuda()
    flat[i] ^= torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).cuda()


def all_rows_equal(torch, rows, row):
    """Every row of the [n][bytes] device tensor equals `row`, a quarter GiB at a time."""
    step = max(1, (1 << 28) // rows.shape[1])
    return all(bool((rows[a:a + step] == row).all()) for a in range(0, rows.shape[0], step))


def check_flags(torch, okbuf, pl, what):
    ok = okbuf.cpu().numpy()
    assert ok[0] == FILL and ok[-1] == FILL, "d_ok guard byte written"
    got, want = ok[1:-1], pl.expected()
    assert set(np.unique(got)) <= {0, 1}, np.unique(got)
    missed = np.flatnonzero((got == 1) & (want == 0))
    at = np.searchsorted(pl.segment, missed[:8])
    assert len(missed) == 0, (
        what, f"{len(missed)} flipped segments read 1; the first (shard, byte, mask):",
        list(zip(pl.shard[at].tolist(), pl.byte[at].tolist(), pl.mask[at].tolist())))
    false_alarm = np.flatnonzero((got == 0) & (want == 1))
    assert len(false_alarm) == 0, (what, "clean segments read 0:", false_alarm[:8].tolist())
    assert np.array_equal(got, want)


# ---- cec_verify_batch ----------------------------------------------------------------------------


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in vf.BATCH_CASES])
def test_verify_batch_bits(torch, cess, corc, case):
    from cess_amd import _lib
    k, m, ln = case.k, case.m, case.ln
    pl = vf.batch_plan(case)
    nseg = pl.nseg
    word = torch.from_numpy(codeword(corc, k, m, ln)).cuda()
    d_data = word[:k].expand(nseg, k, ln).contiguous()
    if case.par_off:  # the same replication into a view that starts off a 16-byte boundary
        alloc = torch.full((nseg * m * ln + case.par_off,), GAP, dtype=torch.uint8, device="cuda")
        d_par = alloc[case.par_off:].view(nseg, m, ln)
        d_par.copy_(word[k:].expand(nseg, m, ln))
        assert d_par.data_ptr() % 16 == case.par_off
    else:
        d_par = word[k:].expand(nseg, m, ln).contiguous()
    in_data = pl.shard < k
    flips = [(d_data.view(-1), pl.segment[in_data] * (k * ln) + pl.shard[in_data] * ln
              + pl.byte[in_data], pl.mask[in_data]),
             (d_par.view(-1), pl.segment[~in_data] * (m * ln) + (pl.shard[~in_data] - k) * ln
              + pl.byte[~in_data], pl.mask[~in_data])]
    flips = [f for f in flips if len(f[1])]
    for f in flips:
        xor_at(torch, *f)
    okbuf = torch.full((nseg + 2,), FILL, dtype=torch.uint8, device="cuda")
    enc = cess.New(k, m)
    if case.generic:
        enc.set_option(_lib.CEC_OPT_FORCE_GENERIC, 1)
    torch.cuda.synchronize()
    enc.VerifyBatch(d_data, d_par, nseg, ln, d_ok=okbuf[1:nseg + 1])
    torch.cuda.synchronize()
    check_flags(torch, okbuf, pl, case.id)
    for f in flips:
        xor_at(torch, *f)
    assert all_rows_equal(torch, d_data.view(nseg, k * ln), word[:k].reshape(-1)), "data written"
    assert all_rows_equal(torch, d_par.view(nseg, m * ln), word[k:].reshape(-1)), "parity written"
    if case.par_off:
        assert bool((alloc[:case.par_off] == GAP).all())
    enc.close()


# ---- cec_verify_ptrs -----------------------------------------------------------------------------


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in vf.PTR_CASES])
def test_verify_ptrs_bits(torch, cess, corc, case):
    """The shards of all segments in one tensor, a shard every `ln` rounded up to 64, plus 64,
    bytes (the rest 0xA5), the address arrays computed from the base address. Sources beyond the k
    survivors hold random bytes and get no flips: a kernel that read them fails clean segments."""
    from cess_amd import _lib
    lib = _lib.load()
    k, m, ln, off = case.k, case.m, case.ln, case.off
    n = k + m
    pl, of_seg = vf.ptr_plan(case)
    nseg = pl.nseg
    shs = -(-ln // 64) * 64 + 64  # shard stride
    ss = n * shs                  # segment stride
    full = codeword(corc, k, m, ln)
    rng = np.random.default_rng(7 * k + m + ln)
    # which shards of a segment are sources / expectations, by its group
    is_src = np.zeros((len(case.groups), n), dtype=bool)
    is_exp = np.zeros((len(case.groups), n), dtype=bool)
    unread = np.ones(n, dtype=bool)  # read by no group: random bytes
    for g, (sources, expects) in enumerate(case.groups):
        is_src[g, sources] = True
        is_exp[g, expects] = True
        unread[vf.ptr_flipped(case, (sources, expects))] = False
        flags = np.zeros(n, dtype=np.uint8)
        flags[sources] = 1
        surv = np.zeros(k, dtype=np.uint8)
        assert lib.cec_survivors(k, m, flags.ctypes.data, surv.ctypes.data) == 0
        assert surv.tolist() == vf.first_k(k, sources)
    host = np.full(ss, GAP, dtype=np.uint8)
    for i in range(n):
        host[i * shs + off:i * shs + off + ln] = (rng.integers(0, 256, ln, dtype=np.uint8)
                                                  if unread[i] else full[i])
    tmpl = torch.from_numpy(host).cuda()
    buf = tmpl.expand(nseg, ss).contiguous()
    assert buf.data_ptr() % 64 == 0
    idx = pl.segment * ss + pl.shard * shs + off + pl.byte
    xor_at(torch, buf.view(-1), idx, pl.mask)
    addr = (np.uint64(buf.data_ptr()) + np.arange(nseg, dtype=np.uint64)[:, None] * np.uint64(ss)
            + np.arange(n, dtype=np.uint64)[None, :] * np.uint64(shs) + np.uint64(off))
    src = np.ascontiguousarray(np.where(is_src[of_seg], addr, np.uint64(0)))
    exp = np.ascontiguousarray(np.where(is_exp[of_seg], addr, np.uint64(0)))
    assert src.dtype == np.uint64 and src.shape == (nseg, n)
    okbuf = torch.full((nseg + 2,), FILL, dtype=torch.uint8, device="cuda")
    enc = cess.New(k, m)
    if case.generic:
        enc.set_option(_lib.CEC_OPT_FORCE_GENERIC, 1)
    if case.rt_mode is not None:
        enc.set_option(_lib.CEC_OPT_RT_MODE, case.rt_mode)
    torch.cuda.synchronize()
    rc = lib.cec_verify_ptrs(enc._h, src.ctypes.data_as(POINTER(c_void_p)),
                             exp.ctypes.data_as(POINTER(c_void_p)), nseg, ln,
                             okbuf[1:].data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    check_flags(torch, okbuf, pl, case.id)
    xor_at(torch, buf.view(-1), idx, pl.mask)
    assert all_rows_equal(torch, buf, tmpl), "a shard or a gap was written"
    enc.close()
