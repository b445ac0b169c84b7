"""The recorded-hash checks built on the checking adds, on the GPU: a miner's scrub of scattered
fragments (audit.scrub_device) and the repair gate as flags in HBM (repair.check_batch_device),
against hashlib and against repair_batch's own host-side check of the same inputs."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = 0xA5


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


def sha_hex(a):
    return hashlib.sha256(a.tobytes()).hexdigest().encode()


@pytest.fixture(scope="module")
def stored(torch):
    """40 fragments of 8 KiB in separate tensors with the hashes recorded for them; fragments 3,
    17 and 39 lost one bit afterwards. (device tensors, recorded hashes, host flags)"""
    rng = np.random.default_rng(40)
    host = rng.integers(0, 256, (40, 8192), dtype=np.uint8)
    recorded = [sha_hex(r) for r in host]
    for f, byte, bit in ((3, 0, 0), (17, 4097, 5), (39, 8191, 7)):
        host[f, byte] ^= 1 << bit
    frags = [torch.from_numpy(r.copy()).cuda() for r in host]
    flags = np.array([sha_hex(r) == h for r, h in zip(host, recorded)], np.uint8)
    assert flags.sum() == 37 and not flags[[3, 17, 39]].any()
    return frags, recorded, flags


def test_scrub_device_with_the_callers_queue(torch, cess, stored):
    frags, recorded, flags = stored
    full = torch.full((42,), FILL, dtype=torch.uint8, device="cuda")
    with cess.HashQueue(capacity=64) as q:
        d_ok = cess.audit.scrub_device(frags, recorded, queue=q, d_ok=full[1:41])
        assert q.live_chains == 0  # ticked to completion, nothing waited for
        torch.cuda.synchronize()
        assert d_ok.data_ptr() == full.data_ptr() + 1
        got = full.cpu().numpy()
        assert got[0] == FILL and got[41] == FILL
        assert np.array_equal(got[1:41], flags)
        # hashes in a device tensor, flags in a tensor of the call's own
        d_rec = torch.from_numpy(np.frombuffer(b"".join(recorded), np.uint8).reshape(40, 64)
                                 .copy()).cuda()
        d_ok = cess.audit.scrub_device(frags, d_rec, queue=q)
        torch.cuda.synchronize()
        assert np.array_equal(d_ok.cpu().numpy(), flags)


def test_scrub_device_with_a_queue_of_its_own(torch, cess, stored):
    frags, recorded, flags = stored
    d_ok = cess.audit.scrub_device(frags, recorded)
    assert d_ok.dtype == torch.uint8 and d_ok.shape == (40,) and d_ok.is_cuda
    torch.cuda.synchronize()
    assert np.array_equal(d_ok.cpu().numpy(), flags)
    one = cess.audit.scrub_device(frags[3:4], recorded[3:4])
    none = cess.audit.scrub_device([], [])
    torch.cuda.synchronize()
    assert one.cpu().tolist() == [0] and none.numel() == 0


def test_check_batch_device_agrees_with_repair_batch(torch, cess):
    """RS(2,1), 8 segments of 4 KiB fragments, one fragment erased per segment and rebuilt; two
    recorded hashes are wrong. The flags in HBM name the same fragments as the completion calls
    of repair_batch's host-side check, and the same segments fail."""
    from cess_amd import repair
    k, m, F, nseg = 2, 1, 4096, 8
    rng = np.random.default_rng(21)
    enc = cess.New(k, m)
    d_data = torch.from_numpy(rng.integers(0, 256, (nseg, k, F), dtype=np.uint8)).cuda()
    d_par = torch.zeros((nseg, m, F), dtype=torch.uint8, device="cuda")
    enc.EncodeBatch(d_data, d_par, nseg, F)
    torch.cuda.synchronize()
    data, par = d_data.cpu().numpy(), d_par.cpu().numpy()
    present = np.ones((nseg, k + m), np.uint8)
    expected = []
    for s in range(nseg):
        i = s % 3
        present[s, i] = 0
        expected.append({i: sha_hex(data[s, i] if i < k else par[s, i - k])})
    expected[2] = {2: b"0" * 64}
    good = expected[5][2]
    expected[5] = {2: good[:63] + (b"0" if good[63:] != b"0" else b"1")}

    def erased():
        dd = torch.from_numpy(data * present[:, :k, None]).cuda()
        dp = torch.from_numpy(par * present[:, k:, None]).cuda()
        return dd, dp

    dd, dp = erased()
    want_ok, calls = repair.repair_batch(enc, dd, dp, nseg, F, present, expected, hash_on="host",
                                         complete_calls=True)
    assert want_ok == [s not in (2, 5) for s in range(nseg)]

    dd, dp = erased()
    enc.ReconstructBatch(dd, dp, nseg, F, present)
    with cess.HashQueue(capacity=16) as q:
        d_ok, index = repair.check_batch_device(q, dd, dp, nseg, k, m, F, expected)
        assert q.live_chains == 0
        torch.cuda.synchronize()
    assert index == [(s, s % 3) for s in range(nseg)]
    flags = d_ok.cpu().numpy()
    assert flags.dtype == np.uint8 and flags.shape == (nseg,)
    assert [bool(f) for f in flags] == [pair in calls for pair in index]
    assert [all(f for f, (s, _) in zip(flags, index) if s == seg) for seg in range(nseg)] == want_ok
    assert set(flags.tolist()) == {0, 1}
