"""audit.scrub_repair_device: a scrub whose verdicts never leave the GPU. The hash queue flags
every held fragment against its recorded hash, and Encoder.RepairFlaggedDevice, next on the same
stream, rebuilds the one fragment of a segment that no longer matches. Fragments are separate
tensors of 8 KiB holding C-oracle codewords, hashes are recorded with hashlib. Of 12 segments,
five lost one bit in one fragment (spread over d0, d1 and p0), one lost a bit in each of two
fragments, and one has a wrong *recorded* hash for an intact fragment."""
import hashlib

import numpy as np
import pytest

from oracle.c_oracle import c_encode

pytestmark = pytest.mark.gpu

CLEAN, REBUILT, MANY, LOST = 0, 1, 2, 3
NSEG, F = 12, 8192


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


def stored(corc, k, m, drop):
    """(truth [NSEG][n][F], held [NSEG][n], damaged copy, recorded hashes [NSEG][n], expected
    flags [NSEG][n]); `drop`: one shard per segment is not held (segment s: shard s % n)."""
    n = k + m
    rng = np.random.default_rng(k * 100 + m)
    data = rng.integers(0, 256, (k, NSEG * F), dtype=np.uint8)
    par = np.stack(c_encode(corc, k, m, list(data)))
    full = np.ascontiguousarray(
        np.concatenate([data, par]).reshape(n, NSEG, F).transpose(1, 0, 2))
    held = np.ones((NSEG, n), dtype=bool)
    if drop:
        held[np.arange(NSEG), np.arange(NSEG) % n] = False
    recorded = [[sha_hex(full[s, i]) for i in range(n)] for s in range(NSEG)]
    now = full.copy()

    def pick(s, i, skip=()):  # the first held fragment of segment s from index i on
        while not held[s, i] or i in skip:
            i = (i + 1) % n
        return i

    flips = {}
    for s, at, byte, bit in ((1, 0, 0, 0), (3, 1, 4097, 5), (4, 1, 8191, 7), (8, k, 63, 1),
                             (10, 0, 64, 2)):
        i = pick(s, at)
        now[s, i, byte] ^= 1 << bit
        flips[s] = [i]
    a = pick(6, 0)
    b = pick(6, 0, skip=(a,))
    now[6, a, 100] ^= 1
    now[6, b, 8000] ^= 0x80
    flips[6] = [a, b]
    w = pick(9, 2)
    h = recorded[9][w]
    recorded[9][w] = h[:10] + (b"0" if h[10:11] != b"0" else b"1") + h[11:]
    flips[9] = [w]
    assert {i for s in (1, 3, 4, 8, 10) for i in flips[s]} >= {0, 1, k}  # d0, d1 and p0
    flags = np.array([[sha_hex(now[s, i]) == recorded[s][i] for i in range(n)]
                      for s in range(NSEG)], np.uint8)
    return full, held, now, recorded, flags


def run(torch, cess, corc, k, m, drop, own_queue, recorded_as_tensor=False):
    n = k + m
    full, held, now, recorded, flags = stored(corc, k, m, drop)
    want = np.array([cess.flag_status(k, m, held[s], flags[s]) for s in range(NSEG)])
    assert (want[:, 0] == REBUILT).sum() == 6 and want[6, 0] == LOST
    assert (want[:, 0] == CLEAN).sum() == 5
    segments = [[torch.from_numpy(now[s, i].copy()).cuda() if held[s, i] else None
                 for i in range(n)] for s in range(NSEG)]
    rec = recorded
    if recorded_as_tensor:
        rec = torch.from_numpy(np.frombuffer(b"".join(h for row in recorded for h in row),
                                             np.uint8).reshape(NSEG, n, 64).copy()).cuda()
    with cess.New(k, m) as enc:
        if own_queue:
            d_flags, d_status = cess.audit.scrub_repair_device(enc, segments, rec)
        else:
            with cess.HashQueue(capacity=128) as q:
                d_flags, d_status = cess.audit.scrub_repair_device(enc, segments, rec, queue=q)
                assert q.live_chains == 0  # ticked to completion, nothing waited for
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        assert d_flags.shape == (NSEG, n) and d_status.shape == (NSEG,)
        got_flags = d_flags.cpu().numpy()
        assert np.array_equal(got_flags[held] != 0, flags[held] != 0)
        assert np.array_equal(d_status.cpu().numpy(), want[:, 0])
        for s in range(NSEG):
            for i in range(n):
                if not held[s, i]:
                    continue
                got = segments[s][i].cpu().numpy()
                if want[s, 0] == REBUILT:  # healed: every fragment hashes to its truth
                    assert sha_hex(got) == sha_hex(full[s, i]), (s, i)
                else:  # untouched, the double-flip segment included
                    assert np.array_equal(got, now[s, i]), (s, i)
        # proof is a second scrub: only the wrong record and the lost segment are flagged now
        again = cess.audit.scrub_device(
            [t for seg in segments for t in seg if t is not None],
            [recorded[s][i] for s in range(NSEG) for i in range(n) if held[s, i]])
        torch.cuda.synchronize()
        ok = np.ones((NSEG, n), np.uint8)
        ok[held] = again.cpu().numpy()
        assert set(zip(*np.nonzero(ok == 0))) == \
            {(6, i) for i in range(n) if held[6, i] and not flags[6, i]} | \
            {(9, i) for i in range(n) if held[9, i] and not flags[9, i]}


@pytest.mark.parametrize("own_queue", [False, True])
def test_rs21(torch, cess, corc, own_queue):
    run(torch, cess, corc, 2, 1, drop=False, own_queue=own_queue)


@pytest.mark.parametrize("own_queue", [False, True])
def test_rs42_one_shard_not_held(torch, cess, corc, own_queue):
    run(torch, cess, corc, 4, 2, drop=True, own_queue=own_queue, recorded_as_tensor=own_queue)
