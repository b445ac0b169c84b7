"""audit.scrub_repair_confirm_device: the scrub that heals and then proves it, all on the GPU. After
the repair only the rebuilt fragments are hashed again (HashQueue.add_check_where_ptrs, chosen on
the device from the scrub's flags and the repair's statuses) and cess_amd.confirm_flagged folds
their flags into one code per segment. The stored fragments are those of test_gpu_scrub_repair.py:
12 segments of 8 KiB fragments, five with one flipped bit, one with a bit flipped in each of two
fragments, one whose *recorded* hash is wrong for an intact fragment."""
import numpy as np
import pytest

from tests.test_gpu_scrub_repair import NSEG, sha_hex, stored

pytestmark = pytest.mark.gpu

CLEAN, REBUILT, MANY, LOST = 0, 1, 2, 3
NONE, PROVEN, REFUTED = 0, 1, 2
SKIPPED = 2


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


def run(torch, cess, corc, k, m, drop, max_bad, own_queue, healed, recorded_as_tensor=False):
    n = k + m
    full, held, now, recorded, flags = stored(corc, k, m, drop)
    status = np.array([cess.flag_status_multi(k, m, held[s], flags[s], max_bad)[0]
                       for s in range(NSEG)], np.uint8)
    rebuilt = (status == REBUILT)[:, None] & held & (flags == 0)
    assert sorted(np.nonzero(status == REBUILT)[0]) == sorted(healed + [9])
    assert rebuilt.sum() == len(healed) + 1 + (6 in healed)  # the double flip heals two
    # what the proof must find, from hashlib alone: the rebuilt bytes are the truth's
    want_ok = np.full((NSEG, n), SKIPPED, np.uint8)
    for s, i in zip(*np.nonzero(rebuilt)):
        want_ok[s, i] = sha_hex(full[s, i]) == recorded[s][i]
    assert want_ok[9].min() == 0 and (want_ok == 0).sum() == 1
    want_confirm = np.array([NONE if status[s] != REBUILT else REFUTED if s == 9 else PROVEN
                             for s in range(NSEG)], np.uint8)
    assert [cess.confirm_rule(int(status[s]), want_ok[s]) for s in range(NSEG)] == \
        want_confirm.tolist()

    def fresh():
        return [[torch.from_numpy(now[s, i].copy()).cuda() if held[s, i] else None
                 for i in range(n)] for s in range(NSEG)]

    rec = recorded
    if recorded_as_tensor:
        rec = torch.from_numpy(np.frombuffer(b"".join(h for row in recorded for h in row),
                                             np.uint8).reshape(NSEG, n, 64).copy()).cuda()
    segments = fresh()
    with cess.New(k, m) as enc:
        if own_queue:
            out = cess.audit.scrub_repair_confirm_device(enc, segments, rec, max_bad=max_bad)
        else:
            with cess.HashQueue(capacity=64) as q:  # smaller than RS(4,2)'s table of 72
                out = cess.audit.scrub_repair_confirm_device(enc, segments, rec, max_bad=max_bad,
                                                             queue=q)
                assert q.live_chains == 0  # ticked to completion, nothing waited for
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        d_flags, d_status, d_ok, d_confirm = out
        assert d_flags.shape == (NSEG, n) and d_ok.shape == (NSEG, n)
        assert d_status.shape == (NSEG,) and d_confirm.shape == (NSEG,)
        assert np.array_equal(d_flags.cpu().numpy()[held] != 0, flags[held] != 0)
        assert np.array_equal(d_status.cpu().numpy(), status)
        assert np.array_equal(d_ok.cpu().numpy(), want_ok)
        assert np.array_equal(d_confirm.cpu().numpy(), want_confirm)
        for s in range(NSEG):
            for i in range(n):
                if not held[s, i]:
                    continue
                got = segments[s][i].cpu().numpy()
                if status[s] == REBUILT:  # healed: every fragment is its truth
                    assert np.array_equal(got, full[s, i]), (s, i)
                else:
                    assert np.array_equal(got, now[s, i]), (s, i)
        # the call without the proof leaves the same flags and statuses
        again = fresh()
        if max_bad == 1:
            f2, s2 = cess.audit.scrub_repair_device(enc, again, rec)
        else:
            f2, s2 = cess.audit.scrub_repair_multi_device(enc, again, rec, max_bad=max_bad)
        torch.cuda.synchronize()
        assert np.array_equal(s2.cpu().numpy(), d_status.cpu().numpy())
        assert np.array_equal(f2.cpu().numpy()[held] != 0, d_flags.cpu().numpy()[held] != 0)


@pytest.mark.parametrize("own_queue", [False, True])
def test_rs21(torch, cess, corc, own_queue):
    run(torch, cess, corc, 2, 1, drop=False, max_bad=1, own_queue=own_queue,
        healed=[1, 3, 4, 8, 10])


@pytest.mark.parametrize("own_queue", [False, True])
def test_rs42_one_shard_not_held(torch, cess, corc, own_queue):
    run(torch, cess, corc, 4, 2, drop=True, max_bad=1, own_queue=own_queue,
        healed=[1, 3, 4, 8, 10], recorded_as_tensor=own_queue)


@pytest.mark.parametrize("own_queue", [False, True])
def test_rs42_double_flip_max_bad_2(torch, cess, corc, own_queue):
    run(torch, cess, corc, 4, 2, drop=False, max_bad=2, own_queue=own_queue,
        healed=[1, 3, 4, 6, 8, 10], recorded_as_tensor=not own_queue)
