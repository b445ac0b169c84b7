"""cec_hashq_add_ptrs on the GPU: chains over buffers that lie in separate allocations, their
addresses carried in kernel arguments (256 per launch). Every hex is compared with hashlib, and
with cec_hashq_add on the same bytes packed contiguously; exact."""
import ctypes
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HQOPT_TICK = 1
EINVAL, ENOMEM = -1, -5
NS = [1, 64, 65, 300, 513]       # one launch, a group of 64 and one more, two and three launches
LENS = [1, 55, 56, 64, 4113]     # padding edges, one block, 64 blocks and an odd tail
_CASES = {}


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


def mkq(cess, tick, **kw):
    q = cess.HashQueue(stream=None, **kw)
    q.set_option(HQOPT_TICK, tick)
    return q


def case(torch, n, ln):
    """(host bytes [n][ln], n separate device tensors, every third one byte off its allocation's
    base, expected hex [n][64] as bytes): made once per shape and read-only afterwards."""
    key = (n, ln)
    if key not in _CASES:
        host = np.random.default_rng(n * 100003 + ln).integers(0, 256, (n, ln), dtype=np.uint8)
        stage = torch.from_numpy(host).cuda()
        bufs = []
        for i in range(n):
            off = 1 if i % 3 == 1 else 0
            base = torch.empty(ln + 17, dtype=torch.uint8, device="cuda")
            v = base[off:off + ln]
            v.copy_(stage[i])
            bufs.append(v)
        want = np.stack([np.frombuffer(hashlib.sha256(r.tobytes()).hexdigest().encode(), np.uint8)
                         for r in host])
        host.setflags(write=False)
        want.setflags(write=False)
        _CASES[key] = (host, bufs, want)
    return _CASES[key]


def drain(q, how):
    if how == "finish":
        q.finish()
    else:
        while q.live_chains:
            q.tick(3)


@pytest.mark.parametrize("how", ["finish", "tick3"])
@pytest.mark.parametrize("tick", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("n", NS)
def test_hex_equals_hashlib(torch, cess, n, tick, how):
    q = mkq(cess, tick, capacity=1024)
    last = 0
    for ln in LENS:
        _, bufs, want = case(torch, n, ln)
        d_hex = torch.full((n + 2, 64), 0xA5, dtype=torch.uint8, device="cuda")
        t = q.add_ptrs(bufs, d_hex, hex_offset=64)
        assert t == last + 1
        last = t
        assert q.live_chains == n and not q.done(t)
        drain(q, how)
        assert q.done(t) and q.live_chains == 0
        torch.cuda.synchronize()
        got = d_hex.cpu().numpy()
        assert (got[0] == 0xA5).all() and (got[-1] == 0xA5).all(), (n, ln, "guard rows")
        assert np.array_equal(got[1:-1], want), (n, ln)
    q.close()


@pytest.mark.parametrize("ln", LENS)
def test_agrees_with_the_strided_add(torch, cess, ln):
    n = 300
    host, bufs, want = case(torch, n, ln)
    packed = torch.from_numpy(host.copy()).cuda()
    a = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    b = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    with mkq(cess, 0, capacity=1024) as q:
        q.add_ptrs(bufs, a)
        q.add(packed, n, 1, ln, ln, ln, b, 1, 0)
        q.finish()
        torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), want)


@pytest.mark.parametrize("tick", [0, 3, 4])
def test_interleaved_with_strided_adds(torch, cess, tick):
    """A strided add, a pointer add and another strided add in one queue, ticked one block at a
    time: tickets increase, each add is reported complete exactly when its blocks are covered."""
    adds = [(64, 10, "strided"), (300, 70, "ptrs"), (4113, 5, "strided")]
    q = mkq(cess, tick, capacity=128)
    tickets, outs = [], []
    for ln, n, kind in adds:
        host, bufs, want = case(torch, n, ln)
        d_hex = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
        if kind == "ptrs":
            tickets.append(q.add_ptrs(bufs, d_hex))
        else:
            packed = torch.from_numpy(host.copy()).cuda()
            outs.append(packed)  # alive until the chains are complete
            tickets.append(q.add(packed, n, 1, ln, ln, ln, d_hex, 1, 0))
        outs.append((d_hex, want))
    assert tickets == [1, 2, 3]
    assert q.live_chains == 85
    blocks = [cess.sha256_blocks(ln) for ln, _, _ in adds]
    assert blocks == sorted(blocks)
    for done in range(1, blocks[-1] + 1):
        q.tick(1)
        assert [q.done(t) for t in tickets] == [done >= b for b in blocks], done
    assert q.live_chains == 0
    torch.cuda.synchronize()
    for o in outs:
        if isinstance(o, tuple):
            assert np.array_equal(o[0].cpu().numpy(), o[1])
    q.close()


def test_ring_wrap(torch, cess):
    _, bufs, want = case(torch, 300, 56)
    q = mkq(cess, 0, capacity=128)
    for lo in (0, 100):  # slots 0..99, then 100..199: the second add wraps the 128-slot ring
        d_hex = torch.zeros((100, 64), dtype=torch.uint8, device="cuda")
        q.add_ptrs(bufs[lo:lo + 100], d_hex)
        q.finish()
        torch.cuda.synchronize()
        assert np.array_equal(d_hex.cpu().numpy(), want[lo:lo + 100]), lo
    q.close()


def test_two_launches_across_the_wrap_with_and_without_output(torch, cess):
    """257 chains are two add launches, the second of one chain: with no output it must not make
    an address of the null hex, and its slots follow the first launch's over the wrap point."""
    _, bufs, want = case(torch, 300, 56)
    q = mkq(cess, 0, capacity=512)
    # slots 0..299, 300..556 (wraps, no output), 557..813, 814..1070 (wraps)
    for lo, n, out in ((0, 300, True), (0, 257, False), (43, 257, True), (0, 257, True)):
        d_hex = torch.zeros((n, 64), dtype=torch.uint8, device="cuda") if out else None
        t = q.add_ptrs(bufs[lo:lo + n], d_hex)
        assert q.live_chains == n
        q.finish()
        torch.cuda.synchronize()
        assert q.done(t) and q.live_chains == 0
        if out:
            assert np.array_equal(d_hex.cpu().numpy(), want[lo:lo + n]), (lo, n)
    q.close()


def test_queue_full_adds_nothing(torch, cess):
    _, bufs, want = case(torch, 300, 4113)
    q = mkq(cess, 0, capacity=64)
    first = torch.zeros((40, 64), dtype=torch.uint8, device="cuda")
    second = torch.full((40, 64), 0xA5, dtype=torch.uint8, device="cuda")
    t1 = q.add_ptrs(bufs[:40], first)
    with pytest.raises(cess.CecError) as ei:
        q.add_ptrs(bufs[40:80], second)
    assert ei.value.code == ENOMEM
    assert q.live_chains == 40 and not q.done(t1)
    q.finish()
    torch.cuda.synchronize()
    assert q.done(t1)
    assert np.array_equal(first.cpu().numpy(), want[:40])
    assert bool((second == 0xA5).all())
    assert q.add_ptrs(bufs[40:80], second) == t1 + 1  # the refused add took no ticket
    q.finish()
    torch.cuda.synchronize()
    assert np.array_equal(second.cpu().numpy(), want[40:80])
    q.close()


def test_null_entry_is_refused_and_the_ring_unchanged(torch, cess):
    _, bufs, want = case(torch, 300, 64)
    q = mkq(cess, 0, capacity=1024)
    d_hex = torch.full((300, 64), 0xA5, dtype=torch.uint8, device="cuda")
    t1 = q.add_ptrs(bufs[:20], d_hex)
    for bad in ([None] + bufs[21:30], bufs[20:290] + [None]):  # first launch / a later launch
        with pytest.raises(cess.CecError) as ei:
            q.add_ptrs(bad, d_hex, hex_offset=20 * 64)
        assert ei.value.code == EINVAL
        assert q.live_chains == 20
    assert q.add_ptrs([], d_hex) == 0 and q.live_chains == 20
    t2 = q.add_ptrs(bufs[20:30], d_hex, hex_offset=20 * 64)
    assert t2 == t1 + 1
    q.finish()
    torch.cuda.synchronize()
    got = d_hex.cpu().numpy()
    assert np.array_equal(got[:30], want[:30])
    assert (got[30:] == 0xA5).all()
    q.close()


def test_no_output(torch, cess):
    _, bufs, _ = case(torch, 65, 4113)
    q = mkq(cess, 0, capacity=128)
    t = q.add_ptrs(bufs)
    assert q.live_chains == 65
    q.finish()
    torch.cuda.synchronize()
    assert q.done(t) and q.live_chains == 0
    q.close()


def test_array_belongs_to_the_caller_on_return(torch, cess):
    """The pointer array is overwritten right after the call returns, before any tick."""
    from cess_amd import _lib
    n = 513
    _, bufs, want = case(torch, n, 4113)
    q = mkq(cess, 0, capacity=1024)
    d_hex = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    ptrs = (ctypes.c_void_p * n)(*[b.data_ptr() for b in bufs])
    ticket = ctypes.c_uint64()
    rc = _lib.load().cec_hashq_add_ptrs(q._h, ptrs, n, 4113, d_hex.data_ptr(),
                                        ctypes.byref(ticket))
    for i in range(n):
        ptrs[i] = 0xDEAD0000
    assert rc == 0 and ticket.value == 1
    q.finish()
    torch.cuda.synchronize()
    assert np.array_equal(d_hex.cpu().numpy(), want)
    q.close()
