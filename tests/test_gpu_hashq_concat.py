"""cec_hashq_add_concat_ptrs on the GPU: chains that run over several buffers back to back. The
parts of every chain are disjoint slices of one arena, laid out in shuffled order with random
bytes between them, so a chain that reads the wrong part, or runs on past a part's end, gets a
wrong digest. Every hex is compared with hashlib over the joined bytes; exact."""
import ctypes
import hashlib
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HQOPT_TICK = 1
EINVAL, ENOMEM = -1, -5
PARTS = [1, 2, 3, 5]
PART_LENS = [64, 128, 192]
_ARENAS = {}


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


def lasts(part_len):
    """Bytes of the last part: the padding edges, a whole block, the whole part."""
    return sorted({1, 55, 56, 63, 64, part_len})


def hexrow(b):
    return np.frombuffer(hashlib.sha256(b).hexdigest().encode(), np.uint8)


class Arena:
    """One device tensor that holds the parts of several groups of chains. A group is (n chains,
    parts, part_len, last); `mis` gives part p of every chain an offset mis[p % len(mis)] from its
    16-byte aligned slot. Made once per key and read-only afterwards."""

    def __init__(self, torch, seed, groups, mis=(0,)):
        rng = np.random.default_rng(seed)
        slot = max(g[2] for g in groups) + 64   # a part, then at least 48 bytes that are not its own
        where = [(gi, c, p) for gi, g in enumerate(groups) for c in range(g[0])
                 for p in range(g[1])]
        order = rng.permutation(len(where))
        self.host = rng.integers(0, 256, len(where) * slot + 64, dtype=np.uint8)
        self.dev = torch.from_numpy(self.host).cuda()
        off = {w: int(order[i]) * slot + mis[w[2] % len(mis)] for i, w in enumerate(where)}
        self.chains, self.want, self.want_pre, self.length = [], [], [], []
        for gi, (n, parts, part_len, last) in enumerate(groups):
            rows, want, pre = [], [], []
            for c in range(n):
                o = [off[(gi, c, p)] for p in range(parts)]
                rows.append([self.dev[x:x + part_len] for x in o])
                joined = b"".join(self.host[x:x + part_len].tobytes() for x in o[:-1])
                joined += self.host[o[-1]:o[-1] + last].tobytes()
                want.append(hexrow(joined))
                pre.append(hexrow(self.host[o[0]:o[0] + part_len].tobytes()))
            self.chains.append(rows)
            self.want.append(np.stack(want))
            self.want_pre.append(np.stack(pre))
            self.length.append((parts - 1) * part_len + last)
        self.host.setflags(write=False)


def arena(torch, key, groups, mis=(0,)):
    if key not in _ARENAS:
        _ARENAS[key] = Arena(torch, zlib.crc32(repr(key).encode()), groups, mis)
    return _ARENAS[key]


def drain(q, how):
    if how == "finish":
        q.finish()
    else:
        while q.live_chains:
            q.tick(3)


def out(torch, n):
    return torch.full((n + 2, 64), 0xA5, dtype=torch.uint8, device="cuda")


def check_out(d, want, what):
    got = d.cpu().numpy()
    assert (got[0] == 0xA5).all() and (got[-1] == 0xA5).all(), (what, "guard rows")
    assert np.array_equal(got[1:-1], want), what


@pytest.mark.parametrize("how", ["finish", "tick3"])
@pytest.mark.parametrize("tick", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("part_len", PART_LENS)
def test_digest_and_prefix_equal_hashlib(torch, cess, part_len, tick, how):
    """Every parts x last-part length of one part_len, three chains each, live together: a
    3-block tick against 1-, 2- and 3-block parts cuts at the start, middle and end of ticks."""
    groups = [(3, parts, part_len, last) for parts in PARTS for last in lasts(part_len)]
    a = arena(torch, ("digest", part_len), groups)
    q = mkq(cess, tick, capacity=256)
    outs = []
    for gi, (n, parts, _, last) in enumerate(groups):
        d_hex = out(torch, n)
        d_pre = out(torch, n) if parts >= 2 else None
        t = q.add_concat_ptrs(a.chains[gi], d_hex, 64, d_pre, 64, length=a.length[gi])
        assert t == gi + 1 and not q.done(t)
        outs.append((d_hex, d_pre))
    assert q.live_chains == 3 * len(groups)
    drain(q, how)
    assert q.live_chains == 0 and q.done(len(groups))
    torch.cuda.synchronize()
    for gi, g in enumerate(groups):
        check_out(outs[gi][0], a.want[gi], g)
        if outs[gi][1] is not None:
            check_out(outs[gi][1], a.want_pre[gi], (g, "prefix"))
    q.close()


@pytest.mark.parametrize("part_len", PART_LENS)
def test_one_part_is_add_ptrs(torch, cess, part_len):
    groups = [(3, 1, part_len, part_len)]
    a = arena(torch, ("one", part_len), groups)
    bufs = [row[0] for row in a.chains[0]]
    x = torch.zeros((3, 64), dtype=torch.uint8, device="cuda")
    y = torch.zeros((3, 64), dtype=torch.uint8, device="cuda")
    pre = torch.zeros((3, 64), dtype=torch.uint8, device="cuda")
    with mkq(cess, 0, capacity=16) as q:
        q.add_concat_ptrs(a.chains[0], x, d_prefix_hex=pre)
        q.add_ptrs(bufs, y)
        q.finish()
        torch.cuda.synchronize()
    assert torch.equal(x, y) and torch.equal(x, pre)
    assert np.array_equal(x.cpu().numpy(), a.want[0])


@pytest.mark.parametrize("tick", [0, 3, 4])
def test_parts_at_mixed_alignments(torch, cess, tick):
    """Parts of one chain at a 16-byte boundary, one byte and eight bytes past one: the tick
    kernels choose the 16-byte loads or the byte path per part."""
    groups = [(4, 3, 128, 128), (4, 5, 192, 55), (4, 2, 64, 64)]
    a = arena(torch, "align", groups, mis=(0, 1, 8))
    assert [r.data_ptr() % 16 for r in a.chains[0][0]] == [0, 1, 8]
    for how in ("finish", "tick3"):
        q = mkq(cess, tick, capacity=16)
        outs = []
        for gi in range(len(groups)):
            d_hex, d_pre = out(torch, 4), out(torch, 4)
            q.add_concat_ptrs(a.chains[gi], d_hex, 64, d_pre, 64, length=a.length[gi])
            outs.append((d_hex, d_pre))
        drain(q, how)
        torch.cuda.synchronize()
        for gi, g in enumerate(groups):
            check_out(outs[gi][0], a.want[gi], (g, how))
            check_out(outs[gi][1], a.want_pre[gi], (g, how, "prefix"))
        q.close()


@pytest.mark.parametrize("tick", [0, 3])
def test_more_chains_than_one_launch_carries(torch, cess, tick):
    groups = [(300, 2, 64, 64)]
    a = arena(torch, "n300", groups)
    q = mkq(cess, tick, capacity=512)
    d_hex, d_pre = out(torch, 300), out(torch, 300)
    t = q.add_concat_ptrs(a.chains[0], d_hex, 64, d_pre, 64)
    assert q.live_chains == 300
    q.tick(1)
    assert not q.done(t) and q.blocks_left == 2
    q.finish()
    torch.cuda.synchronize()
    check_out(d_hex, a.want[0], "n300")
    check_out(d_pre, a.want_pre[0], "n300 prefix")
    q.close()


@pytest.mark.parametrize("tick", [0, 1, 3, 4])
def test_interleaved_with_other_adds(torch, cess, tick):
    """Concat, strided and pointer adds of different lengths, added between ticks, so that their
    part boundaries fall at different places of the same tick. After each tick(T) the most blocks
    any chain still needs fell by exactly min(T, left)."""
    groups = [(5, 3, 128, 55), (70, 2, 192, 192), (3, 5, 64, 1), (2, 4, 128, 63)]
    a = arena(torch, "mix", groups)
    rng = np.random.default_rng(11)
    plain = rng.integers(0, 256, (6, 1000), dtype=np.uint8)
    d_plain = torch.from_numpy(plain).cuda()
    want_plain = np.stack([hexrow(r.tobytes()) for r in plain])
    want_short = np.stack([hexrow(r[:300].tobytes()) for r in plain])
    q = mkq(cess, tick, capacity=128)
    outs, tickets = [], []

    def add(kind):
        if kind == "strided":
            d = out(torch, 6)
            tickets.append(q.add(d_plain, 6, 1, 1000, 1000, 1000, d, 1, 64))
            outs.append((d, want_plain, kind))
        elif kind == "ptrs":
            d = out(torch, 6)
            tickets.append(q.add_ptrs([d_plain[i, :300] for i in range(6)], d, 64))
            outs.append((d, want_short, kind))
        else:
            d, p = out(torch, groups[kind][0]), out(torch, groups[kind][0])
            tickets.append(q.add_concat_ptrs(a.chains[kind], d, 64, p, 64, length=a.length[kind]))
            outs.append((d, a.want[kind], groups[kind]))
            outs.append((p, a.want_pre[kind], (groups[kind], "prefix")))

    def tick_and_check(T):
        before, live = q.blocks_left, q.live_chains
        q.tick(T)
        assert q.blocks_left == before - min(T, before), (T, before)
        assert q.live_chains <= live

    add(0)
    add("strided")
    tick_and_check(1)          # group 0 stands one block into its two-block part
    add(1)
    add("ptrs")
    tick_and_check(2)          # group 0 crosses after 1, group 1 has not reached its boundary
    add(2)
    tick_and_check(3)          # group 1 crosses after 1, group 2 after every block
    add(3)
    for T in (5, 1, 2, 7):
        tick_and_check(T)
    while q.live_chains:
        tick_and_check(3)
    assert tickets == list(range(1, 7)) and all(q.done(t) for t in tickets)
    torch.cuda.synchronize()
    for d, want, what in outs:
        check_out(d, want, what)
    q.close()


def test_ring_wrap(torch, cess):
    groups = [(5, 3, 128, 56)] * 4
    a = arena(torch, "wrap", groups)
    q = mkq(cess, 0, capacity=8)
    for gi in range(4):  # slots 0..4, 5..9, 10..14, 15..19 of an 8-slot ring
        d_hex, d_pre = out(torch, 5), out(torch, 5)
        q.add_concat_ptrs(a.chains[gi], d_hex, 64, d_pre, 64, length=a.length[gi])
        drain(q, "tick3" if gi % 2 else "finish")
        torch.cuda.synchronize()
        check_out(d_hex, a.want[gi], gi)
        check_out(d_pre, a.want_pre[gi], (gi, "prefix"))
    q.close()


def test_queue_full_adds_nothing(torch, cess):
    groups = [(5, 2, 192, 63)] * 2
    a = arena(torch, "full", groups)
    q = mkq(cess, 0, capacity=8)
    first, second = out(torch, 5), out(torch, 5)
    t1 = q.add_concat_ptrs(a.chains[0], first, 64, length=a.length[0])
    with pytest.raises(cess.CecError) as ei:
        q.add_concat_ptrs(a.chains[1], second, 64, length=a.length[1])
    assert ei.value.code == ENOMEM
    assert q.live_chains == 5 and not q.done(t1)
    q.finish()
    torch.cuda.synchronize()
    assert q.done(t1)
    check_out(first, a.want[0], "first")
    assert bool((second == 0xA5).all())
    assert q.add_concat_ptrs(a.chains[1], second, 64, length=a.length[1]) == t1 + 1
    q.finish()
    torch.cuda.synchronize()
    check_out(second, a.want[1], "second")
    q.close()


def test_refusals_leave_the_ring_unchanged(torch, cess):
    from cess_amd import _lib
    groups = [(4, 3, 128, 55), (4, 3, 128, 128)]
    a = arena(torch, "refuse", groups)
    q = mkq(cess, 0, capacity=64)
    first, second, spare = out(torch, 4), out(torch, 4), out(torch, 4)
    t1 = q.add_concat_ptrs(a.chains[0], first, 64, length=a.length[0])
    q.tick(1)
    # a NULL entry, first and last of the array
    flat = [t.data_ptr() for row in a.chains[1] for t in row]
    for hole in (0, len(flat) - 1):
        ptrs = (ctypes.c_void_p * len(flat))(*[None if i == hole else p
                                               for i, p in enumerate(flat)])
        ticket = ctypes.c_uint64(99)
        rc = _lib.load().cec_hashq_add_concat_ptrs(q._h, ptrs, 4, 3, 128, 0,
                                                   spare.data_ptr() + 64, None,
                                                   ctypes.byref(ticket))
        assert rc == EINVAL and ticket.value == 99
        assert q.live_chains == 4
    # part_len 96: the library's refusal, as ErrInvalidInput
    odd = [[a.dev[0:96], a.dev[128:224]]]
    with pytest.raises(cess.ErrInvalidInput) as ei:
        q.add_concat_ptrs(odd, spare, 64)
    assert ei.value.code == EINVAL
    # len that ends before the last part, in no part at all, or past the last part
    for bad in (2 * 128, 1, 3 * 128 + 1):
        with pytest.raises(cess.ErrInvalidInput) as ei:
            q.add_concat_ptrs(a.chains[1], spare, 64, length=bad)
        assert ei.value.code == EINVAL
        assert q.live_chains == 4 and q.blocks_left == cess.sha256_blocks(a.length[0]) - 1
    t2 = q.add_concat_ptrs(a.chains[1], second, 64)  # the refused adds took no ticket
    assert t2 == t1 + 1 and q.live_chains == 8
    q.finish()
    torch.cuda.synchronize()
    check_out(first, a.want[0], "first")
    check_out(second, a.want[1], "second")
    assert bool((spare == 0xA5).all())
    q.close()


def test_array_belongs_to_the_caller_on_return(torch, cess):
    """The pointer array is overwritten right after the call returns, before any tick."""
    from cess_amd import _lib
    groups = [(300, 3, 64, 56)]
    a = arena(torch, "caller", groups)
    q = mkq(cess, 0, capacity=512)
    d_hex = torch.zeros((300, 64), dtype=torch.uint8, device="cuda")
    flat = [t.data_ptr() for row in a.chains[0] for t in row]
    ptrs = (ctypes.c_void_p * len(flat))(*flat)
    ticket = ctypes.c_uint64()
    rc = _lib.load().cec_hashq_add_concat_ptrs(q._h, ptrs, 300, 3, 64, a.length[0],
                                               d_hex.data_ptr(), None, ctypes.byref(ticket))
    bogus = a.chains[0][0][0].data_ptr()  # a valid address, the wrong bytes
    for i in range(len(flat)):
        ptrs[i] = bogus
    assert rc == 0 and ticket.value == 1
    q.finish()
    torch.cuda.synchronize()
    assert np.array_equal(d_hex.cpu().numpy(), a.want[0])
    q.close()


@pytest.mark.parametrize("k,m", [(2, 1), (4, 2)])
def test_segment_lists_of_scattered_shards(torch, cess, k, m):
    nseg, F = 3, 256
    rng = np.random.default_rng(100 * k + m)
    data = rng.integers(0, 256, (nseg, k, F), dtype=np.uint8)
    par = rng.integers(0, 256, (nseg, m, F), dtype=np.uint8)
    d_data, d_par = torch.from_numpy(data).cuda(), torch.from_numpy(par).cuda()
    segments = []
    for s in range(nseg):  # every shard a tensor of its own, parity first in memory
        ps = [torch.empty(F, dtype=torch.uint8, device="cuda").copy_(d_par[s, j]) for j in range(m)]
        ds = [torch.empty(F, dtype=torch.uint8, device="cuda").copy_(d_data[s, j])
              for j in reversed(range(k))]
        segments.append(ds[::-1] + ps)
    seg_a = torch.zeros((nseg, 64), dtype=torch.uint8, device="cuda")
    frag_a = torch.zeros((nseg, k + m, 64), dtype=torch.uint8, device="cuda")
    seg_b, frag_b = torch.zeros_like(seg_a), torch.zeros_like(frag_a)
    with mkq(cess, 0, capacity=64) as q:
        t = q.add_segment_lists_device(segments, k, m, seg_a, frag_a)
        q.add_segment_lists(d_data, d_par, nseg, k, m, F, seg_b, frag_b)
        assert q.live_chains == 2 * nseg * (k + m)
        q.tick(F // 64 * k)
        assert not q.done(t)
        q.tick(1)
        assert q.done(t)
        q.finish()
        torch.cuda.synchronize()
    assert torch.equal(seg_a, seg_b) and torch.equal(frag_a, frag_b)
    want_seg = np.stack([hexrow(data[s].tobytes()) for s in range(nseg)])
    want_frag = np.stack([np.stack([hexrow(x.tobytes()) for x in list(data[s]) + list(par[s])])
                          for s in range(nseg)])
    assert np.array_equal(seg_a.cpu().numpy(), want_seg)
    assert np.array_equal(frag_a.cpu().numpy(), want_frag)
