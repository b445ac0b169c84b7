"""cec_hashq_add_resume on the GPU (HashQueue.add_resume): chains that start from a state computed
elsewhere and hash bytes start_len .. len of their buffer, on every tick kernel.

In every test the first start_len bytes of each DEVICE buffer are junk: every byte differs from
the byte the state was computed over. The states come from tests/sha_model.py (a restatement of
FIPS 180-4, or the library's host hasher in the handoff test) over the true bytes, the expected
hexes from hashlib over the true bytes. A queue that reads the prefix, ignores the state or starts
at the wrong block gets a wrong digest; exact comparisons throughout.

The last test plays the script of tests/test_hashq_script.py: all five kinds of add in a ring of
64 slots that wraps, against that file's model of the ring after every operation."""
import ctypes
import hashlib

import numpy as np
import pytest

from tests.sha_model import IV, state_after
from tests.test_hashq_script import CAPACITY, SEED, Ring, blocks_of, script

pytestmark = pytest.mark.gpu

HQOPT_TICK = 1
EINVAL, ENOMEM = -1, -5
FILL = 0xA5
TICKS = [0, 1, 2, 3, 4]
FORMS = {"scalar": 0, "ni1": 1, "ni2": 2, "ni4": 3, "x16": 4}
# (len, start_len): the empty message, only the padding block left, every start of three blocks
# (start_len 0 from the IV), the padding edges r = 1, 55, 56 (two blocks left), 63, and the
# aligned fast loop entered mid-buffer and near the front
POINTS = [(0, 0), (64, 64), (192, 0), (192, 64), (192, 128), (192, 192), (192 + 1, 192),
          (192 + 55, 192), (192 + 56, 192), (192 + 63, 64), (64 * 40 + 17, 64 * 33),
          (64 * 40 + 17, 64)]
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


def hexrow(b):
    return np.frombuffer(hashlib.sha256(bytes(b)).hexdigest().encode(), np.uint8)


def out(torch, rows):
    """A hex output of `rows` rows between two guard rows, every byte FILL."""
    return torch.full((rows + 2, 64), FILL, dtype=torch.uint8, device="cuda")


def hex_image(rows, where, want):
    """What `out(rows)` must hold once row where[i] (guard row not counted) got want[i]."""
    img = np.full((rows + 2, 64), FILL, np.uint8)
    for r, w in zip(where, want):
        img[1 + r] = w
    return img


class Resumed:
    """Host side of one resumed add of n chains of `length` bytes in the strided layout of
    cec_hashq_add (chain i at base_off + (i // per) * outer + (i % per) * inner). `true` holds
    the bytes the digests are of, `image` what goes to the device: `true` with the first
    start_len bytes of every chain XORed with nonzero bytes. `states` are the chains' states
    after start_len true bytes, `want` the hex image of an `out` of `rows` rows."""

    def __init__(self, seed, n, length, start_len, per=1, outer=None, inner=None, base_off=0,
                 hex_outer=None):
        rng = np.random.default_rng(seed)
        inner = length if inner is None else inner
        outer = per * inner if outer is None else outer
        hex_outer = per if hex_outer is None else hex_outer
        self.n, self.length, self.start_len, self.per = n, length, start_len, per
        self.outer, self.inner, self.base_off, self.hex_outer = outer, inner, base_off, hex_outer
        self.offs = [base_off + (i // per) * outer + (i % per) * inner for i in range(n)]
        srt = sorted(self.offs)
        assert all(b - a >= length for a, b in zip(srt, srt[1:])), "chains overlap"
        size = max(self.offs) + length + 64
        self.true = rng.integers(0, 256, size, dtype=np.uint8)
        self.image = self.true.copy()
        junk = rng.integers(1, 256, size, dtype=np.uint8)
        for o in self.offs:
            self.image[o:o + start_len] ^= junk[o:o + start_len]
        self.bufs = [self.true[o:o + length].tobytes() for o in self.offs]
        self.states = np.array([state_after(b, start_len // 64) for b in self.bufs], np.uint32)
        self.blocks = (length >> 6) + (2 if (length & 63) >= 56 else 1) - start_len // 64
        self.rows = (n + per - 1) // per * hex_outer
        self.want = hex_image(self.rows, [(i // per) * hex_outer + i % per for i in range(n)],
                              [hexrow(b) for b in self.bufs])
        for a in (self.true, self.image, self.states, self.want):
            a.setflags(write=False)

    def upload(self, torch, states=None):
        """(data, states, hex) on the device; `states` replaces the model's (the handoff test)."""
        d = torch.from_numpy(self.image.copy()).cuda()
        assert d.data_ptr() % 16 == 0
        st = self.states if states is None else states
        d_states = torch.from_numpy(np.ascontiguousarray(st).view(np.uint8).copy()).cuda()
        return d, d_states, out(torch, self.rows)

    def add(self, q, d, states, d_hex):
        return q.add_resume(d.data_ptr() + self.base_off, self.n, self.per, self.outer,
                            self.inner, self.length, self.start_len, states, d_hex,
                            self.hex_outer, 64)

    def check(self, d_hex, what):
        got = d_hex.cpu().numpy()
        bad = [r - 1 for r in range(got.shape[0]) if not np.array_equal(got[r], self.want[r])]
        assert not bad, (what, "hex rows", bad)


def case(key, *a, **kw):
    """One Resumed per key for the whole module: made once, read-only afterwards."""
    if key not in _CASES:
        _CASES[key] = Resumed(*a, **kw)
    return _CASES[key]


@pytest.mark.parametrize("tick", TICKS)
def test_resume_points(torch, cess, tick):
    """Every (len, start_len) of POINTS, three chains each with their own data, live together.
    The start_len == 0 add, from the IV, also equals a plain add of the same buffer."""
    cases = [case(("point", p), 1000 + i, 3, p[0], p[1]) for i, p in enumerate(POINTS)]
    q = mkq(cess, tick, capacity=64)
    live = []
    for c in cases:
        d, st, hx = c.upload(torch)
        t = c.add(q, d, st, hx)
        assert t == len(live) + 1 and not q.done(t)
        live.append((c, d, st, hx))
    fresh = cases[POINTS.index((192, 0))]
    assert fresh.states.tolist() == [IV] * 3 and np.array_equal(fresh.image, fresh.true)
    plain = out(torch, 3)
    q.add(live[POINTS.index((192, 0))][1], 3, 1, 192, 192, 192, plain, 1, 64)
    assert q.live_chains == 3 * len(cases) + 3
    assert q.blocks_left == max(c.blocks for c in cases)
    q.finish()
    assert q.live_chains == 0 and all(q.done(t) for t in range(1, len(cases) + 2))
    torch.cuda.synchronize()
    for c, _, _, hx in live:
        c.check(hx, (c.length, c.start_len))
    fresh.check(plain, "plain add")
    q.close()


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("point", [(64 * 40 + 17, 64 * 33), (192 + 56, 192)])
@pytest.mark.parametrize("tick", TICKS)
def test_tick_granularity_and_bookkeeping(torch, cess, tick, point, T):
    """The add counts only the blocks from start_len on: it is done after exactly
    ceil(blocks / T) ticks of T blocks, not one sooner."""
    c = case(("point", point), 1000 + POINTS.index(point), 3, point[0], point[1])
    assert c.blocks == cess.sha256_blocks(c.length) - c.start_len // 64
    q = mkq(cess, tick, capacity=16)
    d, st, hx = c.upload(torch)
    t = c.add(q, d, st, hx)
    assert q.blocks_left == c.blocks and q.live_chains == 3
    ticks = -(-c.blocks // T)
    for i in range(ticks - 1):
        q.tick(T)
        assert not q.done(t) and q.live_chains == 3
        assert q.blocks_left == c.blocks - T * (i + 1)
    q.tick(T)
    assert q.done(t) and q.live_chains == 0 and q.blocks_left == 0
    torch.cuda.synchronize()
    c.check(hx, (point, T))
    q.close()


@pytest.mark.parametrize("tick", TICKS)
def test_unaligned_buffers(torch, cess, tick):
    """Nine chains per add at a stride of 1 mod 16 from an aligned base: buffer starts 0 .. 8
    bytes past a 16-byte boundary, so aligned chains (16-byte loads from block blk0 on) share an
    add and a wave with chains that take the byte path for every block from blk0 on."""
    cases = []
    for i, p in enumerate(POINTS):
        stride = (p[0] + 15) // 16 * 16 + 17
        cases.append(case(("align", p), 2000 + i, 9, p[0], p[1], outer=stride, inner=stride))
    q = mkq(cess, tick, capacity=128)
    live = []
    for c in cases:
        assert c.outer % 16 == 1 and [o % 16 for o in c.offs] == list(range(9))
        d, st, hx = c.upload(torch)
        c.add(q, d, st, hx)
        live.append((c, d, st, hx))
    assert q.live_chains == 9 * len(cases)
    while q.live_chains:
        q.tick(3)
    torch.cuda.synchronize()
    for c, _, _, hx in live:
        c.check(hx, (c.length, c.start_len))
    q.close()


@pytest.mark.parametrize("tick", TICKS)
def test_layout_and_state_indexing(torch, cess, tick):
    """Chain i takes states 8 i .. 8 i + 7 whatever its place in the layout: 300 chains (two
    workgroups of the add kernel), and 12 chains as 3 rows of 4 with gaps between buffers, rows
    and hex rows. Every chain has its own data, so its own state; hex rows nobody owns keep their
    fill."""
    many = case("n300", 3001, 300, 192 + 17, 128, outer=224, inner=224)
    grid = case("per4", 3002, 12, 192 + 1, 64, per=4, inner=208, outer=4 * 208 + 48, hex_outer=6)
    assert len({tuple(s) for s in many.states.tolist()}) == 300
    assert grid.rows == 18 and (grid.want[1 + 4] == FILL).all() and (grid.want[1 + 6] != FILL).all()
    q = mkq(cess, tick, capacity=512)
    live = []
    for c in (many, grid):
        d, st, hx = c.upload(torch)
        c.add(q, d, st, hx)
        live.append((c, d, st, hx))
    assert q.live_chains == 312 and q.blocks_left == 3
    q.tick(1)
    assert q.live_chains == 312 and q.blocks_left == 2
    q.finish()
    torch.cuda.synchronize()
    for c, _, _, hx in live:
        c.check(hx, c.n)
    q.close()


@pytest.mark.parametrize("where", ["device", "pinned"])
@pytest.mark.parametrize("tick", TICKS)
def test_states_are_read_by_the_add(torch, cess, tick, where):
    """The states belong to the caller again once the add's kernel has run on the queue's stream:
    they are zeroed after a synchronise and before any tick, from a device tensor and from pinned
    host memory (given by address)."""
    c = case("states", 4001, 5, 64 * 5 + 9, 128)
    q = mkq(cess, tick, capacity=16)
    d, d_states, hx = c.upload(torch)
    if where == "pinned":
        keep = torch.from_numpy(c.states.view(np.uint8).copy()).pin_memory()
        assert keep.is_pinned()
        t = c.add(q, d, keep.data_ptr(), hx)
    else:
        keep = d_states
        t = c.add(q, d, keep, hx)
    torch.cuda.synchronize()
    keep.zero_()
    torch.cuda.synchronize()
    assert not q.done(t) and q.blocks_left == c.blocks
    while q.live_chains:
        q.tick(2)
    torch.cuda.synchronize()
    c.check(hx, where)
    q.close()


@pytest.mark.parametrize("tick", TICKS)
def test_beside_fresh_and_prefix_chains(torch, cess, tick):
    """Five resumed chains at their last block between 20 fresh 40-block chains and 10 chains
    with a prefix digest: 35 chains, one group of 64 ring slots for every tick."""
    rng = np.random.default_rng(5001)
    fresh = rng.integers(0, 256, (20, 64 * 39 + 30), dtype=np.uint8)
    pre = rng.integers(0, 256, (10, 64 * 9 + 57), dtype=np.uint8)
    c = case("beside", 5002, 5, 64 * 6 + 20, 64 * 6)
    assert cess.sha256_blocks(fresh.shape[1]) == 40 and c.blocks == 1
    q = mkq(cess, tick, capacity=64)
    d_fresh, d_pre = torch.from_numpy(fresh).cuda(), torch.from_numpy(pre).cuda()
    h_fresh, h_pre, p_pre = out(torch, 20), out(torch, 10), out(torch, 10)
    t1 = q.add(d_fresh, 20, 1, fresh.shape[1], fresh.shape[1], fresh.shape[1], h_fresh, 1, 64)
    d, st, hx = c.upload(torch)
    t2 = c.add(q, d, st, hx)
    t3 = q.add(d_pre, 10, 1, pre.shape[1], pre.shape[1], pre.shape[1], h_pre, 1, 64, 64 * 5,
               p_pre, 1, 64)
    assert q.live_chains == 35 and q.blocks_left == 40
    q.tick(2)
    assert q.done(t2) and not q.done(t1) and not q.done(t3) and q.live_chains == 30
    while q.live_chains:
        q.tick(2)
    assert q.done(t1) and q.done(t3)
    torch.cuda.synchronize()
    c.check(hx, "resumed")
    rows = list(range(20))
    assert np.array_equal(h_fresh.cpu().numpy(), hex_image(20, rows, [hexrow(r) for r in fresh]))
    assert np.array_equal(h_pre.cpu().numpy(), hex_image(10, rows, [hexrow(r) for r in pre]))
    assert np.array_equal(p_pre.cpu().numpy(),
                          hex_image(10, rows, [hexrow(r[:64 * 5]) for r in pre]))
    q.close()


def host_forms(lib):
    have = [name for name, f in FORMS.items() if lib.cec_host_sha_set_form(f) == 0]
    lib.cec_host_sha_set_form(-1)
    return have


@pytest.mark.parametrize("tick", TICKS)
def test_host_handoff(torch, cess, tick):
    """The pipeline's handoff: cec_sha256_host_state over the first start_len bytes of 19 host
    buffers, in every form the CPU has, gives the states (and the prefix's own hex); the queue
    continues over device copies whose prefix is junk."""
    from cess_amd import _lib
    lib = _lib.load()
    c = case("handoff", 6001, 19, 64 * 7 + 33, 64 * 5, outer=512, inner=512)
    host = [np.frombuffer(b, np.uint8) for b in c.bufs]
    ptrs = (ctypes.c_void_p * c.n)(*[h.ctypes.data for h in host])
    want_pre = [hashlib.sha256(b[:c.start_len]).hexdigest() for b in c.bufs]
    have = host_forms(lib)
    assert "scalar" in have
    q = mkq(cess, tick, capacity=128)
    live = []
    try:
        for name in have:
            assert lib.cec_host_sha_set_form(FORMS[name]) == 0
            hexo = np.zeros(64 * c.n, np.uint8)
            st = np.zeros(8 * c.n, np.uint32)
            assert lib.cec_sha256_host_state(ptrs, c.n, c.start_len, hexo.ctypes.data,
                                             st.ctypes.data, 1) == 0
            assert [bytes(hexo[64 * i:64 * i + 64]).decode() for i in range(c.n)] == want_pre
            d, d_states, hx = c.upload(torch, states=st)
            c.add(q, d, d_states, hx)
            live.append((name, d, d_states, hx))
    finally:
        lib.cec_host_sha_set_form(-1)
    q.finish()
    torch.cuda.synchronize()
    for name, _, _, hx in live:
        c.check(hx, name)
    q.close()


def test_refusals_leave_the_ring_unchanged(torch, cess):
    first = case("refuse0", 7001, 4, 192 + 56, 64)
    legal = case("refuse1", 7002, 3, 100, 64)       # 64 <= 100 & ~63: the last legal start
    big = case("refuse2", 7003, 10, 192, 128)
    after = case("refuse3", 7004, 9, 192 + 63, 192)
    q = mkq(cess, 0, capacity=16)
    d0, s0, h0 = first.upload(torch)
    t1 = first.add(q, d0, s0, h0)
    q.tick(1)
    left = first.blocks - 1
    d, st, spare = big.upload(torch)

    def refused(code, n, per, length, start_len, states):
        with pytest.raises(cess.CecError) as ei:
            q.add_resume(d, n, per, 192, 192, length, start_len, states, spare, 1, 64)
        assert ei.value.code == code
        assert q.live_chains == 4 and q.blocks_left == left and not q.done(t1)
        assert not q.done(t1 + 1)

    refused(EINVAL, 3, 1, 192, 63, st)
    refused(EINVAL, 3, 1, 127, 128, st)
    refused(EINVAL, 3, 1, 100, 128, st)
    refused(EINVAL, 3, 1, 192, 64, None)
    refused(EINVAL, 3, 0, 192, 64, st)
    assert q.add_resume(d, 0, 1, 192, 192, 192, 64, st, spare, 1, 64) == 0
    assert q.add_resume(d, 0, 1, 192, 192, 192, 64, None, spare, 1, 64) == 0
    assert q.live_chains == 4
    d1, s1, h1 = legal.upload(torch)
    t2 = legal.add(q, d1, s1, h1)               # the refused adds took no ticket
    assert t2 == t1 + 1 and q.live_chains == 7
    with pytest.raises(cess.CecError) as ei:    # 7 + 10 > 16
        big.add(q, d, st, spare)
    assert ei.value.code == ENOMEM
    assert q.live_chains == 7 and q.blocks_left == left and not q.done(t2 + 1)
    d3, s3, h3 = after.upload(torch)
    t3 = after.add(q, d3, s3, h3)               # 7 + 9 == 16: the ring is exactly full
    assert t3 == t2 + 1 and q.live_chains == 16
    with pytest.raises(cess.CecError) as ei:
        q.add_resume(d, 1, 1, 192, 192, 192, 128, st, spare, 1, 64)
    assert ei.value.code == ENOMEM and q.live_chains == 16
    q.finish()
    torch.cuda.synchronize()
    assert all(q.done(t) for t in (t1, t2, t3)) and not q.done(t3 + 1)
    first.check(h0, "first")
    legal.check(h1, "legal")
    after.check(h3, "after")
    assert bool((spare == FILL).all())
    q.close()


# ---- the mixed run ------------------------------------------------------------------------------

class Mixed:
    """Host side of one add of the script: the bytes to upload, and how to add them. Made once
    for the module (mixed_adds) and read-only afterwards."""

    def __init__(self, j, op):
        self.op, n, length = op, op["n"], op["length"]
        kind = op["kind"]
        rng = np.random.default_rng([SEED, j])
        rows = list(range(n))
        if kind == "resume":
            self.c = Resumed(rng.integers(1 << 30), n, length, op["start_len"],
                             outer=length + 9, inner=length + 9)
            return
        if kind == "strided":
            per = op["per"]
            self.inner, self.outer = length + 3, per * (length + 3) + 5
            self.offs = [(i // per) * self.outer + (i % per) * self.inner for i in rows]
            span = length
        elif kind == "concat":
            slot = op["part_len"] + 64      # a part, then 64 bytes that are not its own
            span = op["parts"] * slot
            self.offs = [i * span for i in rows]
        else:
            self.inner = self.outer = (length + 15) // 16 * 16 + (0 if kind == "prefix" else 16)
            self.offs = [i * self.outer for i in rows]
            span = length
        self.data = rng.integers(0, 256, self.offs[-1] + span + 64, dtype=np.uint8)
        if kind == "concat":
            self.parts = [[o + p * slot for p in range(op["parts"])] for o in self.offs]
            part_len = op["part_len"]
            bufs = [b"".join(self.data[x:x + part_len].tobytes() for x in row)[:length]
                    for row in self.parts]
            self.prefix = part_len if length >= part_len else 0
        else:
            bufs = [self.data[o:o + length].tobytes() for o in self.offs]
            self.prefix = op.get("prefix_len", 0)
        assert all(len(b) == length for b in bufs)
        self.want = hex_image(n, rows, [hexrow(b) for b in bufs])
        self.want_pre = hex_image(n, rows, [hexrow(b[:self.prefix]) for b in bufs])

    def upload(self, torch):
        """The add's device memory: (data, states or None, hex, prefix hex or None)."""
        if self.op["kind"] == "resume":
            return self.c.upload(torch) + (None,)
        n = self.op["n"]
        return torch.from_numpy(self.data).cuda(), None, out(torch, n), out(torch, n)

    def add(self, q, dev):
        """The add's ticket; raises what the queue raises."""
        op, n, length = self.op, self.op["n"], self.op["length"]
        kind = op["kind"]
        d, st, hx, px = dev
        if kind == "resume":
            return self.c.add(q, d, st, hx)
        if kind == "strided":
            return q.add(d, n, op["per"], self.outer, self.inner, length, hx, op["per"], 64)
        if kind == "prefix":
            return q.add(d, n, 1, self.outer, self.inner, length, hx, 1, 64, self.prefix, px, 1,
                         64)
        if kind == "ptrs":
            return q.add_ptrs([d[o:o + length] for o in self.offs], hx, 64)
        rows = [[d[x:x + op["part_len"]] for x in row] for row in self.parts]
        return q.add_concat_ptrs(rows, hx, 64, px if self.prefix else None, 64, length=length)

    def expect(self, dev, taken):
        """[(hex tensor, the image it must hold at the end)]; all fill where the add was refused
        or the output was not asked for."""
        _, _, hx, px = dev
        if self.op["kind"] == "resume":
            return [(hx, self.c.want if taken else np.full_like(self.c.want, FILL))]
        blank = np.full_like(self.want, FILL)
        return [(hx, self.want if taken else blank),
                (px, self.want_pre if taken and self.prefix else blank)]


def mixed_adds():
    if "mixed" not in _CASES:
        ops = script(SEED)
        _CASES["mixed"] = (ops, {j: Mixed(j, op) for j, op in enumerate(ops)
                                 if op["op"] == "add"})
    return _CASES["mixed"]


@pytest.mark.parametrize("tick", TICKS)
def test_mixed_script_against_the_ring_model(torch, cess, tick):
    """script(SEED): strided, prefix, resumed, pointer and concat adds between ticks of 1, 2, 3
    and 7 blocks in a ring of 64 slots that wraps several times and fills up. After every
    operation the queue's live_chains, blocks_left and done() of every ticket so far equal the
    model's, refusals included; at the end every digest and prefix digest equals hashlib's."""
    ops, adds = mixed_adds()
    ring = Ring(CAPACITY)
    q = mkq(cess, tick, capacity=CAPACITY)
    outs = []     # (op index, its device memory, whether the ring took it): alive to the end
    for j, op in enumerate(ops):
        if op["op"] == "tick":
            ring.tick(op["T"])
            q.tick(op["T"])
        else:
            want = ring.add(op["n"], blocks_of(op))
            dev = adds[j].upload(torch)
            if want is None:
                with pytest.raises(cess.CecError) as ei:
                    adds[j].add(q, dev)
                assert ei.value.code == ENOMEM, (j, op)
            else:
                assert adds[j].add(q, dev) == want, (j, op)
            outs.append((j, dev, want is not None))
        done, live, left = q.status(ring.next_ticket)
        assert (done, live, left) == (False, ring.live_chains, ring.blocks_left), (j, op)
        for t in range(1, ring.next_ticket):
            assert q.done(t) == ring.done(t), (j, op, t)
    ring.tick(0)
    q.finish()
    assert q.live_chains == 0 and all(q.done(t) for t in range(1, ring.next_ticket))
    torch.cuda.synchronize()
    for j, dev, taken in outs:
        for x, w in adds[j].expect(dev, taken):
            assert np.array_equal(x.cpu().numpy(), w), (j, ops[j], taken)
    q.close()
