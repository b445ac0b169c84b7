"""The checking adds of the hash queue on the GPU (cec_hashq_add_check,
cec_hashq_add_check_concat_ptrs; HashQueue.add_check, add_check_ptrs, add_check_concat_ptrs): each
chain compares its digest with a recorded hash and leaves one flag byte in HBM, written by the tick
launch that completes it.

Expectations come from hashlib. Every flag buffer is pre-filled with 0xA5 and carries a guard byte
on each side, every hex output a guard row on each side, and the whole vectors are asserted: a
flag that is not written, written early, or written beside its place shows."""
import ctypes
import hashlib

import numpy as np
import pytest

from tests.sha_model import state_after

pytestmark = pytest.mark.gpu

HQOPT_TICK = 1
EINVAL, ENOMEM = -1, -5
FILL = 0xA5
TICKS = [0, 1, 2, 3, 4]
LENS = [0, 55, 56, 64, 119, 4113]  # one and two padding blocks, one block, an odd tail
HEXDIGITS = b"0123456789abcdef"
_TABLES = {}


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


def other_digit(row, pos):
    """`row` with the character at `pos` replaced by another lowercase hex digit."""
    out = row.copy()
    out[pos] = HEXDIGITS[(HEXDIGITS.index(bytes([row[pos]])) + 1 + pos % 15) % 16]
    assert out[pos] != row[pos] and bytes([out[pos]]) in HEXDIGITS
    return out


def every_position(want):
    """Expectations and flags for the 129 digests `want`: chain 2i is wrong in character i alone,
    chain 2i + 1 is clean, chain 128 is its true digest in upper case."""
    assert len(want) == 129
    exp = want.copy()
    for i in range(64):
        exp[2 * i] = other_digit(want[2 * i], i)
    upper = np.frombuffer(bytes(want[128]).upper(), np.uint8)
    assert not np.array_equal(upper, want[128]), "the digest holds no letter"
    exp[128] = upper
    flags = np.array([0, 1] * 64 + [0], np.uint8)
    assert int((exp != want).sum()) >= 65 and all((exp[2 * i] != want[2 * i]).sum() == 1
                                                  for i in range(64))
    return exp, flags


def some_wrong(want):
    """Every third expectation wrong in one character; the flags that go with them."""
    exp = want.copy()
    for i in range(0, len(want), 3):
        exp[i] = other_digit(want[i], (7 * i) % 64)
    return exp, np.array([0 if i % 3 == 0 else 1 for i in range(len(want))], np.uint8)


def table(torch, n, ln):
    """n buffers of ln bytes in separate allocations, every third one byte off its allocation's
    base: (host bytes, allocations, addresses, views or None for ln == 0, hex [n][64]). Made once
    per shape and read-only afterwards."""
    key = (n, ln)
    if key not in _TABLES:
        host = np.random.default_rng(n * 100003 + ln).integers(0, 256, (n, ln), dtype=np.uint8)
        stage = torch.from_numpy(host).cuda()
        bases, addrs, views = [], [], []
        for i in range(n):
            off = 1 if i % 3 == 1 else 0
            base = torch.empty(ln + 17, dtype=torch.uint8, device="cuda")
            if ln:
                base[off:off + ln].copy_(stage[i])
                views.append(base[off:off + ln])
            bases.append(base)
            addrs.append(base.data_ptr() + off)
        want = np.stack([hexrow(r) for r in host])
        host.setflags(write=False)
        want.setflags(write=False)
        _TABLES[key] = (host, bases, addrs, views if ln else None, want)
    return _TABLES[key]


def guarded(torch, n, width=None):
    """n flags (or n rows of `width`) of FILL between two guards, and the view between them."""
    shape = (n + 2,) if width is None else (n + 2, width)
    full = torch.full(shape, FILL, dtype=torch.uint8, device="cuda")
    return full, full[1:-1]


def image(n, where=(), rows=(), width=None):
    img = np.full((n + 2,) if width is None else (n + 2, width), FILL, np.uint8)
    for w, r in zip(where, rows):
        img[1 + w] = r
    return img


def add_table(torch, q, n, ln, exp, d_ok, d_hex):
    """The table form over table(n, ln): through HashQueue.add_check_ptrs, or for empty buffers
    (a tensor without elements has no address) through the C call."""
    _, _, addrs, views, _ = table(torch, n, ln)
    if views is not None:
        t, ok = q.add_check_ptrs(views, exp, d_ok, d_hex)
        assert ok is d_ok
        return t
    from cess_amd import _lib
    ptrs = (ctypes.c_void_p * n)(*addrs)
    t = ctypes.c_uint64()
    rc = _lib.load().cec_hashq_add_check_concat_ptrs(
        q._h, ptrs, n, 1, 0, 0, exp.data_ptr(), d_ok.data_ptr(),
        None if d_hex is None else d_hex.data_ptr(), None, ctypes.byref(t))
    assert rc == 0
    return t.value


@pytest.mark.parametrize("tick", TICKS)
def test_every_hex_position_can_fail_a_chain_table_form(torch, cess, tick):
    n = 129
    q = mkq(cess, tick, capacity=256)
    for ln in LENS:
        want = table(torch, n, ln)[4]
        exp, flags = every_position(want)
        d_exp = torch.from_numpy(exp).cuda()
        ok_full, d_ok = guarded(torch, n)
        hex_full, d_hex = guarded(torch, n, 64)
        t = add_table(torch, q, n, ln, d_exp, d_ok, d_hex)
        assert q.live_chains == n and not q.done(t)
        q.finish()
        assert q.done(t) and q.live_chains == 0
        torch.cuda.synchronize()
        assert np.array_equal(ok_full.cpu().numpy(), image(n, range(n), flags)), ln
        assert np.array_equal(hex_full.cpu().numpy(), image(n, range(n), want, 64)), ln
        assert np.array_equal(d_exp.cpu().numpy(), exp), ln
    q.close()


@pytest.mark.parametrize("tick", TICKS)
def test_every_hex_position_can_fail_a_chain_strided_form(torch, cess, tick):
    """per = 3 with unequal outer strides for the data, the hex, the expectations and the flags;
    an odd data stride, so groups alternate between aligned and unaligned buffers."""
    n, per = 129, 3
    groups = n // per
    hex_outer, exp_outer, ok_outer = 4, 5, 7
    q = mkq(cess, tick, capacity=256)
    for ln in LENS:
        rng = np.random.default_rng(977 + ln)
        inner = ln + 16 - ln % 16
        outer = per * inner + 7
        data = rng.integers(0, 256, groups * outer + 64, dtype=np.uint8)
        want = np.stack([hexrow(data[(i // per) * outer + (i % per) * inner:][:ln])
                         for i in range(n)])
        exp, flags = every_position(want)
        place = [(i // per, i % per) for i in range(n)]
        exp_img = rng.integers(0, 256, (groups * exp_outer, 64), dtype=np.uint8)
        for (a, b), e in zip(place, exp):
            exp_img[a * exp_outer + b] = e
        d_data = torch.from_numpy(data).cuda()
        d_exp = torch.from_numpy(exp_img).cuda()
        ok_full, d_ok = guarded(torch, groups * ok_outer)
        hex_full, d_hex = guarded(torch, groups * hex_outer, 64)
        t = q.add_check(d_data, n, per, outer, inner, ln, d_exp, exp_outer, d_ok, ok_outer, d_hex,
                        hex_outer)
        assert q.live_chains == n and not q.done(t)
        q.finish()
        assert q.done(t) and q.live_chains == 0
        torch.cuda.synchronize()
        assert np.array_equal(ok_full.cpu().numpy(),
                              image(groups * ok_outer, [a * ok_outer + b for a, b in place],
                                    flags)), ln
        assert np.array_equal(hex_full.cpu().numpy(),
                              image(groups * hex_outer, [a * hex_outer + b for a, b in place],
                                    want, 64)), ln
        assert np.array_equal(d_exp.cpu().numpy(), exp_img), ln
    q.close()


@pytest.mark.parametrize("tick", TICKS)
def test_flags_are_written_by_the_completing_launch_only(torch, cess, tick):
    """Chains of 64 blocks ticked three blocks at a time: nothing of a chain's outputs exists
    before the tick that completes it."""
    n, ln = 66, 63 * 64 + 10
    assert cess.sha256_blocks(ln) == 64
    want = table(torch, n, ln)[4]
    exp, flags = some_wrong(want)
    q = mkq(cess, tick, capacity=128)
    ok_full, d_ok = guarded(torch, n)
    hex_full, d_hex = guarded(torch, n, 64)
    d_exp = torch.from_numpy(exp).cuda()  # read by the completing tick: alive until then
    t = add_table(torch, q, n, ln, d_exp, d_ok, d_hex)
    q.tick(3)
    torch.cuda.synchronize()
    assert not q.done(t) and q.blocks_left == 61
    assert bool((ok_full == FILL).all()) and bool((hex_full == FILL).all())
    ticks = 1
    while q.live_chains:
        q.tick(3)
        ticks += 1
        if q.live_chains:  # 63 blocks done at the most: still nothing
            torch.cuda.synchronize()
            assert bool((ok_full == FILL).all()), ticks
    assert ticks == 22 and q.done(t)
    torch.cuda.synchronize()
    assert np.array_equal(ok_full.cpu().numpy(), image(n, range(n), flags))
    assert np.array_equal(hex_full.cpu().numpy(), image(n, range(n), want, 64))
    q.close()


@pytest.mark.parametrize("tick", [0, 3])
@pytest.mark.parametrize("n", [1, 64, 65, 300, 513])
def test_group_and_launch_boundaries(torch, cess, n, tick):
    """A group of 64 and one more, two and three add launches of the table form (256 chains
    each) and of the strided form (256 threads a block)."""
    ln = 119
    host, _, _, _, want = table(torch, n, ln)
    exp, flags = some_wrong(want)
    d_exp = torch.from_numpy(exp).cuda()
    q = mkq(cess, tick, capacity=2048)
    ok_a, d_ok_a = guarded(torch, n)
    ok_b, d_ok_b = guarded(torch, n)
    hex_a, d_hex_a = guarded(torch, n, 64)
    packed = torch.from_numpy(host.copy()).cuda()
    t1 = add_table(torch, q, n, ln, d_exp, d_ok_a, d_hex_a)
    t2 = q.add_check(packed, n, 1, ln, ln, ln, d_exp, 1, d_ok_b, 1)
    assert (t1, t2) == (1, 2) and q.live_chains == 2 * n
    q.finish()
    torch.cuda.synchronize()
    assert np.array_equal(ok_a.cpu().numpy(), image(n, range(n), flags))
    assert np.array_equal(ok_b.cpu().numpy(), image(n, range(n), flags))
    assert np.array_equal(hex_a.cpu().numpy(), image(n, range(n), want, 64))
    q.close()


def test_ring_wrap(torch, cess):
    want = table(torch, 300, 56)[4]
    views = table(torch, 300, 56)[3]
    exp, flags = some_wrong(want)
    q = mkq(cess, 0, capacity=128)
    for lo in (0, 100, 200):  # slots 0..99, 100..199 and 200..299 of a ring of 128
        ok_full, d_ok = guarded(torch, 100)
        t, _ = q.add_check_ptrs(views[lo:lo + 100], [bytes(e) for e in exp[lo:lo + 100]], d_ok)
        assert t == lo // 100 + 1
        q.finish()
        torch.cuda.synchronize()
        assert np.array_equal(ok_full.cpu().numpy(), image(100, range(100), flags[lo:lo + 100])), lo
    q.close()


def _mixed_run(torch, cess, tick, checking):
    """A plain pointer add, a checking strided add, a resumed add and a checking concat add with
    a prefix digest in one ring of 64 slots, ticked two blocks at a time. Without `checking` only
    the plain and the resumed add. Returns every output as host arrays."""
    q = mkq(cess, tick, capacity=64)
    keep, res = [], {}
    # plain
    _, _, _, views, want_plain = table(torch, 10, 4113)
    hex_plain, d = guarded(torch, 10, 64)
    tickets = [q.add_ptrs(views, d)]
    # checking, strided
    if checking:
        rng = np.random.default_rng(31)
        data = rng.integers(0, 256, (7, 200), dtype=np.uint8)
        want_s = np.stack([hexrow(r) for r in data])
        exp_s, flags_s = some_wrong(want_s)
        d_data, d_exp = torch.from_numpy(data).cuda(), torch.from_numpy(exp_s).cuda()
        ok_s, d_ok = guarded(torch, 7)
        hex_s, d_hex = guarded(torch, 7, 64)
        keep += [d_data, d_exp]
        tickets.append(q.add_check(d_data, 7, 1, 200, 200, 200, d_exp, 1, d_ok, 1, d_hex, 1))
    # resumed: the device holds junk where the state already covers the bytes
    rng = np.random.default_rng(32)
    ln, start = 64 * 40 + 17, 64 * 33
    true = rng.integers(0, 256, (5, ln), dtype=np.uint8)
    img = true.copy()
    img[:, :start] ^= rng.integers(1, 256, (5, start), dtype=np.uint8)
    states = np.array([state_after(r.tobytes(), start // 64) for r in true], np.uint32)
    d_img, d_states = torch.from_numpy(img).cuda(), torch.from_numpy(states.view(np.int32)).cuda()
    hex_res, d = guarded(torch, 5, 64)
    keep += [d_img, d_states]
    tickets.append(q.add_resume(d_img, 5, 1, ln, ln, ln, start, d_states, d, 1))
    # checking, chains over three scattered parts, the last in part, with the prefix digest
    if checking:
        rng = np.random.default_rng(33)
        parts = rng.integers(0, 256, (6, 3, 128), dtype=np.uint8)
        chains = [[torch.from_numpy(parts[i, p].copy()).cuda() for p in range(3)]
                  for i in range(6)]
        want_c = np.stack([hexrow(parts[i].reshape(-1)[:300]) for i in range(6)])
        want_p = np.stack([hexrow(parts[i, 0]) for i in range(6)])
        exp_c, flags_c = some_wrong(want_c)
        ok_c, d_ok = guarded(torch, 6)
        hex_c, d_hex = guarded(torch, 6, 64)
        pre_c, d_pre = guarded(torch, 6, 64)
        d_exp_c = torch.from_numpy(exp_c).cuda()
        t, ok = q.add_check_concat_ptrs(chains, d_exp_c, d_ok, d_hex, d_pre, length=300)
        assert ok is d_ok
        keep += [chains, d_exp_c]
        tickets.append(t)
    assert tickets == list(range(1, len(tickets) + 1))
    assert q.live_chains == (28 if checking else 15)
    while q.live_chains:
        q.tick(2)
    assert all(q.done(t) for t in tickets)
    torch.cuda.synchronize()
    q.close()
    res["plain"] = hex_plain.cpu().numpy()
    res["resumed"] = hex_res.cpu().numpy()
    assert np.array_equal(res["plain"], image(10, range(10), want_plain, 64))
    assert np.array_equal(res["resumed"], image(5, range(5), [hexrow(r) for r in true], 64))
    if checking:
        assert np.array_equal(hex_s.cpu().numpy(), image(7, range(7), want_s, 64))
        assert np.array_equal(ok_s.cpu().numpy(), image(7, range(7), flags_s))
        assert np.array_equal(hex_c.cpu().numpy(), image(6, range(6), want_c, 64))
        assert np.array_equal(pre_c.cpu().numpy(), image(6, range(6), want_p, 64))
        assert flags_c.tolist() == [0, 1, 1, 0, 1, 1]
        assert np.array_equal(ok_c.cpu().numpy(), image(6, range(6), flags_c))
    return res


@pytest.mark.parametrize("tick", TICKS)
def test_mixed_ring(torch, cess, tick):
    with_checks = _mixed_run(torch, cess, tick, True)
    without = _mixed_run(torch, cess, tick, False)
    for name in ("plain", "resumed"):
        assert np.array_equal(with_checks[name], without[name]), name


@pytest.mark.parametrize("tick", [0, 3])
def test_flags_only(torch, cess, tick):
    """d_hex NULL: the flags are all the add writes."""
    n, ln = 65, 4113
    host, _, _, views, want = table(torch, n, ln)
    exp, flags = some_wrong(want)
    d_exp = torch.from_numpy(exp).cuda()
    packed = torch.from_numpy(host.copy()).cuda()
    q = mkq(cess, tick, capacity=256)
    ok_a, d_ok_a = guarded(torch, n)
    ok_b, d_ok_b = guarded(torch, n)
    q.add_check_ptrs(views, d_exp, d_ok_a)
    q.add_check(packed, n, 1, ln, ln, ln, d_exp, 1, d_ok_b, 1)
    q.finish()
    torch.cuda.synchronize()
    assert np.array_equal(ok_a.cpu().numpy(), image(n, range(n), flags))
    assert np.array_equal(ok_b.cpu().numpy(), image(n, range(n), flags))
    assert np.array_equal(d_exp.cpu().numpy(), exp)
    assert np.array_equal(packed.cpu().numpy(), host)
    q.close()


def test_a_new_flag_tensor_and_a_list_of_hashes(torch, cess):
    """d_ok None makes the flags; a list of bytes is uploaded and kept until its add is done."""
    n, ln = 65, 119
    views, want = table(torch, n, ln)[3:]
    exp, flags = some_wrong(want)
    q = mkq(cess, 0, capacity=128)
    t, d_ok = q.add_check_ptrs(views, [bytes(e) for e in exp])
    assert d_ok.dtype == torch.uint8 and d_ok.shape == (n,) and d_ok.is_cuda
    assert [k[0] for k in q._kept] == [t]
    q.finish()
    assert q._kept == []
    torch.cuda.synchronize()
    assert np.array_equal(d_ok.cpu().numpy(), flags)
    with pytest.raises(cess.ErrInvalidInput):
        q.add_check_ptrs(views, [bytes(e) for e in exp[:-1]])
    with pytest.raises(cess.ErrInvalidInput):
        q.add_check_ptrs(views, [bytes(e)[:63] for e in exp])
    assert q.live_chains == 0
    q.close()


@pytest.mark.parametrize("tick", [0, 3])
def test_expectations_in_pinned_host_memory(torch, cess, tick):
    n, ln = 65, 119
    host, _, _, views, want = table(torch, n, ln)
    exp, flags = some_wrong(want)
    pinned = torch.from_numpy(exp.copy()).pin_memory()
    packed = torch.from_numpy(host.copy()).cuda()
    q = mkq(cess, tick, capacity=256)
    ok_a, d_ok_a = guarded(torch, n)
    ok_b, d_ok_b = guarded(torch, n)
    q.add_check_ptrs(views, pinned, d_ok_a)
    q.add_check(packed, n, 1, ln, ln, ln, pinned.data_ptr(), 1, d_ok_b, 1)
    q.finish()
    torch.cuda.synchronize()
    assert np.array_equal(ok_a.cpu().numpy(), image(n, range(n), flags))
    assert np.array_equal(ok_b.cpu().numpy(), image(n, range(n), flags))
    assert np.array_equal(pinned.numpy(), exp)
    q.close()


def test_errors_leave_the_ring_and_the_flags_alone(torch, cess):
    from cess_amd import _lib
    lib = _lib.load()
    n, ln = 40, 4113
    host, _, addrs, views, want = table(torch, 300, ln)
    d_exp = torch.from_numpy(want[:n].copy()).cuda()
    packed = torch.from_numpy(host[:n].copy()).cuda()
    ok_full, d_ok = guarded(torch, n)
    hex_full, d_hex = guarded(torch, n, 64)
    q = mkq(cess, 0, capacity=64)
    t1 = q.add_ptrs(views[:10])
    ptrs = (ctypes.c_void_p * n)(*addrs[:n])
    ticket = ctypes.c_uint64(77)
    E, O, H, P = d_exp.data_ptr(), d_ok.data_ptr(), d_hex.data_ptr(), packed.data_ptr()
    assert E % 4 == 0

    def table_form(ptrs_=ptrs, n_=n, parts=1, part_len=0, ln_=ln, e=E, o=O, h=H, pre=None):
        return lib.cec_hashq_add_check_concat_ptrs(q._h, ptrs_, n_, parts, part_len, ln_, e, o, h,
                                                   pre, ctypes.byref(ticket))

    def strided_form(base=P, n_=n, per=1, e=E, o=O):
        return lib.cec_hashq_add_check(q._h, base, n_, per, ln, ln, ln, e, 1, o, 1, H, 1,
                                       ctypes.byref(ticket))

    with_null = (ctypes.c_void_p * n)(*addrs[:n])
    with_null[n - 1] = None
    pairs = (ctypes.c_void_p * n)(*addrs[:n])  # 20 chains of two parts
    refused = {
        "table: NULL d_expect": lambda: table_form(e=None),
        "table: NULL d_ok": lambda: table_form(o=None),
        "table: d_expect at an odd address": lambda: table_form(e=E + 1),
        "table: d_expect two bytes off": lambda: table_form(e=E + 2),
        "table: NULL array": lambda: table_form(ptrs_=None),
        "table: NULL entry": lambda: table_form(ptrs_=with_null),
        "concat: parts == 0": lambda: table_form(parts=0, part_len=64, ln_=0),
        "concat: part_len == 0": lambda: table_form(pairs, 20, 2, 0, 0),
        "concat: part_len no multiple of 64": lambda: table_form(pairs, 20, 2, 96, 0),
        "concat: len ends before the last part": lambda: table_form(pairs, 20, 2, 128, 128),
        "concat: len past the last part": lambda: table_form(pairs, 20, 2, 128, 257),
        "concat: NULL entry": lambda: table_form(with_null, 20, 2, 128, 0),
        "concat: prefix digest without a whole first part":
            lambda: table_form(parts=1, part_len=128, ln_=100, pre=H),
        "strided: NULL d_expect": lambda: strided_form(e=None),
        "strided: NULL d_ok": lambda: strided_form(o=None),
        "strided: d_expect at an odd address": lambda: strided_form(e=E + 3),
        "strided: NULL base": lambda: strided_form(base=None),
        "strided: per == 0": lambda: strided_form(per=0),
    }
    for what, call in refused.items():
        assert call() == EINVAL, what
        assert q.live_chains == 10 and not q.done(t1), what
    # a full ring: 10 live, 60 more do not fit in 64 slots
    many = (ctypes.c_void_p * 60)(*addrs[:60])
    assert table_form(ptrs_=many, n_=60) == ENOMEM
    packed60 = torch.from_numpy(host[:60].copy()).cuda()
    assert strided_form(base=packed60.data_ptr(), n_=60) == ENOMEM
    with pytest.raises(cess.CecError) as ei:
        q.add_check_ptrs(views[:60], torch.from_numpy(want[:60].copy()).cuda())
    assert ei.value.code == ENOMEM
    assert q.live_chains == 10 and ticket.value == 77
    # n == 0 is no error and takes no ticket, whatever the other arguments
    assert table_form(ptrs_=None, n_=0, e=None, o=None, h=None) == 0 and ticket.value == 0
    ticket.value = 77
    assert strided_form(base=None, n_=0, e=None, o=None) == 0 and ticket.value == 0
    q.finish()
    torch.cuda.synchronize()
    assert bool((ok_full == FILL).all()) and bool((hex_full == FILL).all())
    # the refused adds took no ticket, and the arguments they were refused with were good ones
    assert table_form() == 0 and ticket.value == t1 + 1
    q.finish()
    torch.cuda.synchronize()
    assert np.array_equal(ok_full.cpu().numpy(), image(n, range(n), np.ones(n, np.uint8)))
    assert np.array_equal(hex_full.cpu().numpy(), image(n, range(n), want[:n], 64))
    q.close()
