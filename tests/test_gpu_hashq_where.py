"""Checked chains the GPU admits (cec_hashq_add_check_where_ptrs; HashQueue.add_check_where_ptrs):
which of an add's chains run is read from flag and gate bytes in HBM by the add's kernels, the
admitted chains are packed into the add's front slots and the rest parked behind them.

600 separate tensors, so an add takes three launches. Digests come from hashlib and every third
expectation is wrong in one character. Every flag buffer is pre-filled with 0xA5 and carries a
guard byte on each side, every hex output a guard row on each side, and the whole images are
asserted: an admitted chain shows 1 or 0 and its hex, every other chain 2 and an untouched hex
row. A chain that is not admitted has a real tensor or None, never an invented address."""
import ctypes
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HQOPT_TICK = 1
EINVAL, ENOMEM = -1, -5
FILL = 0xA5
SKIPPED = 2
REBUILT = 1
N = 600
TICKS = [1, 2, 3, 4]
LENS = [0, 55, 56, 64, 119, 8192]  # one and two padding blocks, one block, an odd tail, long
HEXDIGITS = b"0123456789abcdef"
_TABLES = {}


def plan(name, n=N):
    """(held, flags, per, gate bytes or None, gate, admitted) of a pattern over n chains."""
    rng = np.random.default_rng(len(name) * 1000 + n)
    held = np.ones(n, bool)
    want = np.zeros(n, bool)
    per, gates, gate = 1, None, 0
    if name == "all":
        want[:] = True
    elif name == "every64":
        want[::64] = True
    elif name == "last":
        want[-1] = True
    elif name == "tenth":
        want = rng.random(n) < 0.1
    elif name == "nulls":  # a third of the slots hold nothing, wanted or not
        want = rng.random(n) < 0.5
        held = rng.random(n) >= 1 / 3
    elif name == "gated":  # half wanted, in groups of six whose gate bytes take every status
        want = rng.random(n) < 0.5
        per, gate = 6, REBUILT
        gates = (np.arange((n + per - 1) // per) * 3 % 5).astype(np.uint8)
    flags = np.where(want, 0, rng.integers(1, 256, n)).astype(np.uint8)
    adm = held & (flags == 0)
    if gates is not None:
        adm &= gates[np.arange(n) // per] == gate
    return held, flags, per, gates, gate, adm


PATTERNS = ["none", "all", "every64", "last", "tenth", "nulls", "gated"]
PLANS = {name: plan(name) for name in PATTERNS}
# what each pattern admits, settled on the CPU before any GPU work
ADMITTED = {name: int(p[5].sum()) for name, p in PLANS.items()}
assert ADMITTED["none"] == 0 and ADMITTED["all"] == N and ADMITTED["every64"] == 10
assert ADMITTED["last"] == 1 and PLANS["last"][5][N - 1]
assert 30 <= ADMITTED["tenth"] <= 90
assert 150 <= ADMITTED["nulls"] <= 250 and (~PLANS["nulls"][0] & (PLANS["nulls"][1] == 0)).any()
assert 30 <= ADMITTED["gated"] <= 90 and set(PLANS["gated"][3]) == {0, 1, 2, 3, 4}


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


def some_wrong(want):
    """Every third expectation wrong in one character; the flags that go with them."""
    exp = want.copy()
    for i in range(0, len(want), 3):
        pos = (7 * i) % 64
        exp[i, pos] = HEXDIGITS[(HEXDIGITS.index(bytes([want[i, pos]])) + 1 + pos % 15) % 16]
        assert exp[i, pos] != want[i, pos]
    return exp, np.array([0 if i % 3 == 0 else 1 for i in range(len(want))], np.uint8)


def table(torch, ln, off=0):
    """N buffers of ln bytes in separate allocations, `off` bytes past their allocation's base:
    (allocations, addresses, views or None for ln == 0, hex [N][64], expectations, their flags).
    Made once per shape and read-only afterwards."""
    key = (ln, off)
    if key not in _TABLES:
        host = np.random.default_rng(100003 * off + ln).integers(0, 256, (N, ln), dtype=np.uint8)
        stage = torch.from_numpy(host).cuda()
        bases, addrs, views = [], [], []
        for i in range(N):
            base = torch.empty(ln + 17, dtype=torch.uint8, device="cuda")
            if ln:
                base[off:off + ln].copy_(stage[i])
                views.append(base[off:off + ln])
            bases.append(base)
            addrs.append(base.data_ptr() + off)
        want = np.stack([hexrow(r) for r in host])
        exp, right = some_wrong(want)
        for a in (want, exp, right):
            a.setflags(write=False)
        _TABLES[key] = (bases, addrs, views if ln else None, want, exp, right)
    return _TABLES[key]


def guarded(torch, n, width=None):
    """n flags (or n rows of `width`) of FILL between two guards, and the view between them."""
    shape = (n + 2,) if width is None else (n + 2, width)
    full = torch.full(shape, FILL, dtype=torch.uint8, device="cuda")
    return full, full[1:-1]


def images(adm, right, want):
    """The flag and hex buffers, guards included, after an add that admitted `adm`."""
    n = len(adm)
    ok = np.full(n + 2, FILL, np.uint8)
    ok[1:-1] = np.where(adm, right, SKIPPED)
    hx = np.full((n + 2, 64), FILL, np.uint8)
    hx[1:-1][adm] = want[adm]
    return ok, hx


def where_add(torch, q, tab, lo, hi, p, d_exp, d_ok, d_hex):
    """The where-add over chains lo..hi of a table with pattern p (held, flags, per, gates, gate):
    through HashQueue.add_check_where_ptrs, or for empty buffers (a tensor without elements has no
    address) through the C call. Returns (ticket, what has to stay alive until the add is done)."""
    _, addrs, views, _, _, _ = tab
    held, flags, per, gates, gate = p[:5]
    d_flags = torch.from_numpy(flags.copy()).cuda()
    d_gate = None if gates is None else torch.from_numpy(gates.copy()).cuda()
    if views is not None:
        tensors = [views[lo + i] if held[i] else None for i in range(hi - lo)]
        t, ok = q.add_check_where_ptrs(tensors, d_exp, d_flags, per, d_gate, gate, d_ok, d_hex)
        assert ok is d_ok
        return t, (d_flags, d_gate)
    from cess_amd import _lib
    ptrs = (ctypes.c_void_p * (hi - lo))(*[addrs[lo + i] if held[i] else None
                                           for i in range(hi - lo)])
    t = ctypes.c_uint64()
    rc = _lib.load().cec_hashq_add_check_where_ptrs(
        q._h, ptrs, hi - lo, 0, d_exp.data_ptr(), d_flags.data_ptr(), per,
        None if d_gate is None else d_gate.data_ptr(), gate, d_ok.data_ptr(),
        None if d_hex is None else d_hex.data_ptr(), ctypes.byref(t))
    assert rc == 0
    return t.value, (d_flags, d_gate)


@pytest.mark.parametrize("tick", TICKS)
@pytest.mark.parametrize("name", PATTERNS)
def test_admitted_chains_are_checked_and_the_rest_skipped(torch, cess, name, tick):
    p = PLANS[name]
    adm = p[5]
    assert int(adm.sum()) == ADMITTED[name]
    q = mkq(cess, tick, capacity=1024)
    for ln, off in [(ln, 0) for ln in LENS] + [(119, 1), (8192, 1)]:  # and at odd addresses
        tab = table(torch, ln, off)
        _, addrs, _, want, exp, right = tab
        assert all(a % 2 == off for a in addrs)
        d_exp = torch.from_numpy(exp.copy()).cuda()
        ok_full, d_ok = guarded(torch, N)
        hex_full, d_hex = guarded(torch, N, 64)
        t, keep = where_add(torch, q, tab, 0, N, p, d_exp, d_ok, d_hex)
        # the host cannot know what was admitted: N chains of the whole length
        assert q.live_chains == N and not q.done(t)
        assert q.blocks_left == cess.sha256_blocks(ln)
        q.finish()
        assert q.done(t) and q.live_chains == 0
        torch.cuda.synchronize()
        ok_img, hex_img = images(adm, right, want)
        assert np.array_equal(ok_full.cpu().numpy(), ok_img), (ln, off)
        assert np.array_equal(hex_full.cpu().numpy(), hex_img), (ln, off)
        assert np.array_equal(keep[0].cpu().numpy(), p[1]), (ln, off)  # the flags are only read
    q.close()


@pytest.mark.parametrize("tick", TICKS)
def test_flags_only_and_a_new_flag_tensor(torch, cess, tick):
    """d_hex None and d_ok None; expectations as a list, kept until the add is done."""
    tab = table(torch, 119)
    _, _, views, want, exp, right = tab
    held, flags, per, gates, gate, adm = plan("gated", 300)
    q = mkq(cess, tick, capacity=512)
    d_flags = torch.from_numpy(flags).cuda()
    d_gate = torch.from_numpy(gates).cuda()
    t, d_ok = q.add_check_where_ptrs(views[:300], [bytes(e) for e in exp[:300]], d_flags, per,
                                     d_gate, gate)
    assert d_ok.dtype == torch.uint8 and d_ok.shape == (300,) and d_ok.is_cuda
    assert [k[0] for k in q._kept] == [t]
    q.finish()
    assert q._kept == []
    torch.cuda.synchronize()
    assert 10 <= adm.sum() <= 50
    assert np.array_equal(d_ok.cpu().numpy(), np.where(adm, right[:300], SKIPPED))
    q.close()


@pytest.mark.parametrize("tick", TICKS)
def test_mixed_ring(torch, cess, tick):
    """A plain add of 40 chains, a where-add of 100 and a plain add of 30 in one ring, ticked
    five blocks at a time: parked chains share their 64-chain groups with running chains of the
    adds on both sides."""
    tab = table(torch, 8192)
    _, _, views, want, exp, right = tab
    p = plan("tenth", 100)
    adm = p[5]
    assert 3 <= adm.sum() <= 25
    q = mkq(cess, tick, capacity=256)
    hex_a, d_hex_a = guarded(torch, 40, 64)
    hex_c, d_hex_c = guarded(torch, 30, 64)
    ok_b, d_ok_b = guarded(torch, 100)
    hex_b, d_hex_b = guarded(torch, 100, 64)
    d_exp = torch.from_numpy(exp[100:200].copy()).cuda()
    t1 = q.add_ptrs(views[:40], d_hex_a)
    t2, keep = where_add(torch, q, tab, 100, 200, p, d_exp, d_ok_b, d_hex_b)
    t3 = q.add_ptrs(views[300:330], d_hex_c)
    assert (t1, t2, t3) == (1, 2, 3) and q.live_chains == 170
    ticks = 0
    while not all(q.status(t)[0] for t in (t1, t2, t3)):
        q.tick(5)
        ticks += 1
    assert ticks == -(-cess.sha256_blocks(8192) // 5) and q.live_chains == 0
    torch.cuda.synchronize()
    ok_img, hex_img = images(adm, right[100:200], want[100:200])
    assert np.array_equal(ok_b.cpu().numpy(), ok_img)
    assert np.array_equal(hex_b.cpu().numpy(), hex_img)
    full = np.ones(40, bool)
    assert np.array_equal(hex_a.cpu().numpy(), images(full, right[:40], want[:40])[1])
    assert np.array_equal(hex_c.cpu().numpy(), images(full[:30], right[:30], want[300:330])[1])
    q.close()


@pytest.mark.parametrize("name", ["tenth", "nulls"])
def test_ring_wrap(torch, cess, name):
    """Capacity 1024: 700 chains added and finished, then a where-add of 600 in slots 700..1299,
    across the mask; its parked chains count down from the far side of the wrap."""
    tab = table(torch, 119)
    _, _, views, want, exp, right = tab
    p = PLANS[name]
    q = mkq(cess, 0, capacity=1024)
    assert q.add_ptrs(views + views[:100]) == 1
    q.finish()
    d_exp = torch.from_numpy(exp.copy()).cuda()
    ok_full, d_ok = guarded(torch, N)
    hex_full, d_hex = guarded(torch, N, 64)
    t, keep = where_add(torch, q, tab, 0, N, p, d_exp, d_ok, d_hex)
    assert t == 2 and q.live_chains == N
    q.finish()
    torch.cuda.synchronize()
    ok_img, hex_img = images(p[5], right, want)
    assert np.array_equal(ok_full.cpu().numpy(), ok_img)
    assert np.array_equal(hex_full.cpu().numpy(), hex_img)
    q.close()


def test_errors_leave_the_ring_and_the_outputs_alone(torch, cess):
    from cess_amd import _lib
    lib = _lib.load()
    tab = table(torch, 119)
    _, addrs, views, want, exp, right = tab
    held, flags, per, gates, gate, adm = PLANS["gated"]
    d_exp = torch.from_numpy(exp.copy()).cuda()
    d_flags = torch.from_numpy(flags.copy()).cuda()
    d_gate = torch.from_numpy(gates.copy()).cuda()
    ok_full, d_ok = guarded(torch, N)
    hex_full, d_hex = guarded(torch, N, 64)
    q = mkq(cess, 0, capacity=512)
    t1 = q.add_ptrs(views[:10])
    ptrs = (ctypes.c_void_p * N)(*addrs)
    ticket = ctypes.c_uint64(77)
    E, FL, G, O, H = (d_exp.data_ptr(), d_flags.data_ptr(), d_gate.data_ptr(), d_ok.data_ptr(),
                      d_hex.data_ptr())

    def call(ptrs_=ptrs, n=100, e=E, fl=FL, per_=per, g=G, gate_=gate, o=O, h=H):
        return lib.cec_hashq_add_check_where_ptrs(q._h, ptrs_, n, 119, e, fl, per_, g, gate_, o, h,
                                                  ctypes.byref(ticket))

    refused = {
        "NULL array": lambda: call(ptrs_=None),
        "NULL d_expect": lambda: call(e=None),
        "NULL d_flags": lambda: call(fl=None),
        "NULL d_ok": lambda: call(o=None),
        "d_expect at an odd address": lambda: call(e=E + 1),
        "d_expect two bytes off": lambda: call(e=E + 2),
        "gate bytes with per == 0": lambda: call(per_=0),
        "gate 256": lambda: call(gate_=256),
        "gate -1": lambda: call(gate_=-1),
    }
    for what, f in refused.items():
        assert f() == EINVAL, what
        assert q.live_chains == 10 and not q.done(t1), what
    # a full ring: 10 live, 600 slots more do not fit in 512, whatever would be admitted
    assert call(n=N) == ENOMEM
    with pytest.raises(cess.CecError) as ei:
        q.add_check_where_ptrs(views, d_exp, d_flags, per, d_gate, gate, d_ok, d_hex)
    assert ei.value.code == ENOMEM
    assert q.live_chains == 10 and ticket.value == 77
    assert call(ptrs_=None, n=0, e=None, fl=None, o=None, h=None) == 0 and ticket.value == 0
    ticket.value = 77
    q.finish()
    torch.cuda.synchronize()
    assert bool((ok_full == FILL).all()) and bool((hex_full == FILL).all())
    # the refused adds took no ticket, and the arguments they were refused with were good ones
    assert call() == 0 and ticket.value == t1 + 1
    q.finish()
    torch.cuda.synchronize()
    ok_img, hex_img = images(adm[:100], right[:100], want[:100])
    assert np.array_equal(ok_full.cpu().numpy()[:101], ok_img[:101])
    assert np.array_equal(hex_full.cpu().numpy()[:101], hex_img[:101])
    assert bool((ok_full[101:] == FILL).all()) and bool((hex_full[101:] == FILL).all())
    q.close()


def test_confirm_flagged_on_the_gpu(torch, cess):
    """Every status against every ok vector of three, and a wide segment (n = 130: three ballots)
    whose only 0 or only 1 sits in the last lane's stride."""
    import itertools
    rows = [(st, ok) for st in (0, 1, 2, 3) for ok in itertools.product((0, 1, 2), repeat=3)]
    d_status = torch.tensor([st for st, _ in rows], dtype=torch.uint8, device="cuda")
    d_ok = torch.tensor([ok for _, ok in rows], dtype=torch.uint8, device="cuda")
    full, d_confirm = guarded(torch, len(rows))
    out = cess.confirm_flagged(d_status, d_ok, 3, d_confirm)
    assert out is d_confirm
    torch.cuda.synchronize()
    want = np.array([cess.confirm_rule(st, ok) for st, ok in rows], np.uint8)
    assert set(want) == {0, 1, 2}
    img = np.full(len(rows) + 2, FILL, np.uint8)
    img[1:-1] = want
    assert np.array_equal(full.cpu().numpy(), img)
    wide = np.full((5, 130), SKIPPED, np.uint8)
    wide[0, 129] = 0
    wide[1, 129] = 1
    wide[2, 128], wide[2, 3] = 0, 1
    wide[4, 64] = 0  # not rebuilt: NONE whatever its flags
    st = np.array([1, 1, 1, 1, 2], np.uint8)
    got = cess.confirm_flagged(torch.from_numpy(st).cuda(), torch.from_numpy(wide).cuda(), 130)
    torch.cuda.synchronize()
    assert got.cpu().numpy().tolist() == [2, 1, 2, 0, 0]
    assert got.cpu().numpy().tolist() == [cess.confirm_rule(int(s), w) for s, w in zip(st, wide)]
