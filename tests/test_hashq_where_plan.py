"""Where cec_hashq_add_check_where_ptrs puts its chains, and what cec_confirm_flagged makes of
their flags (CPU): the arithmetic of the admit kernel (cess_amd/csrc/hashq_where.h) through
cec_hashq_where_plan and through a program of its own (tests/native/hashq_where.cpp) under
AddressSanitizer + UndefinedBehaviorSanitizer, both against the restatement below. The sizes
cross the kernel's wave (64) and launch (256) boundaries; 600 takes three launches."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8P = ctypes.POINTER(ctypes.c_uint8)
REBUILT = 1
NONE, PROVEN, REFUTED = 0, 1, 2
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 600]
PATTERNS = ["none", "all", "every64", "last", "tenth", "nulls"]


def model(held, flags, per, gates, gate):
    """(pos, nsel): admitted chains count up from 0 in index order, the others down from n - 1."""
    n = len(held)
    pos, a, b = [0] * n, 0, 0
    for i in range(n):
        if held[i] and flags[i] == 0 and (gates is None or gates[i // per] == gate):
            pos[i], a = a, a + 1
        else:
            pos[i], b = n - 1 - b, b + 1
    return pos, a


def pattern(name, n):
    """(held, flags): flag 0 = wanted. `nulls`: a third of the slots hold nothing, wanted or not."""
    rng = np.random.default_rng(n * 7 + len(name))
    held = np.ones(n, np.uint8)
    want = np.zeros(n, bool)
    if name == "all":
        want[:] = True
    elif name == "every64":
        want[::64] = True
    elif name == "last" and n:
        want[-1] = True
    elif name == "tenth":
        want = rng.random(n) < 0.1
    elif name == "nulls":
        want = rng.random(n) < 0.5
        held = (rng.random(n) >= 1 / 3).astype(np.uint8) * rng.integers(1, 256, n, dtype=np.uint8)
    flags = np.where(want, 0, rng.integers(1, 256, n)).astype(np.uint8)
    return held, flags


def cases():
    for n, name in itertools.product(SIZES, PATTERNS):
        held, flags = pattern(name, n)
        yield held, flags, 1, None, 0
        for per in (1, 3, 6):
            # gate bytes of every status value, and one that is no status
            gates = (np.arange((n + per - 1) // per) * 3 % 5).astype(np.uint8)
            yield held, flags, per, gates, REBUILT
    held, flags = pattern("tenth", 600)
    yield held, flags, 6, np.full(100, 255, np.uint8), 255
    yield held, flags, 1000, np.zeros(1, np.uint8), 0


def check(pos, nsel, held, flags, per, gates, gate):
    n = len(held)
    want_pos, want_nsel = model(held, flags, per, gates, gate)
    assert nsel == want_nsel
    assert list(pos) == want_pos
    sel = [i for i in range(n) if held[i] and flags[i] == 0 and
           (gates is None or gates[i // per] == gate)]
    chosen = set(sel)
    rest = [i for i in range(n) if i not in chosen]
    assert sorted(pos) == list(range(n))  # a permutation of [0, n)
    assert [pos[i] for i in sel] == list(range(nsel))  # [0, nsel) in index order
    assert [pos[i] for i in rest] == list(range(n - 1, nsel - 1, -1))  # [nsel, n) descending


def test_cases_cover_what_they_claim():
    seen = set()
    for held, flags, per, gates, gate in cases():
        nsel = model(held, flags, per, gates, gate)[1]
        seen.add((len(held), nsel == 0, nsel == len(held)))
        if gates is not None and len(gates) >= 5 and gate == REBUILT:
            assert set(gates) == {0, 1, 2, 3, 4}
    assert (600, True, False) in seen and (600, False, True) in seen and \
        (600, False, False) in seen
    held, flags = pattern("every64", 600)
    assert model(held, flags, 1, None, 0)[1] == 10
    held, flags = pattern("last", 257)
    assert model(held, flags, 1, None, 0) == (list(range(256, 0, -1)) + [0], 1)
    held, flags = pattern("nulls", 600)
    assert 100 < (held == 0).sum() < 300 and ((held == 0) & (flags == 0)).any()


def test_library_plan():
    from cess_amd import _lib
    lib = _lib.load()
    for held, flags, per, gates, gate in cases():
        n = len(held)
        pos = np.full(n + 1, 0xEEEEEEEE, np.uint32)
        nsel = ctypes.c_size_t(12345)
        rc = lib.cec_hashq_where_plan(
            held.ctypes.data_as(U8P), flags.ctypes.data_as(U8P), n, per,
            None if gates is None else gates.ctypes.data_as(U8P), gate,
            pos.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(nsel))
        assert rc == 0
        assert pos[n] == 0xEEEEEEEE  # nothing past n is written
        check(pos[:n].tolist(), nsel.value, held, flags, per, gates, gate)


def test_library_plan_refuses():
    from cess_amd import _lib
    lib = _lib.load()
    b = np.zeros(4, np.uint8)
    p = b.ctypes.data_as(U8P)
    pos = np.full(4, 7, np.uint32)
    pp = pos.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    assert lib.cec_hashq_where_plan(None, p, 4, 1, None, 0, pp, None) == _lib.CEC_EINVAL
    assert lib.cec_hashq_where_plan(p, None, 4, 1, None, 0, pp, None) == _lib.CEC_EINVAL
    assert lib.cec_hashq_where_plan(p, p, 4, 1, None, 0, None, None) == _lib.CEC_EINVAL
    assert lib.cec_hashq_where_plan(p, p, 4, 0, p, 0, pp, None) == _lib.CEC_EINVAL
    assert lib.cec_hashq_where_plan(p, p, 4, 1, None, 256, pp, None) == _lib.CEC_EINVAL
    assert lib.cec_hashq_where_plan(p, p, 4, 1, None, -1, pp, None) == _lib.CEC_EINVAL
    assert (pos == 7).all()
    assert lib.cec_hashq_where_plan(None, None, 0, 0, None, 0, None, None) == 0
    assert lib.cec_hashq_where_plan(p, p, 4, 0, None, 0, pp, None) == 0  # per unused without gate


@pytest.fixture(scope="module")
def where_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("hashq_where") / "hashq_where"
    subprocess.run(["g++", "-std=c++20", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1", "-g",
                    f"{ROOT}/tests/native/hashq_where.cpp", "-o", str(exe)], check=True)
    return str(exe)


def run_native(exe, text):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    return r.stdout.splitlines()


def test_native_plan_under_sanitizers(where_exe):
    todo = list(cases())
    text = "".join(
        " ".join(map(str, [len(held), per, gate, int(gates is not None), *held, *flags,
                           *([] if gates is None else gates)])) + "\n"
        for held, flags, per, gates, gate in todo)
    out = run_native(where_exe, text)
    assert len(out) == len(todo)
    for line, (held, flags, per, gates, gate) in zip(out, todo):
        w = [int(x) for x in line.split()]
        assert len(w) == 1 + len(held)
        check(w[1:], w[0], held, flags, per, gates, gate)


def rule(status, ok):
    if status != REBUILT:
        return NONE
    return REFUTED if 0 in ok else PROVEN if 1 in ok else NONE


def test_confirm_rule_every_status_and_ok_vector(where_exe):
    """n = 3: the four statuses and a value that is none, every vector over {0, 1, 2, 3}."""
    from cess_amd import _lib
    import cess_amd
    lib = _lib.load()
    todo = [(st, ok) for st in (0, 1, 2, 3, 4) for ok in itertools.product((0, 1, 2, 3), repeat=3)]
    native = run_native(where_exe, "".join("rule %d %d %d %d\n" % (st, *ok) for st, ok in todo))
    for (st, ok), line in zip(todo, native):
        buf = (ctypes.c_uint8 * 3)(*ok)
        out = ctypes.c_int(-7)
        assert lib.cec_confirm_rule(3, st, buf, ctypes.byref(out)) == 0
        assert out.value == rule(st, ok) == int(line), (st, ok)
        assert cess_amd.confirm_rule(st, ok) == rule(st, ok)
    out = ctypes.c_int(-7)
    assert lib.cec_confirm_rule(0, REBUILT, None, ctypes.byref(out)) == 0 and out.value == NONE
    assert lib.cec_confirm_rule(3, REBUILT, None, ctypes.byref(out)) == _lib.CEC_EINVAL
    assert lib.cec_confirm_rule(-1, REBUILT, None, ctypes.byref(out)) == _lib.CEC_EINVAL
    assert lib.cec_confirm_rule(0, REBUILT, None, None) == _lib.CEC_EINVAL
    assert (cess_amd.CEC_CONFIRM_NONE, cess_amd.CEC_CONFIRM_PROVEN,
            cess_amd.CEC_CONFIRM_REFUTED) == (NONE, PROVEN, REFUTED)
