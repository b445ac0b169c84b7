"""cec_flag_status_multi and cec_flag_solve (CPU): the rule and the decode rows that the planner
kernel of cec_repair_flagged_multi_ptrs computes per segment, through the host functions built
from the kernel's own pieces (cess_amd/csrc/flag_solve.h).

The rule is checked against its restatement in Python. The rows are checked against two
independent sources: the numpy oracle (mat_invert of E[S], times E[j]) and cec_decode_rows called
with `present` = exactly the first k good shards and `required` = the bad ones, so that
cec_survivors has no choice. The chunk writer runs in a program of its own
(tests/native/flag_solve.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer and its hb and
mask words are checked bit by bit against the rows."""
import ctypes
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

from oracle import rs_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAN, REBUILT, MANY, LOST = 0, 1, 2, 3
MULTI_MAX = 4
U8P = ctypes.POINTER(ctypes.c_uint8)


def rule(k, held, flags, max_bad):
    """(status, [lost...]): bad = held and flag == 0, good = held and flag != 0."""
    bad = [i for i, h in enumerate(held) if h and flags[i] == 0]
    good = sum(1 for i, h in enumerate(held) if h and flags[i] != 0)
    if not bad:
        return CLEAN, []
    if good < k:
        return LOST, []
    return (REBUILT, bad) if len(bad) <= max_bad else (MANY, [])


def c_status_multi(k, m, held, flags, max_bad):
    from cess_amd import _lib
    h = np.ascontiguousarray(held, dtype=np.uint8)
    f = np.ascontiguousarray(flags, dtype=np.uint8)
    st, nl = ctypes.c_int(-7), ctypes.c_int(-7)
    lost = (ctypes.c_uint8 * MULTI_MAX)(0xEE, 0xEE, 0xEE, 0xEE)
    rc = _lib.load().cec_flag_status_multi(k, m, h.ctypes.data_as(U8P), f.ctypes.data_as(U8P),
                                           max_bad, ctypes.byref(st), ctypes.byref(nl), lost)
    assert rc == 0
    assert all(x == 0xEE for x in lost[max(nl.value, 0):])  # nothing past the count is written
    return st.value, list(lost[:nl.value])


def c_status_single(k, m, held, flags):
    from cess_amd import _lib
    h = np.ascontiguousarray(held, dtype=np.uint8)
    f = np.ascontiguousarray(flags, dtype=np.uint8)
    st, lost = ctypes.c_int(-7), ctypes.c_int(-7)
    assert _lib.load().cec_flag_status(k, m, h.ctypes.data_as(U8P), f.ctypes.data_as(U8P),
                                       ctypes.byref(st), ctypes.byref(lost)) == 0
    return st.value, ([lost.value] if st.value == REBUILT else [])


def c_solve(k, m, held, flags, max_bad):
    """cec_flag_solve -> (status, out_idx list, in_idx array, rows [nout][k]); the buffers have
    exactly the documented sizes and their unused tails must stay as they were."""
    from cess_amd import _lib
    h = np.ascontiguousarray(held, dtype=np.uint8)
    f = np.ascontiguousarray(flags, dtype=np.uint8)
    st, no = ctypes.c_int(-7), ctypes.c_int(-7)
    out = np.full(MULTI_MAX, 0xEE, np.uint8)
    inn = np.full(k, 0xEE, np.uint8)
    rows = np.full(MULTI_MAX * k, 0xEE, np.uint8)
    rc = _lib.load().cec_flag_solve(k, m, h.ctypes.data_as(U8P), f.ctypes.data_as(U8P), max_bad,
                                    ctypes.byref(st), ctypes.byref(no), out.ctypes.data_as(U8P),
                                    inn.ctypes.data_as(U8P), rows.ctypes.data_as(U8P))
    assert rc == 0
    e = no.value
    assert (out[e:] == 0xEE).all() and (rows[e * k:] == 0xEE).all()
    if st.value != REBUILT:
        assert e == 0 and (inn == 0xEE).all()
    return st.value, [int(x) for x in out[:e]], inn, rows[:e * k].reshape(e, k)


# ---- the rule ---------------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(2, 1), (4, 2)])
def test_rule_exhaustive(k, m):
    n = k + m
    seen = set()
    for held in itertools.product((0, 1), repeat=n):
        for flags in itertools.product((0, 1, 0xFF), repeat=n):
            for max_bad in range(1, MULTI_MAX + 1):
                want = rule(k, held, flags, max_bad)
                assert c_status_multi(k, m, held, flags, max_bad) == want, (held, flags, max_bad)
                seen.add((want[0], len(want[1])))
            assert c_status_multi(k, m, held, flags, 1) == c_status_single(k, m, held, flags)
    if m == 2:
        assert seen == {(CLEAN, 0), (REBUILT, 1), (REBUILT, 2), (MANY, 0), (LOST, 0)}


def random_row(k, m, rng, r):
    """held counts around k and bad counts 0..6, so every status and every bucket comes up."""
    n = k + m
    held = np.ones(n, np.uint8)
    held[rng.choice(n, size=int(rng.integers(0, min(n, m + 2) + 1)), replace=False)] = 0
    flags = rng.choice(np.array([1, 0xFF], np.uint8), size=n)
    flags[rng.choice(n, size=int(rng.integers(0, min(n, 6) + 1)), replace=False)] = 0
    if r % 7 == 0:
        flags = rng.choice(np.array([0, 1, 0xFF], np.uint8), size=n)
    return held, flags


@pytest.mark.parametrize("k,m", [(32, 32), (200, 56)])
def test_rule_random_rows(k, m):
    rng = np.random.default_rng(k * 1009 + m + 1)
    seen = set()
    for r in range(2000):
        held, flags = random_row(k, m, rng, r)
        max_bad = 1 + r % MULTI_MAX
        want = rule(k, held, flags, max_bad)
        assert c_status_multi(k, m, held, flags, max_bad) == want, r
        assert c_status_multi(k, m, held, flags, 1) == c_status_single(k, m, held, flags), r
        seen.add((want[0], len(want[1])))
    assert {(CLEAN, 0), (MANY, 0), (LOST, 0)} <= seen
    assert {(REBUILT, e) for e in range(1, MULTI_MAX + 1)} <= seen


def test_rule_refusals_and_python_form():
    import cess_amd
    from cess_amd import _lib
    lib = _lib.load()
    st, nl = ctypes.c_int(9), ctypes.c_int(9)
    buf = (ctypes.c_uint8 * 6)(1, 1, 1, 1, 1, 1)
    lost = (ctypes.c_uint8 * 4)()
    fn = lib.cec_flag_status_multi
    sp, np_ = ctypes.byref(st), ctypes.byref(nl)
    assert fn(4, 2, None, buf, 2, sp, np_, lost) == _lib.CEC_EINVAL
    assert fn(4, 2, buf, None, 2, sp, np_, lost) == _lib.CEC_EINVAL
    assert fn(4, 2, buf, buf, 2, None, np_, lost) == _lib.CEC_EINVAL
    assert fn(4, 2, buf, buf, 2, sp, None, lost) == _lib.CEC_EINVAL
    assert fn(4, 2, buf, buf, 0, sp, np_, lost) == _lib.CEC_EINVAL
    assert fn(4, 2, buf, buf, 5, sp, np_, lost) == _lib.CEC_EINVAL
    assert fn(0, 2, buf, buf, 2, sp, np_, lost) == _lib.CEC_EINVAL
    assert fn(4, 0, buf, buf, 2, sp, np_, lost) == _lib.CEC_EINVAL
    assert fn(200, 57, buf, buf, 2, sp, np_, lost) == _lib.CEC_EINVAL
    assert st.value == 9 and nl.value == 9
    assert fn(4, 2, buf, buf, 2, sp, np_, None) == 0 and st.value == CLEAN  # lost is optional
    sv = lib.cec_flag_solve
    assert sv(4, 2, buf, buf, 0, sp, np_, None, None, None) == _lib.CEC_EINVAL
    assert sv(4, 2, buf, buf, 5, sp, np_, None, None, None) == _lib.CEC_EINVAL
    assert sv(4, 2, None, buf, 2, sp, np_, None, None, None) == _lib.CEC_EINVAL
    assert sv(4, 2, buf, buf, 2, sp, None, None, None, None) == _lib.CEC_EINVAL
    assert sv(4, 2, buf, buf, 2, sp, np_, None, None, None) == 0  # the arrays are optional
    assert cess_amd.flag_status_multi(4, 2, [1] * 6, [1, 0, 1, 0xFF, 0, 1], 2) == (REBUILT, [1, 4])
    assert cess_amd.flag_status_multi(4, 2, [1] * 6, [1, 0, 1, 0xFF, 0, 1], 1) == (MANY, [])
    assert cess_amd.flag_status_multi(4, 2, [1, 0, 1, 1, 1, 1], [1, 0, 1, 1, 0, 0], 2) == (LOST, [])
    with pytest.raises(cess_amd.CecError):
        cess_amd.flag_status_multi(4, 2, [1] * 6, [1] * 6, 5)


# ---- the rows ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_matrix(k, m):
    return rs_oracle.build_matrix(k, k + m)


def oracle_rows(k, m, survivors, outs):
    E = oracle_matrix(k, m)
    inv = rs_oracle.mat_invert([E[i] for i in survivors])
    return np.array(rs_oracle.mat_mul([E[j] for j in outs], inv), dtype=np.uint8)


def library_rows(k, m, survivors, outs):
    """cec_decode_rows with nothing present but the survivors."""
    import cess_amd
    n = k + m
    present, required = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    present[survivors] = 1
    required[outs] = 1
    idx, rows = cess_amd.decode_rows(k, m, present, required)
    assert list(idx) == list(outs)
    return rows


def check_solved(k, m, held, flags, max_bad, oracle=True):
    """One row of cec_flag_solve against the rule and both sources. Returns (status, nout)."""
    st, outs, inn, rows = c_solve(k, m, held, flags, max_bad)
    want_st, want_lost = rule(k, held, flags, max_bad)
    assert (st, outs) == (want_st, want_lost)
    if st != REBUILT:
        return st, 0
    good = [i for i in range(k + m) if held[i] and flags[i] != 0]
    assert list(inn) == good[:k]                       # the first k good, ascending
    assert outs == sorted(outs) and not set(outs) & set(good)
    assert (rows != 0).all()                           # no zero column
    assert np.array_equal(rows, library_rows(k, m, good[:k], outs))
    if oracle:
        assert np.array_equal(rows, oracle_rows(k, m, good[:k], outs))
    return st, len(outs)


@pytest.mark.parametrize("k,m", [(4, 2), (3, 2)])
def test_rows_exhaustive(k, m):
    """Every held set and every flag pattern (flags of shards not held both ways)."""
    n = k + m
    seen = set()
    for held in itertools.product((0, 1), repeat=n):
        for flags in itertools.product((0, 0xFF), repeat=n):
            for max_bad in (1, 2, MULTI_MAX):
                seen.add(check_solved(k, m, held, flags, max_bad))
    assert {(REBUILT, 1), (REBUILT, 2), (CLEAN, 0), (LOST, 0), (MANY, 0)} <= seen


# per code: seeded rows, and how many of them are also checked against the oracle: all, but for
# the two codes where one Gauss-Jordan in pure Python takes seconds (every row of theirs is still
# checked against cec_decode_rows)
RANDOM_CODES = [(1, 3, 60, 60), (2, 2, 60, 60), (10, 4, 60, 60), (17, 3, 60, 60), (32, 32, 60, 60),
                (200, 56, 12, 2), (255, 1, 6, 1), (1, 255, 40, 40)]


@pytest.mark.parametrize("k,m,count,with_oracle", RANDOM_CODES)
def test_rows_random(k, m, count, with_oracle):
    n = k + m
    rng = np.random.default_rng(k * 7919 + m)
    buckets, done = set(), 0
    for r in range(count):
        held = np.ones(n, np.uint8)
        e = 1 + r % min(MULTI_MAX, m)
        spare = m - e
        held[rng.choice(n, size=int(rng.integers(0, spare + 1)), replace=False)] = 0
        flags = rng.choice(np.array([1, 0xFF], np.uint8), size=n)
        flags[rng.choice(np.nonzero(held)[0], size=e, replace=False)] = 0
        flags[held == 0] = rng.choice(np.array([0, 1], np.uint8), size=int((held == 0).sum()))
        st, nout = check_solved(k, m, held, flags, MULTI_MAX, oracle=done < with_oracle)
        assert (st, nout) == (REBUILT, e)
        buckets.add(nout)
        done += 1
    assert buckets == set(range(1, min(MULTI_MAX, m) + 1))


def test_rows_parity_heavy_3232():
    """RS(32,32) with 2 data shards and all 32 parity held, 2 of them bad: the survivors are the
    30 or 32 good ones that remain, nearly all parity."""
    k, m, n = 32, 32, 64
    rng = np.random.default_rng(3232)
    for r in range(6):
        held = np.zeros(n, np.uint8)
        held[k:] = 1
        held[rng.choice(k, size=2, replace=False)] = 1
        flags = np.ones(n, np.uint8)
        flags[rng.choice(np.nonzero(held)[0], size=2, replace=False)] = 0
        st, nout = check_solved(k, m, held, flags, 2)
        assert (st, nout) == (REBUILT, 2)


# ---- the chunk writer, under sanitizers ---------------------------------------------------------

@pytest.fixture(scope="module")
def solve_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("flag_solve") / "flag_solve"
    subprocess.run(["g++", "-std=c++20", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1", "-g",
                    f"{ROOT}/tests/native/flag_solve.cpp", "-o", str(exe)], check=True)
    return str(exe)


def chunk_cases():
    """(k, m, max_bad, held, flags): every bucket of the small codes, the wide ones, k and n past
    64, and rows that are not rebuilt."""
    cases = []
    for k, m, count in [(1, 3, 8), (2, 2, 8), (3, 2, 8), (4, 2, 12), (10, 4, 12), (17, 3, 8),
                        (32, 32, 8), (200, 56, 3), (255, 1, 2), (1, 255, 4)]:
        rng = np.random.default_rng(k * 104729 + m)
        for r in range(count):
            held, flags = random_row(k, m, rng, r + 1)
            if r % 3 == 0:  # a rebuild for certain
                e = 1 + (r // 3) % min(MULTI_MAX, m)
                held = np.ones(k + m, np.uint8)
                flags = np.ones(k + m, np.uint8)
                flags[rng.choice(k + m, size=e, replace=False)] = 0
            cases.append((k, m, MULTI_MAX if r % 4 else 2, held, flags))
    return cases


def test_chunk_writer_under_sanitizers(solve_exe):
    cases = chunk_cases()
    text = "".join("%d %d %d %s %s\n" % (k, m, mb, " ".join(map(str, held)),
                                         " ".join(map(str, flags)))
                   for k, m, mb, held, flags in cases)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([solve_exe], input=text, capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = iter(r.stdout.splitlines())
    rebuilt = set()
    for k, m, mb, held, flags in cases:
        w = next(lines).split()
        assert w[0] == "status"
        st, e = int(w[1]), int(w[2])
        want_st, want_lost = rule(k, held, flags, mb)
        assert (st, e) == (want_st, len(want_lost))
        if not e:
            continue
        rebuilt.add((k, e))

        def take(tag):
            w = next(lines).split()
            assert w[0] == tag
            return w[1:]
        outs = [int(x) for x in take("out")]
        inn = [int(x) for x in take("in")]
        rows = np.array([[int(x) for x in take("row")] for _ in range(e)], dtype=np.uint8)
        hdr = [int(x) for x in take("hdr")]
        hb = [int(x) for x in take("hb")]
        mask = np.array([int(x, 16) for x in take("mask")], dtype=np.uint64)
        assert next(lines) == "clean 1", (k, m, "a guard or an unwritten chunk word changed")
        # the same rows as the library's host function, so as both sources above
        st2, outs2, inn2, rows2 = c_solve(k, m, held, flags, mb)
        assert (outs, inn) == (outs2, list(inn2)) and np.array_equal(rows, rows2)
        assert hdr == [k, e, e, 0]
        # hb[t]: highest set bit over column t; masks[t][b][o]: all ones where bit b of rows[o][t]
        col_or = np.bitwise_or.reduce(rows, axis=0)
        assert hb == [int(c).bit_length() - 1 for c in col_or]
        bits = (rows.T[:, None, :] >> np.arange(8, dtype=np.uint8)[None, :, None]) & 1  # [t][b][o]
        want_mask = (bits.astype(np.uint64) * 0xFFFFFFFF).ravel()
        assert mask.size == k * 8 * e and np.array_equal(mask, want_mask)
    assert next(lines, None) is None
    assert {e for _, e in rebuilt} == {1, 2, 3, 4}
    assert {k for k, _ in rebuilt} >= {1, 2, 3, 4, 10, 17, 32, 200, 255}
