"""cec_read_status and cec_read_solve (CPU): the rule, the decode rows and the copy set that the
planner kernels of cec_read_flagged_ptrs compute per segment, through the host functions built
from the kernels' own pieces (cess_amd/csrc/read_plan.h over flag_solve.h).

The rule is checked against its restatement in Python, exhaustively for RS(2,1) and RS(4,2). The
rows are checked against the numpy oracle (mat_invert of E[S], times E[j]) and against
cec_decode_rows with `present` = exactly the first k good shards. With every data shard held and
wanted and no parity bad, the read is the repair: statuses and rows equal cec_flag_solve's. The
row and chunk writers run in a program of their own (tests/native/read_plan.cpp) under
AddressSanitizer + UndefinedBehaviorSanitizer, every buffer at its documented size."""
import ctypes
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import test_flag_solve
from tests.test_flag_solve import c_solve as flag_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAN, REBUILT, MANY, LOST = 0, 1, 2, 3
MULTI_MAX = 4
U8P = ctypes.POINTER(ctypes.c_uint8)


@functools.lru_cache(maxsize=None)
def _rows_of(which, k, m, survivors, outs):
    fn = test_flag_solve.library_rows if which == "library" else test_flag_solve.oracle_rows
    return fn(k, m, list(survivors), list(outs))


def library_rows(k, m, survivors, outs):
    return _rows_of("library", k, m, tuple(survivors), tuple(outs))


def oracle_rows(k, m, survivors, outs):
    return _rows_of("oracle", k, m, tuple(survivors), tuple(outs))


def rule(k, held, flags, wanted, max_bad):
    """(status, [missing...], [copied...])"""
    good = [i for i, h in enumerate(held) if h and flags[i] != 0]
    miss = [j for j in range(k) if wanted[j] and j not in good]
    copy = [j for j in range(k) if wanted[j] and j in good]
    if not miss:
        return CLEAN, [], copy
    if len(good) < k:
        return LOST, [], []
    return (REBUILT, miss, copy) if len(miss) <= max_bad else (MANY, [], [])


def c_status(k, m, held, flags, wanted, max_bad):
    from cess_amd import _lib
    h = np.ascontiguousarray(held, dtype=np.uint8)
    f = np.ascontiguousarray(flags, dtype=np.uint8)
    w = np.ascontiguousarray(wanted, dtype=np.uint8)
    st, nm = ctypes.c_int(-7), ctypes.c_int(-7)
    miss = (ctypes.c_uint8 * MULTI_MAX)(0xEE, 0xEE, 0xEE, 0xEE)
    rc = _lib.load().cec_read_status(k, m, h.ctypes.data_as(U8P), f.ctypes.data_as(U8P),
                                     w.ctypes.data_as(U8P), max_bad, ctypes.byref(st),
                                     ctypes.byref(nm), miss)
    assert rc == 0
    assert all(x == 0xEE for x in miss[max(nm.value, 0):])  # nothing past the count is written
    return st.value, list(miss[:nm.value])


def c_solve(k, m, held, flags, wanted, max_bad):
    """cec_read_solve -> (status, out_idx, in_idx, rows [nout][k], copy_idx); the buffers have
    exactly the documented sizes and their unused tails must stay as they were."""
    from cess_amd import _lib
    h = np.ascontiguousarray(held, dtype=np.uint8)
    f = np.ascontiguousarray(flags, dtype=np.uint8)
    w = np.ascontiguousarray(wanted, dtype=np.uint8)
    st, no, nc = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    out = np.full(MULTI_MAX, 0xEE, np.uint8)
    inn = np.full(k, 0xEE, np.uint8)
    rows = np.full(MULTI_MAX * k, 0xEE, np.uint8)
    cidx = np.full(k, 0xEE, np.uint8)
    rc = _lib.load().cec_read_solve(k, m, h.ctypes.data_as(U8P), f.ctypes.data_as(U8P),
                                    w.ctypes.data_as(U8P), max_bad, ctypes.byref(st),
                                    ctypes.byref(no), out.ctypes.data_as(U8P),
                                    inn.ctypes.data_as(U8P), rows.ctypes.data_as(U8P),
                                    cidx.ctypes.data_as(U8P), ctypes.byref(nc))
    assert rc == 0
    e, c = no.value, nc.value
    assert (out[e:] == 0xEE).all() and (rows[e * k:] == 0xEE).all() and (cidx[c:] == 0xEE).all()
    if st.value != REBUILT:
        assert e == 0 and (inn == 0xEE).all()
    return (st.value, [int(x) for x in out[:e]], inn, rows[:e * k].reshape(e, k),
            [int(x) for x in cidx[:c]])


# ---- the rule ---------------------------------------------------------------------------------

def three_states(n, seed):
    """Every shard absent, good or bad: (held, flags) per combination; the flag of an absent shard
    is anything and a good flag is 1 or 0xFF, drawn per combination."""
    rng = np.random.default_rng(seed)
    for combo in itertools.product((0, 1, 2), repeat=n):
        held = [int(c != 0) for c in combo]
        flags = [int(rng.choice([0, 1, 0xFF])) if c == 0 else int(rng.choice([1, 0xFF])) if c == 1
                 else 0 for c in combo]
        yield held, flags


@pytest.mark.parametrize("k,m", [(2, 1), (4, 2)])
def test_rule_exhaustive(k, m):
    """Every held / good / bad state of every shard x every wanted mask x every bound."""
    n = k + m
    seen = set()
    for held, flags in three_states(n, 11 * k + m):
        for wanted in itertools.product((0, 1), repeat=k):
            for max_bad in range(1, MULTI_MAX + 1):
                st, miss, _ = rule(k, held, flags, wanted, max_bad)
                assert c_status(k, m, held, flags, wanted, max_bad) == (st, miss), \
                    (held, flags, wanted, max_bad)
                seen.add((st, len(miss)))
    if m == 2:
        assert seen == {(CLEAN, 0), (REBUILT, 1), (REBUILT, 2), (MANY, 0), (LOST, 0)}
    else:
        assert seen == {(CLEAN, 0), (REBUILT, 1), (LOST, 0)}


def random_row(k, m, rng, r):
    n = k + m
    held = np.ones(n, np.uint8)
    held[rng.choice(n, size=int(rng.integers(0, min(n, m + 2) + 1)), replace=False)] = 0
    flags = rng.choice(np.array([1, 0xFF], np.uint8), size=n)
    flags[rng.choice(n, size=int(rng.integers(0, min(n, 6) + 1)), replace=False)] = 0
    if r % 7 == 0:
        flags = rng.choice(np.array([0, 1, 0xFF], np.uint8), size=n)
    wanted = np.ones(k, np.uint8)
    if r % 3 == 1:
        wanted = rng.integers(0, 2, k).astype(np.uint8)
    elif r % 3 == 2:  # most of the missing shards not wanted
        wanted[rng.choice(k, size=int(rng.integers(0, k + 1)), replace=False)] = 0
    return held, flags, wanted


@pytest.mark.parametrize("k,m", [(10, 4), (32, 32), (200, 56)])
def test_rule_random_rows(k, m):
    rng = np.random.default_rng(k * 1013 + m + 5)
    seen = set()
    for r in range(1500):
        held, flags, wanted = random_row(k, m, rng, r)
        max_bad = 1 + r % MULTI_MAX
        st, miss, _ = rule(k, held, flags, wanted, max_bad)
        assert c_status(k, m, held, flags, wanted, max_bad) == (st, miss), r
        seen.add((st, len(miss)))
    assert {(CLEAN, 0), (MANY, 0), (LOST, 0)} <= seen
    assert {(REBUILT, e) for e in range(1, MULTI_MAX + 1)} <= seen


# ---- the rows and the copy set ------------------------------------------------------------------

def check_solved(k, m, held, flags, wanted, max_bad, oracle=True):
    st, outs, inn, rows, copy = c_solve(k, m, held, flags, wanted, max_bad)
    want_st, want_miss, want_copy = rule(k, held, flags, wanted, max_bad)
    assert (st, outs) == (want_st, want_miss)
    # the copy set: wanted and good, for CLEAN and REBUILT; nothing for LOST and MANY
    assert copy == want_copy
    if st in (LOST, MANY):
        assert copy == []
    if st != REBUILT:
        return st, 0
    good = [i for i in range(k + m) if held[i] and flags[i] != 0]
    assert list(inn) == good[:k]
    assert not set(outs) & set(good) and set(copy) <= set(good[:k])
    assert (rows != 0).all()
    assert np.array_equal(rows, library_rows(k, m, good[:k], outs))
    if oracle:
        assert np.array_equal(rows, oracle_rows(k, m, good[:k], outs))
    return st, len(outs)


@pytest.mark.parametrize("k,m", [(2, 1), (4, 2)])
def test_rows_exhaustive(k, m):
    n = k + m
    seen = set()
    for held, flags in three_states(n, 13 * k + m):
        for wanted in itertools.product((0, 1), repeat=k):
            for max_bad in (1, 2, MULTI_MAX):
                seen.add(check_solved(k, m, held, flags, wanted, max_bad))
    assert {(REBUILT, 1), (CLEAN, 0), (LOST, 0)} <= seen
    if m == 2:
        assert {(REBUILT, 2), (MANY, 0)} <= seen


@pytest.mark.parametrize("k,m,count,with_oracle", [(10, 4, 80, 80), (32, 32, 60, 60),
                                                   (200, 56, 12, 2)])
def test_rows_random(k, m, count, with_oracle):
    """A rebuild for certain: e wanted data shards absent or bad, enough good ones left."""
    n = k + m
    rng = np.random.default_rng(k * 7927 + m)
    buckets = set()
    for r in range(count):
        e = 1 + r % min(MULTI_MAX, m)
        held = np.ones(n, np.uint8)
        flags = rng.choice(np.array([1, 0xFF], np.uint8), size=n)
        wanted = np.ones(k, np.uint8)
        miss = rng.choice(k, size=e, replace=False)
        for j in miss:
            if rng.integers(0, 2):
                held[j] = 0
                flags[j] = rng.integers(0, 2)
            else:
                flags[j] = 0
        # up to m - e more shards gone, among the parity and the data nobody wants
        rest = [i for i in range(n) if i not in miss]
        for i in rng.choice(rest, size=int(rng.integers(0, m - e + 1)), replace=False):
            if i < k:
                wanted[i] = 0
            if rng.integers(0, 2):
                held[i] = 0
            else:
                flags[i] = 0
        st, nout = check_solved(k, m, held, flags, wanted, MULTI_MAX, oracle=r < with_oracle)
        assert (st, nout) == (REBUILT, e)
        buckets.add(nout)
    assert buckets == set(range(1, min(MULTI_MAX, m) + 1))


@pytest.mark.parametrize("k,m", [(2, 1), (4, 2), (10, 4), (32, 32)])
def test_equals_the_repair_when_all_data_is_held_and_wanted(k, m):
    """Every data shard held and wanted, no parity bad: missing == bad, so statuses, outputs,
    survivors and rows are cec_flag_solve's on the same input."""
    n = k + m
    rng = np.random.default_rng(k * 31 + m)
    seen = set()
    rows_list = []
    if n <= 6:
        for hp in itertools.product((0, 1), repeat=m):
            for fd in itertools.product((0, 1), repeat=k):
                rows_list.append((np.array([1] * k + list(hp), np.uint8),
                                  np.array(list(fd) + [1] * m, np.uint8)))
    else:
        for r in range(200):
            held = np.ones(n, np.uint8)
            held[k + rng.choice(m, size=int(rng.integers(0, m + 1)), replace=False)] = 0
            flags = rng.choice(np.array([1, 0xFF], np.uint8), size=n)
            flags[rng.choice(k, size=int(rng.integers(0, 6)), replace=False)] = 0
            rows_list.append((held, flags))
    wanted = np.ones(k, np.uint8)
    for held, flags in rows_list:
        for max_bad in (1, 2, MULTI_MAX):
            st, outs, inn, rows, _ = c_solve(k, m, held, flags, wanted, max_bad)
            fst, fouts, finn, frows = flag_solve(k, m, held, flags, max_bad)
            assert (st, outs) == (fst, fouts)
            assert np.array_equal(inn, finn) and np.array_equal(rows, frows)
            seen.add(st)
    assert {CLEAN, REBUILT, LOST} <= seen


# ---- the row and chunk writers, under sanitizers ------------------------------------------------

@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("read_plan") / "read_plan"
    subprocess.run(["g++", "-std=c++20", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1", "-g",
                    f"{ROOT}/tests/native/read_plan.cpp", "-o", str(exe)], check=True)
    return str(exe)


def writer_cases():
    cases = []
    for combo in itertools.product(((0, 0), (0, 1), (1, 0), (1, 0xFF)), repeat=3):  # RS(2,1): all
        for w in range(4):
            cases.append((2, 1, 1 + w % 2, [c[0] for c in combo], [c[1] for c in combo],
                          [w & 1, w >> 1]))
    for k, m, count in [(1, 3, 6), (4, 2, 16), (10, 4, 16), (32, 32, 10), (200, 56, 4),
                        (255, 1, 2)]:
        rng = np.random.default_rng(k * 104723 + m)
        for r in range(count):
            held, flags, wanted = random_row(k, m, rng, r + 1)
            if r % 2 == 0:  # a rebuild for certain
                e = 1 + (r // 2) % min(MULTI_MAX, m, k)
                held, flags = np.ones(k + m, np.uint8), np.ones(k + m, np.uint8)
                wanted = np.ones(k, np.uint8)
                miss = rng.choice(k, size=e, replace=False)
                held[miss[: e // 2]] = 0
                flags[miss[e // 2:]] = 0
            cases.append((k, m, 2 if r % 4 == 1 else MULTI_MAX, list(held), list(flags),
                          list(wanted)))
    return cases


FILL = 0xDEADBEEFDEADBEEF


def test_writers_under_sanitizers(plan_exe):
    cases = writer_cases()
    text = "".join("%d %d %d %s %s %s\n" % (k, m, mb, " ".join(map(str, held)),
                                            " ".join(map(str, flags)), " ".join(map(str, wanted)))
                   for k, m, mb, held, flags, wanted in cases)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([plan_exe], input=text, capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = iter(r.stdout.splitlines())

    def take(tag, base=10):
        w = next(lines).split()
        assert w[0] == tag, (w[0], tag)
        return [int(x, base) for x in w[1:]]
    rebuilt = set()
    for k, m, mb, held, flags, wanted in cases:
        st, e, nc = take("status")
        want_st, want_miss, want_copy = rule(k, held, flags, wanted, mb)
        assert (st, e, nc) == (want_st, len(want_miss), len(want_copy))
        assert take("cidx") == want_copy
        src = [0x1000 * (i + 1) if held[i] else 0 for i in range(k + m)]
        dst = [0x100000 + 0x1000 * j if wanted[j] else 0 for j in range(k)]
        # the copy rows: {src, dst} where a shard is copied, zero in both words elsewhere
        crow = take("crow", 16)
        assert crow == [w for j in range(k)
                        for w in ((src[j], dst[j]) if j in want_copy else (0, 0))]
        good = [i for i in range(k + m) if held[i] and flags[i] != 0]
        for b in range(1, MULTI_MAX + 1):
            row = take("b%d" % b, 16)
            if b == e:  # {chunk, the first k good shards, the destinations of the missing}
                assert row == [0xC0000] + [src[i] for i in good[:k]] + [dst[j] for j in want_miss]
            else:       # idle: zero in every word
                assert row == [0] * (k + 1 + b)
        if (k, m) == (2, 1):
            p21 = take("p21", 16)
            assert p21[0] == st and p21[5:] == crow
            if st == REBUILT:
                j = want_miss[0]
                assert p21[1:5] == [src[1 - j], src[2], dst[j], j]
            else:
                assert p21[1:5] == [0, 0, 0, 3]
        if not e:
            continue
        rebuilt.add((k, e))
        outs, inn = take("out"), take("in")
        rows = np.array([take("row") for _ in range(e)], dtype=np.uint8)
        hdr, hb = take("hdr"), take("hb")
        mask = np.array(take("mask", 16), dtype=np.uint64)
        assert next(lines) == "clean 1", (k, m, "an unwritten chunk word changed")
        st2, outs2, inn2, rows2, _ = c_solve(k, m, held, flags, wanted, mb)
        assert (outs, inn) == (outs2, list(inn2)) and np.array_equal(rows, rows2)
        assert hdr == [k, e, e, 0]
        col_or = np.bitwise_or.reduce(rows, axis=0)
        assert hb == [int(c).bit_length() - 1 for c in col_or]
        bits = (rows.T[:, None, :] >> np.arange(8, dtype=np.uint8)[None, :, None]) & 1
        want_mask = (bits.astype(np.uint64) * 0xFFFFFFFF).ravel()
        assert mask.size == k * 8 * e and np.array_equal(mask, want_mask)
    assert next(lines, None) is None
    assert {e for _, e in rebuilt} == {1, 2, 3, 4}
    assert {k for k, _ in rebuilt} >= {1, 2, 4, 10, 32, 200, 255}
