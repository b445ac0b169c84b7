"""The rule of cec_locate_multi_ptrs on a CPU: cec_locate_multi_host (the kernels' own functions,
csrc/locate_multi_rule.h, with loops for lanes) against a numpy restatement of the rule over
oracle.rs_oracle's field, on C-oracle codewords with one, two and three bad shards. With four
checks, one or two bad shards are FOUND with exactly that set, whatever their shape: replaced
whole, one byte each at different offsets in both index orders, at one offset, and the pair that
cancels S_0 everywhere. The header's functions also run in a program of their own under
sanitizers (tests/native/locate_multi_model.cpp)."""
import itertools
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_locate_rule import MUL_TABLE, codeword, div, mul, np_rows

CLEAN, FOUND, AMBIGUOUS, UNCHECKED = 0, 1, 2, 3
CODES = [(4, 4), (10, 4), (2, 4), (32, 32), (200, 56)]
LENGTHS = [1, 2, 7, 40]


def first_dirty(rows):
    """The lowest column at which any of the rows is non-zero."""
    acc = np.zeros_like(rows[0])
    for row in rows:
        acc |= row
    return int(np.flatnonzero(acc)[0])


def np_locate_multi(k, m, shards, nsyn, max_bad):
    """(status, found list) of one segment by the rule of the header, restated on numpy."""
    held = [s is not None for s in shards]
    H = [i for i in range(k + m) if held[i]]
    r, rows = np_rows(k, m, held, nsyn)
    if r == 0:
        return UNCHECKED, []
    S = np.zeros((r, len(shards[H[0]])), np.uint8)
    for a in range(r):
        for i in H:
            S[a] ^= MUL_TABLE[rows[a, i]][shards[i]]
    if not S.any():
        return CLEAN, []
    pair = max_bad >= 2 and r == 4
    s = [int(v) for v in S[:, first_dirty(S)]]
    J = None
    if r >= 2 and s[0]:
        c = [j for j in H if all(mul(j, s[a]) == s[a + 1] for a in range(r - 1))]
        if len(c) == 1:
            J = c
    if J is None and pair:
        det = mul(s[1], s[1]) ^ mul(s[0], s[2])
        if det:
            sg1 = div(mul(s[1], s[2]) ^ mul(s[0], s[3]), det)
            sg2 = div(mul(s[1], s[3]) ^ mul(s[2], s[2]), det)
            roots = [i for i in H if mul(i, i) ^ mul(sg1, i) ^ sg2 == 0]
            if len(roots) == 2:
                J = roots
    if J is None:
        return AMBIGUOUS, []
    if len(J) == 1:
        j = J[0]
        T = [S[a + 1] ^ MUL_TABLE[j][S[a]] for a in range(r - 1)]
        if not any(t.any() for t in T):
            return FOUND, [j]
        if not pair:
            return AMBIGUOUS, []
        t = [int(row[first_dirty(T)]) for row in T]
        if t[0] == 0:
            return AMBIGUOUS, []
        c = [i for i in H if i != j and mul(i, t[0]) == t[1] and mul(i, t[1]) == t[2]]
        if len(c) != 1:
            return AMBIGUOUS, []
        J = [j, c[0]]
    sg1, sg2 = J[0] ^ J[1], mul(J[0], J[1])
    for a in range(2):
        if (S[a + 2] ^ MUL_TABLE[sg1][S[a + 1]] ^ MUL_TABLE[sg2][S[a]]).any():
            return AMBIGUOUS, []
    return FOUND, sorted(J)


def held_sets(k, m, rng):
    """h = k + 4 exactly and all shards; where m > 4 lets a shard go, with and without shard 0."""
    n, out = k + m, []
    for with0 in ((True, False) if n > k + 4 else ()):
        rest = rng.choice(np.arange(1, n), k + 4 - (1 if with0 else 0), replace=False)
        held = np.zeros(n, bool)
        held[rest] = True
        held[0] = with0
        assert held.sum() == k + 4
        if not any(np.array_equal(held, h) for h in out):
            out.append(held)
    out.append(np.ones(n, bool))
    if m > 4:
        held = np.ones(n, bool)
        held[0] = False
        out.append(held)
    return out


SHAPES = ["whole", "low_first", "high_first", "same", "cancel"]


def pair_shape(cw, held, a, b, shape, rng, k, m):
    """The held view of codeword cw with shards a < b bad in the given shape, or None where the
    length has no two offsets."""
    ln = cw[0].size
    shards = [cw[i].copy() if held[i] else None for i in range(k + m)]
    if shape == "whole":
        for j in (a, b):
            shards[j] ^= rng.integers(1, 256, ln, dtype=np.uint8)
    elif shape in ("low_first", "high_first"):
        if ln < 2:
            return None
        x, y = sorted(int(v) for v in rng.choice(ln, 2, replace=False))
        first, second = (a, b) if shape == "low_first" else (b, a)
        shards[first][x] ^= np.uint8(rng.integers(1, 256))
        shards[second][y] ^= np.uint8(rng.integers(1, 256))
    elif shape == "same":
        x = int(rng.integers(0, ln))
        for j in (a, b):
            shards[j][x] ^= np.uint8(rng.integers(1, 256))
    else:  # e_b = (u_a / u_b) e_a at every offset: S_0 is zero everywhere
        u = np_rows(k, m, held, 4)[1][0]
        e = rng.integers(0, 256, ln, dtype=np.uint8)
        e[int(rng.integers(0, ln))] |= 1
        shards[a] ^= e
        shards[b] ^= MUL_TABLE[div(int(u[a]), int(u[b]))][e]
        s0 = MUL_TABLE[u[a]][e] ^ MUL_TABLE[u[b]][MUL_TABLE[div(int(u[a]), int(u[b]))][e]]
        assert not s0.any()
    return shards


def agree(k, m, shards, nsyn, max_bad):
    import cess_amd
    got = cess_amd.locate_multi_host(k, m, shards, nsyn, max_bad)
    assert got == np_locate_multi(k, m, shards, nsyn, max_bad)
    return got


def test_every_pair_of_rs4_4_in_every_shape(corc):
    k, m = 4, 4
    rng = np.random.default_rng(44)
    for ln in LENGTHS:
        cw = codeword(k, m, ln, rng, corc)
        held = np.ones(k + m, bool)
        assert agree(k, m, list(cw), 4, 2) == (CLEAN, [])
        for a, b in itertools.combinations(range(k + m), 2):
            for shape in SHAPES:
                shards = pair_shape(cw, held, a, b, shape, rng, k, m)
                if shards is None:
                    continue
                assert agree(k, m, shards, 4, 2) == (FOUND, [a, b]), (ln, a, b, shape)


@pytest.mark.parametrize("k,m", CODES)
def test_one_and_two_bad_shards_are_found_with_four_checks(k, m, corc):
    rng = np.random.default_rng(k * 1013 + m)
    small = k + m <= 64
    for ln in (LENGTHS if small else [1, 7]):
        cw = codeword(k, m, ln, rng, corc)
        for held in held_sets(k, m, rng):
            H = np.flatnonzero(held)
            base = [cw[i] if held[i] else None for i in range(k + m)]
            assert agree(k, m, base, 4, 2) == (CLEAN, [])
            pairs = [(H[0], H[-1]), (H[0], H[1])] + [
                tuple(sorted(rng.choice(H, 2, replace=False))) for _ in range(3 if small else 1)]
            for a, b in pairs:
                a, b = int(a), int(b)
                for shape in SHAPES:
                    shards = pair_shape(cw, held, a, b, shape, rng, k, m)
                    if shards is None:
                        continue
                    assert agree(k, m, shards, 4, 2) == (FOUND, [a, b]), (ln, a, b, shape)
            for j in {int(H[0]), int(H[-1]), int(rng.choice(H))}:  # a single bad shard
                for whole in (False, True):
                    shards = list(base)
                    shards[j] = cw[j].copy()
                    if whole:
                        shards[j] ^= rng.integers(1, 256, ln, dtype=np.uint8)
                    else:
                        shards[j][int(rng.integers(0, ln))] ^= np.uint8(rng.integers(1, 256))
                    assert agree(k, m, shards, 4, 2) == (FOUND, [j]), (ln, j, whole)


@pytest.mark.parametrize("k,m", CODES)
def test_three_bad_shards_agree_with_the_restatement(k, m, corc):
    """Three errors are past the rule's guarantee: only the agreement of the C rule with the
    restatement is asserted, at one offset (where they can imitate fewer) and replaced whole."""
    rng = np.random.default_rng(k * 2027 + m)
    for ln in (LENGTHS if k + m <= 64 else [7]):
        cw = codeword(k, m, ln, rng, corc)
        for held in held_sets(k, m, rng)[:3]:
            H = np.flatnonzero(held)
            for trial in range(6 if k + m <= 64 else 2):
                shards = [cw[i].copy() if held[i] else None for i in range(k + m)]
                x = int(rng.integers(0, ln))
                for j in rng.choice(H, 3, replace=False):
                    if trial % 2:
                        shards[j] ^= rng.integers(1, 256, ln, dtype=np.uint8)
                    else:
                        shards[j][x] ^= np.uint8(rng.integers(1, 256))
                st, found = agree(k, m, shards, 4, 2)
                assert st in (FOUND, AMBIGUOUS)


@pytest.mark.parametrize("k,m", [(4, 4), (10, 4), (2, 4), (32, 32), (200, 56), (4, 2), (4, 3)])
def test_two_bad_shards_with_fewer_checks_are_never_found(k, m, corc):
    rng = np.random.default_rng(k * 307 + m)
    for ln in ([2, 7, 40] if k + m <= 64 else [7]):
        cw = codeword(k, m, ln, rng, corc)
        for r, by_nsyn in ((3, False), (3, True), (2, False), (2, True)):
            if m < r:
                continue
            held = np.ones(k + m, bool)
            nsyn = 4
            if by_nsyn:  # all held, fewer checks asked for
                nsyn = r
            else:  # r by the held set: k + r shards
                held[:] = False
                held[rng.choice(k + m, k + r, replace=False)] = True
            H = np.flatnonzero(held)
            for trial in range(8 if k + m <= 64 else 2):
                a, b = sorted(int(v) for v in rng.choice(H, 2, replace=False))
                shape = ["whole", "low_first", "high_first", "cancel"][trial % 4]
                # "same" is left to the restatement below: two errors at one offset can imitate
                # one under two checks
                shards = pair_shape(cw, held, a, b, shape, rng, k, m)
                st, found = agree(k, m, shards, nsyn, 2)
                assert (st, found) == (AMBIGUOUS, []), (ln, r, by_nsyn, a, b, shape)
            shards = pair_shape(cw, held, int(H[0]), int(H[-1]), "same", rng, k, m)
            st, found = agree(k, m, shards, nsyn, 2)
            assert r == 2 or (st, found) == (AMBIGUOUS, [])
            assert len(found) <= 1


@pytest.mark.parametrize("k,m", [(4, 4), (10, 4), (4, 2), (2, 2), (32, 32)])
def test_max_bad_1_is_locate_host(k, m, corc):
    import cess_amd
    rng = np.random.default_rng(k * 409 + m)
    seen = set()
    for ln in LENGTHS:
        cw = codeword(k, m, ln, rng, corc)
        for trial in range(20):
            h = int(rng.integers(k, k + m + 1))
            held = np.zeros(k + m, bool)
            held[rng.choice(k + m, h, replace=False)] = True
            shards = [cw[i].copy() if held[i] else None for i in range(k + m)]
            for j in rng.choice(np.flatnonzero(held), min(h, trial % 4), replace=False):
                shards[j][int(rng.integers(0, ln))] ^= np.uint8(rng.integers(1, 256))
            for nsyn in (1, 2, 3, 4):
                st, found = cess_amd.locate_host(k, m, shards, nsyn)
                got = cess_amd.locate_multi_host(k, m, shards, nsyn, 1)
                assert got == (st, [found] if found >= 0 else []), (ln, trial, nsyn)
                seen.add(st)
    assert seen == {CLEAN, FOUND, AMBIGUOUS, UNCHECKED}


def test_single_rule_segments_under_max_bad_2_match_locate_host(corc):
    """A segment with fewer than four checks gets the single rule: with one bad shard, or none,
    the status and shard are cec_locate_host's."""
    import cess_amd
    rng = np.random.default_rng(77)
    for k, m in [(4, 2), (4, 3), (10, 4)]:
        cw = codeword(k, m, 7, rng, corc)
        for h in range(k, min(k + m, k + 3) + 1):
            held = np.zeros(k + m, bool)
            held[rng.choice(k + m, h, replace=False)] = True
            for nbad in (0, 1):
                shards = [cw[i].copy() if held[i] else None for i in range(k + m)]
                for j in rng.choice(np.flatnonzero(held), nbad, replace=False):
                    shards[j][int(rng.integers(0, 7))] ^= np.uint8(rng.integers(1, 256))
                st, found = cess_amd.locate_host(k, m, shards, 4)
                assert agree(k, m, shards, 4, 2) == (st, [found] if found >= 0 else [])


# ---- the header's functions in a program of their own, under sanitizers --------------------------

def test_locate_multi_model_under_sanitizers(tmp_path):
    exe = tmp_path / "locate_multi_model"
    subprocess.run(["g++", "-std=c++20", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1", "-g",
                    f"{ROOT}/tests/native/locate_multi_model.cpp", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert "locate_multi_model ok" in out, out
