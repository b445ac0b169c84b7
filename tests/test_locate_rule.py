"""The rule of cec_locate_ptrs on a CPU: cec_locate_rows against a numpy restatement of
  S_a = XOR_{i in H} u_i * i^a * v_i,   u_i = 1 / prod_{i' in H, i' != i} (i ^ i'),   0^0 = 1
written here over oracle.rs_oracle's field, rows . codeword = 0 for C-oracle codewords, and
cec_locate_host (the kernels' own functions, csrc/locate_rule.h, with loops for lanes) against the
same restatement: every held shard as the single bad one, the held-set edges, two bad shards. The
header's functions also run in a program of their own under sanitizers
(tests/native/locate_model.cpp)."""
import subprocess

import numpy as np
import pytest

from oracle import rs_oracle
from oracle.c_oracle import c_encode
from tests.conftest import ROOT

CLEAN, FOUND, AMBIGUOUS, UNCHECKED = 0, 1, 2, 3
SYN_MAX = 4
CODES = [(2, 2), (4, 2), (10, 4), (17, 3), (32, 32), (200, 56)]

mul, div, gexp = rs_oracle.gal_mul, rs_oracle.gal_div, rs_oracle.gal_exp


def np_rows(k, m, held, nsyn):
    """(r, rows [r][k+m]) from the formula."""
    H = [i for i in range(k + m) if held[i]]
    r = 0 if len(H) <= k else min(nsyn, len(H) - k)
    rows = np.zeros((r, k + m), np.uint8)
    for i in H:
        d = 1
        for i2 in H:
            if i2 != i:
                d = mul(d, i ^ i2)
        u = div(1, d)
        for a in range(r):
            rows[a, i] = mul(u, gexp(i, a))
    return r, rows


MUL_TABLE = np.array([[mul(a, b) for b in range(256)] for a in range(256)], np.uint8)


def np_locate(k, m, shards, nsyn):
    """(status, found) of one segment by the rule of the header, restated on numpy."""
    held = [s is not None for s in shards]
    H = [i for i in range(k + m) if held[i]]
    r, rows = np_rows(k, m, held, nsyn)
    if r == 0:
        return UNCHECKED, -1
    S = np.zeros((r, len(shards[H[0]])), np.uint8)
    for a in range(r):
        for i in H:
            S[a] ^= MUL_TABLE[rows[a, i]][shards[i]]
    if not S.any():
        return CLEAN, -1
    nz = np.flatnonzero(S[0])
    if r < 2 or nz.size == 0:
        return AMBIGUOUS, -1
    x = nz[0]
    cands = [j for j in H if mul(j, int(S[0, x])) == int(S[1, x])]
    if len(cands) != 1:
        return AMBIGUOUS, -1
    j = cands[0]
    for a in range(r - 1):
        if (S[a + 1] ^ MUL_TABLE[j][S[a]]).any():
            return AMBIGUOUS, -1
    return FOUND, j


def codeword(k, m, ln, rng, corc):
    """One C-oracle codeword, k + m shards of ln bytes."""
    data = [rng.integers(0, 256, ln, dtype=np.uint8) for _ in range(k)]
    return data + [np.ascontiguousarray(p) for p in c_encode(corc, k, m, data)]


def random_held(k, m, rng, h):
    held = np.zeros(k + m, np.uint8)
    held[rng.choice(k + m, h, replace=False)] = 1
    return held


@pytest.mark.parametrize("k,m", CODES)
def test_rows_match_the_formula(k, m):
    import cess_amd
    rng = np.random.default_rng(k * 1009 + m)
    for h in sorted({k + m, k + 2, k + 1, k, max(1, k - 1), min(k + m, k + 5)}):
        held = random_held(k, m, rng, h)
        for nsyn in (1, 2, 3, 4):
            r, rows = cess_amd.locate_rows(k, m, held, nsyn)
            wr, wrows = np_rows(k, m, held, nsyn)
            assert r == wr == (0 if h <= k else min(nsyn, h - k))
            assert np.array_equal(rows, wrows), (h, nsyn)
            if r:
                assert rows[:, held == 0].sum() == 0 and (rows[0, held == 1] != 0).all()


def test_rows_annihilate_golden_codewords(golden, corc):
    import cess_amd
    codes = sorted({(c["k"], c["m"]) for c in golden["cases"]})
    assert (4, 2) in codes and (32, 32) in codes
    for k, m in codes:
        rng = np.random.default_rng(k * 7919 + m)
        cw = codeword(k, m, 96, rng, corc)
        for trial in range(6):
            h = int(rng.integers(k, k + m + 1))
            held = random_held(k, m, rng, h)
            r, rows = cess_amd.locate_rows(k, m, held, SYN_MAX)
            for a in range(r):
                acc = np.zeros(96, np.uint8)
                for i in np.flatnonzero(held):
                    acc ^= MUL_TABLE[rows[a, i]][cw[i]]
                assert not acc.any(), (k, m, h, a)


def corrupt(shard, rng, whole=False):
    out = shard.copy()
    if whole:
        out ^= rng.integers(1, 256, out.size, dtype=np.uint8)
    else:
        out[int(rng.integers(0, out.size))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    return out


@pytest.mark.parametrize("k,m", CODES)
def test_every_held_shard_as_the_single_bad_one(k, m, corc):
    import cess_amd
    rng = np.random.default_rng(k * 31 + m)
    ln = 24
    cw = codeword(k, m, ln, rng, corc)
    for h in sorted({k + m, k + 2}):
        held = random_held(k, m, rng, h)
        if h == k + m:
            held[:] = 1
        base = [cw[i] if held[i] else None for i in range(k + m)]
        assert cess_amd.locate_host(k, m, base, SYN_MAX) == (CLEAN, -1)
        bad = list(np.flatnonzero(held))
        if k + m > 40:  # shard 0 (if held), every held parity shard, a sample of the rest
            bad = [j for j in bad if j == 0 or j >= k] + list(rng.choice(bad, 8, replace=False))
        for j in bad:
            for nsyn in ((2, SYN_MAX) if k + m <= 40 else (SYN_MAX,)):
                shards = list(base)
                shards[j] = corrupt(cw[j], rng, whole=bool(j & 1))
                got = cess_amd.locate_host(k, m, shards, nsyn)
                assert got == (FOUND, int(j)), (h, j, nsyn)
                assert got == np_locate(k, m, shards, nsyn)


@pytest.mark.parametrize("k,m", CODES + [(2, 1)])
def test_held_set_edges(k, m, corc):
    import cess_amd
    rng = np.random.default_rng(k * 53 + m)
    cw = codeword(k, m, 20, rng, corc)
    # h = k + 1: one check, a dirty segment is AMBIGUOUS whichever shard is bad
    held = random_held(k, m, rng, k + 1)
    base = [cw[i] if held[i] else None for i in range(k + m)]
    assert cess_amd.locate_host(k, m, base, SYN_MAX) == (CLEAN, -1)
    for j in np.flatnonzero(held)[:6]:
        shards = list(base)
        shards[j] = corrupt(cw[j], rng)
        assert cess_amd.locate_host(k, m, shards, SYN_MAX) == (AMBIGUOUS, -1)
    # h = k (and fewer): nothing is checked, whatever the bytes
    for h in (k, max(1, k - 1)):
        held = random_held(k, m, rng, h)
        shards = [corrupt(cw[i], rng, True) if held[i] else None for i in range(k + m)]
        assert cess_amd.locate_host(k, m, shards, SYN_MAX) == (UNCHECKED, -1)
    # nsyn = 1 detects only, with every shard held
    if m >= 2:
        shards = list(cw)
        shards[k] = corrupt(cw[k], rng)
        assert cess_amd.locate_host(k, m, shards, 1) == (AMBIGUOUS, -1)


@pytest.mark.parametrize("k,m", [(4, 3), (10, 4), (17, 3), (32, 32), (200, 56)])
def test_two_bad_shards_with_three_checks_are_never_found(k, m, corc):
    import cess_amd
    rng = np.random.default_rng(k * 97 + m)
    cw = codeword(k, m, 16, rng, corc)
    for trial in range(24 if k + m <= 64 else 6):
        h = int(rng.integers(k + 3, k + m + 1))
        held = random_held(k, m, rng, h)
        shards = [cw[i] if held[i] else None for i in range(k + m)]
        a, b = rng.choice(np.flatnonzero(held), 2, replace=False)
        same_offset = trial % 2 == 0  # the hard case: both errors at one byte offset
        x = int(rng.integers(0, 16))
        for j in (a, b):
            shards[j] = cw[j].copy()
            shards[j][x if same_offset else int(rng.integers(0, 16))] ^= np.uint8(
                rng.integers(1, 256))
        for nsyn in (3, 4):
            got = cess_amd.locate_host(k, m, shards, nsyn)
            assert got == (AMBIGUOUS, -1), (trial, h, a, b, nsyn)
            assert got == np_locate(k, m, shards, nsyn)


@pytest.mark.parametrize("k,m", [(2, 2), (4, 2), (10, 4)])
def test_two_bad_shards_with_two_checks_agree_with_the_restatement(k, m, corc):
    """With r = 2 two errors at one offset can imitate one (a wrong FOUND is inherent): only the
    agreement of the C rule with the restatement is asserted."""
    import cess_amd
    rng = np.random.default_rng(k * 211 + m)
    cw = codeword(k, m, 8, rng, corc)
    seen = set()
    for trial in range(200):
        shards = list(cw)
        a, b = rng.choice(k + m, 2, replace=False)
        x = int(rng.integers(0, 8))
        for j in (a, b):
            shards[j] = cw[j].copy()
            shards[j][x] ^= np.uint8(rng.integers(1, 256))
        got = cess_amd.locate_host(k, m, shards, 2)
        assert got == np_locate(k, m, shards, 2), (trial, a, b)
        seen.add(got[0])
    assert AMBIGUOUS in seen and CLEAN not in seen


# ---- the header's functions in a program of their own, under sanitizers --------------------------

def test_locate_model_under_sanitizers(tmp_path):
    exe = tmp_path / "locate_model"
    subprocess.run(["g++", "-std=c++20", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1", "-g",
                    f"{ROOT}/tests/native/locate_model.cpp", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert "locate_model ok" in out, out
