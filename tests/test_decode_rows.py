"""cec_decode_rows (host only, CPU): the decode rows of a required subset of the lost shards,
against the oracle. For random patterns of several codes the required shards must equal
rows x survivors over GF(2^8), computed in numpy (the Python oracle's multiplication table) from
oracle codewords; the survivors are those cec_survivors names, in its order."""
import ctypes

import numpy as np
import pytest

from oracle.c_oracle import c_encode

LEN = 257  # bytes per shard of the codewords (odd: no alignment to lean on)
CODES = [(2, 1), (4, 2), (10, 4), (32, 32), (128, 128)]


def _codeword(corc, k, m, rng):
    data = [rng.integers(0, 256, LEN, dtype=np.uint8) for _ in range(k)]
    return data + c_encode(corc, k, m, data)


def _survivors(k, m, present):
    from cess_amd import _lib
    flags = np.asarray(present, dtype=np.uint8)
    out = np.zeros(k, dtype=np.uint8)
    rc = _lib.load().cec_survivors(k, m, flags.ctypes.data, out.ctypes.data)
    assert rc == 0
    return [int(i) for i in out]


def _apply(orc, rows, inputs):
    """rows x inputs over GF(2^8) in numpy."""
    outs = []
    for row in rows:
        acc = np.zeros(LEN, dtype=np.uint8)
        for c, src in zip(row, inputs):
            if c:
                acc ^= orc.MUL[int(c)][src]
        outs.append(acc)
    return outs


def _patterns(k, m, rng, count):
    """Random erasure patterns with 1..m lost shards and a random required subset of them."""
    n = k + m
    for t in range(count):
        ne = int(rng.integers(1, m + 1))
        lost = sorted(rng.choice(n, size=ne, replace=False).tolist())
        nreq = int(rng.integers(1, ne + 1)) if t else 1  # the restoral case first: one fragment
        req = sorted(rng.choice(lost, size=nreq, replace=False).tolist())
        present = np.ones(n, dtype=np.uint8)
        present[lost] = 0
        yield present, lost, req


@pytest.mark.parametrize("k,m", CODES)
def test_rows_rebuild_the_required_shards(corc, orc, k, m):
    import cess_amd
    rng = np.random.default_rng(1000 * k + m)
    full = _codeword(corc, k, m, rng)
    n = k + m
    for present, lost, req in _patterns(k, m, rng, 8 if k < 100 else 3):
        required = np.zeros(n, dtype=np.uint8)
        required[req] = 1
        idx, rows = cess_amd.decode_rows(k, m, present, required)
        assert idx.tolist() == req, (present.tolist(), req)  # ascending, exactly the asked ones
        assert rows.shape == (len(req), k)
        surv = _survivors(k, m, present)
        got = _apply(orc, rows, [full[i] for i in surv])
        for i, g in zip(idx, got):
            assert np.array_equal(g, full[int(i)]), (k, m, present.tolist(), int(i))


@pytest.mark.parametrize("k,m", [(2, 1), (4, 2), (10, 4), (32, 32)])
def test_required_flags_on_present_shards_are_ignored(corc, orc, k, m):
    import cess_amd
    rng = np.random.default_rng(77 + k)
    n = k + m
    for present, lost, req in _patterns(k, m, rng, 4):
        required = np.zeros(n, dtype=np.uint8)
        required[req] = 1
        want = cess_amd.decode_rows(k, m, present, required)
        noisy = required.copy()
        noisy[present != 0] = rng.integers(0, 2, int((present != 0).sum()), dtype=np.uint8)
        noisy[int(np.flatnonzero(present)[0])] = 1
        got = cess_amd.decode_rows(k, m, present, noisy)
        assert got[0].tolist() == want[0].tolist()
        assert np.array_equal(got[1], want[1])


@pytest.mark.parametrize("k,m", CODES)
def test_too_few_at_k_minus_one_present(k, m):
    import cess_amd
    from cess_amd import _lib
    n = k + m
    present = np.zeros(n, dtype=np.uint8)
    present[np.random.default_rng(k).choice(n, size=k - 1, replace=False)] = 1
    with pytest.raises(cess_amd.ErrTooFewShards) as ei:
        cess_amd.decode_rows(k, m, present, np.ones(n, dtype=np.uint8))
    assert ei.value.code == _lib.CEC_ETOOFEW
    present[int(np.flatnonzero(present == 0)[0])] = 1  # k present: fine
    idx, rows = cess_amd.decode_rows(k, m, present, np.ones(n, dtype=np.uint8))
    assert len(idx) == m and rows.shape == (m, k)


@pytest.mark.parametrize("k,m", [(2, 1), (4, 2), (10, 4)])
def test_everything_required_gives_the_full_rebuild_rows(orc, k, m):
    """With every lost shard required the rows are those of the full rebuild: the Python oracle's
    decode plan (first k present shards, which is cec_survivors' choice for these codes)."""
    import cess_amd
    rs = orc.ReedSolomon(k, m)
    rng = np.random.default_rng(5 * k + m)
    n = k + m
    for present, lost, _ in _patterns(k, m, rng, 6):
        surv, outs, want = rs.decode_plan([bool(p) for p in present])
        assert surv == _survivors(k, m, present)
        idx, rows = cess_amd.decode_rows(k, m, present, np.ones(n, dtype=np.uint8))
        assert idx.tolist() == outs == lost
        assert rows.tolist() == [list(r) for r in want]


def test_full_rows_wide_code_match_any_subset(corc, orc):
    """RS(32,32): the rows of a subset are the same rows the full request returns for those
    shards (the survivors do not depend on what is required)."""
    import cess_amd
    k = m = 32
    rng = np.random.default_rng(3232)
    for present, lost, req in _patterns(k, m, rng, 6):
        allreq = np.ones(k + m, dtype=np.uint8)
        idx_all, rows_all = cess_amd.decode_rows(k, m, present, allreq)
        assert idx_all.tolist() == lost
        required = np.zeros(k + m, dtype=np.uint8)
        required[req] = 1
        idx, rows = cess_amd.decode_rows(k, m, present, required)
        pos = [lost.index(i) for i in req]
        assert np.array_equal(rows, rows_all[pos])
        assert idx.tolist() == req


def test_bad_arguments():
    from cess_amd import _lib
    lib = _lib.load()
    u8 = ctypes.POINTER(ctypes.c_uint8)
    buf = (ctypes.c_uint8 * 256)()
    nreq = ctypes.c_int(0)
    assert lib.cec_decode_rows(0, 1, buf, buf, buf, buf, ctypes.byref(nreq)) == _lib.CEC_EINVAL
    assert lib.cec_decode_rows(200, 100, buf, buf, buf, buf,
                               ctypes.byref(nreq)) == _lib.CEC_EINVAL
    assert lib.cec_decode_rows(2, 1, ctypes.cast(None, u8), buf, buf, buf,
                               ctypes.byref(nreq)) == _lib.CEC_EINVAL
