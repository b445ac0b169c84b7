"""cec_flag_status (CPU): the per-segment rule of cec_repair_flagged_ptrs, which the planner
kernels apply on the GPU, against a statement of the same rule in Python. Exhaustive over held x
flags for RS(2,1) and RS(4,2) with flag values from {0, 1, 0xFF}; 2,000 seeded random rows each
for RS(32,32) and RS(200,56). The index of the rebuilt shard (*lost) is checked on every row."""
import ctypes
import itertools

import numpy as np
import pytest

CLEAN, REBUILT, MANY, LOST = 0, 1, 2, 3


def rule(k, held, flags):
    """(status, lost): bad = held and flag == 0, good = held and flag != 0."""
    bad = [i for i, h in enumerate(held) if h and flags[i] == 0]
    good = sum(1 for i, h in enumerate(held) if h and flags[i] != 0)
    if not bad:
        return CLEAN, -1
    if good < k:
        return LOST, -1
    return (REBUILT, bad[0]) if len(bad) == 1 else (MANY, -1)


def c_status(k, m, held, flags):
    from cess_amd import _lib
    h = np.ascontiguousarray(held, dtype=np.uint8)
    f = np.ascontiguousarray(flags, dtype=np.uint8)
    st, lost = ctypes.c_int(-7), ctypes.c_int(-7)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    rc = _lib.load().cec_flag_status(k, m, h.ctypes.data_as(u8p), f.ctypes.data_as(u8p),
                                     ctypes.byref(st), ctypes.byref(lost))
    assert rc == 0
    return st.value, lost.value


@pytest.mark.parametrize("k,m", [(2, 1), (4, 2)])
def test_exhaustive(k, m):
    n = k + m
    seen = set()
    for held in itertools.product((0, 1), repeat=n):
        for flags in itertools.product((0, 1, 0xFF), repeat=n):
            want = rule(k, held, flags)
            assert c_status(k, m, held, flags) == want, (held, flags)
            seen.add(want[0])
    assert seen == ({CLEAN, REBUILT, LOST} if m == 1 else {CLEAN, REBUILT, MANY, LOST})


@pytest.mark.parametrize("k,m", [(32, 32), (200, 56)])
def test_random_rows(k, m):
    n = k + m
    rng = np.random.default_rng(k * 1009 + m)
    seen = set()
    for r in range(2000):
        # held counts around k and bad counts around 0..2, so every status comes up
        held = np.ones(n, np.uint8)
        held[rng.choice(n, size=int(rng.integers(0, m + 3)), replace=False)] = 0
        flags = rng.choice(np.array([1, 0xFF], np.uint8), size=n)
        flags[rng.choice(n, size=int(rng.integers(0, 4)), replace=False)] = 0
        if r % 5 == 0:
            flags = rng.choice(np.array([0, 1, 0xFF], np.uint8), size=n)
        want = rule(k, held, flags)
        assert c_status(k, m, held, flags) == want, r
        seen.add(want[0])
    assert seen == {CLEAN, REBUILT, MANY, LOST}


def test_python_form_and_refusals():
    import cess_amd
    from cess_amd import _lib
    assert cess_amd.flag_status(2, 1, [1, 1, 1], [1, 0, 0xFF]) == (REBUILT, 1)
    assert cess_amd.flag_status(2, 1, [1, 0, 1], [1, 0, 1]) == (CLEAN, -1)
    lib = _lib.load()
    st = ctypes.c_int(9)
    buf = (ctypes.c_uint8 * 3)(1, 1, 1)
    assert lib.cec_flag_status(2, 1, None, buf, ctypes.byref(st), None) == _lib.CEC_EINVAL
    assert lib.cec_flag_status(2, 1, buf, buf, None, None) == _lib.CEC_EINVAL
    assert lib.cec_flag_status(0, 1, buf, buf, ctypes.byref(st), None) == _lib.CEC_EINVAL
    assert lib.cec_flag_status(200, 57, buf, buf, ctypes.byref(st), None) == _lib.CEC_EINVAL
    assert st.value == 9
    # *lost is optional
    assert lib.cec_flag_status(2, 1, buf, buf, ctypes.byref(st), None) == 0 and st.value == CLEAN
