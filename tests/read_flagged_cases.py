"""The segments of tests/test_gpu_read_flagged.py, generated without a GPU so that
tests/test_read_flagged_cases.py can say on a CPU which classes each of them covers.

A case is (held, bad, wanted): held [nseg][n] and bad [nseg][n] (a held shard whose flag is 0) as
in tests/test_gpu_repair_flagged.py's Case, wanted [nseg][k] the data shards to deliver. A shard is
absent (not held), good (held, flag set) or bad (held, flag 0)."""
import itertools

import numpy as np

CLEAN, REBUILT, MANY, LOST = 0, 1, 2, 3
ABSENT, GOOD, BAD = 0, 1, 2


def from_states(states, wanted):
    states = np.asarray(states)
    return states != ABSENT, states == BAD, np.asarray(wanted, dtype=bool)


def rs21_all():
    """RS(2,1): all 27 shard states x all 4 wanted masks, 108 segments."""
    rows = [(st, (w & 1, w >> 1)) for st in itertools.product((ABSENT, GOOD, BAD), repeat=3)
            for w in range(4)]
    return from_states([r[0] for r in rows], [r[1] for r in rows])


def rs42_all(random_wanted=False):
    """RS(4,2): all 3^6 shard states; everything wanted, or a seeded random mask."""
    states = list(itertools.product((ABSENT, GOOD, BAD), repeat=6))
    wanted = np.ones((len(states), 4), dtype=bool)
    if random_wanted:
        wanted = np.random.default_rng(4242).integers(0, 2, wanted.shape).astype(bool)
    return from_states(states, wanted)


def rs104_random(nseg=64, seed=1004):
    """RS(10,4): seeded segments with 0..6 shards absent or bad and wanted masks of every weight;
    the first rows are fixed so that every bucket and every status is there under max_bad 4."""
    k, n = 10, 14
    rng = np.random.default_rng(seed)
    states = np.full((nseg, n), GOOD)
    wanted = np.ones((nseg, k), dtype=bool)
    fixed = [([], []), ([0], []), ([3], [9]), ([1, 2], [7]), ([0, 4], [5, 9]),  # clean, 1..4
             ([0, 1, 2], [3, 4]),                                               # 5 missing: LOST
             ([10, 11], [12, 13]),                                              # no parity: clean
             ([0, 10, 11], [1, 12])]                                            # 2 missing, 9 good
    for s in range(nseg):
        if s < len(fixed):
            gone, bad = fixed[s]
        else:
            idx = rng.choice(n, size=int(rng.integers(0, 7)), replace=False)
            cut = int(rng.integers(0, len(idx) + 1))
            gone, bad = idx[:cut], idx[cut:]
            wanted[s] = rng.integers(0, 2, k).astype(bool) if s % 3 else True
        states[s, list(gone)] = ABSENT
        states[s, list(bad)] = BAD
    # MANY under max_bad 4 needs more than four missing and k good: impossible with m = 4, so the
    # class comes up under the smaller bounds the test also runs
    return from_states(states, wanted)


def rs3232_rows(seed=3232):
    """RS(32,32), 16 segments: up to 4 missing and more (MANY), exactly k held, and all data shards
    absent but wanted."""
    k, n = 32, 64
    rng = np.random.default_rng(seed)
    states = np.full((16, n), GOOD)
    wanted = np.ones((16, k), dtype=bool)

    def pick(cnt, lo=0, hi=k):
        return rng.choice(np.arange(lo, hi), size=cnt, replace=False)
    states[1, pick(1)] = BAD
    states[2, pick(2)] = ABSENT
    m3 = pick(3)
    states[3, m3[:2]] = BAD
    states[3, m3[2:]] = ABSENT
    states[4, pick(4)] = BAD
    states[5, pick(5)] = BAD                      # five missing: MANY
    states[6, pick(9)] = ABSENT                   # nine missing: MANY
    states[7, k:] = ABSENT                        # exactly k held, all good: CLEAN
    g = pick(2)
    states[8, g] = ABSENT                         # exactly k held again: 2 data for 2 parity gone
    states[8, pick(30, k, n)] = ABSENT
    states[9, :k] = ABSENT                        # every data shard absent but wanted
    states[10, :k] = ABSENT                       # ... and only three of them wanted
    wanted[10] = False
    wanted[10, [0, 13, 31]] = True
    states[11, pick(3)] = BAD                     # missing shards that nobody wants: CLEAN
    wanted[11] = states[11, :k] == GOOD
    states[12, pick(20)] = ABSENT                 # fewer than k good: LOST
    states[12, pick(20, k, n)] = BAD
    states[13, pick(4, k, n)] = BAD               # bad parity only: CLEAN
    wanted[14] = False                            # nothing wanted: CLEAN
    states[14, pick(6)] = BAD
    m15 = pick(4)                                 # four missing, parity partly bad, junk past k
    states[15, m15] = ABSENT
    states[15, pick(10, k, n)] = BAD
    return from_states(states, wanted)


def rs20056_rows(seed=20056):
    """RS(200,56), 4 segments: the planner's lane stride is past 64."""
    k, n = 200, 256
    rng = np.random.default_rng(seed)
    states = np.full((4, n), GOOD)
    wanted = np.ones((4, k), dtype=bool)
    states[0, [3, 130]] = BAD                                   # bad but not wanted: CLEAN
    wanted[0, [3, 130]] = False
    states[0, 240:] = BAD
    m1 = rng.choice(np.arange(60, k), size=3, replace=False)   # missing shards past lane 64
    states[1, m1[:1]] = BAD
    states[1, m1[1:]] = ABSENT
    states[1, [0, 70, 140]] = BAD                               # missing but not wanted
    wanted[1, [0, 70, 140]] = False
    states[2, [5, 64, 128, 199]] = ABSENT
    states[2, 200:230] = BAD
    states[3, rng.choice(n, size=60, replace=False)] = ABSENT   # fewer than k good: LOST
    return from_states(states, wanted)


def read_statuses(k, m, held, bad, wanted, max_bad, flags=None):
    """cec_read_status of every row -> (status [nseg], [missing...] per row)."""
    import ctypes
    from cess_amd import _lib
    lib = _lib.load()
    held = np.ascontiguousarray(held, dtype=np.uint8)
    if flags is None:
        flags = (held != 0) & ~np.asarray(bad, dtype=bool)
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    wanted = np.ascontiguousarray(wanted, dtype=np.uint8)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    st, nm = ctypes.c_int(), ctypes.c_int()
    miss = (ctypes.c_uint8 * 4)()
    status, missing = np.zeros(len(held), np.int64), []
    for s in range(len(held)):
        assert lib.cec_read_status(k, m, held[s].ctypes.data_as(u8p), flags[s].ctypes.data_as(u8p),
                                   wanted[s].ctypes.data_as(u8p), max_bad, ctypes.byref(st),
                                   ctypes.byref(nm), miss) == 0
        status[s] = st.value
        missing.append([int(x) for x in miss[:nm.value]])
    return status, missing


def classes(k, m, case, max_bads):
    """{(status, shards rebuilt)} of a case over the bounds it is run with."""
    held, bad, wanted = case
    seen = set()
    for mb in max_bads:
        st, miss = read_statuses(k, m, held, bad, wanted, mb)
        seen |= {(int(a), len(b)) for a, b in zip(st, miss)}
    return seen
