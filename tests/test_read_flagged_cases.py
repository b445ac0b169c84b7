"""What the segments of tests/test_gpu_read_flagged.py cover (CPU): each case generator, at its
fixed seed and over the bounds its test runs, yields every class the code and the segment count
allow: CLEAN, REBUILT with 1 to 4 shards rebuilt, MANY, LOST. The classes come from
cec_read_status alone.

RS(2,1) can rebuild one shard and RS(4,2) two (a rebuild of e shards needs e <= m), and RS(2,1)
has no MANY (two missing leave fewer than k good); RS(200,56) has four segments, so its classes are
spread over the two bounds it runs with."""
from tests import read_flagged_cases as rc
from tests.read_flagged_cases import CLEAN, LOST, MANY, REBUILT

ALL = {(CLEAN, 0), (REBUILT, 1), (REBUILT, 2), (REBUILT, 3), (REBUILT, 4), (MANY, 0), (LOST, 0)}


def test_rs21_classes():
    case = rc.rs21_all()
    assert len(case[0]) == 108
    assert rc.classes(2, 1, case, [1]) == {(CLEAN, 0), (REBUILT, 1), (LOST, 0)}
    assert rc.classes(2, 1, case, [4]) == {(CLEAN, 0), (REBUILT, 1), (LOST, 0)}


def test_rs42_classes():
    for random_wanted in (False, True):
        case = rc.rs42_all(random_wanted)
        assert len(case[0]) == 729
        assert rc.classes(4, 2, case, [1]) == {(CLEAN, 0), (REBUILT, 1), (MANY, 0), (LOST, 0)}
        assert rc.classes(4, 2, case, [2]) == {(CLEAN, 0), (REBUILT, 1), (REBUILT, 2), (LOST, 0)}


def test_rs104_classes():
    case = rc.rs104_random()
    assert len(case[0]) == 64
    assert rc.classes(10, 4, case, [4]) == ALL - {(MANY, 0)}  # five missing leave nine good
    assert rc.classes(10, 4, case, [1, 2, 3, 4]) == ALL
    assert (MANY, 0) in rc.classes(10, 4, case, [3])


def test_rs3232_classes():
    case = rc.rs3232_rows()
    assert len(case[0]) == 16
    assert rc.classes(32, 32, case, [4]) == ALL
    held, bad, wanted = case
    st, miss = rc.read_statuses(32, 32, held, bad, wanted, 4)
    assert held[7].sum() == 32 and st[7] == CLEAN          # exactly k held
    assert held[8].sum() == 32 and (st[8], len(miss[8])) == (REBUILT, 2)
    assert not held[9, :32].any() and wanted[9].all() and st[9] == MANY
    assert not held[10, :32].any() and (st[10], miss[10]) == (REBUILT, [0, 13, 31])
    assert rc.read_statuses(32, 32, held, bad, wanted, 2)[0][10] == MANY


def test_rs20056_classes():
    case = rc.rs20056_rows()
    assert len(case[0]) == 4
    assert rc.classes(200, 56, case, [4]) == {(CLEAN, 0), (REBUILT, 3), (REBUILT, 4), (LOST, 0)}
    assert rc.classes(200, 56, case, [2]) == {(CLEAN, 0), (MANY, 0), (LOST, 0)}
    st, miss = rc.read_statuses(200, 56, *case, 4)
    assert all(j >= 60 for j in miss[1]) and miss[2] == [5, 64, 128, 199]
