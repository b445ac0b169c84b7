"""The large-geometry helpers (tests/large_geom.py) on toy arrays: the periodic comparers must see
every way a kernel with a wrapped or truncated offset goes wrong, or the GPU tests that lean on
them prove nothing."""
import numpy as np
import pytest

from tests import large_geom as lg

# the segment strides of test_gpu_large_batch.py: RS(2,1) data / parity at 8 MiB fragments,
# RS(32,32) at 512 KiB, RS(4,4) at 1 MiB
STRIDES = (1 << 24, 1 << 23, 1 << 22)


def _alloc(n):
    return np.empty(n, np.uint8)


def _toy(nseg=23, sb=64, seed=1):
    base = np.random.default_rng(seed).integers(0, 256, (lg.P, sb), dtype=np.uint8)
    arr = np.full((nseg, sb), lg.POISON, np.uint8)
    lg.tile_segments(arr, base)
    return base, arr


@pytest.mark.parametrize("stride", STRIDES)
def test_power_of_two_displacements_never_hit_the_period(stride):
    whole = 0
    for j in range(20, 41):
        d = lg.segment_displacement(j, stride)
        if d is not None:
            whole += 1
            assert d % lg.P != 0, (j, stride, d)
    assert whole == 41 - stride.bit_length() + 1  # every j from log2(stride) up is whole
    assert lg.segment_displacement(stride.bit_length() - 2, stride) is None


def test_power_of_two_column_displacements_never_hit_the_window():
    assert lg.W == 7168
    for j in range(0, 41):
        assert (1 << j) % lg.W != 0, j


def test_tile_segments_and_clean_compare():
    base, arr = _toy()
    for s in range(arr.shape[0]):
        assert np.array_equal(arr[s], base[s % lg.P]), s
    assert lg.periodic_mismatch(arr, base) == []
    # groups smaller than the batch, and a batch shorter than one period
    assert lg.periodic_mismatch(arr, base, group_bytes=1) == []
    assert lg.periodic_mismatch(arr[:3], base) == []
    lg.assert_periodic(arr, base)


@pytest.mark.parametrize("group_bytes", [1, 7 * 64 * 2, 1 << 29])
def test_comparer_reports_displaced_segments(group_bytes):
    base, clean = _toy()
    for a in range(5):
        for s in range(1 << a, clean.shape[0]):
            arr = clean.copy()
            arr[s] = clean[s - (1 << a)]  # what a write or read 2^a segments off leaves
            assert lg.periodic_mismatch(arr, base, group_bytes) == [s], (a, s)
            assert f"period {(s - (1 << a)) % lg.P}" in lg.describe_row(arr[s], base, s)


def test_comparer_reports_poison_flipped_bits_and_several_rows():
    base, clean = _toy()
    for s in (0, 6, 7, 21, 22):
        arr = clean.copy()
        arr[s] = lg.POISON
        assert lg.periodic_mismatch(arr, base) == [s]
        assert "never written" in lg.describe_row(arr[s], base, s)
    for s, byte in ((0, 0), (13, 63), (22, 31)):
        for bit in range(8):
            arr = clean.copy()
            arr[s, byte] ^= 1 << bit
            assert lg.periodic_mismatch(arr, base, group_bytes=1) == [s], (s, byte, bit)
            assert f"byte {byte}," in lg.describe_row(arr[s], base, s)
    arr = clean.copy()
    arr[[2, 9, 22], 5] ^= 0x80
    assert lg.periodic_mismatch(arr, base) == [2, 9, 22]
    with pytest.raises(AssertionError):
        lg.assert_periodic(arr, base, "three rows")


def test_constant_compare_on_a_strided_view():
    arr = np.full((9, 3, 32), lg.GUARD_BYTE, np.uint8)
    view = arr[1::2, 1]  # rows 1, 3, 5, 7 of shard 1
    assert lg.constant_mismatch(view, lg.GUARD_BYTE) == []
    arr[5, 1, 31] ^= 0x10
    arr[4, 1, 0] = 0  # not in the view
    assert lg.constant_mismatch(view, lg.GUARD_BYTE) == [2]
    assert lg.constant_mismatch(view, 0) == [0, 1, 2, 3]


@pytest.mark.parametrize("offset", [0, 1])
def test_guarded_sees_a_damaged_guard(offset):
    g = lg.Guarded(_alloc, 100, offset=offset, fill=lg.POISON)
    assert g.arr.shape == (100,) and (g.arr == lg.POISON).all()
    assert g.flat.shape == (2 * lg.GUARD + offset + 100,)
    assert (g.arr.ctypes.data - g.flat.ctypes.data) == lg.GUARD + offset
    g.arr[:] = 7  # the array itself may be written
    assert g.guards_ok()
    for pos in (0, g.lo - 1, g.hi, g.flat.shape[0] - 1):
        keep = g.flat[pos]
        g.flat[pos] ^= 1
        assert not g.guards_ok(), pos
        g.flat[pos] = keep
    assert g.guards_ok()


def test_boundary_segments_of_the_batch_shapes():
    # RS(2,1), F = 8 MiB, 520 segments: data stride 2^24 (2^31 = segment 128, 2^32 = 256)
    assert lg.boundary_segments(1 << 24, 520) == [0, 1, 126, 127, 128, 129, 254, 255, 256, 257,
                                                  518, 519]
    # its parity, stride 2^23 (2^31 = segment 256, 2^32 = 512)
    assert lg.boundary_segments(1 << 23, 520) == [0, 1, 254, 255, 256, 257, 510, 511, 512, 513,
                                                  518, 519]
    # RS(32,32), F = 512 KiB, 264 segments, both arrays stride 2^24
    assert lg.boundary_segments(1 << 24, 264) == [0, 1, 126, 127, 128, 129, 254, 255, 256, 257,
                                                  262, 263]
    # RS(4,4), F = 1 MiB, 1032 segments, both arrays stride 2^22 (2^31 = 512, 2^32 = 1024)
    assert lg.boundary_segments(1 << 22, 1032) == [0, 1, 510, 511, 512, 513, 1022, 1023, 1024,
                                                   1025, 1030, 1031]
    # an array that ends before 2^32, and a tiny one
    assert lg.boundary_segments(1 << 24, 200) == [0, 1, 126, 127, 128, 129, 198, 199]
    assert lg.boundary_segments(1 << 24, 1) == [0]
    # every batch shape really crosses 2^32 inside the array
    for stride, nseg in ((1 << 24, 520), (1 << 23, 520), (1 << 24, 264), (1 << 22, 1032)):
        assert stride * nseg > (1 << 32) + stride


def test_column_tiling_and_compare():
    rng = np.random.default_rng(2)
    rows, length = 11, 3 * lg.W + 1000  # a partial last period
    win = rng.integers(0, 256, (rows, lg.W), dtype=np.uint8)
    arr = lg.tile_columns(win, length).copy()
    assert arr.shape == (rows, length)
    for c in (0, lg.W - 1, lg.W, 2 * lg.W + 5, length - 1):
        assert np.array_equal(arr[:, c], win[:, c % lg.W]), c
    assert lg.column_mismatch(arr, win) == []
    assert lg.column_mismatch(arr, win, rows_per_step=3) == []
    # a row read 2^j columns off, one flipped bit in the partial period, a row left at poison
    for j in range(0, 14):
        bad = arr.copy()
        bad[4, :length - (1 << j)] = arr[4, (1 << j):]
        assert lg.column_mismatch(bad, win) == [4], j
    bad = arr.copy()
    bad[10, length - 1] ^= 1
    bad[0] = lg.POISON
    assert lg.column_mismatch(bad, win, rows_per_step=4) == [0, 10]
