"""Helpers of the large-geometry GPU tests (test_gpu_large_batch.py, test_gpu_large_stride.py),
checked on small numpy arrays in test_large_geom.py.

A batch of more than 4 GiB cannot be checked byte for byte against the host oracle in a few
seconds, and must not be checked against the code under test. It is made periodic instead:

 * segment-periodic: segment s holds the bytes of base[s % P], P = 7, so the oracle runs on P
   segments and the expectation of segment s is that of s % P. A 32-bit product or a truncated
   offset displaces an access by 2^j bytes, a power-of-two number of segments for the
   power-of-two segment strides in use, and 2^j mod 7 is 1, 2 or 4, never 0: the displaced segment
   is not the expected one.
 * column-periodic (a few huge segments): a shard is a window of W = 7 * 1024 bytes tiled along
   its length (the last period may be partial). The codes are column-wise, so the expected output
   is the oracle's output on the windows, tiled the same way; 2^j mod W is never 0.

Every function takes numpy arrays or torch tensors (the arithmetic is `!=`, slices, reshape).
Outputs are pre-filled with POISON, and every array lies between two GUARD-byte bands of
GUARD_BYTE inside one flat allocation (Guarded)."""
import numpy as np

P = 7
W = 7 * 1024
GUARD = 4096
GUARD_BYTE = 0xA5
POISON = 0x3C

BOUNDARY_OFFSETS = ((1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32)


def _is_np(a):
    return isinstance(a, np.ndarray)


def _host(a):
    return a if _is_np(a) else a.cpu().numpy()


def _any_last(d):
    return d.any(axis=-1) if _is_np(d) else d.any(dim=-1)


def segment_displacement(j, stride):
    """How many segments of `stride` bytes an offset error of 2^j bytes skips (None: not whole)."""
    d, r = divmod(1 << j, stride)
    return d if r == 0 else None


def boundary_segments(stride, nseg):
    """The segments (of `stride` bytes, nseg of them) that hold the byte offsets 2^31 - 1, 2^31,
    2^32 - 1 and 2^32 of their array, segment 0, the last segment, and the neighbours of each
    (inside the array), ascending."""
    marks = {0, nseg - 1} | {off // stride for off in BOUNDARY_OFFSETS}
    return sorted({t for s in marks for t in (s - 1, s, s + 1) if 0 <= t < nseg})


class Guarded:
    """`nbytes` bytes (`arr`, a view) between two guard bands in one flat allocation made by
    alloc(n) -> 1-D uint8 array or tensor of n bytes. `offset` shifts the array off the
    allocation's alignment (0: as aligned as GUARD allows, 16 bytes and more)."""

    def __init__(self, alloc, nbytes, offset=0, fill=None):
        self.lo = GUARD + offset
        self.hi = self.lo + nbytes
        self.flat = alloc(self.hi + GUARD)
        self.flat[:self.lo] = GUARD_BYTE
        self.flat[self.hi:] = GUARD_BYTE
        self.arr = self.flat[self.lo:self.hi]
        if fill is not None:
            self.arr[:] = fill

    def guards_ok(self):
        return bool((self.flat[:self.lo] == GUARD_BYTE).all()) and \
            bool((self.flat[self.hi:] == GUARD_BYTE).all())


def tile_segments(dst, base):
    """dst[s] = base[s % len(base)] for the rows of dst ([nseg][seg_bytes])."""
    per, nseg = base.shape[0], dst.shape[0]
    full = nseg // per
    if full:
        dst[:full * per].reshape(full, per, -1)[:] = base[None]
    if nseg > full * per:
        dst[full * per:] = base[:nseg - full * per]


def periodic_mismatch(arr, expect, group_bytes=1 << 29):
    """The rows s of arr ([nseg][seg_bytes]) that differ from expect[s % len(expect)], ascending;
    every byte is compared, group_bytes at a time."""
    nseg, sb = arr.shape
    per = expect.shape[0]
    step = per * max(1, group_bytes // (per * sb))  # a multiple of the period
    bad = []
    for g in range(0, nseg, step):
        n = min(step, nseg - g)
        full = n // per
        flags = []
        if full:
            blk = arr[g:g + full * per].reshape(full, per, sb)
            flags.append(_host(_any_last(blk != expect[None])).reshape(-1))
        if n > full * per:
            flags.append(_host(_any_last(arr[g + full * per:g + n] != expect[:n - full * per])))
        bad += [g + int(i) for i in np.flatnonzero(np.concatenate(flags))]
    return bad


def describe_row(row, expect, s):
    """What a mismatching row s holds, for an assertion message: its first differing byte, and
    whether the row is another period's bytes (a displaced access) or still poison."""
    want = expect[s % expect.shape[0]]
    i = int(np.flatnonzero(_host(row != want))[0])
    what = [f"segment {s}: first difference at byte {i}, got {int(row[i]):#x}, "
            f"want {int(want[i]):#x}"]
    for j in range(expect.shape[0]):
        if not bool((row != expect[j]).any()):
            what.append(f"holds the bytes of period {j} (expected {s % expect.shape[0]})")
    if bool((row == POISON).all()):
        what.append("all poison: never written")
    return "; ".join(what)


def assert_periodic(arr, expect, what=""):
    bad = periodic_mismatch(arr, expect)
    assert not bad, (what, len(bad), bad[:8], describe_row(arr[bad[0]], expect, bad[0]))


def constant_mismatch(arr, value):
    """The rows of arr ([rows][row_bytes]) that are not `value` in every byte, ascending (junk a
    call must leave alone), compared in pieces like periodic_mismatch."""
    if _is_np(arr):
        row = np.full((1, arr.shape[1]), value, np.uint8)
    else:
        row = arr.new_full((1, arr.shape[1]), value)
    return periodic_mismatch(arr, row)


def tile_columns(window, length):
    """window [..., W'] tiled along the last axis to `length` columns (a partial last period)."""
    reps = -(-length // window.shape[-1])
    if _is_np(window):
        return np.tile(window, reps)[..., :length]
    return window.repeat(*([1] * (window.dim() - 1)), reps)[..., :length]


def column_mismatch(arr, window, rows_per_step=8):
    """The rows r of arr ([rows][length]) that differ from window[r] ([rows][W']) tiled along
    the row, ascending; every byte is compared, rows_per_step rows at a time."""
    rows, length = arr.shape
    bad = []
    for r in range(0, rows, rows_per_step):
        want = tile_columns(window[r:r + rows_per_step], length)
        flags = _host(_any_last(arr[r:r + rows_per_step] != want))
        bad += [r + int(i) for i in np.flatnonzero(flags)]
    return bad
