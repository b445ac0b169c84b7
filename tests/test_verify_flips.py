"""The flip plans of tests/verify_flips.py hold what the GPU sensitivity tests rely on (no GPU
needed): every claimed place is touched, every (byte of a column, bit) is covered, one bit per
flipped segment, between 1/32 and 1/8 of the segments clean. And on one small shape the reference
itself, fed the planned segments, gives exactly the expected flags."""
import numpy as np
import pytest

from tests import verify_flips as vf

BATCH = [pytest.param(c, id=c.id) for c in vf.BATCH_CASES]
PTRS = [pytest.param(c, id=c.id) for c in vf.PTR_CASES]


def check_inputs(pl):
    """(c) one flipped bit per flipped segment, every segment clean or flipped once; (d) the
    share of clean segments. Conditions on the inputs."""
    assert np.isin(pl.mask, 1 << np.arange(8)).all()
    assert (np.diff(pl.segment) > 0).all(), "two flips in one segment"
    both = np.concatenate([pl.segment, pl.clean])
    assert np.array_equal(np.sort(both), np.arange(pl.nseg))
    assert pl.clean[0] == 0 and pl.clean[-1] == pl.nseg - 1
    assert np.isin(np.arange(0, pl.nseg, 16), pl.clean).all()
    assert pl.nseg / 32 <= len(pl.clean) <= pl.nseg / 8, (len(pl.clean), pl.nseg)
    assert np.array_equal(pl.expected() == 1, np.isin(np.arange(pl.nseg), pl.clean))


def check_shard(pl, sel, shard, ln, positions, every_byte, fft):
    """(a) the flips `sel` of `shard` touch exactly `positions`, each with the rule's bit, and
    its last byte with every bit; (b) where every byte is flipped, every (p % 16, bit), and with
    `fft` every (p // 512 % 2, p % 16, bit), is covered."""
    by, mk = pl.byte[sel], pl.mask[sel]
    assert (pl.shard[sel] == shard).all()
    rule = mk == 1 << vf.bit_of(by)
    assert np.array_equal(np.unique(by[rule]), np.unique(np.append(positions, ln - 1)))
    assert (by[~rule] == ln - 1).all()
    assert set(mk[by == ln - 1]) == {1 << b for b in range(8)}
    if not every_byte:
        return
    assert np.array_equal(np.unique(by), np.arange(ln))
    bit = np.log2(mk).astype(np.int64)
    halves = min(2, -(-ln // 512)) if fft else 1
    half = by // 512 % 2 if fft else np.zeros_like(by)
    seen = np.zeros((halves, 16, 8), dtype=bool)
    seen[half, by % 16, bit] = True
    assert seen.all(), np.argwhere(~seen)[:4]


@pytest.mark.parametrize("case", BATCH)
def test_batch_plan(case):
    pl = vf.batch_plan(case)
    check_inputs(pl)
    n = case.k + case.m
    assert set(case.full) <= set(case.shards)
    claimed = {}
    for s, pos in zip(case.shards,
                      case.positions if np.ndim(case.positions[0]) else
                      [case.positions] * len(case.shards)):
        claimed.setdefault(int(s), []).extend(int(p) for p in pos)
    assert set(pl.shard) == set(claimed)
    for s, pos in claimed.items():
        if s in case.full:
            assert sorted(pos) == list(range(case.ln))
        check_shard(pl, pl.shard == s, s, case.ln, pos, s in case.full, (case.k, case.m) == (32, 32))
    assert len(pl.segment) == sum(len(p) for p in claimed.values()) + 8 * len(claimed)
    # what the table of cases says of each
    if case.id.endswith("second-wg"):
        col = pl.byte[:-8 * 64] // 16  # ahead of the last bytes' masks
        assert np.array_equal(np.bincount(col), np.full(case.ln // 16, 4))
        assert set(claimed) == set(range(64))
    elif case.par_off:
        assert case.full == list(range(case.k, n))
        assert all(claimed[s] == list(range(0, case.ln, 7)) for s in range(case.k))
    elif case.id.startswith("rs32_32-fft"):
        assert case.full in (list(range(32)), list(range(32, 64)))
        assert pl.nseg < 65535, "each half stays below the grid-y seam"
    else:
        assert case.full == list(range(n))
    # device memory: the shards and the generic path's recomputed parity
    assert pl.nseg * (case.k + 2 * case.m) * case.ln < 4 << 30


def test_the_two_fft_halves_cover_all_64_shards():
    halves = [c for c in vf.BATCH_CASES if c.id in ("rs32_32-fft-data", "rs32_32-fft-parity")]
    assert sorted(halves[0].full + halves[1].full) == list(range(64))


@pytest.mark.parametrize("case", PTRS)
def test_ptr_plan(case):
    pl, of_seg = vf.ptr_plan(case)
    check_inputs(pl)
    n = case.k + case.m
    assert case.ln % 8 == 5 or case.off, "a byte tail behind 16-, 8- and 4-byte columns"
    assert len(of_seg) == pl.nseg
    for g, (sources, expects) in enumerate(case.groups):
        assert not set(sources) & set(expects) and len(sources) >= case.k
        flipped = vf.ptr_flipped(case, (sources, expects))
        assert set(expects) <= set(flipped) <= set(sources) | set(expects)
        assert len(flipped) == case.k + len(expects)
        in_g = of_seg[pl.segment] == g
        assert set(pl.shard[in_g]) == set(flipped)
        assert (of_seg[pl.clean] == g).sum() >= 2, "every group has clean segments"
        for s in flipped:
            check_shard(pl, in_g & (pl.shard == s), s, case.ln, np.arange(case.ln), True, False)
    stride = -(-case.ln // 64) * 64 + 64
    assert pl.nseg * n * stride < 4 << 30


def test_reference_flags_rs4_2(orc):
    """RS(4,2), 160-byte shards: the planned segments built on the host and the parity of each
    recomputed by the Python oracle give exactly the expected flags."""
    k, m, ln = 4, 2, 160
    n = k + m
    pl = vf.plan(n, ln, range(n), np.arange(ln))
    check_inputs(pl)
    for s in range(n):
        check_shard(pl, pl.shard == s, s, ln, np.arange(ln), True, False)
    rs = orc.ReedSolomon(k, m)
    rng = np.random.default_rng(42)
    data = [rng.integers(0, 256, ln, dtype=np.uint8) for _ in range(k)]
    word = np.stack(data + rs.encode(data))
    segs = np.broadcast_to(word, (pl.nseg, n, ln)).copy()
    segs[pl.segment, pl.shard, pl.byte] ^= pl.mask
    assert (segs != word).sum() == len(pl.segment)
    par = rs.encode([segs[:, i].reshape(-1) for i in range(k)])
    same = np.stack([p.reshape(pl.nseg, ln) for p in par], axis=1) == segs[:, k:]
    assert np.array_equal(same.all(axis=(1, 2)).astype(np.uint8), pl.expected())
