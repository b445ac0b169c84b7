"""Flip plans of the verify sensitivity tests (tests/test_gpu_verify_bits.py; their conditions are
checked on the CPU by tests/test_verify_flips.py). Pure numpy: a helper module, not a test.

One call verifies thousands of copies of one codeword. Every copy but the clean ones carries one
flipped bit at a planned (shard, byte, mask), so the call's flags say for every planned place
whether the kernel looks there: a flipped segment must read 0, a clean one 1.

The bit rule is fixed: byte p gets bit (p // 16) % 8. Within any 8 consecutive 16-byte groups
every (byte within a 16-, 8- or 4-byte column, bit) is then hit once. For the bit-sliced RS(32,32)
kernel, whose lane pair q = (p // 16) % 32 owns bytes 16q..16q+15 and 512+16q.. of each KiB, every
(half, byte, plane) is hit four times per KiB. The last byte of every flipped shard gets all 8
single-bit masks in 8 further segments: the byte tail's compare, every bit of it.

Clean segments: the first, the last and every 16th in between."""
from typing import NamedTuple

import numpy as np


def bit_of(p):
    """The flipped bit of byte position p (array or int)."""
    return (np.asarray(p) // 16) % 8


class Plan(NamedTuple):
    segment: np.ndarray  # segment of each flip, ascending, one flip per segment
    shard: np.ndarray
    byte: np.ndarray
    mask: np.ndarray     # uint8, one bit set
    clean: np.ndarray    # the segments without a flip

    @property
    def nseg(self):
        return len(self.segment) + len(self.clean)

    def expected(self):
        """The flags a correct verify returns: 1 for a clean segment, 0 for a flipped one."""
        ok = np.zeros(self.nseg, dtype=np.uint8)
        ok[self.clean] = 1
        return ok


def _flips(n_shards, ln, shards, positions):
    shards = [int(s) for s in shards]
    assert shards and all(0 <= s < n_shards for s in shards)
    if np.ndim(positions[0]) == 0:
        positions = [positions] * len(shards)
    assert len(positions) == len(shards)
    sh, by = [], []
    for s, pos in zip(shards, positions):
        pos = np.asarray(pos, dtype=np.int64)
        assert pos.ndim == 1 and (pos >= 0).all() and (pos < ln).all()
        sh.append(np.full(len(pos), s, dtype=np.int64))
        by.append(pos)
    sh, by = np.concatenate(sh), np.concatenate(by)
    mk = (1 << bit_of(by)).astype(np.uint8)
    distinct = np.array(list(dict.fromkeys(shards)), dtype=np.int64)
    sh = np.concatenate([sh, np.repeat(distinct, 8)])
    by = np.concatenate([by, np.full(8 * len(distinct), ln - 1, dtype=np.int64)])
    mk = np.concatenate([mk, np.tile((1 << np.arange(8)).astype(np.uint8), len(distinct))])
    return sh, by, mk


def _layout(sh, by, mk):
    # segment 0 is clean, then 15 flipped and 1 clean in turn, and a clean one ends the batch
    i = np.arange(len(sh), dtype=np.int64)
    seg = 1 + i + i // 15
    nseg = int(seg[-1]) + 2
    is_clean = np.ones(nseg, dtype=bool)
    is_clean[seg] = False
    return Plan(seg, sh, by, mk, np.flatnonzero(is_clean))


def plan(n_shards, ln, shards, positions):
    """One flip per segment: for every entry i of `shards`, every byte position of positions[i]
    (or of `positions` itself where that is one flat sequence, used for every shard) with the
    rule's bit; then for every distinct shard, in order of first appearance, the 8 single-bit
    masks of its last byte. -> Plan"""
    return _layout(*_flips(n_shards, ln, shards, positions))


def first_k(k, sources):
    """The survivors a decode reads: the first k sources in index order (cec_survivors)."""
    assert len(sources) >= k
    return sorted(sources)[:k]


# ---- cec_verify_batch ----------------------------------------------------------------------------


class BatchCase(NamedTuple):
    id: str
    k: int
    m: int
    ln: int
    generic: int    # CEC_OPT_FORCE_GENERIC
    par_off: int    # the parity tensor starts this many bytes into its allocation
    shards: list    # plan() arguments
    positions: list
    full: list      # the shards of which every byte is flipped


def _every(shards, ln):
    shards = list(shards)
    return dict(shards=shards, positions=np.arange(ln), full=shards)


def _second_workgroup(ln=5120):
    """RS(32,32), 5 KiB shards, 1 KiB per wave, so the fifth wave is the second workgroup's first:
    for each 16-byte column c four flips j, in shard (c + 16 j) % 64 at byte 16 c + (c + 5 j) % 16."""
    c = np.repeat(np.arange(ln // 16), 4)
    j = np.tile(np.arange(4), ln // 16)
    return dict(shards=list((c + 16 * j) % 64), positions=[[p] for p in 16 * c + (c + 5 * j) % 16],
                full=[])


def _batch(id, k, m, ln, generic=0, par_off=0, **flips):
    if not flips:
        flips = _every(range(k + m), ln)
    return BatchCase(id, k, m, ln, generic, par_off, **flips)


BATCH_CASES = [
    # k_verify21: one workgroup of 16-byte columns and one lane
    _batch("rs2_1-fused", 2, 1, 4112),
    # a length the fused kernel refuses: the generic path, k_cmp_segments<false>
    _batch("rs2_1-bytes", 2, 1, 4099),
    # k_rt + k_cmp_segments<true>
    _batch("rs2_1-generic", 2, 1, 4112, generic=1),
    # parity 1 byte into its allocation: the byte paths for the whole call; every parity byte,
    # every 7th data byte
    _batch("rs2_1-generic-parity+1", 2, 1, 4112, generic=1, par_off=1, shards=[0, 1, 2],
           positions=[np.arange(0, 4112, 7), np.arange(0, 4112, 7), np.arange(4112)], full=[2]),
    # k_rtb bucket 4, and the byte compare (m * ln = 4004)
    _batch("rs10_4", 10, 4, 1001),
    # k_fft3232_verify, one full tile: the data shards and the parity shards in two calls
    _batch("rs32_32-fft-data", 32, 32, 1024, **_every(range(32), 1024)),
    _batch("rs32_32-fft-parity", 32, 32, 1024, **_every(range(32, 64), 1024)),
    # k_fft3232_verify, a second workgroup of one wave
    _batch("rs32_32-fft-second-wg", 32, 32, 5120, **_second_workgroup()),
    # no multiple of 1024: k_hg, or forced generic k_rthx, + k_cmp_segments<true>
    _batch("rs32_32-matrix", 32, 32, 264),
    _batch("rs32_32-generic", 32, 32, 264, generic=1),
]


def batch_plan(case):
    return plan(case.k + case.m, case.ln, case.shards, case.positions)


# ---- cec_verify_ptrs -----------------------------------------------------------------------------


class PtrCase(NamedTuple):
    id: str
    k: int
    m: int
    ln: int
    off: int        # every view starts this many bytes past a 64-byte boundary
    generic: int    # CEC_OPT_FORCE_GENERIC
    rt_mode: int    # CEC_OPT_RT_MODE, None: the default
    groups: list    # (sources, expectations): every segment of the call is of one of them


def _parity(k, m):
    return (list(range(k)), list(range(k, k + m)))


def _data0(k, m):
    """Data shard 0 expected from all the other shards: k survivors, the rest unread."""
    return (list(range(1, k + m)), [0])


def _ptr(id, k, m, ln, groups=None, off=0, generic=0, rt_mode=None):
    return PtrCase(id, k, m, ln, off, generic, rt_mode, groups or [_parity(k, m)])


# every ln is one workgroup's bytes (4096 / 2048 / 1024 for 16- / 8- / 4-byte columns) + one
# column + a byte tail: ln % 16 == 13 gives tails of 13, 5 and 1 bytes, 1029 one of 1 (and of 5
# for the 16-byte columns of RS(5,37)'s second chunk)
PTR_CASES = [
    # k_ptr21<CmpSink>, cases 2 / 0 / 1 in one call
    _ptr("rs2_1-cases", 2, 1, 4125, groups=[([0, 1], [2]), ([1, 2], [0]), ([0, 2], [1])]),
    _ptr("rs2_1-generic", 2, 1, 4125, generic=1),                  # k_ptrt<1, u32x4>
    _ptr("rs4_2", 4, 2, 2061),                                     # k_ptrb<2>
    _ptr("rs10_4", 10, 4, 2061),                                   # k_ptrb<4>
    _ptr("rs10_4-masks", 10, 4, 4125, rt_mode=1),                  # k_ptrt<4>
    _ptr("rs10_4-data0", 10, 4, 2061, groups=[_data0(10, 4)]),     # k_ptrb<1>
    _ptr("rs3_5", 3, 5, 4125),                                     # k_ptrt<5, u32x4>
    _ptr("rs6_8", 6, 8, 2061),                                     # k_ptrt<8, u32x2>
    _ptr("rs20_17", 20, 17, 1029),                                 # k_ptrt<24, uint32_t>
    # two program chunks with different column widths: k_ptrt<32, uint32_t> + k_ptrt<5, u32x4>
    _ptr("rs5_37", 5, 37, 1029),
    # every view 3 bytes off: the byte path for the whole call, two 256-byte blocks
    _ptr("rs2_1-off3", 2, 1, 300, off=3),
    _ptr("rs10_4-off3", 10, 4, 300, off=3),
]


def ptr_flipped(case, group):
    """The shards of a group that get flips: its expectations and the survivors among its
    sources, ascending."""
    sources, expects = group
    return sorted(set(expects) | set(first_k(case.k, sources)))


def ptr_plan(case):
    """-> (Plan of the call, the group of every segment): every byte of every expectation and of
    every survivor, the groups' flips one after the other, the clean segments dealt to the groups
    in turn."""
    flips, group = [], []
    for g, (sources, expects) in enumerate(case.groups):
        shards = ptr_flipped(case, (sources, expects))
        flips.append(_flips(case.k + case.m, case.ln, shards, np.arange(case.ln)))
        group.append(np.full(len(flips[-1][0]), g, dtype=np.int64))
    pl = _layout(*(np.concatenate(f) for f in zip(*flips)))
    of_seg = np.empty(pl.nseg, dtype=np.int64)
    of_seg[pl.segment] = np.concatenate(group)
    of_seg[pl.clean] = np.arange(len(pl.clean)) % len(case.groups)
    return pl, of_seg
