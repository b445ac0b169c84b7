"""CPU-side checks of the parity accumulation calls (cec_encode_idx*, cec_update*): they refuse a
NULL codec without a GPU, the Python forms raise klauspost's errors before any C call, and no
acc.hip kernel of the product library uses scratch."""
import ctypes
import os
import sys

import numpy as np
import pytest

from tests.conftest import ROOT


def test_null_codec_is_refused_without_gpu():
    from cess_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data
    flags = (ctypes.c_uint8 * 2)(1, 0)
    ptrs = (ctypes.c_void_p * 3)(p, p, p)
    assert lib.cec_encode_idx_batch(None, p, 16, 0, p + 32, 1, 16, 1, None) == _lib.CEC_EINVAL
    assert lib.cec_update_batch(None, p, p + 16, p + 32, 1, 8, flags, None) == _lib.CEC_EINVAL
    assert lib.cec_encode_idx(None, p, 0, ptrs, 16) == _lib.CEC_EINVAL
    assert lib.cec_update(None, ptrs, ptrs, 16) == _lib.CEC_EINVAL
    assert not buf.any()


def test_acc_kernels_use_no_scratch():
    """Every instantiation of acc.hip's kernel family keeps its accumulators and the run-time
    indexed argument arrays out of private memory: no private segment and no spilled register."""
    from cess_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sha_slots
    res = sha_slots.kernel_resources(_lib.LIB_PATH)
    ks = {n: r for n, r in res.items() if "k_acc" in n}
    assert len(ks) >= 24, sorted(ks)  # 12 output buckets, EncodeIdx and Update
    for n, r in ks.items():
        assert int(r["private_segment_fixed_size"]) == 0, (n, r["private_segment_fixed_size"])
        assert int(r["vgpr_spill_count"]) == 0 and int(r["sgpr_spill_count"]) == 0, n


def host_encoder(k, m):
    """An Encoder without a device codec: any C call would fail on the missing library handle."""
    from cess_amd import reedsolomon as rs
    enc = object.__new__(rs.Encoder)
    enc.DataShards, enc.ParityShards, enc.Shards = k, m, k + m
    enc._lib, enc._h = None, None
    return enc


def test_python_errors_are_raised_before_any_c_call():
    import cess_amd
    k, m, ln = 4, 2, 32
    enc = host_encoder(k, m)
    rng = np.random.default_rng(1)
    data = [rng.integers(0, 256, ln, dtype=np.uint8) for _ in range(k)]
    par = [rng.integers(0, 256, ln, dtype=np.uint8) for _ in range(m)]
    keep = [p.copy() for p in par]
    for bad in (-1, k):
        with pytest.raises(cess_amd.ErrInvShardNum):
            enc.EncodeIdx(data[0], bad, par)
        with pytest.raises(cess_amd.ErrInvShardNum):
            enc.EncodeIdxBatch(0, ln, bad, 0, 1, ln)
    with pytest.raises(cess_amd.ErrTooFewShards):
        enc.EncodeIdx(data[0], 0, par[:1])
    with pytest.raises(cess_amd.ErrShardSize):
        enc.EncodeIdx(data[0][:5], 0, par)
    with pytest.raises(cess_amd.ErrShardSize):
        enc.EncodeIdx(data[0], 0, [par[0], par[1][:5]])
    with pytest.raises(cess_amd.ErrShardNoData):
        enc.EncodeIdx(np.zeros(0, np.uint8), 0, par)
    with pytest.raises(cess_amd.ErrInvalidInput):
        enc.EncodeIdx(data[0], 0, [par[0], None])
    shards = data + par
    new = [data[1].copy()] + [None] * (k - 1)
    with pytest.raises(cess_amd.ErrTooFewShards):
        enc.Update(shards[:-1], new)
    with pytest.raises(cess_amd.ErrTooFewShards):
        enc.Update(shards, new[:-1])
    with pytest.raises(cess_amd.ErrTooFewShards):
        enc.UpdateBatch(0, 0, 0, 1, ln, [1] * (k + 1))
    with pytest.raises(cess_amd.ErrShardSize):
        enc.Update(shards, [data[1][:5].copy()] + [None] * (k - 1))
    with pytest.raises(cess_amd.ErrShardNoData):
        enc.Update([None] * (k + m), [None] * k)
    with pytest.raises(cess_amd.ErrInvalidInput):
        enc.Update([None] + shards[1:], new)
    with pytest.raises(cess_amd.ErrInvalidInput):
        enc.Update(shards[:-1] + [None], new)
    enc.Update(shards, [None] * k)  # nothing changed: returns before the C call
    assert all(np.array_equal(a, b) for a, b in zip(par, keep))
