"""cec_encode_idx_ptrs and cec_update_ptrs at every boundary (CPU): the header, the ctypes table,
the Rust externs and wrappers, the built library's exports, the Encoder methods over them, their
refusals without a GPU, and the resource use of the table-addressed acc.hip kernels."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_acc_host import host_encoder
from tests.test_boundary import header_prototypes, rust_prototypes

ARITY = {"cec_encode_idx_ptrs": 7, "cec_update_ptrs": 7}


@pytest.mark.parametrize("name", sorted(ARITY))
def test_declared_in_header_ctypes_and_rust(name):
    from cess_amd import _lib
    protos = header_prototypes()
    assert name in protos, "not in include/cess_ec.h"
    assert len(protos[name][1]) == ARITY[name]
    assert name in _lib.SIGNATURES, "not in cess_amd/_lib.SIGNATURES"
    assert len(_lib.SIGNATURES[name][1]) == ARITY[name]
    assert name in rust_prototypes(), "not in the Rust externs"
    assert len(rust_prototypes()[name][1]) == ARITY[name]


def test_rust_crate_has_safe_wrappers():
    with open(ROOT + "/utils/ec-hip/src/lib.rs") as f:
        txt = f.read()
    assert re.search(r"pub unsafe fn encode_idx_device\(", txt)
    assert re.search(r"pub unsafe fn update_device\(", txt)


@pytest.mark.parametrize("name", sorted(ARITY))
def test_library_exports(name):
    from cess_amd import _lib
    assert hasattr(_lib.load(), name)


@pytest.mark.parametrize("method,params", [
    ("EncodeIdxDevice", ["self", "dataShard", "idx", "parity", "accumulate", "stream"]),
    ("EncodeIdxDeviceBatch", ["self", "data", "parity", "accumulate", "stream"]),
    ("UpdateDevice", ["self", "shards", "newDatashards", "stream"]),
    ("UpdateDeviceBatch", ["self", "olds", "news", "parities", "stream"])])
def test_encoder_methods(method, params):
    from cess_amd.reedsolomon import Encoder
    assert hasattr(Encoder, method)
    sig = inspect.signature(getattr(Encoder, method))
    assert list(sig.parameters) == params
    assert sig.parameters["stream"].default is None
    if "accumulate" in params:
        assert sig.parameters["accumulate"].default is True


def test_null_codec_is_refused_without_gpu():
    from cess_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data
    data = (ctypes.c_void_p * 2)(p, p + 16)
    new = (ctypes.c_void_p * 2)(p + 16, p)
    par = (ctypes.c_void_p * 1)(p + 32)
    assert lib.cec_encode_idx_ptrs(None, data, par, 1, 16, 1, None) == _lib.CEC_EINVAL
    assert lib.cec_encode_idx_ptrs(None, data, par, 1, 16, 0, None) == _lib.CEC_EINVAL
    assert lib.cec_update_ptrs(None, data, new, par, 1, 16, None) == _lib.CEC_EINVAL
    assert not buf.any()


def test_python_errors_are_raised_before_any_c_call():
    """Host tensors and an encoder without a library handle: every error below comes from the
    Python checks, and what returns quietly made no C call."""
    import torch
    import cess_amd
    k, m, ln = 4, 2, 32
    enc = host_encoder(k, m)
    g = torch.Generator().manual_seed(1)

    def t(n=ln):
        return torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)

    data, par = [t() for _ in range(k)], [t() for _ in range(m)]
    keep = [p.clone() for p in par]
    for bad in (-1, k):
        with pytest.raises(cess_amd.ErrInvShardNum):
            enc.EncodeIdxDevice(data[0], bad, par)
    with pytest.raises(cess_amd.ErrTooFewShards):
        enc.EncodeIdxDevice(data[0], 0, par[:1])
    with pytest.raises(cess_amd.ErrTooFewShards):
        enc.EncodeIdxDeviceBatch([data[:-1]], [par])
    with pytest.raises(cess_amd.ErrTooFewShards):
        enc.EncodeIdxDeviceBatch([data, data], [par, par + par])
    with pytest.raises(cess_amd.ErrInvalidInput):
        enc.EncodeIdxDeviceBatch([data], [par, par])
    with pytest.raises(cess_amd.ErrShardSize):
        enc.EncodeIdxDevice(t(5), 0, par)
    with pytest.raises(cess_amd.ErrShardSize):
        enc.EncodeIdxDevice(data[0], 0, [par[0], t(5)])
    with pytest.raises(cess_amd.ErrShardNoData):
        enc.EncodeIdxDevice(t(0), 0, par)
    with pytest.raises(cess_amd.ErrShardNoData):
        enc.EncodeIdxDevice(None, 0, par)
    enc.EncodeIdxDevice(data[0], 0, [None] * m)        # no parity held: nothing to do
    enc.EncodeIdxDeviceBatch([None, [None] * k], [par, None])  # nothing fed
    shards = data + par
    new = [t()] + [None] * (k - 1)
    with pytest.raises(cess_amd.ErrTooFewShards):
        enc.UpdateDevice(shards[:-1], new)
    with pytest.raises(cess_amd.ErrTooFewShards):
        enc.UpdateDevice(shards, new[:-1])
    with pytest.raises(cess_amd.ErrTooFewShards):
        enc.UpdateDeviceBatch([data], [new], [par[:1]])
    with pytest.raises(cess_amd.ErrInvalidInput):
        enc.UpdateDeviceBatch([data], [new, new], [par])
    with pytest.raises(cess_amd.ErrShardSize):
        enc.UpdateDevice(shards, [t(5)] + [None] * (k - 1))
    with pytest.raises(cess_amd.ErrShardNoData):
        enc.UpdateDevice([None] * (k + m), [None] * k)
    with pytest.raises(cess_amd.ErrInvalidInput):
        enc.UpdateDevice([None] + shards[1:], new)
    with pytest.raises(cess_amd.ErrInvalidInput):
        enc.UpdateDeviceBatch([None], [new], [par])
    enc.UpdateDevice(shards, [None] * k)               # nothing changed
    enc.UpdateDevice(data + [None] * m, new)           # no parity held
    enc.UpdateDeviceBatch([], [], [])
    assert all(torch.equal(a, b) for a, b in zip(par, keep))


def test_acc_ptrs_kernels_use_no_scratch():
    """Every instantiation of the table-addressed kernel keeps its accumulators, the row's
    addresses and the run-time indexed argument arrays out of private memory."""
    from cess_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sha_slots
    res = sha_slots.kernel_resources(_lib.LIB_PATH)
    ks = {n: r for n, r in res.items() if "k_acc_ptrs" in n}
    assert len(ks) >= 24, sorted(ks)  # 12 output buckets, EncodeIdx and Update
    for n, r in ks.items():
        assert int(r["private_segment_fixed_size"]) == 0, (n, r["private_segment_fixed_size"])
        assert int(r["vgpr_spill_count"]) == 0 and int(r["sgpr_spill_count"]) == 0, n
