"""cec_hashq_add_concat_ptrs at every boundary (CPU): the header, the ctypes table, the Rust extern
and wrapper, the built library's export, the Python wrappers over it, their refusals without a
GPU, and the resource use of the two new kernels beside the untouched tick kernels."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_boundary import header_prototypes, rust_prototypes

NAME = "cec_hashq_add_concat_ptrs"
ARITY = 9


def test_declared_in_header_ctypes_and_rust():
    from cess_amd import _lib
    protos = header_prototypes()
    assert NAME in protos, "not in include/cess_ec.h"
    assert protos[NAME] == ("i32", ["ptr", "ptr", "u64", "u64", "u64", "u64", "ptr", "ptr", "ptr"])
    assert NAME in _lib.SIGNATURES, "not in cess_amd/_lib.SIGNATURES"
    assert len(_lib.SIGNATURES[NAME][1]) == ARITY
    assert NAME in rust_prototypes(), "not in the Rust externs"
    assert len(rust_prototypes()[NAME][1]) == ARITY


def test_rust_crate_has_wrapper():
    with open(ROOT + "/utils/ec-hip/src/lib.rs") as f:
        txt = f.read()
    assert re.search(r"pub unsafe fn hashq_add_concat_ptrs\(", txt)


def test_library_exports():
    from cess_amd import _lib
    assert hasattr(_lib.load(), NAME)


def test_python_wrappers():
    from cess_amd.hashq import HashQueue
    sig = inspect.signature(HashQueue.add_concat_ptrs)
    assert list(sig.parameters) == ["self", "chains", "d_hex", "hex_offset", "d_prefix_hex",
                                    "prefix_hex_offset", "length"]
    assert sig.parameters["d_hex"].default is None
    assert sig.parameters["hex_offset"].default == 0
    assert sig.parameters["d_prefix_hex"].default is None
    assert sig.parameters["prefix_hex_offset"].default == 0
    assert sig.parameters["length"].default is None
    sig = inspect.signature(HashQueue.add_segment_lists_device)
    assert list(sig.parameters) == ["self", "segments", "k", "m", "d_seg_hex", "d_frag_hex"]


def test_null_queue_is_refused_without_gpu():
    from cess_amd import _lib
    lib = _lib.load()
    buf = np.zeros(512, dtype=np.uint8)
    p = buf.ctypes.data
    parts = (ctypes.c_void_p * 4)(p, p + 64, p + 128, p + 192)
    ticket = ctypes.c_uint64(7)
    assert lib.cec_hashq_add_concat_ptrs(None, parts, 2, 2, 64, 0, p + 256, p + 384,
                                         ctypes.byref(ticket)) == _lib.CEC_EINVAL
    assert lib.cec_hashq_add_concat_ptrs(None, parts, 2, 2, 64, 100, None, None,
                                         None) == _lib.CEC_EINVAL
    assert lib.cec_hashq_add_concat_ptrs(None, None, 0, 1, 64, 0, None, None,
                                         None) == _lib.CEC_EINVAL
    assert ticket.value == 7
    assert not buf.any()


def test_python_errors_are_raised_before_any_c_call():
    """Host tensors and a queue without a library handle: every error below comes from the Python
    checks, and what returns quietly made no C call."""
    import torch
    import cess_amd
    from cess_amd.hashq import HashQueue
    q = object.__new__(HashQueue)
    q._h = None
    g = torch.Generator().manual_seed(5)

    def t(n=64):
        return torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)

    out = torch.full((1024,), 0xA5, dtype=torch.uint8)
    assert q.add_concat_ptrs([], d_hex=out, d_prefix_hex=out) == 0
    assert q.add_concat_ptrs((), out) == 0
    with pytest.raises(cess_amd.ErrShardSize):
        q.add_concat_ptrs([[t(), t()], [t()]], out)
    with pytest.raises(cess_amd.ErrShardSize):
        q.add_concat_ptrs([[t(), t(128)]], out)
    with pytest.raises(cess_amd.ErrShardSize):
        q.add_concat_ptrs([[t(), t()], [t(128), t(128)]], out)
    with pytest.raises(cess_amd.ErrInvalidInput):
        q.add_concat_ptrs([[t(), None]], out, d_prefix_hex=out)
    with pytest.raises(cess_amd.ErrInvalidInput):
        q.add_concat_ptrs([[None]], out)
    with pytest.raises(cess_amd.ErrShardNoData):
        q.add_concat_ptrs([[t(0), t(0)]], out)
    with pytest.raises(cess_amd.ErrShardNoData):
        q.add_concat_ptrs([[]], out)
    assert q.add_segment_lists_device([], 2, 1, out, out) == 0
    with pytest.raises(cess_amd.ErrShardSize):
        q.add_segment_lists_device([[t(), t()]], 2, 1, out, out)          # k + m tensors wanted
    with pytest.raises(cess_amd.ErrShardSize):
        q.add_segment_lists_device([[t(), t(), t(128)]], 2, 1, out, out)
    with pytest.raises(cess_amd.ErrShardSize):
        q.add_segment_lists_device([[t(96), t(96), t(96)]], 2, 1, out, out)  # not a multiple of 64
    with pytest.raises(cess_amd.ErrInvalidInput):
        q.add_segment_lists_device([[t(), None, t()]], 2, 1, out, out)
    with pytest.raises(cess_amd.ErrShardNoData):
        q.add_segment_lists_device([[t(0), t(0), t(0)]], 2, 1, out, out)
    assert bool((out == 0xA5).all())


def test_new_kernels_use_no_scratch_and_the_ticks_are_as_many():
    """The concat add and the rebase index their 2 KiB argument arrays in the kernarg segment: no
    private segment, no spilled register. The tick kernels keep their four instantiations."""
    from cess_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sha_slots
    res = sha_slots.kernel_resources(_lib.LIB_PATH)
    for pat in ("k_hashq_add_concat", "k_hashq_rebase"):
        ks = {n: r for n, r in res.items() if pat in n}
        assert len(ks) == 1, (pat, sorted(ks))
        for n, r in ks.items():
            assert int(r["private_segment_fixed_size"]) == 0, (n, r["private_segment_fixed_size"])
            assert int(r["vgpr_spill_count"]) == 0 and int(r["sgpr_spill_count"]) == 0, n
    # the pointer add is the concat add with one part: two add kernels, strided and by address
    assert len([n for n in res if "k_hashq_add" in n]) == 2
    assert len([n for n in res if "k_sha256_tick" in n]) == 4
