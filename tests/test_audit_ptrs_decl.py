"""cec_audit_chunks_ptrs and cec_hashq_add_ptrs at every boundary (CPU): the header, the ctypes
table, the Rust externs and wrappers, the built library's exports, the Python wrappers over them,
their refusals without a GPU, and the resource use of the new kernels."""
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

ARITY = {"cec_audit_chunks_ptrs": 10, "cec_hashq_add_ptrs": 6}


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


def test_header_capture_note_names_the_audit_call():
    with open(ROOT + "/include/cess_ec.h") as f:
        txt = f.read()
    note = txt[txt.index("HIP graph capture: the calls whose kernels"):txt.index("int cec_encode_batch(")]
    assert "cec_audit_chunks_ptrs" in note


def test_rust_crate_has_wrappers():
    with open(ROOT + "/utils/ec-hip/src/lib.rs") as f:
        txt = f.read()
    assert re.search(r"pub unsafe fn audit_chunks_device\(", txt)
    assert re.search(r"pub unsafe fn hashq_add_ptrs\(", txt)


@pytest.mark.parametrize("name", sorted(ARITY))
def test_library_exports(name):
    from cess_amd import _lib
    assert hasattr(_lib.load(), name)


def test_python_wrappers():
    from cess_amd import audit
    from cess_amd.hashq import HashQueue
    sig = inspect.signature(audit.audit_chunks_device)
    assert list(sig.parameters) == ["enc", "frags", "indices", "d_chunks", "d_hex", "chunk_count",
                                    "stream"]
    assert sig.parameters["d_chunks"].default is None
    assert sig.parameters["d_hex"].default is None
    assert sig.parameters["chunk_count"].default == audit.CHUNK_COUNT == 1024
    assert sig.parameters["stream"].default is None
    sig = inspect.signature(HashQueue.add_ptrs)
    assert list(sig.parameters) == ["self", "tensors", "d_hex", "hex_offset"]
    assert sig.parameters["d_hex"].default is None
    assert sig.parameters["hex_offset"].default == 0


def test_null_codec_and_null_queue_are_refused_without_gpu():
    from cess_amd import _lib
    lib = _lib.load()
    buf = np.zeros(256, dtype=np.uint8)
    p = buf.ctypes.data
    frags = (ctypes.c_void_p * 2)(p, p + 32)
    idx = (ctypes.c_uint32 * 2)(0, 1)
    assert lib.cec_audit_chunks_ptrs(None, frags, 2, 32, 2, idx, 2, p + 64, p + 128,
                                     None) == _lib.CEC_EINVAL
    assert lib.cec_audit_chunks_ptrs(None, frags, 2, 32, 2, idx, 2, None, p + 128,
                                     None) == _lib.CEC_EINVAL
    ticket = ctypes.c_uint64(7)
    assert lib.cec_hashq_add_ptrs(None, frags, 2, 32, p + 64,
                                  ctypes.byref(ticket)) == _lib.CEC_EINVAL
    assert lib.cec_hashq_add_ptrs(None, None, 0, 32, None, None) == _lib.CEC_EINVAL
    assert ticket.value == 7
    assert not buf.any()


def test_python_errors_are_raised_before_any_c_call():
    """Host tensors and an encoder without a library handle: every error below comes from the
    Python checks, and what returns quietly made no C call."""
    import torch
    import cess_amd
    from cess_amd import audit
    enc = host_encoder(2, 1)
    g = torch.Generator().manual_seed(3)

    def t(n=64):
        return torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)

    out = torch.full((4096,), 0xA5, dtype=torch.uint8)
    audit.audit_chunks_device(enc, [], [0, 1], d_chunks=out, d_hex=out, chunk_count=4)
    audit.audit_chunks_device(enc, (), [0, 1], d_hex=out)
    with pytest.raises(cess_amd.ErrInvalidInput):
        audit.audit_chunks_device(enc, [t(), None], [0], d_hex=out, chunk_count=4)
    with pytest.raises(cess_amd.ErrInvalidInput):
        audit.audit_chunks_device(enc, [None], [0], d_chunks=out, chunk_count=4)
    with pytest.raises(cess_amd.ErrShardSize):
        audit.audit_chunks_device(enc, [t(), t(32)], [0], d_hex=out, chunk_count=4)
    with pytest.raises(cess_amd.ErrShardNoData):
        audit.audit_chunks_device(enc, [t(0)], [0], d_hex=out, chunk_count=4)
    with pytest.raises(cess_amd.ErrShardNoData):
        audit.audit_chunks_device(enc, [t(0), t(0)], [0], d_chunks=out, chunk_count=4)
    assert bool((out == 0xA5).all())


def test_new_kernels_use_no_scratch():
    """The table-addressed gather (both column widths), the chunk address expansion and the
    argument-block queue add: no private segment (the 2 KiB argument array is indexed in the
    kernarg segment, not copied) and no spilled register."""
    from cess_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sha_slots
    res = sha_slots.kernel_resources(_lib.LIB_PATH)
    for pat, count in (("k_chunk_gather_tab", 2), ("k_chunk_addrs", 1), ("k_hashq_add_concat", 1)):
        ks = {n: r for n, r in res.items() if pat in n}
        assert len(ks) == count, (pat, sorted(ks))
        for n, r in ks.items():
            assert int(r["private_segment_fixed_size"]) == 0, (n, r["private_segment_fixed_size"])
            assert int(r["vgpr_spill_count"]) == 0 and int(r["sgpr_spill_count"]) == 0, n
    # the batch call's instantiations are what they were: two, by column width
    assert len([n for n in res if "k_chunk_gather" in n and "_tab" not in n]) == 2
