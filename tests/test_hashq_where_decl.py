"""Checked chains the device admits, and what they prove, at every boundary (CPU):
cec_hashq_add_check_where_ptrs, cec_hashq_where_plan, cec_confirm_rule and cec_confirm_flagged in
the header, the ctypes table, the Rust externs and the built library's exports; their constants in
C, Python and Rust; the refusal of a NULL queue without a device; the Python surface over them;
and the two new kernels' resources."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_boundary import header_prototypes, rust_prototypes

PROTOS = {
    "cec_hashq_add_check_where_ptrs": ("i32", ["ptr", "ptr", "u64", "u64", "ptr", "ptr", "u64",
                                               "ptr", "i32", "ptr", "ptr", "ptr"]),
    "cec_hashq_where_plan": ("i32", ["ptr", "ptr", "u64", "u64", "ptr", "i32", "ptr", "ptr"]),
    "cec_confirm_rule": ("i32", ["i32", "i32", "ptr", "ptr"]),
    "cec_confirm_flagged": ("i32", ["ptr", "ptr", "u64", "i32", "ptr", "ptr"]),
}
CONSTANTS = {"CEC_HASHQ_SKIPPED": 2, "CEC_CONFIRM_NONE": 0, "CEC_CONFIRM_PROVEN": 1,
             "CEC_CONFIRM_REFUTED": 2}


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_declared_in_header_ctypes_and_rust(name):
    from cess_amd import _lib
    protos = header_prototypes()
    assert name in protos, "not in include/cess_ec.h"
    assert protos[name] == PROTOS[name]
    assert name in _lib.SIGNATURES, "not in cess_amd/_lib.SIGNATURES"
    assert len(_lib.SIGNATURES[name][1]) == len(PROTOS[name][1])
    assert name in rust_prototypes(), "not in the Rust externs"
    assert rust_prototypes()[name] == PROTOS[name]


def test_rust_crate_has_wrappers():
    with open(ROOT + "/utils/ec-hip/src/lib.rs") as f:
        txt = f.read()
    assert re.search(r"pub unsafe fn hashq_add_check_where_ptrs\(", txt)
    assert re.search(r"pub unsafe fn confirm_flagged\(", txt)
    assert re.search(r"pub fn confirm_rule\(", txt)


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_library_exports(name):
    from cess_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name)
    assert len(getattr(lib, name).argtypes) == len(PROTOS[name][1])


@pytest.mark.parametrize("name", sorted(CONSTANTS))
def test_constant_in_c_python_and_rust(name):
    import cess_amd
    from cess_amd import _lib
    value = CONSTANTS[name]
    with open(ROOT + "/include/cess_ec.h") as f:
        m = re.search(r"^#define %s (\d+)\b" % name, f.read(), re.M)
    assert m and int(m.group(1)) == value
    assert getattr(_lib, name) == value
    assert getattr(cess_amd, name) == value and name in cess_amd.__all__
    with open(ROOT + "/utils/ec-hip/src/lib.rs") as f:
        m = re.search(r"^pub const %s: \w+ = (\d+);" % name, f.read(), re.M)
    assert m and int(m.group(1)) == value


def test_null_queue_is_refused_without_gpu():
    from cess_amd import _lib
    lib = _lib.load()
    buf = np.zeros(1024, dtype=np.uint8)
    p = buf.ctypes.data
    assert p % 4 == 0
    bufs = (ctypes.c_void_p * 4)(p, None, p + 128, p + 192)
    ticket = ctypes.c_uint64(7)
    # expect, flags, gate bytes, ok, hex: all inside buf, which must stay zero
    assert lib.cec_hashq_add_check_where_ptrs(None, bufs, 4, 64, p + 256, p + 512, 2, p + 520, 1,
                                              p + 528, p + 576,
                                              ctypes.byref(ticket)) == _lib.CEC_EINVAL
    assert lib.cec_hashq_add_check_where_ptrs(None, bufs, 4, 64, p + 256, p + 512, 1, None, 0,
                                              p + 528, None, None) == _lib.CEC_EINVAL
    assert lib.cec_hashq_add_check_where_ptrs(None, None, 0, 0, None, None, 0, None, 0, None,
                                              None, None) == _lib.CEC_EINVAL
    assert ticket.value == 7
    assert not buf.any()


def test_confirm_flagged_validates_before_any_device_call():
    """The refusals and the empty call need no GPU: nothing is enqueued."""
    from cess_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data
    assert lib.cec_confirm_flagged(None, p + 8, 2, 3, p + 32, None) == _lib.CEC_EINVAL
    assert lib.cec_confirm_flagged(p, None, 2, 3, p + 32, None) == _lib.CEC_EINVAL
    assert lib.cec_confirm_flagged(p, p + 8, 2, 3, None, None) == _lib.CEC_EINVAL
    assert lib.cec_confirm_flagged(p, p + 8, 2, -1, p + 32, None) == _lib.CEC_EINVAL
    assert lib.cec_confirm_flagged(None, None, 0, 3, None, None) == _lib.CEC_OK
    assert not buf.any()


def test_python_surface():
    import cess_amd
    from cess_amd import audit
    from cess_amd.hashq import HashQueue
    sig = inspect.signature(HashQueue.add_check_where_ptrs)
    assert list(sig.parameters) == ["self", "tensors", "expect", "d_flags", "per", "d_gate",
                                    "gate", "d_ok", "d_hex"]
    assert [sig.parameters[p].default for p in ("per", "d_gate", "gate", "d_ok", "d_hex")] == \
        [1, None, 0, None, None]
    sig = inspect.signature(cess_amd.confirm_flagged)
    assert list(sig.parameters) == ["d_status", "d_ok", "n", "d_confirm", "stream"]
    assert sig.parameters["d_confirm"].default is None and sig.parameters["stream"].default is None
    assert list(inspect.signature(cess_amd.confirm_rule).parameters) == ["status", "ok"]
    sig = inspect.signature(audit.scrub_repair_confirm_device)
    assert list(sig.parameters) == ["enc", "segments", "recorded", "max_bad", "queue"]
    assert sig.parameters["max_bad"].default == 1 and sig.parameters["queue"].default is None
    for name in ("confirm_flagged", "confirm_rule"):
        assert name in cess_amd.__all__


def test_new_kernels_use_no_scratch_and_spill_nothing():
    from cess_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sha_slots
    res = sha_slots.kernel_resources(_lib.LIB_PATH)
    for kernel in ("k_hashq_admit", "k_confirm_flagged"):
        rows = {n: r for n, r in res.items() if kernel in n}
        assert len(rows) == 1, (kernel, sorted(rows))
        for n, r in rows.items():
            assert int(r["private_segment_fixed_size"]) == 0, (n, r["private_segment_fixed_size"])
            assert int(r["vgpr_spill_count"]) == 0 and int(r["sgpr_spill_count"]) == 0, n
