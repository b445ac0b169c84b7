"""cec_locate_rows, cec_locate_host and cec_locate_ptrs at every boundary (CPU): the header, the
ctypes table, the Rust externs and wrappers, the built library's exports, the refusals that need
no device, the Python surface over them, and the CEC_LOCATE_* values, which add nothing to the
CEC_FLAG_* list."""
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
    "cec_locate_rows": ("i32", ["i32", "i32", "ptr", "i32", "ptr", "ptr"]),
    "cec_locate_host": ("i32", ["i32", "i32", "ptr", "u64", "i32", "ptr", "ptr"]),
    "cec_locate_ptrs": ("i32", ["ptr", "ptr", "u64", "u64", "i32", "ptr", "ptr", "ptr"]),
}
VALUES = {"CEC_LOCATE_SYN_MAX": 4, "CEC_LOCATE_CLEAN": 0, "CEC_LOCATE_FOUND": 1,
          "CEC_LOCATE_AMBIGUOUS": 2, "CEC_LOCATE_UNCHECKED": 3}


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_declared_in_header_ctypes_and_rust(name):
    from cess_amd import _lib
    from tests.test_boundary import ctypes_prototypes
    protos = header_prototypes()
    assert name in protos, "not in include/cess_ec.h"
    assert protos[name] == PROTOS[name]
    assert name in _lib.SIGNATURES, "not in cess_amd/_lib.SIGNATURES"
    assert ctypes_prototypes({name: _lib.SIGNATURES[name]})[name] == PROTOS[name]
    assert name in rust_prototypes(), "not in the Rust externs"
    assert rust_prototypes()[name] == PROTOS[name]


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_library_exports(name):
    from cess_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name)
    assert len(getattr(lib, name).argtypes) == len(PROTOS[name][1])


def test_locate_defines():
    import cess_amd
    from cess_amd import _lib
    with open(ROOT + "/include/cess_ec.h") as f:
        hdr = f.read()
    values = {k: int(v) for k, v in re.findall(r"#define\s+(CEC_LOCATE_\w+)\s+(\d+)", hdr)}
    assert values == VALUES
    for name, v in VALUES.items():
        assert getattr(_lib, name) == v and getattr(cess_amd, name) == v
        assert name in cess_amd.__all__
    with open(ROOT + "/utils/ec-hip/src/lib.rs") as f:
        rust = f.read()
    for name, v in VALUES.items():
        assert re.search(r"pub const %s: c_int = %d;" % (name, v), rust), name
    # the flag list the repairs pin is as it was
    assert sorted(re.findall(r"#define\s+(CEC_FLAG_\w+)", hdr)) == [
        "CEC_FLAG_CLEAN", "CEC_FLAG_LOST", "CEC_FLAG_MANY", "CEC_FLAG_MULTI_MAX",
        "CEC_FLAG_REBUILT"]
    # the rule's header has no HIP types and is a dependency of the units that include it
    with open(ROOT + "/cess_amd/csrc/Makefile") as f:
        mk = f.read()
    for target in ("kernels.o", "kernels_tune.o", "cess_ec.o", "cess_ec_tune.o"):
        rule = re.search(r"^\$\(OBJDIR\)/%s:(.*)$" % re.escape(target), mk, re.M).group(1)
        assert "locate_rule.h" in rule.split(), target
    with open(ROOT + "/cess_amd/csrc/locate_rule.h") as f:
        txt = f.read()
    assert not re.search(r"#include\s*<hip|hipStream_t|__global__|__shared__", txt)


def test_rust_crate_has_wrappers():
    with open(ROOT + "/utils/ec-hip/src/lib.rs") as f:
        txt = f.read()
    assert re.search(r"pub unsafe fn locate_ptrs\(", txt)
    assert re.search(r"pub fn locate_rows\(", txt)
    assert re.search(r"pub fn locate_host\(", txt)


def test_refusals_without_gpu():
    """A NULL codec is refused before anything touches a device, whatever else is passed."""
    from cess_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 128)()
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 3)(p, p + 16, p + 32)
    fn = lib.cec_locate_ptrs
    assert fn(None, ptrs, 1, 16, 2, p + 48, p + 56, None) == _lib.CEC_EINVAL
    assert fn(None, ptrs, 1, 0, 2, p + 48, p + 56, None) == _lib.CEC_EINVAL
    assert fn(None, ptrs, 1, 16, 0, p + 48, p + 56, None) == _lib.CEC_EINVAL
    assert fn(None, None, 0, 16, 2, None, None, None) == _lib.CEC_EINVAL
    assert not any(buf)


def test_host_refusals():
    from cess_amd import _lib
    lib = _lib.load()
    r, st, found = ctypes.c_int(9), ctypes.c_int(9), ctypes.c_int(9)
    held = (ctypes.c_uint8 * 6)(1, 1, 1, 1, 1, 1)
    rows = (ctypes.c_uint8 * 24)(*([7] * 24))
    rp, sp, fp = ctypes.byref(r), ctypes.byref(st), ctypes.byref(found)
    fn = lib.cec_locate_rows
    assert fn(4, 2, None, 2, rp, rows) == _lib.CEC_EINVAL
    assert fn(4, 2, held, 2, None, rows) == _lib.CEC_EINVAL
    assert fn(4, 2, held, 2, rp, None) == _lib.CEC_EINVAL
    assert fn(4, 2, held, 0, rp, rows) == _lib.CEC_EINVAL
    assert fn(4, 2, held, 5, rp, rows) == _lib.CEC_EINVAL
    assert fn(0, 2, held, 2, rp, rows) == _lib.CEC_EINVAL
    assert fn(4, 0, held, 2, rp, rows) == _lib.CEC_EINVAL
    assert fn(200, 57, held, 2, rp, rows) == _lib.CEC_EINVAL
    assert r.value == 9 and list(rows) == [7] * 24
    assert fn(4, 2, held, 4, rp, rows) == 0 and r.value == 2
    assert any(rows[:12]) and not any(rows[12:])  # written whole: rows past r are zero
    bufs = [np.zeros(8, np.uint8) for _ in range(6)]
    ptrs = (ctypes.c_void_p * 6)(*[b.ctypes.data for b in bufs])
    fn = lib.cec_locate_host
    assert fn(4, 2, None, 8, 2, sp, fp) == _lib.CEC_EINVAL
    assert fn(4, 2, ptrs, 8, 2, None, fp) == _lib.CEC_EINVAL
    assert fn(4, 2, ptrs, 8, 2, sp, None) == _lib.CEC_EINVAL
    assert fn(4, 2, ptrs, 8, 0, sp, fp) == _lib.CEC_EINVAL
    assert fn(4, 2, ptrs, 8, 5, sp, fp) == _lib.CEC_EINVAL
    assert fn(0, 2, ptrs, 8, 2, sp, fp) == _lib.CEC_EINVAL
    assert fn(200, 57, ptrs, 8, 2, sp, fp) == _lib.CEC_EINVAL
    assert st.value == 9 and found.value == 9
    assert fn(4, 2, ptrs, 8, 2, sp, fp) == 0 and (st.value, found.value) == (0, -1)


def test_python_surface():
    import cess_amd
    from cess_amd import _lib, audit
    sig = inspect.signature(cess_amd.Encoder.LocateDevice)
    assert list(sig.parameters) == ["self", "segments", "nsyn", "d_flags", "d_status", "stream"]
    assert sig.parameters["nsyn"].default == _lib.CEC_LOCATE_SYN_MAX
    for name in ("d_flags", "d_status", "stream"):
        assert sig.parameters[name].default is None
    sig = inspect.signature(audit.locate_repair_device)
    assert list(sig.parameters) == ["enc", "segments", "nsyn", "recorded", "queue"]
    assert sig.parameters["nsyn"].default == _lib.CEC_LOCATE_SYN_MAX
    assert sig.parameters["recorded"].default is None and sig.parameters["queue"].default is None
    sig = inspect.signature(audit.scrub_located_device)
    assert list(sig.parameters) == ["enc", "segments", "recorded", "nsyn", "queue"]
    assert sig.parameters["nsyn"].default == _lib.CEC_LOCATE_SYN_MAX
    assert list(inspect.signature(cess_amd.locate_rows).parameters) == [
        "data_shards", "parity_shards", "held", "nsyn"]
    assert list(inspect.signature(cess_amd.locate_host).parameters) == [
        "data_shards", "parity_shards", "shards", "nsyn"]
    assert "locate_rows" in cess_amd.__all__ and "locate_host" in cess_amd.__all__
    # RS(2,2), all held: u = 1 / (i ^ i') products over the points 0..3; row 1 is u_i * i
    r, rows = cess_amd.locate_rows(2, 2, [1, 1, 1, 1], 4)
    assert r == 2 and rows.shape == (2, 4) and rows[1, 0] == 0 and (rows[0] != 0).all()
    assert cess_amd.locate_rows(2, 2, [1, 0, 1, 1], 4)[0] == 1
    assert cess_amd.locate_rows(2, 2, [1, 0, 1, 0], 4)[0] == 0
    z = [np.zeros(4, np.uint8) for _ in range(4)]
    assert cess_amd.locate_host(2, 2, z, 2) == (cess_amd.CEC_LOCATE_CLEAN, -1)
    bad = [a.copy() for a in z]
    bad[3][2] = 0x40
    assert cess_amd.locate_host(2, 2, bad, 2) == (cess_amd.CEC_LOCATE_FOUND, 3)
    assert cess_amd.locate_host(2, 2, bad[:2] + [None, bad[3]], 2) == (
        cess_amd.CEC_LOCATE_AMBIGUOUS, -1)
    assert cess_amd.locate_host(2, 2, [None, None] + bad[2:], 2) == (
        cess_amd.CEC_LOCATE_UNCHECKED, -1)
    with pytest.raises(cess_amd.CecError):
        cess_amd.locate_rows(2, 2, [1, 1, 1, 1], 5)
    with pytest.raises(cess_amd.CecError):
        cess_amd.locate_host(2, 2, z, 0)


def test_locate_kernels_use_no_scratch():
    """k_syn in its seven forms (four locate buckets, three confirm buckets), the planner and the
    finish keep everything in registers: no private segment, no spill, no LDS."""
    from cess_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sha_slots
    res = sha_slots.kernel_resources(_lib.LIB_PATH)
    syn = {n: r for n, r in res.items() if "k_syn" in n}
    assert len(syn) == 7, sorted(syn)
    ks = dict(syn)
    for name in ("k_locate_plan", "k_locate_finish"):
        hit = {n: r for n, r in res.items() if name in n}
        assert len(hit) == 1, (name, sorted(hit))
        ks.update(hit)
    for n, r in ks.items():
        assert int(r["private_segment_fixed_size"]) == 0, (n, r["private_segment_fixed_size"])
        assert int(r["vgpr_spill_count"]) == 0 and int(r["sgpr_spill_count"]) == 0, n
        assert int(r["group_segment_fixed_size"]) == 0, (n, r["group_segment_fixed_size"])
