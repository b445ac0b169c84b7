"""cec_locate_multi_host and cec_locate_multi_ptrs at every boundary (CPU): the header, the
ctypes table, the Rust externs and wrappers, the built library's exports, the refusals that need
no device, the Python surface over them, CEC_LOCATE_BAD_MAX, and the resource report of the
k_pair_* kernels."""
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
    "cec_locate_multi_host": ("i32", ["i32", "i32", "ptr", "u64", "i32", "i32", "ptr", "ptr",
                                      "ptr"]),
    "cec_locate_multi_ptrs": ("i32", ["ptr", "ptr", "u64", "u64", "i32", "i32", "ptr", "ptr",
                                      "ptr", "ptr"]),
}


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


def test_bad_max_define_and_rule_header():
    import cess_amd
    from cess_amd import _lib
    with open(ROOT + "/include/cess_ec.h") as f:
        hdr = f.read()
    assert re.findall(r"#define\s+CEC_LOCATE_BAD_MAX\s+\(?(\d+)\)?", hdr) == ["2"]
    assert _lib.CEC_LOCATE_BAD_MAX == 2 and cess_amd.CEC_LOCATE_BAD_MAX == 2
    assert "CEC_LOCATE_BAD_MAX" in cess_amd.__all__ and "locate_multi_host" in cess_amd.__all__
    with open(ROOT + "/utils/ec-hip/src/lib.rs") as f:
        rust = f.read()
    assert re.search(r"pub const CEC_LOCATE_BAD_MAX: c_int = 2;", rust)
    assert re.search(r"pub unsafe fn locate_multi_ptrs\(", rust)
    assert re.search(r"pub fn locate_multi_host\(", rust)
    # the rule's header has no HIP types and is a dependency of the units that include it
    with open(ROOT + "/cess_amd/csrc/Makefile") as f:
        mk = f.read()
    for target in ("kernels.o", "kernels_tune.o", "cess_ec.o", "cess_ec_tune.o"):
        rule = re.search(r"^\$\(OBJDIR\)/%s:(.*)$" % re.escape(target), mk, re.M).group(1)
        assert "locate_multi_rule.h" in rule.split(), target
    with open(ROOT + "/cess_amd/csrc/locate_multi_rule.h") as f:
        txt = f.read()
    assert not re.search(r"#include\s*<hip|hipStream_t|__global__|__shared__", txt)
    assert '#include "locate_rule.h"' in txt


def test_refusals_without_gpu():
    """A NULL codec is refused before anything touches a device, whatever else is passed."""
    from cess_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 128)()
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 3)(p, p + 16, p + 32)
    fn = lib.cec_locate_multi_ptrs
    assert fn(None, ptrs, 1, 16, 4, 2, p + 48, p + 56, p + 64, None) == _lib.CEC_EINVAL
    assert fn(None, ptrs, 1, 16, 4, 2, p + 48, p + 56, None, None) == _lib.CEC_EINVAL
    assert fn(None, ptrs, 1, 0, 4, 2, p + 48, p + 56, p + 64, None) == _lib.CEC_EINVAL
    assert fn(None, ptrs, 1, 16, 4, 0, p + 48, p + 56, p + 64, None) == _lib.CEC_EINVAL
    assert fn(None, ptrs, 1, 16, 4, 3, p + 48, p + 56, p + 64, None) == _lib.CEC_EINVAL
    assert fn(None, None, 0, 16, 4, 2, None, None, None, None) == _lib.CEC_EINVAL
    assert not any(buf)


def test_host_refusals():
    from cess_amd import _lib
    lib = _lib.load()
    st, nf = ctypes.c_int(9), ctypes.c_int(9)
    found = (ctypes.c_int * 2)(9, 9)
    sp, np_ = ctypes.byref(st), ctypes.byref(nf)
    bufs = [np.zeros(8, np.uint8) for _ in range(8)]
    ptrs = (ctypes.c_void_p * 8)(*[b.ctypes.data for b in bufs])
    fn = lib.cec_locate_multi_host
    assert fn(4, 4, None, 8, 4, 2, sp, np_, found) == _lib.CEC_EINVAL
    assert fn(4, 4, ptrs, 8, 4, 2, None, np_, found) == _lib.CEC_EINVAL
    assert fn(4, 4, ptrs, 8, 4, 2, sp, None, found) == _lib.CEC_EINVAL
    assert fn(4, 4, ptrs, 8, 4, 2, sp, np_, None) == _lib.CEC_EINVAL
    assert fn(4, 4, ptrs, 8, 0, 2, sp, np_, found) == _lib.CEC_EINVAL
    assert fn(4, 4, ptrs, 8, 5, 2, sp, np_, found) == _lib.CEC_EINVAL
    assert fn(4, 4, ptrs, 8, 4, 0, sp, np_, found) == _lib.CEC_EINVAL
    assert fn(4, 4, ptrs, 8, 4, 3, sp, np_, found) == _lib.CEC_EINVAL
    assert fn(0, 4, ptrs, 8, 4, 2, sp, np_, found) == _lib.CEC_EINVAL
    assert fn(200, 57, ptrs, 8, 4, 2, sp, np_, found) == _lib.CEC_EINVAL
    assert (st.value, nf.value, list(found)) == (9, 9, [9, 9])
    assert fn(4, 4, ptrs, 8, 4, 2, sp, np_, found) == 0
    assert (st.value, nf.value, list(found)) == (0, 0, [-1, -1])


def test_python_surface():
    import cess_amd
    from cess_amd import _lib, audit
    sig = inspect.signature(cess_amd.Encoder.LocateMultiDevice)
    assert list(sig.parameters) == ["self", "segments", "nsyn", "max_bad", "d_flags", "d_status",
                                    "d_nbad", "stream"]
    assert sig.parameters["nsyn"].default == _lib.CEC_LOCATE_SYN_MAX == 4
    assert sig.parameters["max_bad"].default == _lib.CEC_LOCATE_BAD_MAX == 2
    for name in ("d_flags", "d_status", "d_nbad", "stream"):
        assert sig.parameters[name].default is None
    sig = inspect.signature(audit.locate_repair_multi_device)
    assert list(sig.parameters) == ["enc", "segments", "max_bad", "nsyn", "recorded", "queue"]
    assert sig.parameters["max_bad"].default == 2 and sig.parameters["nsyn"].default == 4
    assert sig.parameters["recorded"].default is None and sig.parameters["queue"].default is None
    assert list(inspect.signature(cess_amd.locate_multi_host).parameters) == [
        "data_shards", "parity_shards", "shards", "nsyn", "max_bad"]
    # the existing calls keep their signatures
    assert list(inspect.signature(cess_amd.Encoder.LocateDevice).parameters) == [
        "self", "segments", "nsyn", "d_flags", "d_status", "stream"]
    assert list(inspect.signature(audit.locate_repair_device).parameters) == [
        "enc", "segments", "nsyn", "recorded", "queue"]
    # RS(2,4), all zero is a codeword: errors placed by hand
    z = [np.zeros(4, np.uint8) for _ in range(6)]
    assert cess_amd.locate_multi_host(2, 4, z, 4, 2) == (cess_amd.CEC_LOCATE_CLEAN, [])
    bad = [a.copy() for a in z]
    bad[0][1] = 0x40
    assert cess_amd.locate_multi_host(2, 4, bad, 4, 2) == (cess_amd.CEC_LOCATE_FOUND, [0])
    bad[5][3] = 0x07
    assert cess_amd.locate_multi_host(2, 4, bad, 4, 2) == (cess_amd.CEC_LOCATE_FOUND, [0, 5])
    assert cess_amd.locate_multi_host(2, 4, bad, 4, 1) == (cess_amd.CEC_LOCATE_AMBIGUOUS, [])
    assert cess_amd.locate_multi_host(2, 4, bad, 3, 2) == (cess_amd.CEC_LOCATE_AMBIGUOUS, [])
    assert cess_amd.locate_multi_host(2, 4, bad[:2] + [None] + bad[3:], 4, 2) == (
        cess_amd.CEC_LOCATE_AMBIGUOUS, [])
    assert cess_amd.locate_multi_host(2, 4, [None] * 4 + bad[4:], 4, 2) == (
        cess_amd.CEC_LOCATE_UNCHECKED, [])
    with pytest.raises(cess_amd.CecError):
        cess_amd.locate_multi_host(2, 4, z, 4, 3)
    with pytest.raises(cess_amd.CecError):
        cess_amd.locate_multi_host(2, 4, z, 0, 2)


def test_pair_kernels_use_no_scratch():
    """Every k_pair_* kernel keeps everything in registers: no private segment, no spill, no LDS.
    The syndrome product has eight forms (four locate buckets, three T buckets, one U bucket)."""
    from cess_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sha_slots
    res = sha_slots.kernel_resources(_lib.LIB_PATH)
    ks = {n: r for n, r in res.items() if "k_pair_" in n}
    assert len([n for n in ks if "k_pair_syn" in n]) == 8, sorted(ks)
    for name in ("k_pair_plan", "k_pair_finish"):
        assert len([n for n in ks if name in n]) == 1, (name, sorted(ks))
    for n, r in ks.items():
        assert int(r["private_segment_fixed_size"]) == 0, (n, r["private_segment_fixed_size"])
        assert int(r["vgpr_spill_count"]) == 0 and int(r["sgpr_spill_count"]) == 0, n
        assert int(r["group_segment_fixed_size"]) == 0, (n, r["group_segment_fixed_size"])
