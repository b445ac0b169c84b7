"""cec_read_status, cec_read_solve and cec_read_flagged_ptrs at every boundary (CPU): the header,
the ctypes table, the Rust externs and wrappers, the built library's exports, the refusals that
need no device, the Python surface over them, and the CEC_FLAG_* defines, which the read adds
nothing to."""
import ctypes
import inspect
import re

import pytest

from tests.conftest import ROOT
from tests.test_boundary import header_prototypes, rust_prototypes

PROTOS = {
    "cec_read_status": ("i32", ["i32", "i32", "ptr", "ptr", "ptr", "i32", "ptr", "ptr", "ptr"]),
    "cec_read_solve": ("i32", ["i32", "i32", "ptr", "ptr", "ptr", "i32", "ptr", "ptr", "ptr",
                               "ptr", "ptr", "ptr", "ptr"]),
    "cec_read_flagged_ptrs": ("i32", ["ptr", "ptr", "ptr", "ptr", "u64", "u64", "i32", "ptr",
                                      "ptr"]),
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


def test_flag_defines_unchanged():
    with open(ROOT + "/include/cess_ec.h") as f:
        hdr = f.read()
    assert sorted(re.findall(r"#define\s+(CEC_FLAG_\w+)", hdr)) == [
        "CEC_FLAG_CLEAN", "CEC_FLAG_LOST", "CEC_FLAG_MANY", "CEC_FLAG_MULTI_MAX",
        "CEC_FLAG_REBUILT"]
    values = dict(re.findall(r"#define\s+(CEC_FLAG_\w+)\s+(\d+)", hdr))
    assert values == {"CEC_FLAG_CLEAN": "0", "CEC_FLAG_REBUILT": "1", "CEC_FLAG_MANY": "2",
                      "CEC_FLAG_LOST": "3", "CEC_FLAG_MULTI_MAX": "4"}
    # the shared header without HIP types is a dependency of both units that include it
    with open(ROOT + "/cess_amd/csrc/Makefile") as f:
        mk = f.read()
    for target in ("kernels.o", "kernels_tune.o", "cess_ec.o", "cess_ec_tune.o"):
        rule = re.search(r"^\$\(OBJDIR\)/%s:(.*)$" % re.escape(target), mk, re.M).group(1)
        assert "read_plan.h" in rule.split(), target
    with open(ROOT + "/cess_amd/csrc/read_plan.h") as f:
        txt = f.read()
    assert not re.search(r"#include\s*<hip|hipStream_t|__global__|__shared__", txt)


def test_rust_crate_has_wrappers():
    with open(ROOT + "/utils/ec-hip/src/lib.rs") as f:
        txt = f.read()
    assert re.search(r"pub unsafe fn read_flagged_ptrs\(", txt)
    assert re.search(r"pub fn read_status\(", txt)


def test_refusals_without_gpu():
    """A NULL codec is refused before anything touches a device, whatever else is passed."""
    from cess_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 128)()
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 3)(p, p + 16, p + 32)
    dst = (ctypes.c_void_p * 2)(p + 64, p + 80)
    fn = lib.cec_read_flagged_ptrs
    assert fn(None, ptrs, p + 48, dst, 1, 16, 2, p + 56, None) == _lib.CEC_EINVAL
    assert fn(None, ptrs, p + 48, dst, 1, 0, 2, p + 56, None) == _lib.CEC_EINVAL
    assert fn(None, None, None, None, 0, 16, 2, None, None) == _lib.CEC_EINVAL
    assert not any(buf)


def test_host_refusals():
    from cess_amd import _lib
    lib = _lib.load()
    st, nm, nc = ctypes.c_int(9), ctypes.c_int(9), ctypes.c_int(9)
    buf = (ctypes.c_uint8 * 6)(1, 1, 1, 1, 1, 1)
    miss = (ctypes.c_uint8 * 4)()
    sp, mp, cp = ctypes.byref(st), ctypes.byref(nm), ctypes.byref(nc)
    fn = lib.cec_read_status
    assert fn(4, 2, None, buf, buf, 2, sp, mp, miss) == _lib.CEC_EINVAL
    assert fn(4, 2, buf, None, buf, 2, sp, mp, miss) == _lib.CEC_EINVAL
    assert fn(4, 2, buf, buf, None, 2, sp, mp, miss) == _lib.CEC_EINVAL
    assert fn(4, 2, buf, buf, buf, 2, None, mp, miss) == _lib.CEC_EINVAL
    assert fn(4, 2, buf, buf, buf, 2, sp, None, miss) == _lib.CEC_EINVAL
    assert fn(4, 2, buf, buf, buf, 0, sp, mp, miss) == _lib.CEC_EINVAL
    assert fn(4, 2, buf, buf, buf, 5, sp, mp, miss) == _lib.CEC_EINVAL
    assert fn(0, 2, buf, buf, buf, 2, sp, mp, miss) == _lib.CEC_EINVAL
    assert fn(4, 0, buf, buf, buf, 2, sp, mp, miss) == _lib.CEC_EINVAL
    assert fn(200, 57, buf, buf, buf, 2, sp, mp, miss) == _lib.CEC_EINVAL
    assert st.value == 9 and nm.value == 9
    assert fn(4, 2, buf, buf, buf, 2, sp, mp, None) == 0 and st.value == 0  # miss is optional
    sv = lib.cec_read_solve
    assert sv(4, 2, buf, buf, buf, 0, sp, mp, None, None, None, None, cp) == _lib.CEC_EINVAL
    assert sv(4, 2, buf, buf, None, 2, sp, mp, None, None, None, None, cp) == _lib.CEC_EINVAL
    assert sv(4, 2, buf, buf, buf, 2, sp, mp, None, None, None, None, None) == _lib.CEC_EINVAL
    assert sv(4, 2, buf, buf, buf, 2, sp, mp, None, None, None, None, cp) == 0
    assert nc.value == 4  # the arrays are optional; every data shard is copied


def test_python_surface():
    import cess_amd
    from cess_amd import _lib, retrieve
    sig = inspect.signature(cess_amd.Encoder.ReadFlaggedDevice)
    assert list(sig.parameters) == ["self", "segments", "d_flags", "out", "max_bad", "wanted",
                                    "d_status", "stream"]
    assert sig.parameters["max_bad"].default == _lib.CEC_FLAG_MULTI_MAX
    for name in ("wanted", "d_status", "stream"):
        assert sig.parameters[name].default is None
    sig = inspect.signature(retrieve.read_segments_device)
    assert list(sig.parameters) == ["enc", "segments", "recorded", "seg_recorded", "out",
                                    "max_bad", "queue"]
    assert sig.parameters["max_bad"].default == 1
    for name in ("seg_recorded", "out", "queue"):
        assert sig.parameters[name].default is None
    assert list(inspect.signature(cess_amd.read_status).parameters) == [
        "data_shards", "parity_shards", "held", "flags", "wanted", "max_bad"]
    assert "read_status" in cess_amd.__all__
    assert cess_amd.read_status(4, 2, [1, 1, 0, 1, 1, 1], [1, 0, 9, 1, 1, 1], [1] * 4, 2) == \
        (cess_amd.CEC_FLAG_REBUILT, [1, 2])
    assert cess_amd.read_status(4, 2, [1, 1, 0, 1, 1, 1], [1, 0, 9, 1, 1, 1], [1, 0, 0, 1], 1) == \
        (cess_amd.CEC_FLAG_CLEAN, [])
    assert cess_amd.read_status(4, 2, [1, 1, 0, 1, 1, 1], [1, 0, 9, 1, 1, 1], [1] * 4, 1) == \
        (cess_amd.CEC_FLAG_MANY, [])
    with pytest.raises(cess_amd.CecError):
        cess_amd.read_status(4, 2, [1] * 6, [1] * 6, [1] * 4, 5)
    # the retriever keeps its surface
    assert hasattr(retrieve, "Retriever") and hasattr(retrieve, "retrieve_file")
