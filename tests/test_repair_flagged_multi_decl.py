"""cec_flag_status_multi, cec_flag_solve and cec_repair_flagged_multi_ptrs at every boundary (CPU):
the header, the ctypes table, the Rust externs and wrappers, the built library's exports,
CEC_FLAG_MULTI_MAX in C, Python and Rust, the refusals that need no device, and the Python surface
over them."""
import ctypes
import inspect
import re

import pytest

from tests.conftest import ROOT
from tests.test_boundary import header_prototypes, rust_prototypes

PROTOS = {
    "cec_flag_status_multi": ("i32", ["i32", "i32", "ptr", "ptr", "i32", "ptr", "ptr", "ptr"]),
    "cec_flag_solve": ("i32", ["i32", "i32", "ptr", "ptr", "i32", "ptr", "ptr", "ptr", "ptr",
                               "ptr"]),
    "cec_repair_flagged_multi_ptrs": ("i32", ["ptr", "ptr", "ptr", "u64", "u64", "i32", "ptr",
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


def test_multi_max_everywhere():
    import cess_amd
    from cess_amd import _lib
    with open(ROOT + "/include/cess_ec.h") as f:
        hdr = f.read()
    with open(ROOT + "/utils/ec-hip/src/lib.rs") as f:
        rust = f.read()
    with open(ROOT + "/cess_amd/csrc/flag_solve.h") as f:
        dev = f.read()
    m = re.search(r"#define\s+CEC_FLAG_MULTI_MAX\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 4
    assert _lib.CEC_FLAG_MULTI_MAX == 4
    assert cess_amd.CEC_FLAG_MULTI_MAX == 4 and "CEC_FLAG_MULTI_MAX" in cess_amd.__all__
    m = re.search(r"pub const CEC_FLAG_MULTI_MAX: c_int = (\d+);", rust)
    assert m and int(m.group(1)) == 4
    m = re.search(r"constexpr int kFlagMultiMax = (\d+);", dev)
    assert m and int(m.group(1)) == 4
    # no status value was added
    assert len(re.findall(r"#define\s+CEC_FLAG_(?:CLEAN|REBUILT|MANY|LOST)\s+\d", hdr)) == 4
    assert sorted(re.findall(r"#define\s+(CEC_FLAG_\w+)", hdr)) == [
        "CEC_FLAG_CLEAN", "CEC_FLAG_LOST", "CEC_FLAG_MANY", "CEC_FLAG_MULTI_MAX",
        "CEC_FLAG_REBUILT"]


def test_rust_crate_has_wrappers():
    with open(ROOT + "/utils/ec-hip/src/lib.rs") as f:
        txt = f.read()
    assert re.search(r"pub unsafe fn repair_flagged_multi_ptrs\(", txt)
    assert re.search(r"pub fn flag_status_multi\(", txt)


def test_refusals_without_gpu():
    """A NULL codec is refused before anything touches a device, whatever else is passed."""
    from cess_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 3)(p, p + 16, p + 32)
    fn = lib.cec_repair_flagged_multi_ptrs
    assert fn(None, ptrs, p + 48, 1, 16, 2, p + 56, None) == _lib.CEC_EINVAL
    assert fn(None, None, None, 0, 16, 2, None, None) == _lib.CEC_EINVAL
    assert not any(buf)


def test_python_surface():
    import cess_amd
    from cess_amd import _lib, audit
    sig = inspect.signature(cess_amd.Encoder.RepairFlaggedMultiDevice)
    assert list(sig.parameters) == ["self", "segments", "d_flags", "max_bad", "d_status", "stream"]
    assert sig.parameters["max_bad"].default == _lib.CEC_FLAG_MULTI_MAX
    assert sig.parameters["d_status"].default is None and sig.parameters["stream"].default is None
    # the single-failure form keeps its signature
    sig = inspect.signature(cess_amd.Encoder.RepairFlaggedDevice)
    assert list(sig.parameters) == ["self", "segments", "d_flags", "d_status", "stream"]
    sig = inspect.signature(audit.scrub_repair_multi_device)
    assert list(sig.parameters) == ["enc", "segments", "recorded", "max_bad", "queue"]
    assert sig.parameters["max_bad"].default == _lib.CEC_FLAG_MULTI_MAX
    assert sig.parameters["queue"].default is None
    assert list(inspect.signature(cess_amd.flag_status_multi).parameters) == [
        "data_shards", "parity_shards", "held", "flags", "max_bad"]
    assert "flag_status_multi" in cess_amd.__all__
