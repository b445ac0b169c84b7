"""cec_flag_status and cec_repair_flagged_ptrs at every boundary (CPU): the header, the ctypes
table, the Rust externs and wrapper, the built library's exports, the CEC_FLAG_* values in C,
Python and Rust, the refusals that need no device, and the Python surface over them."""
import ctypes
import inspect
import re

import pytest

from tests.conftest import ROOT
from tests.test_boundary import header_prototypes, rust_prototypes

PROTOS = {
    "cec_flag_status": ("i32", ["i32", "i32", "ptr", "ptr", "ptr", "ptr"]),
    "cec_repair_flagged_ptrs": ("i32", ["ptr", "ptr", "ptr", "u64", "u64", "ptr", "ptr"]),
}
FLAGS = {"CEC_FLAG_CLEAN": 0, "CEC_FLAG_REBUILT": 1, "CEC_FLAG_MANY": 2, "CEC_FLAG_LOST": 3}


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


def test_flag_values_everywhere():
    import cess_amd
    from cess_amd import _lib
    with open(ROOT + "/include/cess_ec.h") as f:
        hdr = f.read()
    with open(ROOT + "/utils/ec-hip/src/lib.rs") as f:
        rust = f.read()
    for name, val in FLAGS.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, hdr)
        assert m and int(m.group(1)) == val, name
        assert getattr(_lib, name) == val
        assert getattr(cess_amd, name) == val and name in cess_amd.__all__
        m = re.search(r"pub const %s: c_int = (\d+);" % name, rust)
        assert m and int(m.group(1)) == val, name


def test_rust_crate_has_wrappers():
    with open(ROOT + "/utils/ec-hip/src/lib.rs") as f:
        txt = f.read()
    assert re.search(r"pub unsafe fn repair_flagged_ptrs\(", txt)
    assert re.search(r"pub fn flag_status\(", txt)


def test_refusals_without_gpu():
    """A NULL codec is refused before anything touches a device, whatever else is passed."""
    from cess_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 3)(p, p + 16, p + 32)
    assert lib.cec_repair_flagged_ptrs(None, ptrs, p + 48, 1, 16, p + 56, None) == _lib.CEC_EINVAL
    assert lib.cec_repair_flagged_ptrs(None, None, None, 0, 16, None, None) == _lib.CEC_EINVAL
    assert not any(buf)


def test_python_surface():
    import cess_amd
    from cess_amd import audit, repair
    sig = inspect.signature(cess_amd.Encoder.RepairFlaggedDevice)
    assert list(sig.parameters) == ["self", "segments", "d_flags", "d_status", "stream"]
    assert sig.parameters["d_status"].default is None and sig.parameters["stream"].default is None
    sig = inspect.signature(audit.scrub_repair_device)
    assert list(sig.parameters) == ["enc", "segments", "recorded", "queue"]
    assert sig.parameters["queue"].default is None
    assert "scrubs again" in audit.scrub_repair_device.__doc__
    assert "scrub_repair_device" in repair.check_batch_device.__doc__
    assert list(inspect.signature(cess_amd.flag_status).parameters) == [
        "data_shards", "parity_shards", "held", "flags"]
