"""cec_reconstruct_partial_ptrs and cec_xor_ptrs at every boundary (CPU): the header, the ctypes
table, the Rust externs, the built library's exports, and the Encoder methods over them."""
import inspect
import re

import pytest

from tests.conftest import ROOT
from tests.test_boundary import header_prototypes, rust_prototypes

ARITY = {"cec_reconstruct_partial_ptrs": 8, "cec_xor_ptrs": 7}


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
    assert re.search(r"pub unsafe fn reconstruct_partial_device\(", txt)
    assert re.search(r"pub unsafe fn xor_device\(", txt)


@pytest.mark.parametrize("name", sorted(ARITY))
def test_library_exports(name):
    from cess_amd import _lib
    assert hasattr(_lib.load(), name)


@pytest.mark.parametrize("method,params", [
    ("ReconstructPartialDevice", ["self", "shards", "present", "out", "accumulate", "stream"]),
    ("ReconstructPartialDeviceBatch",
     ["self", "segments", "present", "outs", "accumulate", "stream"]),
    ("XorDevice", ["self", "dsts", "srcs", "stream"])])
def test_encoder_methods(method, params):
    from cess_amd.reedsolomon import Encoder
    assert hasattr(Encoder, method)
    sig = inspect.signature(getattr(Encoder, method))
    assert list(sig.parameters) == params
    assert sig.parameters["stream"].default is None
    if "accumulate" in params:
        assert sig.parameters["accumulate"].default is False
    if method == "ReconstructPartialDevice":
        assert sig.parameters["out"].default is None
