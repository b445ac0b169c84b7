"""cec_verify_ptrs is declared at every boundary (the C header, the ctypes table, the Rust crate's
externs; tests/test_boundary.py compares their arguments) and the Encoder has its Python forms.
No GPU needed."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_declared_in_header_ctypes_and_rust():
    from cess_amd import _lib
    assert re.search(r"\bint\s+cec_verify_ptrs\s*\(", read("include", "cess_ec.h"))
    assert re.search(r"\bpub fn cec_verify_ptrs\s*\(", read("utils", "ec-hip", "src", "lib.rs"))
    assert "cec_verify_ptrs" in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES["cec_verify_ptrs"]
    assert len(argtypes) == 7  # codec, src, expect, nseg, shard_len, d_ok, hip_stream


def test_library_exports_the_symbol():
    from cess_amd import _lib
    assert hasattr(_lib.load(), "cec_verify_ptrs")


def test_encoder_has_the_device_forms():
    from cess_amd.reedsolomon import Encoder
    assert list(inspect.signature(Encoder.VerifyDevice).parameters) == ["self", "shards", "stream"]
    assert list(inspect.signature(Encoder.VerifyDeviceBatch).parameters) == [
        "self", "segments", "check", "d_ok", "stream"]
