"""The checking adds of the hash queue at every boundary (CPU): cec_hashq_add_check and
cec_hashq_add_check_concat_ptrs in the header, the ctypes table, the Rust externs and the built
library's exports; their refusal of a NULL queue without a device; the Python surface over them;
and the chain record, which took the two new pointers in place of its padding and is still one
128-byte record (tests/native/sha_chain_layout.cpp)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_boundary import header_prototypes, rust_prototypes

PROTOS = {
    "cec_hashq_add_check": ("i32", ["ptr", "ptr", "u64", "u64", "u64", "u64", "u64", "ptr", "u64",
                                    "ptr", "u64", "ptr", "u64", "ptr"]),
    "cec_hashq_add_check_concat_ptrs": ("i32", ["ptr", "ptr", "u64", "u64", "u64", "u64", "ptr",
                                                "ptr", "ptr", "ptr", "ptr"]),
}


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


def test_rust_crate_has_wrapper():
    with open(ROOT + "/utils/ec-hip/src/lib.rs") as f:
        txt = f.read()
    assert re.search(r"pub unsafe fn hashq_add_check_concat_ptrs\(", txt)


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_library_exports(name):
    from cess_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name)
    assert len(getattr(lib, name).argtypes) == len(PROTOS[name][1])


def test_null_queue_is_refused_without_gpu():
    from cess_amd import _lib
    lib = _lib.load()
    buf = np.zeros(1024, dtype=np.uint8)
    p = buf.ctypes.data
    assert p % 4 == 0
    parts = (ctypes.c_void_p * 4)(p, p + 64, p + 128, p + 192)
    ticket = ctypes.c_uint64(7)
    assert lib.cec_hashq_add_check(None, p, 4, 2, 128, 64, 64, p + 256, 2, p + 512, 2, p + 576, 2,
                                   ctypes.byref(ticket)) == _lib.CEC_EINVAL
    assert lib.cec_hashq_add_check(None, None, 0, 1, 0, 0, 0, None, 0, None, 0, None, 0,
                                   None) == _lib.CEC_EINVAL
    assert lib.cec_hashq_add_check_concat_ptrs(None, parts, 2, 2, 64, 0, p + 256, p + 512,
                                               p + 576, p + 768,
                                               ctypes.byref(ticket)) == _lib.CEC_EINVAL
    assert lib.cec_hashq_add_check_concat_ptrs(None, parts, 4, 1, 0, 64, p + 256, p + 512, None,
                                               None, None) == _lib.CEC_EINVAL
    assert lib.cec_hashq_add_check_concat_ptrs(None, None, 0, 1, 64, 0, None, None, None, None,
                                               None) == _lib.CEC_EINVAL
    assert ticket.value == 7
    assert not buf.any()


def test_chain_record_is_still_128_bytes(tmp_path):
    """expect and ok stand where the two padding words stood: the record's size, and the offset
    of every field that was there before, are unchanged."""
    exe = tmp_path / "sha_chain_layout"
    subprocess.run(["g++", "-std=c++20", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    f"{ROOT}/tests/native/sha_chain_layout.cpp", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    assert rows[0] == ["sizeof", "128"]
    got = {r[0]: (int(r[1]), int(r[2])) for r in rows[1:]}
    assert got == {"src": (0, 8), "len": (8, 8), "blk": (16, 8), "hex": (24, 8), "h": (32, 32),
                   "pre_hex": (64, 8), "pre_blk": (72, 8), "pre_h": (80, 32),
                   "expect": (112, 8), "ok": (120, 8)}


def test_python_surface():
    from cess_amd import audit, repair
    from cess_amd.hashq import HashQueue
    sig = inspect.signature(HashQueue.add_check)
    assert list(sig.parameters)[:13] == ["self", "d_base", "n", "per", "outer_stride",
                                         "inner_stride", "length", "d_expect", "expect_outer",
                                         "d_ok", "ok_outer", "d_hex", "hex_outer"]
    sig = inspect.signature(HashQueue.add_check_ptrs)
    assert list(sig.parameters) == ["self", "tensors", "expect", "d_ok", "d_hex"]
    assert sig.parameters["d_ok"].default is None and sig.parameters["d_hex"].default is None
    sig = inspect.signature(HashQueue.add_check_concat_ptrs)
    assert list(sig.parameters)[:3] == ["self", "chains", "expect"]
    sig = inspect.signature(audit.scrub_device)
    assert list(sig.parameters) == ["frags", "recorded", "queue", "d_ok"]
    assert sig.parameters["queue"].default is None and sig.parameters["d_ok"].default is None
    sig = inspect.signature(repair.check_batch_device)
    assert list(sig.parameters) == ["queue", "d_data", "d_parity", "nseg", "k", "m", "shard_len",
                                    "expected"]


def test_tick_kernels_are_as_many_and_use_no_scratch():
    """The check sits in the finisher the three tick kernels share: no new kernel, no private
    segment, no spilled register in any instantiation, and still two add kernels."""
    import sys
    from cess_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sha_slots
    res = sha_slots.kernel_resources(_lib.LIB_PATH)
    ticks = {n: r for n, r in res.items() if "k_sha256_tick" in n}
    assert len(ticks) == 4, sorted(ticks)
    for n, r in ticks.items():
        assert int(r["private_segment_fixed_size"]) == 0, (n, r["private_segment_fixed_size"])
        assert int(r["vgpr_spill_count"]) == 0 and int(r["sgpr_spill_count"]) == 0, n
        # the occupancy step the ticks are built for: at most 128 registers, four waves per SIMD
        assert int(r["vgpr_count"]) <= 128, (n, r["vgpr_count"])
    assert len([n for n in res if "k_hashq_add" in n]) == 2
