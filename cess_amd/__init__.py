"""cess_amd: MI355X-native Reed-Solomon codec for CESS's segment -> fragment path.

The compute path is libcessec (HIP kernels for gfx950 behind the C ABI in include/cess_ec.h);
this package is the host-side mirror of the off-chain codec API (klauspost/reedsolomon shape)
plus the CESS segment / fragment records.
"""
from . import audit, geometry, records
from ._lib import (
    CEC_CONFIRM_NONE,
    CEC_CONFIRM_PROVEN,
    CEC_CONFIRM_REFUTED,
    CEC_FLAG_CLEAN,
    CEC_FLAG_LOST,
    CEC_FLAG_MANY,
    CEC_FLAG_MULTI_MAX,
    CEC_FLAG_REBUILT,
    CEC_HASHQ_SKIPPED,
    CEC_LOCATE_AMBIGUOUS,
    CEC_LOCATE_BAD_MAX,
    CEC_LOCATE_CLEAN,
    CEC_LOCATE_FOUND,
    CEC_LOCATE_SYN_MAX,
    CEC_LOCATE_UNCHECKED,
)
from .hashq import HashQueue, sha256_blocks
from .records import ErrTooManySegments
from .reedsolomon import (
    CecError,
    Encoder,
    ErrInvShardNum,
    ErrInvalidInput,
    ErrMaxShardNum,
    ErrReconstructRequired,
    ErrShardNoData,
    ErrShardSize,
    ErrShortData,
    ErrTooFewShards,
    HipError,
    New,
    confirm_flagged,
    confirm_rule,
    decode_rows,
    fill_synthetic,
    flag_status,
    flag_status_multi,
    locate_host,
    locate_multi_host,
    locate_rows,
    read_status,
    sha256_hex_device,
    sha256_hex_host,
    xor_batch,
)

__all__ = [
    "geometry", "CecError", "Encoder", "New", "ErrInvShardNum", "ErrMaxShardNum",
    "ErrReconstructRequired", "ErrShardNoData", "ErrShardSize", "ErrShortData",
    "ErrTooFewShards", "HipError", "fill_synthetic", "sha256_hex_device", "sha256_hex_host",
    "HashQueue", "sha256_blocks", "records", "ErrTooManySegments", "audit", "xor_batch",
    "ErrInvalidInput", "decode_rows", "flag_status", "CEC_FLAG_CLEAN", "CEC_FLAG_REBUILT",
    "CEC_FLAG_MANY", "CEC_FLAG_LOST", "CEC_FLAG_MULTI_MAX", "flag_status_multi",
    "confirm_flagged", "confirm_rule", "CEC_CONFIRM_NONE", "CEC_CONFIRM_PROVEN",
    "CEC_CONFIRM_REFUTED", "CEC_HASHQ_SKIPPED", "read_status",
    "locate_rows", "locate_host", "CEC_LOCATE_SYN_MAX", "CEC_LOCATE_CLEAN", "CEC_LOCATE_FOUND",
    "CEC_LOCATE_AMBIGUOUS", "CEC_LOCATE_UNCHECKED", "locate_multi_host", "CEC_LOCATE_BAD_MAX",
]
