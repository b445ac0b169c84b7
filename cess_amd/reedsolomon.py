"""klauspost/reedsolomon-shaped encoder over libcessec (MI355X).

This mirrors the off-chain codec API whose outputs the CESS chain records:
`New(k, m)` returns an Encoder with Encode / EncodeIdx / Update / Verify / Reconstruct /
ReconstructData / ReconstructSome / Split / Join, the same argument meaning and the same error names (ErrTooFewShards, ErrShardNoData,
ErrShardSize, ErrShortData, ErrInvShardNum, ErrMaxShardNum, ErrReconstructRequired). Shards are
host buffers (numpy uint8 arrays / bytearrays) of equal length; a missing shard is None or empty.

For HBM-resident segment batches use the *Batch methods with device tensors laid out
[nseg][k][shard_len] (data) and [nseg][m][shard_len] (parity).

The reference chain fixes k = 2, m = 1 (primitives/common/src/lib.rs:60-61,
runtime/src/lib.rs:1027) and consumes the fragment hashes in
FileBank::upload_declaration (c-pallets/file-bank/src/lib.rs:423).
"""
from __future__ import annotations

import ctypes
from ctypes import POINTER, byref, c_int, c_uint8, c_void_p
from typing import BinaryIO, List, Optional, Sequence

import numpy as np

from . import _lib


class CecError(Exception):
    """Base error; `code` is the C ABI return code."""

    code = _lib.CEC_EINVAL


class ErrInvShardNum(CecError, ValueError):
    """cannot create Encoder with less than one data shard or less than zero parity shards"""


class ErrMaxShardNum(CecError, ValueError):
    """cannot create Encoder with more than 256 data+parity shards"""


class ErrTooFewShards(CecError, ValueError):
    """too few shards given"""

    code = _lib.CEC_ETOOFEW


class ErrShardNoData(CecError, ValueError):
    """no shard data"""

    code = _lib.CEC_ESHARDLEN


class ErrShardSize(CecError, ValueError):
    """shard sizes do not match"""

    code = _lib.CEC_ESHARDLEN


class ErrShortData(CecError, ValueError):
    """not enough data to fill the number of requested shards"""

    code = _lib.CEC_ESHORTDATA


class ErrReconstructRequired(CecError, ValueError):
    """reconstruction required as one or more required data shards are nil"""


class ErrInvalidInput(CecError, ValueError):
    """invalid input"""


class HipError(CecError, RuntimeError):
    code = _lib.CEC_EHIP


_CODE_TO_EXC = {
    _lib.CEC_ETOOFEW: ErrTooFewShards,
    _lib.CEC_ESHARDLEN: ErrShardSize,
    _lib.CEC_ESHORTDATA: ErrShortData,
    _lib.CEC_EHIP: HipError,
    _lib.CEC_ENOMEM: HipError,
    _lib.CEC_ENODEV: HipError,
    _lib.CEC_ENCCL: HipError,
}


def check(rc: int, what: str = "") -> None:
    if rc == _lib.CEC_OK:
        return
    lib = _lib.load()
    msg = lib.cec_strerror(rc).decode()
    detail = lib.cec_last_error().decode()
    exc = _CODE_TO_EXC.get(rc, CecError)
    e = exc(f"{what}: {msg}" + (f" ({detail})" if detail else ""))
    e.code = rc
    raise e


_check_rc = check  # for methods with a parameter named `check`


def _as_u8(buf) -> np.ndarray:
    if isinstance(buf, np.ndarray):
        if buf.dtype != np.uint8 or not buf.flags.c_contiguous:
            raise TypeError("shards must be contiguous uint8 arrays")
        return buf
    if isinstance(buf, (bytearray, memoryview)):
        return np.frombuffer(buf, dtype=np.uint8)
    raise TypeError(f"unsupported shard type {type(buf)!r}")


def _present(s) -> bool:
    return s is not None and len(s) > 0


def _ptr_array(arrs: Sequence[np.ndarray]):
    return (c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])


def _dev_ptr(t) -> int:
    """Device address of a torch tensor (or an int address)."""
    if isinstance(t, int):
        return t
    if not t.is_cuda or not t.is_contiguous():
        raise TypeError("batch buffers must be contiguous device tensors")
    return t.data_ptr()


def _on_gpu(t, dev):
    """Tensor t, refused unless it lives on the codec's GPU `dev` (_dev_ptr refuses host and
    strided tensors)."""
    if t.device != dev:
        raise TypeError("device shards must live on the codec's GPU")
    return t


def _stream_handle(stream) -> Optional[int]:
    if stream is None:
        return None
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream  # torch.cuda.Stream


class Encoder:
    """One codec bound to one GPU (klauspost Encoder). `tuning=True` binds the tuning build of
    the library (kernel variants for sweeps; never the product path)."""

    def __init__(self, data_shards: int, parity_shards: int, device: int = 0,
                 tuning: bool = False):
        if data_shards <= 0 or parity_shards < 0:
            raise ErrInvShardNum(ErrInvShardNum.__doc__)
        if data_shards + parity_shards > 256:
            raise ErrMaxShardNum(ErrMaxShardNum.__doc__)
        self.DataShards = data_shards
        self.ParityShards = parity_shards
        self.Shards = data_shards + parity_shards
        self.device = device
        self._h = c_void_p()
        self._lib = None
        if parity_shards > 0:
            self._lib = _lib.load(tuning)
            check(self._lib.cec_create(data_shards, parity_shards, device, byref(self._h)), "New")

    # -- lifetime ----------------------------------------------------------------------------
    def close(self) -> None:
        if self._h:
            self._lib.cec_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- helpers -----------------------------------------------------------------------------
    def matrix(self) -> np.ndarray:
        """(k+m) x k encode matrix."""
        out = np.zeros((self.Shards, self.DataShards), dtype=np.uint8)
        if self.ParityShards == 0:
            return np.eye(self.DataShards, dtype=np.uint8)
        check(self._lib.cec_matrix(self._h, out.ctypes.data_as(POINTER(c_uint8))), "matrix")
        return out

    def set_option(self, option: int, value: int) -> None:
        """cec_set_option on this codec only (CEC_OPT_*)."""
        check(self._lib.cec_set_option(self._h, option, value), "set_option")

    def stat(self, which: int) -> int:
        v = ctypes.c_uint64()
        check(self._lib.cec_get_stat(self._h, which, byref(v)), "stat")
        return v.value

    def _check_shards(self, shards, nil_ok: bool) -> int:
        size = next((len(s) for s in shards if _present(s)), 0)
        if size == 0:
            raise ErrShardNoData(ErrShardNoData.__doc__)
        for s in shards:
            n = len(s) if s is not None else 0
            if n != size and (n != 0 or not nil_ok):
                raise ErrShardSize(ErrShardSize.__doc__)
        return size

    # -- klauspost API -----------------------------------------------------------------------
    def Encode(self, shards: List) -> None:
        """Compute parity shards[k:] from data shards[:k] in place."""
        if len(shards) != self.Shards:
            raise ErrTooFewShards(ErrTooFewShards.__doc__)
        size = self._check_shards(shards, nil_ok=False)
        if self.ParityShards == 0:
            return
        arrs = [_as_u8(s) for s in shards]
        check(self._lib.cec_encode(self._h, _ptr_array(arrs), size), "Encode")

    def Verify(self, shards: Sequence) -> bool:
        if len(shards) != self.Shards:
            raise ErrTooFewShards(ErrTooFewShards.__doc__)
        size = self._check_shards(shards, nil_ok=False)
        if self.ParityShards == 0:
            return True
        arrs = [_as_u8(s) for s in shards]
        ok = c_int(0)
        check(self._lib.cec_verify(self._h, _ptr_array(arrs), size, byref(ok)), "Verify")
        return bool(ok.value)

    def _reconstruct(self, shards: List, data_only: bool) -> None:
        if len(shards) != self.Shards:
            raise ErrTooFewShards(ErrTooFewShards.__doc__)
        size = self._check_shards(shards, nil_ok=True)
        present = [_present(s) for s in shards]
        if all(present) or (data_only and all(present[: self.DataShards])):
            return
        if sum(present) < self.DataShards:
            raise ErrTooFewShards(ErrTooFewShards.__doc__)
        for i in range(self.Shards):
            if not present[i] and (i < self.DataShards or not data_only):
                shards[i] = np.zeros(size, dtype=np.uint8)
        arrs = [_as_u8(s) if _present(s) else np.zeros(size, dtype=np.uint8) for s in shards]
        flags = (c_uint8 * self.Shards)(*[1 if p else 0 for p in present])
        check(self._lib.cec_reconstruct(self._h, _ptr_array(arrs), flags, size,
                                          1 if data_only else 0), "Reconstruct")
        for i in range(self.Shards):
            if not present[i] and (i < self.DataShards or not data_only):
                shards[i] = arrs[i]

    def Reconstruct(self, shards: List) -> None:
        """Recreate every missing (None / empty) shard in place."""
        self._reconstruct(shards, data_only=False)

    def ReconstructData(self, shards: List) -> None:
        """Recreate only missing data shards."""
        self._reconstruct(shards, data_only=True)

    def _required_flags(self, required) -> List[bool]:
        """klauspost's `required` argument: Shards flags, or DataShards flags (data shards only)."""
        req = [bool(r) for r in required]
        if len(req) == self.DataShards:
            req += [False] * self.ParityShards
        if len(req) != self.Shards:
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        return req

    def ReconstructSome(self, shards: List, required: Sequence) -> None:
        """klauspost ReconstructSome: recreate only the missing shards flagged in `required`
        (len Shards, or len DataShards to ask for data shards only). Missing shards that were not
        asked for stay None; flags on present shards are ignored. The k survivors are staged in
        HBM as separate buffers and rebuilt by cec_reconstruct_ptrs."""
        if len(shards) != self.Shards:
            raise ErrTooFewShards(ErrTooFewShards.__doc__)
        req = self._required_flags(required)
        size = self._check_shards(shards, nil_ok=True)
        present = [_present(s) for s in shards]
        want = [i for i in range(self.Shards) if req[i] and not present[i]]
        if not want:
            return
        if sum(present) < self.DataShards:
            raise ErrTooFewShards(ErrTooFewShards.__doc__)
        import torch
        dev = torch.device("cuda", self.device)
        flags = (c_uint8 * self.Shards)(*[1 if p else 0 for p in present])
        surv = (c_uint8 * self.DataShards)()
        check(self._lib.cec_survivors(self.DataShards, self.ParityShards, flags, surv),
              "ReconstructSome")
        d_shards: List = [None] * self.Shards
        for i in surv:
            d_shards[i] = torch.from_numpy(_as_u8(shards[i])).to(dev)
        self.ReconstructDevice(d_shards, [i in want for i in range(self.Shards)])
        for i in want:
            shards[i] = d_shards[i].cpu().numpy()

    def EncodeIdx(self, dataShard, idx: int, parity: Sequence) -> None:
        """klauspost EncodeIdx: add data shard `idx`'s contribution to the m parity shards in
        place, parity[o] ^= E[k+o][idx] * dataShard. Feeding every data shard once into zeroed
        parity, in any order, gives Encode's parity (cec_encode_idx)."""
        if not 0 <= idx < self.DataShards:
            raise ErrInvShardNum(ErrInvShardNum.__doc__)
        if len(parity) != self.ParityShards:
            raise ErrTooFewShards(ErrTooFewShards.__doc__)
        if any(p is None for p in parity):
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        if not _present(dataShard):
            raise ErrShardNoData(ErrShardNoData.__doc__)
        if self.ParityShards == 0:
            return
        size = self._check_shards(parity, nil_ok=False)
        if len(dataShard) != size:
            raise ErrShardSize(ErrShardSize.__doc__)
        src = np.frombuffer(dataShard, np.uint8) if isinstance(dataShard, bytes) \
            else _as_u8(dataShard)
        arrs = [_as_u8(p) for p in parity]
        check(self._lib.cec_encode_idx(self._h, src.ctypes.data, idx, _ptr_array(arrs), size),
              "EncodeIdx")

    def Update(self, shards: Sequence, newDatashards: Sequence) -> None:
        """klauspost Update: `shards` is an encoded segment (k + m; an unchanged data shard may
        be None), `newDatashards` the k data shards with None (or empty) for unchanged ones. The
        parity shards are brought up to date in place from the old and new bytes of the changed
        shards only; the data shards are not written (cec_update)."""
        if len(shards) != self.Shards or len(newDatashards) != self.DataShards:
            raise ErrTooFewShards(ErrTooFewShards.__doc__)
        k = self.DataShards
        size = self._check_shards(list(shards) + list(newDatashards), nil_ok=True)
        if any(not _present(p) for p in shards[k:]):
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        changed = [j for j in range(k) if _present(newDatashards[j])]
        if any(not _present(shards[j]) for j in changed):
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        if not changed or self.ParityShards == 0:
            return

        def ro(b):
            return np.frombuffer(b, np.uint8) if isinstance(b, bytes) else _as_u8(b)

        old = {j: ro(shards[j]) for j in changed}
        new = {j: ro(newDatashards[j]) for j in changed}
        par = [_as_u8(p) for p in shards[k:]]
        sh = (c_void_p * self.Shards)(*([old[j].ctypes.data if j in old else None
                                         for j in range(k)] + [p.ctypes.data for p in par]))
        nd = (c_void_p * k)(*[new[j].ctypes.data if j in new else None for j in range(k)])
        check(self._lib.cec_update(self._h, sh, nd, size), "Update")

    def EncodeDevice(self, shards: Sequence, stream=None) -> None:
        """Encode one segment whose k + m shards are separate 1-D uint8 device tensors: the m
        parity tensors are written (cec_encode_ptrs). Enqueued on `stream` (default: torch's
        current stream)."""
        if len(shards) != self.Shards:
            raise ErrTooFewShards(ErrTooFewShards.__doc__)
        size = self._check_device_shards(shards)
        if self.ParityShards == 0:
            return
        k = self.DataShards
        data = (c_void_p * k)(*[_dev_ptr(t) for t in shards[:k]])
        par = (c_void_p * self.ParityShards)(*[_dev_ptr(t) for t in shards[k:]])
        check(self._lib.cec_encode_ptrs(self._h, data, par, 1, size,
                                        self._device_stream(stream)), "EncodeDevice")

    def ReconstructDevice(self, shards: List, required=None, out=None, stream=None) -> None:
        """Rebuild missing shards of one segment held as a list of k + m 1-D uint8 device tensors
        (None = absent) without packing them into one buffer (cec_reconstruct_ptrs). `required`
        (klauspost's flags, see ReconstructSome) limits the rebuild to the flagged missing shards;
        None rebuilds every missing shard. Wanted shards are allocated, or taken from `out` (a
        list or {index: tensor} of device tensors of the shard length), and put into `shards`.
        Enqueued on `stream` (default: torch's current stream)."""
        import torch
        if len(shards) != self.Shards:
            raise ErrTooFewShards(ErrTooFewShards.__doc__)
        size = self._check_device_shards([s for s in shards if s is not None])
        req = [True] * self.Shards if required is None else self._required_flags(required)
        want = [i for i in range(self.Shards) if shards[i] is None and req[i]]
        if not want:
            return
        if sum(s is not None for s in shards) < self.DataShards:
            raise ErrTooFewShards(ErrTooFewShards.__doc__)
        dev = torch.device("cuda", self.device)
        outs = {}
        for i in want:
            t = None
            if out is not None:
                t = out.get(i) if isinstance(out, dict) else out[i]
            if t is None:
                t = torch.empty(size, dtype=torch.uint8, device=dev)
            elif t.dtype != torch.uint8 or t.dim() != 1 or t.numel() != size:
                raise ErrShardSize(ErrShardSize.__doc__)
            outs[i] = t
        src = (c_void_p * self.Shards)(*[None if s is None else _dev_ptr(s) for s in shards])
        dst = (c_void_p * self.Shards)(*[_dev_ptr(outs[i]) if i in outs else None
                                         for i in range(self.Shards)])
        check(self._lib.cec_reconstruct_ptrs(self._h, src, dst, 1, size,
                                             self._device_stream(stream)), "ReconstructDevice")
        for i, t in outs.items():
            shards[i] = t

    def VerifyDevice(self, shards: Sequence, stream=None) -> bool:
        """klauspost Verify on one segment whose k + m shards are separate 1-D uint8 device
        tensors: True when the m parity tensors equal the encode of the k data tensors. Nothing is
        written or copied (cec_verify_ptrs). Enqueued on `stream` (default: torch's current
        stream, or a raw integer handle, 0 = the null stream), which is then synchronised to
        read the flag. The flag's byte is allocated on that stream too."""
        import torch
        if len(shards) != self.Shards:
            raise ErrTooFewShards(ErrTooFewShards.__doc__)
        if any(s is None for s in shards):
            raise ErrShardNoData(ErrShardNoData.__doc__)
        self._check_device_shards(shards)
        if self.ParityShards == 0:
            return True
        dev = torch.device("cuda", self.device)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        elif isinstance(stream, int):
            stream = (torch.cuda.ExternalStream(stream, device=dev) if stream
                      else torch.cuda.default_stream(dev))
        with torch.cuda.stream(stream):  # the allocator hands out a block of that stream
            d_ok = torch.empty(1, dtype=torch.uint8, device=dev)
        self.VerifyDeviceBatch([list(shards)], d_ok=d_ok, stream=stream)
        # the copy below runs on torch's current stream, which nothing orders behind `stream`
        stream.synchronize()
        return bool(d_ok.cpu()[0])

    def VerifyDeviceBatch(self, segments: Sequence, check=None, d_ok=None, stream=None):
        """Verify many segments held as lists of k + m 1-D uint8 device tensors (None = absent)
        in place (cec_verify_ptrs). `check` is None, or per segment either None or k + m flags
        naming the present shards to treat as expectations: each is recomputed from the
        segment's other present shards and compared, so any held shard can be checked while
        others are missing. None for a segment: every present parity shard is an expectation and
        the present data shards are the sources. Returns the uint8 device tensor of
        len(segments) flags (1 = every expectation matched, or there was none), `d_ok` if given.
        Every tensor, `d_ok` included, must be contiguous and on the codec's GPU (TypeError for a
        shard, ErrInvalidInput for `d_ok`). Enqueued on `stream` (default: torch's current
        stream) and not waited for: read the flags on that stream, or synchronise it first."""
        import torch
        nseg, n, k = len(segments), self.Shards, self.DataShards
        if check is not None and len(check) != nseg:
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        dev = torch.device("cuda", self.device)
        if d_ok is None:
            d_ok = torch.empty(nseg, dtype=torch.uint8, device=dev)
        elif (d_ok.dtype != torch.uint8 or d_ok.dim() != 1 or d_ok.numel() != nseg
              or d_ok.device != dev or not d_ok.is_contiguous()):
            # the library writes nseg consecutive bytes at its address on the codec's GPU
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        if nseg == 0:
            return d_ok
        if self.ParityShards == 0:
            return d_ok.fill_(1)
        src = (c_void_p * (nseg * n))()
        exp = (c_void_p * (nseg * n))()
        held = []
        for s, shards in enumerate(segments):
            if len(shards) != n:
                raise ErrTooFewShards(ErrTooFewShards.__doc__)
            flags = check[s] if check is not None else None
            if flags is None:
                flags = [False] * k + [True] * self.ParityShards
            elif len(flags) != n:
                raise ErrInvalidInput(ErrInvalidInput.__doc__)
            for i, t in enumerate(shards):
                if t is None:
                    continue
                held.append(_on_gpu(t, dev))
                (exp if flags[i] else src)[s * n + i] = _dev_ptr(t)
        size = self._check_device_shards(held)
        _check_rc(self._lib.cec_verify_ptrs(self._h, src, exp, nseg, size, _dev_ptr(d_ok),
                                            self._device_stream(stream)), "VerifyDeviceBatch")
        return d_ok

    def RepairFlaggedDevice(self, segments: Sequence, d_flags, d_status=None, stream=None):
        """Heal flagged fragments in place (cec_repair_flagged_ptrs): `segments` is a list of
        lists of k + m 1-D uint8 device tensors (None = not held), `d_flags` a uint8 device tensor
        [nseg, k + m] where 0 marks a held shard as bad (what HashQueue.add_check_ptrs writes for
        fragments listed segment-major; bytes of shards not held are ignored). The decision is
        taken per segment on the GPU: a segment with exactly one bad shard and at least k good
        ones gets that shard rebuilt over its tensor; every other segment is left as it is.
        Returns the uint8 device tensor of len(segments) CEC_FLAG_* codes (flag_status states the
        rule), `d_status` if given. Every tensor must be contiguous and on the codec's GPU
        (TypeError for a shard, ErrInvalidInput for `d_flags` / `d_status`, and for a codec
        without parity shards, which can heal nothing). Enqueued on `stream`
        (default: torch's current stream) and not waited for, and no flag is copied to the host:
        the flags may still be in production by work queued earlier on that stream."""
        return self._repair_flagged(segments, d_flags, d_status, stream, None,
                                    "RepairFlaggedDevice")

    def RepairFlaggedMultiDevice(self, segments: Sequence, d_flags,
                                 max_bad: int = _lib.CEC_FLAG_MULTI_MAX, d_status=None,
                                 stream=None):
        """RepairFlaggedDevice for segments with several bad shards
        (cec_repair_flagged_multi_ptrs): a segment with 1 to `max_bad` bad shards (at most
        CEC_FLAG_MULTI_MAX) and at least k good ones gets every bad shard rebuilt over its tensor,
        from the first k good shards in index order; the decode rows are solved per segment on the
        GPU, so nothing is prepared for the patterns on the host. Arguments, checks, stream
        behaviour and the returned status tensor are RepairFlaggedDevice's (flag_status_multi
        states the rule); `max_bad` outside 1..CEC_FLAG_MULTI_MAX raises ErrInvalidInput. With
        max_bad == 1, or one parity shard, it is RepairFlaggedDevice."""
        if not 1 <= int(max_bad) <= _lib.CEC_FLAG_MULTI_MAX:
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        return self._repair_flagged(segments, d_flags, d_status, stream, int(max_bad),
                                    "RepairFlaggedMultiDevice")

    def _repair_flagged(self, segments, d_flags, d_status, stream, max_bad, what):
        """The two forms above: max_bad None is cec_repair_flagged_ptrs."""
        import torch
        nseg, n = len(segments), self.Shards
        dev = torch.device("cuda", self.device)
        if (d_flags.dtype != torch.uint8 or d_flags.numel() != nseg * n or d_flags.device != dev
                or not d_flags.is_contiguous()):
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        if d_status is None:
            d_status = torch.empty(nseg, dtype=torch.uint8, device=dev)
        elif (d_status.dtype != torch.uint8 or d_status.dim() != 1 or d_status.numel() != nseg
              or d_status.device != dev or not d_status.is_contiguous()):
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        if nseg == 0:
            return d_status
        if self.ParityShards == 0:  # no parity, no codec: nothing could ever be rebuilt
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        ptrs = (c_void_p * (nseg * n))()
        held = []
        for s, shards in enumerate(segments):
            if len(shards) != n:
                raise ErrTooFewShards(ErrTooFewShards.__doc__)
            for i, t in enumerate(shards):
                if t is None:
                    continue
                held.append(_on_gpu(t, dev))
                ptrs[s * n + i] = _dev_ptr(t)
        size = self._check_device_shards(held)
        if max_bad is None:
            rc = self._lib.cec_repair_flagged_ptrs(self._h, ptrs, _dev_ptr(d_flags), nseg, size,
                                                   _dev_ptr(d_status),
                                                   self._device_stream(stream))
        else:
            rc = self._lib.cec_repair_flagged_multi_ptrs(self._h, ptrs, _dev_ptr(d_flags), nseg,
                                                         size, max_bad, _dev_ptr(d_status),
                                                         self._device_stream(stream))
        check(rc, what)
        return d_status

    def ReadFlaggedDevice(self, segments: Sequence, d_flags, out,
                          max_bad: int = _lib.CEC_FLAG_MULTI_MAX, wanted=None, d_status=None,
                          stream=None):
        """A verified degraded read decided on the GPU (cec_read_flagged_ptrs): `segments` and
        `d_flags` as in RepairFlaggedMultiDevice, but the shards are only read. `out` receives the
        data: a uint8 device tensor [nseg, k*F] whose row s is segment s's joined data (data
        shard j at columns j*F..), with `wanted` an optional [nseg][k] mask of the shards to
        deliver (default: all); or a list of nseg*k 1-D tensors of F bytes / None (None = not
        wanted), segment-major. Per segment: nothing wanted missing: every wanted shard is copied
        (CLEAN); fewer than k good: nothing written (LOST); up to `max_bad` wanted data shards
        not held or flagged bad: the good wanted ones are copied and the missing ones rebuilt into
        `out` from the first k good shards (REBUILT); else nothing written (MANY). read_status
        states the rule. Returns the uint8 device tensor of len(segments) CEC_FLAG_* codes,
        `d_status` if given. Every tensor must be contiguous and on the codec's GPU; an `out`
        tensor that is a shard of the call, or named twice, is refused (ErrInvalidInput).
        Enqueued on `stream` (default: torch's current stream) and not waited for, and no flag is
        copied to the host."""
        import torch
        if not 1 <= int(max_bad) <= _lib.CEC_FLAG_MULTI_MAX:
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        nseg, n, k = len(segments), self.Shards, self.DataShards
        dev = torch.device("cuda", self.device)
        if (d_flags.dtype != torch.uint8 or d_flags.numel() != nseg * n or d_flags.device != dev
                or not d_flags.is_contiguous()):
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        if d_status is None:
            d_status = torch.empty(nseg, dtype=torch.uint8, device=dev)
        elif (d_status.dtype != torch.uint8 or d_status.dim() != 1 or d_status.numel() != nseg
              or d_status.device != dev or not d_status.is_contiguous()):
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        if nseg == 0:
            return d_status
        if self.ParityShards == 0:  # no parity, no codec: a plain copy is the caller's
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        ptrs = (c_void_p * (nseg * n))()
        held = []
        for s, shards in enumerate(segments):
            if len(shards) != n:
                raise ErrTooFewShards(ErrTooFewShards.__doc__)
            for i, t in enumerate(shards):
                if t is None:
                    continue
                held.append(_on_gpu(t, dev))
                ptrs[s * n + i] = _dev_ptr(t)
        dst = (c_void_p * (nseg * k))()
        if isinstance(out, torch.Tensor):
            if (out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != nseg
                    or out.shape[1] % k or out.shape[1] == 0 or out.device != dev
                    or not out.is_contiguous()):
                raise ErrInvalidInput(ErrInvalidInput.__doc__)
            size = out.shape[1] // k
            if wanted is not None and (len(wanted) != nseg or any(len(w) != k for w in wanted)):
                raise ErrInvalidInput(ErrInvalidInput.__doc__)
            base = _dev_ptr(out)
            for s in range(nseg):
                for j in range(k):
                    if wanted is None or wanted[s][j]:
                        dst[s * k + j] = base + (s * k + j) * size
            if held and self._check_device_shards(held) != size:
                raise ErrShardSize(ErrShardSize.__doc__)
        else:
            if wanted is not None or len(out) != nseg * k:
                raise ErrInvalidInput(ErrInvalidInput.__doc__)
            outs = []
            for i, t in enumerate(out):
                if t is None:
                    continue
                outs.append(_on_gpu(t, dev))
                dst[i] = _dev_ptr(t)
            # one length over the shards and the destinations together
            size = self._check_device_shards(held + outs) if held or outs else 1
        rc = self._lib.cec_read_flagged_ptrs(self._h, ptrs, _dev_ptr(d_flags), dst, nseg, size,
                                             int(max_bad), _dev_ptr(d_status),
                                             self._device_stream(stream))
        if rc == _lib.CEC_EINVAL:  # a destination named twice, or one that is a shard of the call
            detail = self._lib.cec_last_error().decode()
            raise ErrInvalidInput(f"ReadFlaggedDevice: {detail}")
        check(rc, "ReadFlaggedDevice")
        return d_status

    def LocateDevice(self, segments: Sequence, nsyn: int = _lib.CEC_LOCATE_SYN_MAX, d_flags=None,
                     d_status=None, stream=None):
        """Find the corrupt fragment of every segment from parity alone (cec_locate_ptrs), no
        hash involved: `segments` is a list of lists of k + m 1-D uint8 device tensors (None = not
        held), which are only read. With h shards held and r = min(nsyn, h - k) checks, a segment
        is CEC_LOCATE_CLEAN (the held shards agree), FOUND (exactly one held shard disagrees with
        the others; its flag is 0, the other held flags 1), AMBIGUOUS (inconsistent, but no single
        shard explains it, or r == 1: every held flag 0) or UNCHECKED (h <= k: nothing to check
        with, held flags 1). locate_host states the rule. Returns (d_flags uint8 [nseg, k + m],
        d_status uint8 [nseg]), the given tensors or new ones; d_flags is what
        RepairFlaggedDevice, RepairFlaggedMultiDevice, ReadFlaggedDevice and
        HashQueue.add_check_where_ptrs consume. Every tensor must be contiguous and on the codec's
        GPU (TypeError for a shard, ErrInvalidInput for `d_flags` / `d_status` and for `nsyn`
        outside 1..CEC_LOCATE_SYN_MAX). Enqueued on `stream` (default: torch's current stream) and
        not waited for; nothing is copied to the host."""
        import torch
        if not 1 <= int(nsyn) <= _lib.CEC_LOCATE_SYN_MAX:
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        nseg, n = len(segments), self.Shards
        dev = torch.device("cuda", self.device)
        if d_flags is None:
            d_flags = torch.empty((nseg, n), dtype=torch.uint8, device=dev)
        elif (d_flags.dtype != torch.uint8 or d_flags.numel() != nseg * n or d_flags.device != dev
              or not d_flags.is_contiguous()):
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        if d_status is None:
            d_status = torch.empty(nseg, dtype=torch.uint8, device=dev)
        elif (d_status.dtype != torch.uint8 or d_status.dim() != 1 or d_status.numel() != nseg
              or d_status.device != dev or not d_status.is_contiguous()):
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        if nseg == 0:
            return d_flags, d_status
        if self.ParityShards == 0:  # no parity, no check
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        ptrs = (c_void_p * (nseg * n))()
        held = []
        for s, shards in enumerate(segments):
            if len(shards) != n:
                raise ErrTooFewShards(ErrTooFewShards.__doc__)
            for i, t in enumerate(shards):
                if t is None:
                    continue
                held.append(_on_gpu(t, dev))
                ptrs[s * n + i] = _dev_ptr(t)
        size = self._check_device_shards(held) if held else 1
        check(self._lib.cec_locate_ptrs(self._h, ptrs, nseg, size, int(nsyn), _dev_ptr(d_flags),
                                        _dev_ptr(d_status), self._device_stream(stream)),
              "LocateDevice")
        return d_flags, d_status

    def LocateMultiDevice(self, segments: Sequence, nsyn: int = _lib.CEC_LOCATE_SYN_MAX,
                          max_bad: int = _lib.CEC_LOCATE_BAD_MAX, d_flags=None, d_status=None,
                          d_nbad=None, stream=None):
        """Find up to `max_bad` corrupt fragments of every segment from parity alone
        (cec_locate_multi_ptrs): arguments and flags as in LocateDevice. With max_bad = 2 a
        segment with r = min(nsyn, h - k) = 4 checks is FOUND with one or two shards (their flags
        0, the other held flags 1) whenever at most two held shards disagree with the codeword of
        the others; a segment with fewer checks gets the single rule. max_bad = 1 is LocateDevice.
        locate_multi_host states the rule. Returns (d_flags uint8 [nseg, k + m], d_status uint8
        [nseg], d_nbad uint8 [nseg]: the number of shards a FOUND segment names, else 0), the
        given tensors or new ones; d_flags is what RepairFlaggedMultiDevice, ReadFlaggedDevice
        and HashQueue.add_check_where_ptrs consume. ErrInvalidInput for a bad output tensor, for
        `nsyn` outside 1..CEC_LOCATE_SYN_MAX and `max_bad` outside 1..CEC_LOCATE_BAD_MAX.
        Enqueued on `stream` (default: torch's current stream) and not waited for; nothing is
        copied to the host."""
        import torch
        if not 1 <= int(nsyn) <= _lib.CEC_LOCATE_SYN_MAX:
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        if not 1 <= int(max_bad) <= _lib.CEC_LOCATE_BAD_MAX:
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        nseg, n = len(segments), self.Shards
        dev = torch.device("cuda", self.device)
        if d_flags is None:
            d_flags = torch.empty((nseg, n), dtype=torch.uint8, device=dev)
        elif (d_flags.dtype != torch.uint8 or d_flags.numel() != nseg * n or d_flags.device != dev
              or not d_flags.is_contiguous()):
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        per_seg = []
        for t in (d_status, d_nbad):
            if t is None:
                t = torch.empty(nseg, dtype=torch.uint8, device=dev)
            elif (t.dtype != torch.uint8 or t.dim() != 1 or t.numel() != nseg or t.device != dev
                  or not t.is_contiguous()):
                raise ErrInvalidInput(ErrInvalidInput.__doc__)
            per_seg.append(t)
        d_status, d_nbad = per_seg
        if nseg == 0:
            return d_flags, d_status, d_nbad
        if self.ParityShards == 0:  # no parity, no check
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        ptrs = (c_void_p * (nseg * n))()
        held = []
        for s, shards in enumerate(segments):
            if len(shards) != n:
                raise ErrTooFewShards(ErrTooFewShards.__doc__)
            for i, t in enumerate(shards):
                if t is None:
                    continue
                held.append(_on_gpu(t, dev))
                ptrs[s * n + i] = _dev_ptr(t)
        size = self._check_device_shards(held) if held else 1
        check(self._lib.cec_locate_multi_ptrs(self._h, ptrs, nseg, size, int(nsyn), int(max_bad),
                                              _dev_ptr(d_flags), _dev_ptr(d_status),
                                              _dev_ptr(d_nbad), self._device_stream(stream)),
              "LocateMultiDevice")
        return d_flags, d_status, d_nbad

    def ReconstructPartialDevice(self, shards: Sequence, present, out=None,
                                 accumulate: bool = False, stream=None) -> dict:
        """Partial rebuild of one segment in place (cec_reconstruct_partial_ptrs). `shards` is a
        list of k + m 1-D uint8 device tensors or None: non-None means this caller holds the
        shard. `present` is the segment's erasure pattern as every party knows it (k + m flags).
        Every output receives the contribution of the held survivors only; the XOR of the outputs
        over a partition of the survivors is the rebuilt shard (XorDevice). The lost shards named
        in `out` (a list or {index: tensor}, as in ReconstructDevice) are the outputs; with
        out=None every lost shard is allocated. accumulate=True XORs the partial into what the
        outputs hold and requires `out` (ErrInvalidInput otherwise). Returns {index: tensor}.
        Enqueued on `stream` (default: torch's current stream) and not waited for."""
        import torch
        n = self.Shards
        if accumulate and out is None:
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        if len(shards) != n or len(present) != n:
            raise ErrTooFewShards(ErrTooFewShards.__doc__)
        lost = [i for i in range(n) if not present[i]]
        if out is None:
            size = self._check_device_shards([s for s in shards if s is not None])
            dev = torch.device("cuda", self.device)
            outs = {i: torch.empty(size, dtype=torch.uint8, device=dev) for i in lost}
        else:
            get = out.get if isinstance(out, dict) else (lambda i: out[i] if i < len(out) else None)
            outs = {i: get(i) for i in lost if get(i) is not None}
        self.ReconstructPartialDeviceBatch([shards], [present], [outs], accumulate, stream)
        return outs

    def ReconstructPartialDeviceBatch(self, segments: Sequence, present, outs,
                                      accumulate: bool = False, stream=None) -> None:
        """ReconstructPartialDevice for many segments in one call: `segments[s]` the k + m held
        tensors or None, `present[s]` the k + m flags, `outs[s]` a list or {index: tensor} of
        the wanted lost shards' tensors (None: nothing wanted of that segment). Every tensor must
        be a contiguous 1-D uint8 tensor of one length on the codec's GPU (TypeError otherwise).
        With accumulate=False an output of a segment without a held survivor is zeroed, with
        accumulate=True it is left as it is."""
        import torch
        nseg, n = len(segments), self.Shards
        if len(present) != nseg or len(outs) != nseg:
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        if nseg == 0:
            return
        dev = torch.device("cuda", self.device)
        src = (c_void_p * (nseg * n))()
        dst = (c_void_p * (nseg * n))()
        flags = (c_uint8 * (nseg * n))()
        used = []

        def addr(t):
            used.append(_on_gpu(t, dev))
            return _dev_ptr(t)

        for s, shards in enumerate(segments):
            if len(shards) != n or len(present[s]) != n:
                raise ErrTooFewShards(ErrTooFewShards.__doc__)
            out = outs[s]
            for i in range(n):
                flags[s * n + i] = 1 if present[s][i] else 0
                if shards[i] is not None:
                    src[s * n + i] = addr(shards[i])
                if out is None or present[s][i]:
                    continue
                t = out.get(i) if isinstance(out, dict) else (out[i] if i < len(out) else None)
                if t is not None:
                    dst[s * n + i] = addr(t)
        size = self._check_device_shards(used)
        check(self._lib.cec_reconstruct_partial_ptrs(
            self._h, src, dst, flags, nseg, size, 1 if accumulate else 0,
            self._device_stream(stream)), "ReconstructPartialDevice")

    def XorDevice(self, dsts: Sequence, srcs: Sequence, stream=None) -> None:
        """GF(2^8) sum of scattered device tensors (cec_xor_ptrs), the combine step of the
        partials: dsts[r] ^= XOR of the tensors in srcs[r]. `dsts` is a list of 1-D uint8 device
        tensors or None (a None row is skipped), `srcs` a list of lists of tensors or None (rows
        may differ in length; a None entry is skipped). Every tensor must be contiguous, of one
        length and on the codec's GPU (TypeError otherwise). Enqueued on `stream` (default:
        torch's current stream) and not waited for."""
        import torch
        nrows = len(dsts)
        if len(srcs) != nrows:
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        nsrc = max((len(r) for r in srcs if r is not None), default=0)
        if nrows == 0 or nsrc == 0:
            return
        dev = torch.device("cuda", self.device)
        d = (c_void_p * nrows)()
        a = (c_void_p * (nrows * nsrc))()
        used = []
        for r in range(nrows):
            row = [dsts[r]] + list(srcs[r] or [])
            for j, t in enumerate(row):
                if t is None:
                    continue
                used.append(_on_gpu(t, dev))
                if j == 0:
                    d[r] = _dev_ptr(t)
                else:
                    a[r * nsrc + j - 1] = _dev_ptr(t)
        if not used:
            return
        size = self._check_device_shards(used)
        check(self._lib.cec_xor_ptrs(self._h, d, a, nrows, nsrc, size,
                                     self._device_stream(stream)), "XorDevice")

    def EncodeIdxDevice(self, dataShard, idx: int, parity: Sequence, accumulate: bool = True,
                        stream=None) -> None:
        """klauspost EncodeIdx on one segment's scattered device tensors (cec_encode_idx_ptrs):
        parity[o] ^= E[k+o][idx] * dataShard for every parity tensor held here. `parity` is a list
        of m 1-D uint8 device tensors or None (None: that parity shard is not held here; it is
        neither read nor written). accumulate=False overwrites the parity without reading it.
        Enqueued on `stream` (default: torch's current stream) and not waited for."""
        if not 0 <= idx < self.DataShards:
            raise ErrInvShardNum(ErrInvShardNum.__doc__)
        if len(parity) != self.ParityShards:
            raise ErrTooFewShards(ErrTooFewShards.__doc__)
        if dataShard is None:
            raise ErrShardNoData(ErrShardNoData.__doc__)
        data = [None] * self.DataShards
        data[idx] = dataShard
        self.EncodeIdxDeviceBatch([data], [parity], accumulate, stream)

    def EncodeIdxDeviceBatch(self, data: Sequence, parity: Sequence, accumulate: bool = True,
                             stream=None) -> None:
        """EncodeIdxDevice for many segments in one call, each with its own fed set and its own
        parity set: `data[s]` is a list of k 1-D uint8 device tensors or None (a None entry, or
        None for the list: not fed in this call), `parity[s]` a list of m tensors or None (not
        held here). Every named parity receives the contributions of its segment's fed shards.
        With accumulate=False a named parity of a segment that feeds nothing is zeroed (the encode
        of nothing), with accumulate=True it is left as it is. Every tensor must be contiguous,
        of one length and on the codec's GPU (TypeError otherwise)."""
        nseg = len(data)
        if len(parity) != nseg:
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        self._acc_device(data, None, parity, accumulate, stream, "EncodeIdxDevice")

    def UpdateDevice(self, shards: Sequence, newDatashards: Sequence, stream=None) -> None:
        """klauspost Update on one segment's scattered device tensors (cec_update_ptrs): `shards`
        is the encoded segment (k + m 1-D uint8 device tensors; an unchanged data shard may be
        None, and so may a parity shard that is not held here), `newDatashards` the k data shards
        with None for unchanged ones. The held parity tensors are brought up to date in place from
        the old and new bytes of the changed shards; no data tensor is written. Enqueued on
        `stream` (default: torch's current stream) and not waited for."""
        k = self.DataShards
        if len(shards) != self.Shards or len(newDatashards) != k:
            raise ErrTooFewShards(ErrTooFewShards.__doc__)
        self._check_device_shards([t for t in list(shards) + list(newDatashards)
                                   if t is not None])
        self.UpdateDeviceBatch([shards[:k]], [newDatashards], [shards[k:]], stream)

    def UpdateDeviceBatch(self, olds: Sequence, news: Sequence, parities: Sequence,
                          stream=None) -> None:
        """UpdateDevice for many segments in one call, each with its own changed set and its own
        parity set: `olds[s]` and `news[s]` are lists of k tensors or None, `parities[s]` a list
        of m tensors or None (None: not held here). A slot with a new tensor is changed and needs
        its old one (ErrInvalidInput otherwise); an old tensor without a new one is unchanged and
        not read. Every tensor must be contiguous, of one length and on the codec's GPU (TypeError
        otherwise)."""
        nseg = len(olds)
        if len(news) != nseg or len(parities) != nseg:
            raise ErrInvalidInput(ErrInvalidInput.__doc__)
        self._acc_device(olds, news, parities, True, stream, "UpdateDevice")

    def _acc_device(self, olds, news, parities, accumulate, stream, what) -> None:
        """EncodeIdxDeviceBatch (news None: olds are the fed shards) and UpdateDeviceBatch."""
        nseg, k, m = len(olds), self.DataShards, self.ParityShards
        ins, outs, used = [], [], []
        for s in range(nseg):
            old = olds[s] if olds[s] is not None else [None] * k
            par = parities[s] if parities[s] is not None else [None] * m
            new = old if news is None else (news[s] if news[s] is not None else [None] * k)
            if len(old) != k or len(new) != k or len(par) != m:
                raise ErrTooFewShards(ErrTooFewShards.__doc__)
            row = []
            for j in range(k):
                if new[j] is None:
                    continue
                if old[j] is None:
                    raise ErrInvalidInput(ErrInvalidInput.__doc__)
                row.append((s * k + j, old[j], new[j]))
                used += [old[j]] if news is None else [old[j], new[j]]
            ins.append(row)
            outs.append([(s * m + o, t) for o, t in enumerate(par) if t is not None])
            used += [t for _, t in outs[-1]]
        if not used:
            return
        size = self._check_device_shards(used)
        work = [s for s in range(nseg) if outs[s] and (ins[s] or not accumulate)]
        if not work:  # nothing fed or changed, or no parity held: no C call
            return
        import torch
        dev = torch.device("cuda", self.device)
        for t in used:
            _on_gpu(t, dev)
        a = (c_void_p * (nseg * k))()
        b = (c_void_p * (nseg * k))()
        p = (c_void_p * (nseg * m))()
        for s in work:
            for i, t_old, t_new in ins[s]:
                a[i], b[i] = _dev_ptr(t_old), _dev_ptr(t_new)
            for i, t in outs[s]:
                p[i] = _dev_ptr(t)
        st = self._device_stream(stream)
        if news is None:
            check(self._lib.cec_encode_idx_ptrs(self._h, a, p, nseg, size,
                                                1 if accumulate else 0, st), what)
        else:
            check(self._lib.cec_update_ptrs(self._h, a, b, p, nseg, size, st), what)

    def _check_device_shards(self, tensors) -> int:
        import torch
        size = 0
        for t in tensors:
            if t.dtype != torch.uint8 or t.dim() != 1:
                raise TypeError("device shards must be 1-D uint8 tensors")
            if t.numel() == 0:
                raise ErrShardNoData(ErrShardNoData.__doc__)
            if size and t.numel() != size:
                raise ErrShardSize(ErrShardSize.__doc__)
            size = t.numel()
        if size == 0:
            raise ErrShardNoData(ErrShardNoData.__doc__)
        return size

    def _device_stream(self, stream):
        if stream is not None:
            return _stream_handle(stream)
        import torch
        return torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream

    def Split(self, data) -> List[np.ndarray]:
        """Split data into k equal shards (last zero padded) plus m zeroed parity shards."""
        src = _as_u8(data) if not isinstance(data, bytes) else np.frombuffer(data, np.uint8)
        if len(src) == 0:
            raise ErrShortData(ErrShortData.__doc__)
        per = (len(src) + self.DataShards - 1) // self.DataShards
        shards = [np.empty(per, dtype=np.uint8) for _ in range(self.DataShards)]
        check(_lib.load().cec_split_segment(src.ctypes.data, len(src), self.DataShards,
                                            _ptr_array(shards), per), "Split")
        return shards + [np.zeros(per, dtype=np.uint8) for _ in range(self.ParityShards)]

    def Join(self, dst: BinaryIO, shards: Sequence, out_size: int) -> None:
        """Write the first out_size bytes of the concatenated data shards to dst."""
        if len(shards) < self.DataShards:
            raise ErrTooFewShards(ErrTooFewShards.__doc__)
        shards = shards[: self.DataShards]
        if any(not _present(s) for s in shards):
            raise ErrReconstructRequired(ErrReconstructRequired.__doc__)
        if sum(len(s) for s in shards) < out_size:
            raise ErrShortData(ErrShortData.__doc__)
        left = out_size
        for s in shards:
            b = bytes(_as_u8(s)[: left])
            dst.write(b)
            left -= len(b)
            if left == 0:
                break

    # -- HBM-resident batches ----------------------------------------------------------------
    def EncodeBatch(self, d_data, d_parity, nseg: int, shard_len: int, stream=None) -> None:
        """Enqueue encode of nseg segments ([nseg][k][len] -> [nseg][m][len]) on `stream`."""
        check(self._lib.cec_encode_batch(self._h, _dev_ptr(d_data), _dev_ptr(d_parity), nseg,
                                           shard_len, _stream_handle(stream)), "EncodeBatch")

    def EncodeIdxBatch(self, d_shard, shard_seg_stride: int, idx: int, d_parity, nseg: int,
                       shard_len: int, accumulate: bool = True, stream=None) -> None:
        """EncodeIdx over an HBM batch (cec_encode_idx_batch): data shard `idx` of segment s is at
        d_shard + s * shard_seg_stride; d_parity is [nseg][m][len]. accumulate=False overwrites
        the parity without reading it (the first shard of a segment needs no zeroing pass)."""
        if not 0 <= idx < self.DataShards:
            raise ErrInvShardNum(ErrInvShardNum.__doc__)
        check(self._lib.cec_encode_idx_batch(
            self._h, _dev_ptr(d_shard), shard_seg_stride, idx, _dev_ptr(d_parity), nseg,
            shard_len, 1 if accumulate else 0, _stream_handle(stream)), "EncodeIdxBatch")

    def UpdateBatch(self, d_old, d_new, d_parity, nseg: int, shard_len: int, changed,
                    stream=None) -> None:
        """Update over an HBM batch (cec_update_batch): d_old and d_new are [nseg][k][len], of
        which only the slots flagged in `changed` (k flags, one set for the whole call) are read;
        d_parity ([nseg][m][len]) is brought up to date in place."""
        ch = np.ascontiguousarray(np.asarray(changed, dtype=np.uint8))
        if ch.shape != (self.DataShards,):
            raise ErrTooFewShards(ErrTooFewShards.__doc__)
        check(self._lib.cec_update_batch(
            self._h, _dev_ptr(d_old), _dev_ptr(d_new), _dev_ptr(d_parity), nseg, shard_len,
            ch.ctypes.data_as(POINTER(c_uint8)), _stream_handle(stream)), "UpdateBatch")

    def ReconstructBatch(self, d_data, d_parity, nseg: int, shard_len: int, present,
                         data_only: bool = False, stream=None) -> None:
        """Rebuild missing shards in place. `present`: n flags (one pattern) or nseg x n."""
        p = np.ascontiguousarray(np.asarray(present, dtype=np.uint8))
        per_segment = 1 if p.ndim == 2 else 0
        if per_segment and p.shape != (nseg, self.Shards):
            raise ValueError("present must be (nseg, k+m)")
        if not per_segment and p.shape != (self.Shards,):
            raise ValueError("present must have k+m flags")
        check(self._lib.cec_reconstruct_batch(
            self._h, _dev_ptr(d_data), _dev_ptr(d_parity), nseg, shard_len,
            p.ctypes.data_as(POINTER(c_uint8)), per_segment, 1 if data_only else 0,
            _stream_handle(stream)), "ReconstructBatch")

    def ReconstructSomeBatch(self, d_data, d_parity, nseg: int, shard_len: int, present,
                             required, stream=None) -> None:
        """ReconstructBatch for the missing shards flagged in `required` only (the same shape as
        `present`: n flags, or nseg x n); other missing shards' memory is left as it is."""
        p = np.ascontiguousarray(np.asarray(present, dtype=np.uint8))
        r = np.ascontiguousarray(np.asarray(required, dtype=np.uint8))
        per_segment = 1 if p.ndim == 2 else 0
        if per_segment and p.shape != (nseg, self.Shards):
            raise ValueError("present must be (nseg, k+m)")
        if not per_segment and p.shape != (self.Shards,):
            raise ValueError("present must have k+m flags")
        if r.shape != p.shape:
            raise ValueError("required must have the shape of present")
        check(self._lib.cec_reconstruct_some_batch(
            self._h, _dev_ptr(d_data), _dev_ptr(d_parity), nseg, shard_len,
            p.ctypes.data_as(POINTER(c_uint8)), r.ctypes.data_as(POINTER(c_uint8)), per_segment,
            _stream_handle(stream)), "ReconstructSomeBatch")

    def ReconstructPartialBatch(self, d_data, d_parity, nseg: int, shard_len: int, present,
                                held, data_only: bool = False, stream=None) -> None:
        """Partial rebuild (cec_reconstruct_partial_batch): every missing shard of segment s gets
        the contribution of the survivors of `present[s]` flagged in `held[s]` (both nseg x n).
        XOR of the partials over a partition of the survivors = ReconstructBatch's result."""
        p = np.ascontiguousarray(np.asarray(present, dtype=np.uint8))
        h = np.ascontiguousarray(np.asarray(held, dtype=np.uint8))
        if p.shape != (nseg, self.Shards) or h.shape != (nseg, self.Shards):
            raise ValueError("present and held must be (nseg, k+m)")
        check(self._lib.cec_reconstruct_partial_batch(
            self._h, _dev_ptr(d_data), _dev_ptr(d_parity), nseg, shard_len,
            p.ctypes.data_as(POINTER(c_uint8)), h.ctypes.data_as(POINTER(c_uint8)),
            1 if data_only else 0, _stream_handle(stream)), "ReconstructPartialBatch")

    def VerifyBatch(self, d_data, d_parity, nseg: int, shard_len: int, d_ok=None,
                    stream=None):
        """klauspost Verify over an HBM batch (cec_verify_batch): with `d_ok` (device uint8
        [nseg]) the per-segment flags are enqueued there; without, they are returned as a numpy
        bool array (synchronous)."""
        import torch
        out = d_ok
        if out is None:
            out = torch.empty(max(1, nseg), dtype=torch.uint8,
                              device=torch.device("cuda", self.device))
            if stream is None:  # read back below on torch's current stream: launch there too
                stream = torch.cuda.current_stream(out.device)
        check(self._lib.cec_verify_batch(self._h, _dev_ptr(d_data), _dev_ptr(d_parity), nseg,
                                         shard_len, _dev_ptr(out), _stream_handle(stream)),
              "VerifyBatch")
        if d_ok is not None:
            return None
        if stream is not None:
            stream.synchronize()
        return out[:nseg].cpu().numpy().astype(bool)

    def Sha256Batch(self, d_data, d_parity, nseg: int, shard_len: int, d_hex,
                    stream=None) -> None:
        """Hex SHA-256 of every shard into d_hex ([nseg][k+m][64] bytes, device)."""
        check(self._lib.cec_sha256_batch(
            self._h, _dev_ptr(d_data), 0 if d_parity is None else _dev_ptr(d_parity), nseg,
            shard_len, _dev_ptr(d_hex), _stream_handle(stream)), "Sha256Batch")


def New(data_shards: int, parity_shards: int, device: int = 0, tuning: bool = False) -> Encoder:
    """klauspost reedsolomon.New(dataShards, parityShards) on a GPU."""
    return Encoder(data_shards, parity_shards, device, tuning)


def decode_rows(data_shards: int, parity_shards: int, present, required):
    """Host only (cec_decode_rows): the decode rows of the lost shards of pattern `present` flagged
    in `required` (k+m flags each). Returns (shard indices ascending, rows [nreq][k] uint8 over the
    survivors in cec_survivors order)."""
    n = data_shards + parity_shards
    p = np.ascontiguousarray(np.asarray(present, dtype=np.uint8))
    r = np.ascontiguousarray(np.asarray(required, dtype=np.uint8))
    if p.shape != (n,) or r.shape != (n,):
        raise ValueError("present and required must have k+m flags")
    rows = np.zeros((n, data_shards), dtype=np.uint8)
    idx = np.zeros(n, dtype=np.uint8)
    nreq = c_int(0)
    u8p = POINTER(c_uint8)
    check(_lib.load().cec_decode_rows(data_shards, parity_shards, p.ctypes.data_as(u8p),
                                      r.ctypes.data_as(u8p), rows.ctypes.data_as(u8p),
                                      idx.ctypes.data_as(u8p), byref(nreq)), "decode_rows")
    return idx[:nreq.value].copy(), rows[:nreq.value].copy()


def flag_status(data_shards: int, parity_shards: int, held, flags):
    """Host only (cec_flag_status): the rule RepairFlaggedDevice applies to one segment on the
    GPU. `held` and `flags` are k+m values each (a held shard whose flag is 0 is bad). Returns
    (CEC_FLAG_* status, the index of the shard a REBUILT segment rewrites or -1)."""
    n = data_shards + parity_shards
    h = np.ascontiguousarray(np.asarray(held, dtype=np.uint8))
    f = np.ascontiguousarray(np.asarray(flags, dtype=np.uint8))
    if h.shape != (n,) or f.shape != (n,):
        raise ValueError("held and flags must have k+m values")
    status, lost = c_int(-1), c_int(-2)
    u8p = POINTER(c_uint8)
    check(_lib.load().cec_flag_status(data_shards, parity_shards, h.ctypes.data_as(u8p),
                                      f.ctypes.data_as(u8p), byref(status), byref(lost)),
          "flag_status")
    return status.value, lost.value


def flag_status_multi(data_shards: int, parity_shards: int, held, flags, max_bad: int):
    """Host only (cec_flag_status_multi): the rule RepairFlaggedMultiDevice applies to one segment
    on the GPU. `held` and `flags` are k+m values each (a held shard whose flag is 0 is bad).
    Returns (CEC_FLAG_* status, the ascending list of the shards a REBUILT segment rewrites, empty
    for every other status)."""
    n = data_shards + parity_shards
    h = np.ascontiguousarray(np.asarray(held, dtype=np.uint8))
    f = np.ascontiguousarray(np.asarray(flags, dtype=np.uint8))
    if h.shape != (n,) or f.shape != (n,):
        raise ValueError("held and flags must have k+m values")
    status, nlost = c_int(-1), c_int(0)
    lost = (c_uint8 * _lib.CEC_FLAG_MULTI_MAX)()
    u8p = POINTER(c_uint8)
    check(_lib.load().cec_flag_status_multi(data_shards, parity_shards, h.ctypes.data_as(u8p),
                                            f.ctypes.data_as(u8p), max_bad, byref(status),
                                            byref(nlost), lost), "flag_status_multi")
    return status.value, [int(x) for x in lost[:nlost.value]]


def read_status(data_shards: int, parity_shards: int, held, flags, wanted, max_bad: int):
    """Host only (cec_read_status): the rule ReadFlaggedDevice applies to one segment on the GPU.
    `held` and `flags` are k+m values each (a held shard whose flag is not 0 is good), `wanted` k
    values naming the data shards to deliver. A wanted data shard that is not good is missing.
    Returns (CEC_FLAG_* status, the ascending list of the shards a REBUILT segment rebuilds into
    its destination, empty for every other status)."""
    n = data_shards + parity_shards
    h = np.ascontiguousarray(np.asarray(held, dtype=np.uint8))
    f = np.ascontiguousarray(np.asarray(flags, dtype=np.uint8))
    w = np.ascontiguousarray(np.asarray(wanted, dtype=np.uint8))
    if h.shape != (n,) or f.shape != (n,) or w.shape != (data_shards,):
        raise ValueError("held and flags must have k+m values, wanted k")
    status, nmiss = c_int(-1), c_int(0)
    miss = (c_uint8 * _lib.CEC_FLAG_MULTI_MAX)()
    u8p = POINTER(c_uint8)
    check(_lib.load().cec_read_status(data_shards, parity_shards, h.ctypes.data_as(u8p),
                                      f.ctypes.data_as(u8p), w.ctypes.data_as(u8p), max_bad,
                                      byref(status), byref(nmiss), miss), "read_status")
    return status.value, [int(x) for x in miss[:nmiss.value]]


def locate_rows(data_shards: int, parity_shards: int, held, nsyn: int):
    """Host only (cec_locate_rows): the check rows of a held set. `held` is k+m values. Returns
    (r, rows): r = min(nsyn, h - k) checks (0 when h <= k) and rows uint8 [r][k+m] with
    rows[a][i] = u_i * i^a for held i, 0 elsewhere; every row XOR-multiplied into the held shards
    of a consistent segment gives zero at every byte."""
    n = data_shards + parity_shards
    h = np.ascontiguousarray(np.asarray(held, dtype=np.uint8))
    if h.shape != (n,):
        raise ValueError("held must have k+m values")
    r = c_int(-1)
    rows = np.zeros((_lib.CEC_LOCATE_SYN_MAX, n), np.uint8)
    u8p = POINTER(c_uint8)
    check(_lib.load().cec_locate_rows(data_shards, parity_shards, h.ctypes.data_as(u8p), nsyn,
                                      byref(r), rows.ctypes.data_as(u8p)), "locate_rows")
    return r.value, rows[:r.value].copy()


def locate_host(data_shards: int, parity_shards: int, shards, nsyn: int):
    """Host only (cec_locate_host): the rule Encoder.LocateDevice applies to one segment on the
    GPU, on host memory. `shards` is k+m buffers of one length, None = not held. Returns
    (CEC_LOCATE_* status, the shard of a FOUND segment or -1)."""
    n = data_shards + parity_shards
    if len(shards) != n:
        raise ValueError("shards must have k+m entries")
    arrs = [None if s is None else np.frombuffer(s, np.uint8) if isinstance(s, bytes)
            else _as_u8(s) for s in shards]
    sizes = {a.size for a in arrs if a is not None}
    if len(sizes) > 1:
        raise ErrShardSize(ErrShardSize.__doc__)
    ptrs = (c_void_p * n)(*[None if a is None else a.ctypes.data for a in arrs])
    status, found = c_int(-1), c_int(-2)
    check(_lib.load().cec_locate_host(data_shards, parity_shards, ptrs,
                                      sizes.pop() if sizes else 0, nsyn, byref(status),
                                      byref(found)), "locate_host")
    return status.value, found.value


def locate_multi_host(data_shards: int, parity_shards: int, shards, nsyn: int, max_bad: int):
    """Host only (cec_locate_multi_host): the rule Encoder.LocateMultiDevice applies to one
    segment on the GPU, on host memory. `shards` as in locate_host. Returns (CEC_LOCATE_* status,
    the shards of a FOUND segment ascending: a list of one or two, else empty)."""
    n = data_shards + parity_shards
    if len(shards) != n:
        raise ValueError("shards must have k+m entries")
    arrs = [None if s is None else np.frombuffer(s, np.uint8) if isinstance(s, bytes)
            else _as_u8(s) for s in shards]
    sizes = {a.size for a in arrs if a is not None}
    if len(sizes) > 1:
        raise ErrShardSize(ErrShardSize.__doc__)
    ptrs = (c_void_p * n)(*[None if a is None else a.ctypes.data for a in arrs])
    status, nfound, found = c_int(-1), c_int(0), (c_int * 2)(-1, -1)
    check(_lib.load().cec_locate_multi_host(data_shards, parity_shards, ptrs,
                                            sizes.pop() if sizes else 0, nsyn, max_bad,
                                            byref(status), byref(nfound), found),
          "locate_multi_host")
    return status.value, [int(x) for x in found[:nfound.value]]


def confirm_rule(status: int, ok) -> int:
    """Host only (cec_confirm_rule): what confirm_flagged computes for one segment from its
    CEC_FLAG_* status and its k+m ok bytes (1 match, 0 mismatch, CEC_HASHQ_SKIPPED not hashed).
    Returns CEC_CONFIRM_NONE unless the status is CEC_FLAG_REBUILT; then REFUTED if any byte is 0,
    else PROVEN if any is 1, else NONE."""
    o = np.ascontiguousarray(np.asarray(ok, dtype=np.uint8))
    if o.ndim != 1:
        raise ValueError("ok must be one segment's bytes")
    out = c_int(-1)
    check(_lib.load().cec_confirm_rule(o.size, status, o.ctypes.data_as(POINTER(c_uint8)),
                                       byref(out)), "confirm_rule")
    return out.value


def confirm_flagged(d_status, d_ok, n: int, d_confirm=None, stream=None):
    """What a repair proved, per segment, on the GPU (cec_confirm_flagged): d_status is the uint8
    device tensor [nseg] of CEC_FLAG_* codes a flagged repair left, d_ok [nseg][n] the flags of
    HashQueue.add_check_where_ptrs over the rebuilt fragments. Returns the uint8 device tensor
    [nseg] (d_confirm, or a new one) of CEC_CONFIRM_* codes by the rule of `confirm_rule`:
    PROVEN where every rebuilt fragment of a REBUILT segment hashes to its record, REFUTED where
    one still does not (the record is wrong), NONE elsewhere. Enqueued on `stream` and not waited
    for; only d_confirm is written."""
    import torch
    nseg = d_status.numel()
    if d_ok.numel() < nseg * n:
        raise ErrShardSize(ErrShardSize.__doc__)
    if d_confirm is None:
        d_confirm = torch.empty(nseg, dtype=torch.uint8, device=d_status.device)
    elif d_confirm.numel() < nseg:
        raise ErrShardSize(ErrShardSize.__doc__)
    check(_lib.load().cec_confirm_flagged(_dev_ptr(d_status), _dev_ptr(d_ok), nseg, n,
                                          _dev_ptr(d_confirm), _stream_handle(stream)),
          "confirm_flagged")
    return d_confirm


def fill_synthetic(d_out, seg_bytes: int, nseg: int, seg0: int, seed: int, stream=None) -> None:
    """Counter-based synthetic segments in HBM (SURVEY.md §8d input generator)."""
    check(_lib.load().cec_fill_synthetic(_dev_ptr(d_out), seg_bytes, nseg, seg0, seed,
                                         _stream_handle(stream)), "fill_synthetic")


def xor_batch(d_dst, d_src, nsrc: int, src_stride: int, length: int, stream=None) -> None:
    """d_dst[:length] ^= XOR of nsrc buffers at d_src + j * src_stride (cec_xor_batch: GF(2^8)
    addition of the partial rebuilds other GPUs sent)."""
    check(_lib.load().cec_xor_batch(_dev_ptr(d_dst), _dev_ptr(d_src), nsrc, src_stride, length,
                                    _stream_handle(stream)), "xor_batch")


def sha256_hex_host(bufs, length: int, threads: int = 16, prefix_len: int = 0):
    """SHA-256 hex of equal-length HOST buffers (numpy arrays / bytes-likes, or addresses) with
    libcessec's multi-chain host hasher (cec_sha256_host: 16 chains per core in AVX-512 lanes or
    SHA-NI interleaved, on `threads` threads; the GIL is released during the call). With
    `prefix_len` (a multiple of 64, <= length) returns (hexes, hexes of each buffer's first
    prefix_len bytes): a segment chain yields data fragment 0's hash on the way."""
    n = len(bufs)
    if n == 0:
        return ([], []) if prefix_len else []
    keep = []
    ptrs = []
    for b in bufs:
        if isinstance(b, int):
            ptrs.append(b)
            continue
        a = b if isinstance(b, np.ndarray) else np.frombuffer(b, np.uint8)
        if a.nbytes < length:
            raise ValueError("buffer shorter than length")
        if length and not a.flags.c_contiguous:
            a = np.ascontiguousarray(a)
        keep.append(a)
        ptrs.append(a.ctypes.data)
    out = np.zeros(n * 64, dtype=np.uint8)
    pre = np.zeros(n * 64, dtype=np.uint8) if prefix_len else None
    arr = (c_void_p * n)(*ptrs)
    check(_lib.load().cec_sha256_host(arr, n, length, out.ctypes.data, prefix_len,
                                      pre.ctypes.data if prefix_len else None, threads),
          "sha256_hex_host")
    hexes = [out[i * 64:(i + 1) * 64].tobytes() for i in range(n)]
    if prefix_len:
        return hexes, [pre[i * 64:(i + 1) * 64].tobytes() for i in range(n)]
    return hexes


def sha256_hex_device(d_ptrs: Sequence[int], length: int) -> List[bytes]:
    """SHA-256 hex of device buffers (addresses) of equal length, computed on the GPU."""
    n = len(d_ptrs)
    out = np.zeros(n * 64, dtype=np.uint8)
    arr = (c_void_p * n)(*d_ptrs)
    check(_lib.load().cec_sha256_hex(arr, n, length, out.ctypes.data_as(POINTER(c_uint8)),
                                     None), "sha256_hex")
    return [out[i * 64:(i + 1) * 64].tobytes() for i in range(n)]
