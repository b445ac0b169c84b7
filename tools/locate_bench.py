#!/usr/bin/env python3
"""The corrupt fragment found from parity (cec_locate_ptrs) against the hash scrub and the
detect-only verify.

  --geometry rs32   64 segments of RS(32,32), F = 512 KiB
  --geometry rs10   64 segments of RS(10,4),  F = 512 KiB
  --geometry rs4    256 segments of RS(4,2),  F = 512 KiB
  --geometry rs21   64 segments of RS(2,1),   F = 8 MiB

Every fragment is held, in one allocation per load. The data is synthetic and the parity the
codec's own batch encode. Three stores: no segment dirty, one, all (one bit flipped in the middle
of fragment s % n of segment s). Legs, `--reps` interleaved repetitions of `--iters` calls:
    l0, l1, lall   cec_locate_ptrs over the store with 0, 1, all segments dirty;
    s              audit.scrub_device (a checked SHA-256 chain per fragment) over the clean store;
    v              cec_verify_ptrs (parity recomputed and compared, one byte per segment) over it.
Each leg's output is checked before the timing starts. One JSON line per repetition and leg, then
one summary line. Times are HIP events around `--iters` calls."""
import argparse
import os
import sys
from ctypes import c_void_p

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.ptrs_bench import run_legs  # noqa: E402  (same warm-up, interleaving and summary)

SHAPES = {"rs32": (32, 32, 64, 512), "rs10": (10, 4, 64, 512), "rs4": (4, 2, 256, 512),
          "rs21": (2, 1, 64, 8192)}
LOADS = ["0", "1", "all"]


def geometry(torch, cess_amd, args):
    from cess_amd import _lib, audit
    from cess_amd.hashq import HashQueue
    lib = _lib.load()
    k, m, nseg, kib = SHAPES[args.geometry]
    nseg, F = args.nseg or nseg, (args.frag_kib or kib) << 10
    n = k + m
    dev = torch.device("cuda", 0)
    enc = cess_amd.New(k, m)
    data = torch.empty((nseg, k, F), dtype=torch.uint8, device=dev)
    par = torch.empty((nseg, m, F), dtype=torch.uint8, device=dev)
    cess_amd.fill_synthetic(data, k * F, nseg, 0, 0xCE55004C)
    enc.EncodeBatch(data, par, nseg, F)
    hexes = torch.empty((nseg, n, 64), dtype=torch.uint8, device=dev)
    enc.Sha256Batch(data, par, nseg, F, hexes)
    torch.cuda.synchronize()
    stores, dirty = {}, {}
    for name in LOADS:
        st = torch.cat([data, par], dim=1).contiguous()
        dirty[name] = {"0": [], "1": [nseg // 2], "all": list(range(nseg))}[name]
        for s in dirty[name]:
            st[s, s % n, F // 2] ^= 1
        stores[name] = st
    del data, par
    d_flags = torch.empty((nseg, n), dtype=torch.uint8, device=dev)
    d_status = torch.empty(nseg, dtype=torch.uint8, device=dev)
    d_ok = torch.empty(nseg, dtype=torch.uint8, device=dev)
    d_scrub = torch.empty(nseg * n, dtype=torch.uint8, device=dev)

    def ptrs_of(st, lo, hi):
        """[nseg][n] addresses of the store's shards lo .. hi - 1, NULL elsewhere"""
        base = st.data_ptr()
        return (c_void_p * (nseg * n))(*[base + (s * n + i) * F if lo <= i < hi else None
                                         for s in range(nseg) for i in range(n)])

    all_ptrs = {name: ptrs_of(stores[name], 0, n) for name in LOADS}
    src, exp = ptrs_of(stores["0"], 0, k), ptrs_of(stores["0"], k, n)
    frags = [stores["0"][s, i] for s in range(nseg) for i in range(n)]
    queue = HashQueue(capacity=1 << max(0, nseg * n - 1).bit_length(), device=0,
                      stream=torch.cuda.current_stream(dev))
    stream = torch.cuda.current_stream(dev).cuda_stream

    def leg_locate(name):
        def run():
            rc = lib.cec_locate_ptrs(enc._h, all_ptrs[name], nseg, F, args.nsyn,
                                     d_flags.data_ptr(), d_status.data_ptr(), stream)
            assert rc == 0, rc
        return run

    def leg_scrub():
        audit.scrub_device(frags, hexes.view(nseg * n, 64), queue=queue, d_ok=d_scrub)

    def leg_verify():
        rc = lib.cec_verify_ptrs(enc._h, src, exp, nseg, F, d_ok.data_ptr(), stream)
        assert rc == 0, rc

    legs = {"l" + name: leg_locate(name) for name in LOADS}
    legs["s"] = leg_scrub
    legs["v"] = leg_verify

    checks = {}
    hit = _lib.CEC_LOCATE_FOUND if min(args.nsyn, m) >= 2 else _lib.CEC_LOCATE_AMBIGUOUS
    for name in LOADS:
        d_flags.fill_(0xA5)
        d_status.fill_(0xA5)
        legs["l" + name]()
        torch.cuda.synchronize()
        want_st = np.zeros(nseg, np.uint8)
        want_fl = np.ones((nseg, n), np.uint8)
        for s in dirty[name]:
            want_st[s] = hit
            if hit == _lib.CEC_LOCATE_FOUND:
                want_fl[s, s % n] = 0
            else:
                want_fl[s] = 0
        checks["l" + name] = bool(np.array_equal(d_status.cpu().numpy(), want_st) and
                                  np.array_equal(d_flags.cpu().numpy(), want_fl))
    d_scrub.fill_(0xA5)
    leg_scrub()
    torch.cuda.synchronize()
    checks["s"] = bool((d_scrub == 1).all())
    d_ok.fill_(0xA5)
    leg_verify()
    torch.cuda.synchronize()
    checks["v"] = bool((d_ok == 1).all())
    assert all(checks.values()), checks

    def extra(ms):
        med = {x: float(np.median(v)) for x, v in ms.items()}
        held = nseg * n * F  # every held byte, read once by a clean locate, by the scrub, the verify
        out = {"outputs_checked": checks, "k": k, "m": m, "segments": nseg, "fragment_bytes": F,
               "nsyn": args.nsyn, "r": min(args.nsyn, m),
               "spread_ms": {x: round(max(v) - min(v), 5) for x, v in ms.items()}}
        for x in med:
            out[x + "_GBps"] = round(held / med[x] / 1e6, 1)
        if "l0" in med and "s" in med:
            out["l0_over_s"] = round(med["l0"] / med["s"], 4)
        if "l0" in med and "v" in med:
            out["l0_over_v"] = round(med["l0"] / med["v"], 4)
        if "l0" in med and "lall" in med:
            out["lall_over_l0"] = round(med["lall"] / med["l0"], 4)
        return out

    run_legs(torch, legs, args, extra)
    queue.close()
    enc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=sorted(SHAPES), required=True)
    ap.add_argument("--nseg", type=int, default=0)
    ap.add_argument("--frag-kib", type=int, default=0)
    ap.add_argument("--nsyn", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--legs", default="", help="comma-separated legs to time (default: all)")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    import cess_amd
    geometry(torch, cess_amd, args)


if __name__ == "__main__":
    main()
