#!/usr/bin/env python3
"""Healing flagged fragments on the GPU against the host round trip it replaces.

  --geometry cess   `--nseg` (256) segments of RS(2,1), F = 8 MiB, every fragment its own
                    allocation, flags in device memory with a bad fraction of 0, 1/64 and 1 of the
                    segments (one bad fragment each).
  --geometry wide   64 segments of RS(32,32), F = 512 KiB, one bad fragment in every segment
                    (fragment s of segment s).

Legs, `--reps` interleaved repetitions of `--iters` calls, per bad fraction x:
    h<x>  what callers do today: the flags copied to the host (which waits for the stream), the
          erasure patterns and pointer arrays built there from the flags, cec_reconstruct_ptrs of
          the bad fragments;
    f<x>  cec_repair_flagged_ptrs on the same flags: nothing copied out, nothing waited for.

The outputs of h and f are compared with the codewords, on junk in the bad fragments, before the
timing starts. One JSON line per repetition and leg, then one summary line. Times are HIP events
around `--iters` calls."""
import argparse
import os
import sys
from ctypes import c_void_p

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.ptrs_bench import run_legs  # noqa: E402  (same warm-up, interleaving and summary)


def geometry(torch, cess_amd, args):
    from cess_amd import _lib
    lib = _lib.load()
    wide = args.geometry == "wide"
    k, m = (32, 32) if wide else (2, 1)
    n, nseg, F = k + m, args.nseg, args.frag_kib << 10
    dev = torch.device("cuda", 0)
    enc = cess_amd.New(k, m)
    rng = np.random.default_rng(25)
    # the codewords, a few segments at a time, into one allocation per fragment (shuffled order)
    frag = {}
    for j in rng.permutation(nseg * n):
        frag[divmod(int(j), n)] = torch.empty(F, dtype=torch.uint8, device=dev)
    step = 16
    ref_d = torch.empty((step, k, F), dtype=torch.uint8, device=dev)
    ref_p = torch.empty((step, m, F), dtype=torch.uint8, device=dev)
    for s0 in range(0, nseg, step):
        cnt = min(step, nseg - s0)
        cess_amd.fill_synthetic(ref_d, k * F, cnt, s0, 0xCE550019)
        enc.EncodeBatch(ref_d, ref_p, cnt, F)
        for s in range(cnt):
            for i in range(n):
                frag[(s0 + s, i)].copy_(ref_d[s, i] if i < k else ref_p[s, i - k])
    torch.cuda.synchronize()
    del ref_d, ref_p
    truth = {key: t.clone() for key, t in frag.items()} if args.check_all else None
    addr = np.array([frag[(s, i)].data_ptr() for s in range(nseg) for i in range(n)],
                    dtype=np.uint64).reshape(nseg, n)
    ptrs = (c_void_p * (nseg * n))(*[int(x) for x in addr.ravel()])
    d_status = torch.empty(nseg, dtype=torch.uint8, device=dev)

    fractions = {"1": 1} if wide else {"0": 0, "64": 64, "1": 1}
    flags = {}
    for name, every in fractions.items():
        fl = np.ones((nseg, n), np.uint8)
        if every:
            segs = np.arange(0, nseg, every)
            fl[segs, (segs // every) % n] = 0
        flags[name] = (fl, torch.from_numpy(fl).to(dev))

    def leg_f(name):
        d_fl = flags[name][1]

        def run():
            rc = lib.cec_repair_flagged_ptrs(enc._h, ptrs, d_fl.data_ptr(), nseg, F,
                                             d_status.data_ptr(), None)
            assert rc == 0, rc
        return run

    def leg_h(name):
        d_fl = flags[name][1]

        def run():
            fl = d_fl.cpu().numpy()  # the copy waits for the stream
            bad = fl == 0
            rows = np.nonzero(bad.sum(axis=1) == 1)[0]  # one bad fragment: rebuild it
            if rows.size == 0:
                return
            a = addr[rows]
            b = bad[rows]
            src = np.where(b, 0, a).astype(np.uint64)
            dst = np.where(b, a, 0).astype(np.uint64)
            sp = (c_void_p * src.size).from_buffer(src)
            dp = (c_void_p * dst.size).from_buffer(dst)
            rc = lib.cec_reconstruct_ptrs(enc._h, sp, dp, rows.size, F, None)
            assert rc == 0, rc
        return run

    legs = {}
    for name in fractions:
        legs["h" + name] = leg_h(name)
        legs["f" + name] = leg_f(name)

    # equality first: junk in the bad fragments, each leg once, everything equal to the codewords
    checks = {}
    for lname, fn in legs.items():
        fl = flags[lname[1:]][0]
        bad = [(s, i) for s, i in zip(*np.nonzero(fl == 0))]
        ref = {}
        for s, i in bad:
            ref[(s, i)] = frag[(s, i)].clone()
            frag[(s, i)].fill_(0x3C)
        fn()
        torch.cuda.synchronize()
        checks[lname] = all(torch.equal(frag[key], t) for key, t in ref.items())
        if truth is not None:
            checks[lname] = checks[lname] and all(torch.equal(frag[key], t)
                                                  for key, t in truth.items())
        if lname[0] == "f":
            want = np.where((fl == 0).any(axis=1), _lib.CEC_FLAG_REBUILT, _lib.CEC_FLAG_CLEAN)
            checks[lname + "_status"] = bool(np.array_equal(d_status.cpu().numpy(), want))
    assert all(checks.values()), checks

    def extra(ms):
        med = {x: float(np.median(v)) for x, v in ms.items()}
        out = {"outputs_checked": checks, "k": k, "m": m, "segments": nseg, "fragment_bytes": F,
               "spread_ms": {x: round(max(v) - min(v), 5) for x, v in ms.items()}}
        for name, every in fractions.items():
            nbad = len(range(0, nseg, every)) if every else 0
            out["bad_segments_" + name] = nbad
            out["f_over_h_" + name] = round(med["f" + name] / med["h" + name], 4)
            if nbad:  # algorithmic bytes: k fragments read, one written per bad segment
                out["f_TBps_" + name] = round(nbad * (k + 1) * F / (med["f" + name] * 1e-3) / 1e12,
                                              3)
                out["h_TBps_" + name] = round(nbad * (k + 1) * F / (med["h" + name] * 1e-3) / 1e12,
                                              3)
        return out

    run_legs(torch, legs, args, extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=["wide", "cess"], required=True)
    ap.add_argument("--nseg", type=int, default=0, help="segments (default 256 / 64)")
    ap.add_argument("--frag-kib", type=int, default=0, help="fragment size (default 8192 / 512)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warm", type=int, default=30)
    ap.add_argument("--legs", default="", help="comma-separated legs to time (default: all)")
    ap.add_argument("--check-all", action="store_true",
                    help="compare every fragment, not only the bad ones (doubles the memory)")
    args = ap.parse_args()
    if not args.frag_kib:
        args.frag_kib = 512 if args.geometry == "wide" else 8192
    if not args.nseg:
        args.nseg = 64 if args.geometry == "wide" else 256
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    import cess_amd
    geometry(torch, cess_amd, args)


if __name__ == "__main__":
    main()
