#!/usr/bin/env python3
"""Healing several flagged fragments per segment on the GPU against the host round trip it
replaces.

  --geometry rs42   `--nseg` (256) segments of RS(4,2), F = 8 MiB, every fragment its own
                    allocation; workloads: two bad fragments in no segment ("0"), in 4 segments
                    ("4") and in every segment ("all").
  --geometry wide   64 segments of RS(32,32), F = 512 KiB; workloads: 2 and 4 bad fragments in
                    every segment ("2", "4"), and one ("1"), where cec_repair_flagged_ptrs applies
                    too: the price of per-segment programs and per-bucket launches.

Legs, `--reps` interleaved repetitions of `--iters` calls, per workload x:
    h<x>  the baseline, what callers do without the call: the flags copied to the host (which
          waits for the stream), the patterns and pointer arrays built there,
          cec_reconstruct_ptrs of the bad fragments from the good ones;
    m<x>  cec_repair_flagged_multi_ptrs on the same flags: nothing copied out or waited for;
    f1    (wide) cec_repair_flagged_ptrs.

The outputs of every leg are compared with the codewords, on junk in the bad fragments, before
the timing starts. One JSON line per repetition and leg, then one summary line. Times are HIP
events around `--iters` calls."""
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
    k, m = (32, 32) if wide else (4, 2)
    n, nseg, F = k + m, args.nseg, args.frag_kib << 10
    dev = torch.device("cuda", 0)
    enc = cess_amd.New(k, m)
    rng = np.random.default_rng(26)
    frag = {}
    for j in rng.permutation(nseg * n):
        frag[divmod(int(j), n)] = torch.empty(F, dtype=torch.uint8, device=dev)
    step = 16
    ref_d = torch.empty((step, k, F), dtype=torch.uint8, device=dev)
    ref_p = torch.empty((step, m, F), dtype=torch.uint8, device=dev)
    for s0 in range(0, nseg, step):
        cnt = min(step, nseg - s0)
        cess_amd.fill_synthetic(ref_d, k * F, cnt, s0, 0xCE55001A)
        enc.EncodeBatch(ref_d, ref_p, cnt, F)
        for s in range(cnt):
            for i in range(n):
                frag[(s0 + s, i)].copy_(ref_d[s, i] if i < k else ref_p[s, i - k])
    torch.cuda.synchronize()
    del ref_d, ref_p
    addr = np.array([frag[(s, i)].data_ptr() for s in range(nseg) for i in range(n)],
                    dtype=np.uint64).reshape(nseg, n)
    ptrs = (c_void_p * (nseg * n))(*[int(x) for x in addr.ravel()])
    d_status = torch.empty(nseg, dtype=torch.uint8, device=dev)

    # workload -> (bad fragments per bad segment, the bad segments)
    if wide:
        loads = {"2": (2, range(nseg)), "4": (4, range(nseg)), "1": (1, range(nseg))}
    else:
        loads = {"0": (2, range(0)), "4": (2, range(0, nseg, max(1, nseg // 4))),
                 "all": (2, range(nseg))}
    flags = {}
    for name, (e, segs) in loads.items():
        fl = np.ones((nseg, n), np.uint8)
        for s in segs:
            fl[s, [(s + o * (n // e)) % n for o in range(e)]] = 0  # spread over data and parity
        flags[name] = (fl, torch.from_numpy(fl).to(dev))
    max_bad = _lib.CEC_FLAG_MULTI_MAX if wide else 2

    def leg_m(name):
        d_fl = flags[name][1]

        def run():
            rc = lib.cec_repair_flagged_multi_ptrs(enc._h, ptrs, d_fl.data_ptr(), nseg, F, max_bad,
                                                   d_status.data_ptr(), None)
            assert rc == 0, rc
        return run

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
            nb = bad.sum(axis=1)
            rows = np.nonzero((nb >= 1) & (nb <= max_bad) & (n - nb >= k))[0]
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
    for name in loads:
        legs["h" + name] = leg_h(name)
        legs["m" + name] = leg_m(name)
    if wide:
        legs["f1"] = leg_f("1")

    # equality first: junk in the bad fragments, each leg once, everything equal to the codewords
    checks = {}
    for lname, fn in legs.items():
        fl = flags[lname[1:]][0]
        ref = {}
        for s, i in zip(*np.nonzero(fl == 0)):
            ref[(s, i)] = frag[(s, i)].clone()
            frag[(s, i)].fill_(0x3C)
        fn()
        torch.cuda.synchronize()
        checks[lname] = all(torch.equal(frag[key], t) for key, t in ref.items())
        if lname[0] != "h":
            want = np.where((fl == 0).any(axis=1), _lib.CEC_FLAG_REBUILT, _lib.CEC_FLAG_CLEAN)
            checks[lname + "_status"] = bool(np.array_equal(d_status.cpu().numpy(), want))
    assert all(checks.values()), checks

    def extra(ms):
        med = {x: float(np.median(v)) for x, v in ms.items()}
        out = {"outputs_checked": checks, "k": k, "m": m, "segments": nseg, "fragment_bytes": F,
               "max_bad": max_bad,
               "spread_ms": {x: round(max(v) - min(v), 5) for x, v in ms.items()}}
        for name, (e, segs) in loads.items():
            out["bad_segments_" + name] = len(segs)
            out["m_over_h_" + name] = round(med["m" + name] / med["h" + name], 4)
            if len(segs):  # algorithmic bytes: k fragments read, e written per bad segment
                for leg in ("m", "h"):
                    out[leg + "_TBps_" + name] = round(
                        len(segs) * (k + e) * F / (med[leg + name] * 1e-3) / 1e12, 3)
        if wide:
            out["m_over_f_1"] = round(med["m1"] / med["f1"], 4)
        return out

    run_legs(torch, legs, args, extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=["wide", "rs42"], required=True)
    ap.add_argument("--nseg", type=int, default=0, help="segments (default 256 / 64)")
    ap.add_argument("--frag-kib", type=int, default=0, help="fragment size (default 8192 / 512)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warm", type=int, default=30)
    ap.add_argument("--legs", default="", help="comma-separated legs to time (default: all)")
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
