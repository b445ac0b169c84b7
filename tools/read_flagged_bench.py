#!/usr/bin/env python3
"""A degraded read decided on the GPU against the host-decided one and a plain copy.

  --geometry rs21   64 segments of RS(2,1), F = 8 MiB.
  --geometry wide   64 segments of RS(10,4), F = 512 KiB.

Every fragment is held, in one allocation, and every data fragment is wanted in a joined
[nseg, k*F] tensor. The data is synthetic, the parity comes from the C oracle on the host. In 0, 1
or all segments one data fragment (fragment s % k of segment s) is flagged bad and holds junk.
Legs, `--reps` interleaved repetitions of `--iters` calls:
    r0, r1, rall   cec_read_flagged_ptrs on the flags in device memory: nothing copied out or
                   waited for;
    h0, h1, hall   the host-decided control: the flags copied to the host (a synchronising copy),
                   the patterns built there, cec_reconstruct_ptrs into the same destinations (data
                   only, sources: every good fragment), then torch copies of the good data
                   fragments;
    c              a plain device copy of the nseg * k * F joined bytes: the floor of a clean read.
All of r and the rebuild of h go through the C calls with prebuilt pointer arrays. Each leg's
output is compared with the original data before the timing starts. One JSON line per repetition
and leg, then one summary line. Times are HIP events around `--iters` calls."""
import argparse
import json
import os
import sys
from ctypes import c_void_p

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.ptrs_bench import run_legs  # noqa: E402  (same warm-up, interleaving and summary)

LOADS = ["0", "1", "all"]


def geometry(torch, cess_amd, args):
    from cess_amd import _lib
    from oracle.c_oracle import c_encode, load_c_oracle
    lib = _lib.load()
    wide = args.geometry == "wide"
    k, m = (10, 4) if wide else (2, 1)
    n, nseg, F = k + m, args.nseg, args.frag_kib << 10
    dev = torch.device("cuda", 0)
    enc = cess_amd.New(k, m)
    store = torch.empty((nseg, n, F), dtype=torch.uint8, device=dev)
    joined = torch.empty((nseg, k * F), dtype=torch.uint8, device=dev)  # the data, and leg c's source
    cess_amd.fill_synthetic(joined, k * F, nseg, 0, 0xCE55002A)
    torch.cuda.synchronize()
    corc = load_c_oracle()
    for s in range(nseg):  # the parity from the oracle, segment by segment
        data = joined[s].cpu().numpy().reshape(k, F)
        par = np.stack(c_encode(corc, k, m, list(data)))
        store[s, :k] = joined[s].view(k, F)
        store[s, k:] = torch.from_numpy(par).to(dev)
    pristine = store.clone()
    out = torch.empty((nseg, k * F), dtype=torch.uint8, device=dev)
    d_status = torch.empty(nseg, dtype=torch.uint8, device=dev)
    base, ob = store.data_ptr(), out.data_ptr()
    ptrs = (c_void_p * (nseg * n))(*[base + i * F for i in range(nseg * n)])
    dst = (c_void_p * (nseg * k))(*[ob + i * F for i in range(nseg * k)])
    max_bad = 1

    loads = {}
    for name in LOADS:
        segs = {"0": [], "1": [nseg // 2], "all": list(range(nseg))}[name]
        fl = np.ones((nseg, n), np.uint8)
        for s in segs:
            fl[s, s % k] = 0
        loads[name] = (segs, fl, torch.from_numpy(fl).to(dev))

    def spoil(name):
        """The store as load `name` finds it: junk in the fragments flagged bad."""
        store.copy_(pristine)
        for s in loads[name][0]:
            store[s, s % k].fill_(0x5A)

    def leg_read(name):
        d_fl = loads[name][2]

        def run():
            rc = lib.cec_read_flagged_ptrs(enc._h, ptrs, d_fl.data_ptr(), dst, nseg, F, max_bad,
                                           d_status.data_ptr(), None)
            assert rc == 0, rc
        return run

    def leg_host(name):
        d_fl = loads[name][2]

        def run():
            fl = d_fl.cpu().numpy()  # the round trip: waits for the stream, copies the flags out
            src = (c_void_p * (nseg * n))()
            rdst = (c_void_p * (nseg * n))()
            lost = []
            for s in range(nseg):
                bad = [j for j in range(k) if fl[s, j] == 0]
                for i in range(n):
                    if bad and fl[s, i] != 0:
                        src[s * n + i] = base + (s * n + i) * F
                for j in bad:
                    rdst[s * n + j] = ob + (s * k + j) * F
                lost.append(bad)
            if any(lost):
                rc = lib.cec_reconstruct_ptrs(enc._h, src, rdst, nseg, F, None)
                assert rc == 0, rc
            ov = out.view(nseg, k, F)
            for s in range(nseg):
                for j in range(k):
                    if j not in lost[s]:
                        ov[s, j].copy_(store[s, j])
        return run

    def leg_copy():
        out.copy_(joined)

    legs = {}
    for name in LOADS:
        legs["r" + name] = leg_read(name)
        legs["h" + name] = leg_host(name)
    legs["c"] = leg_copy

    checks = {}
    for name, fn in legs.items():
        if name != "c":
            spoil(name[1:])
        out.fill_(0xA5)
        d_status.fill_(0xA5)
        fn()
        torch.cuda.synchronize()
        checks[name] = bool(torch.equal(out, joined))
        if name[0] == "r":
            want = np.zeros(nseg, np.uint8)
            want[loads[name[1:]][0]] = _lib.CEC_FLAG_REBUILT
            checks[name] = checks[name] and bool(np.array_equal(d_status.cpu().numpy(), want))
    assert all(checks.values()), checks
    # the timed legs run over the pristine store: the flags, not the bytes, decide the work
    store.copy_(pristine)
    torch.cuda.synchronize()

    def extra(ms):
        med = {x: float(np.median(v)) for x, v in ms.items()}
        moved = 2 * nseg * k * F  # a clean read: every data byte read once and written once
        out_ = {"outputs_checked": checks, "k": k, "m": m, "segments": nseg, "fragment_bytes": F,
                "max_bad": max_bad,
                "spread_ms": {x: round(max(v) - min(v), 5) for x, v in ms.items()},
                "r0_GBps": round(moved / med["r0"] / 1e6, 1),
                "c_GBps": round(moved / med["c"] / 1e6, 1),
                "r0_over_c": round(med["r0"] / med["c"], 4)}
        for name in LOADS:
            out_["r%s_over_h%s" % (name, name)] = round(med["r" + name] / med["h" + name], 4)
        return out_

    run_legs(torch, legs, args, extra)
    enc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=["wide", "rs21"], required=True)
    ap.add_argument("--nseg", type=int, default=64)
    ap.add_argument("--frag-kib", type=int, default=0, help="fragment size (default 8192 / 512)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--legs", default="", help="comma-separated legs to time (default: all)")
    args = ap.parse_args()
    if not args.frag_kib:
        args.frag_kib = 512 if args.geometry == "wide" else 8192
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    import cess_amd
    geometry(torch, cess_amd, args)


if __name__ == "__main__":
    main()
