#!/usr/bin/env python3
"""Verify of scattered shards against the in-layout verify on one GPU.

  --geometry cess     64 segments of RS(2,1), F = 8 MiB. Legs, `--reps` interleaved repetitions of
                      `--iters` calls:
                        v   cec_verify_ptrs, every fragment its own allocation (shuffled order);
                        c   cec_verify_batch on a batch of the same bytes (the yardstick: the fused
                            read-only k_verify21);
                        vl  cec_verify_ptrs with the addresses of that batch (table addressing
                            without the scattered placement).
  --geometry generic  64 segments of RS(10,4), F = 512 KiB.
                        c   cec_verify_batch (parity re-encoded into scratch, then compared);
                        vl  cec_verify_ptrs with the batch's addresses (one read-only pass).

Every leg's flags are checked first, on clean codewords and with two segments corrupted. One JSON
line per repetition and leg, then one summary line. Times are HIP events around `--iters`
calls."""
import argparse
import json
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
    cess = args.geometry == "cess"
    k, m = (2, 1) if cess else (10, 4)
    n, nseg, F = k + m, args.nseg, args.frag_kib << 10
    dev = torch.device("cuda", 0)
    enc = cess_amd.New(k, m)
    bat_d = torch.empty((nseg, k, F), dtype=torch.uint8, device=dev)
    bat_p = torch.empty((nseg, m, F), dtype=torch.uint8, device=dev)
    cess_amd.fill_synthetic(bat_d, k * F, nseg, 0, 0xCE55000B)
    enc.EncodeBatch(bat_d, bat_p, nseg, F)
    torch.cuda.synchronize()

    def bat(s, i):
        return bat_d[s, i] if i < k else bat_p[s, i - k]

    def arrays(at):
        src = (c_void_p * (nseg * n))(*[at(s, i).data_ptr() if i < k else None
                                        for s in range(nseg) for i in range(n)])
        exp = (c_void_p * (nseg * n))(*[at(s, i).data_ptr() if i >= k else None
                                        for s in range(nseg) for i in range(n)])
        return src, exp

    ok = {name: torch.zeros(nseg, dtype=torch.uint8, device=dev) for name in ("v", "c", "vl")}
    src_l, exp_l = arrays(bat)

    def leg_c():
        enc.VerifyBatch(bat_d, bat_p, nseg, F, d_ok=ok["c"])

    def leg_vl():
        rc = lib.cec_verify_ptrs(enc._h, src_l, exp_l, nseg, F, ok["vl"].data_ptr(), None)
        assert rc == 0, rc

    legs = {"c": leg_c, "vl": leg_vl}
    where = {"c": bat, "vl": bat}
    if cess:  # scattered: every fragment its own allocation, in shuffled order
        rng = np.random.default_rng(11)
        frag = {}
        for j in rng.permutation(nseg * n):
            s, i = divmod(int(j), n)
            frag[(s, i)] = bat(s, i).clone()
        src_v, exp_v = arrays(lambda s, i: frag[(s, i)])

        def leg_v():
            rc = lib.cec_verify_ptrs(enc._h, src_v, exp_v, nseg, F, ok["v"].data_ptr(), None)
            assert rc == 0, rc

        legs = {"v": leg_v, "c": leg_c, "vl": leg_vl}
        where["v"] = lambda s, i: frag[(s, i)]

    # flags first: clean, then a parity byte of segment 1 and a data byte of the last segment
    checks = {}
    for name, fn in legs.items():
        at = where[name]
        ok[name].fill_(0x5A)
        fn()
        torch.cuda.synchronize()
        clean = ok[name].cpu().tolist() == [1] * nseg
        at(1, n - 1)[F - 1] ^= 0x01
        at(nseg - 1, 0)[F // 2] ^= 0x80
        fn()
        torch.cuda.synchronize()
        want = [0 if s in (1, nseg - 1) else 1 for s in range(nseg)]
        flagged = ok[name].cpu().tolist() == want
        at(1, n - 1)[F - 1] ^= 0x01
        at(nseg - 1, 0)[F // 2] ^= 0x80
        checks[name] = bool(clean and flagged)
    assert all(checks.values()), checks

    def extra(ms):
        med = {x: float(np.median(v)) for x, v in ms.items()}
        spread = {x: max(v) - min(v) for x, v in ms.items()}
        out = {"flags_checked": checks, "k": k, "m": m, "segments": nseg, "fragment_bytes": F,
               "vl_over_c": round(med["vl"] / med["c"], 4),
               "spread_ms": {x: round(v, 5) for x, v in spread.items()}}
        for x in med:
            out[f"{x}_TBps_{n}F"] = round(nseg * n * F / (med[x] * 1e-3) / 1e12, 3)
        if "v" in med:
            out["v_over_c"] = round(med["v"] / med["c"], 4)
        return out

    run_legs(torch, legs, args, extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=["cess", "generic"], required=True)
    ap.add_argument("--nseg", type=int, default=64)
    ap.add_argument("--frag-kib", type=int, default=0, help="fragment size (default 8192 / 512)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warm", type=int, default=30)
    ap.add_argument("--legs", default="", help="comma-separated legs to time (default: all)")
    args = ap.parse_args()
    if not args.frag_kib:
        args.frag_kib = 8192 if args.geometry == "cess" else 512
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    import cess_amd
    geometry(torch, cess_amd, args)


if __name__ == "__main__":
    main()
