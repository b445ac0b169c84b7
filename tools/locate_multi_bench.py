#!/usr/bin/env python3
"""One or two corrupt fragments found from parity (cec_locate_multi_ptrs, max_bad = 2) against
cec_locate_ptrs, at tools/locate_bench.py's four shapes:

  --geometry rs32   64 segments of RS(32,32), F = 512 KiB      four checks: the pair rule
  --geometry rs10   64 segments of RS(10,4),  F = 512 KiB      four checks: the pair rule
  --geometry rs4    256 segments of RS(4,2),  F = 512 KiB      two checks: the single rule
  --geometry rs21   64 segments of RS(2,1),   F = 8 MiB        one check: detect only

Every fragment is held, in one allocation per store. The data is synthetic and the parity the
codec's own batch encode. Stores: clean; every segment with one bad shard (one bit in the
middle); every segment with a pair that meets (one bit each at one offset); every segment with a
disjoint pair (one bit each, a quarter and three quarters into the fragment), the last two only
where the code has four checks. Legs, `--reps` interleaved repetitions of `--iters` calls:
    p0, q0   cec_locate_ptrs over the clean store, twice: q0 / p0 is the spread the call shows
             against itself under the same alternation;
    m0       cec_locate_multi_ptrs (max_bad = 2) over the clean store;
    m1, mmeet, mdisj   the same call over the dirty stores.
Each leg's output is checked before the timing starts. One JSON line per repetition and leg, then
one summary line. Times are HIP events around `--iters` calls."""
import argparse
import os
import sys
from ctypes import c_void_p

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.locate_bench import SHAPES  # noqa: E402
from tools.ptrs_bench import run_legs  # noqa: E402  (same warm-up, interleaving and summary)


def geometry(torch, cess_amd, args):
    from cess_amd import _lib
    lib = _lib.load()
    k, m, nseg, kib = SHAPES[args.geometry]
    nseg, F = args.nseg or nseg, (args.frag_kib or kib) << 10
    n, r = k + m, min(4, m)
    dev = torch.device("cuda", 0)
    enc = cess_amd.New(k, m)
    data = torch.empty((nseg, k, F), dtype=torch.uint8, device=dev)
    par = torch.empty((nseg, m, F), dtype=torch.uint8, device=dev)
    cess_amd.fill_synthetic(data, k * F, nseg, 0, 0xCE55004D)
    enc.EncodeBatch(data, par, nseg, F)
    torch.cuda.synchronize()
    loads = ["0", "1"] + (["meet", "disj"] if r == 4 else [])
    stores, bad = {}, {}
    for name in loads:
        st = torch.cat([data, par], dim=1).contiguous()
        bad[name] = []
        for s in range(nseg):
            a, b = s % n, (s + 1 + s % (n - 1)) % n
            J = {"0": [], "1": [a], "meet": [a, b], "disj": [a, b]}[name]
            at = {"0": [], "1": [F // 2], "meet": [F // 2, F // 2],
                  "disj": [F // 4, 3 * F // 4]}[name]
            for j, x in zip(J, at):
                st[s, j, x] ^= 1
            bad[name].append(J)
        stores[name] = st
    del data, par
    d_flags = torch.empty((nseg, n), dtype=torch.uint8, device=dev)
    d_status = torch.empty(nseg, dtype=torch.uint8, device=dev)
    d_nbad = torch.empty(nseg, dtype=torch.uint8, device=dev)

    def ptrs_of(st):
        base = st.data_ptr()
        return (c_void_p * (nseg * n))(*[base + i * F for i in range(nseg * n)])

    ptrs = {name: ptrs_of(stores[name]) for name in loads}
    stream = torch.cuda.current_stream(dev).cuda_stream

    def leg_single():
        rc = lib.cec_locate_ptrs(enc._h, ptrs["0"], nseg, F, 4, d_flags.data_ptr(),
                                 d_status.data_ptr(), stream)
        assert rc == 0, rc

    def leg_multi(name):
        def run():
            rc = lib.cec_locate_multi_ptrs(enc._h, ptrs[name], nseg, F, 4, 2, d_flags.data_ptr(),
                                           d_status.data_ptr(), d_nbad.data_ptr(), stream)
            assert rc == 0, rc
        return run

    legs = {"p0": leg_single, "q0": leg_single}
    for name in loads:
        legs["m" + name] = leg_multi(name)

    checks = {}
    for name in loads:
        for t in (d_flags, d_status, d_nbad):
            t.fill_(0xA5)
        legs["m" + name]()
        torch.cuda.synchronize()
        want_st = np.zeros(nseg, np.uint8)
        want_fl = np.ones((nseg, n), np.uint8)
        want_nb = np.zeros(nseg, np.uint8)
        for s, J in enumerate(bad[name]):
            if not J:
                continue
            if r >= 2:
                want_st[s], want_nb[s] = _lib.CEC_LOCATE_FOUND, len(J)
                want_fl[s, J] = 0
            else:
                want_st[s] = _lib.CEC_LOCATE_AMBIGUOUS
                want_fl[s] = 0
        checks["m" + name] = bool(np.array_equal(d_status.cpu().numpy(), want_st) and
                                  np.array_equal(d_flags.cpu().numpy(), want_fl) and
                                  np.array_equal(d_nbad.cpu().numpy(), want_nb))
    d_flags.fill_(0xA5)
    d_status.fill_(0xA5)
    leg_single()
    torch.cuda.synchronize()
    checks["p0"] = checks["q0"] = bool((d_status == 0).all() and (d_flags == 1).all())
    assert all(checks.values()), checks

    def extra(ms):
        med = {x: float(np.median(v)) for x, v in ms.items()}
        held = nseg * n * F  # every held byte, read once by a clean call
        out = {"outputs_checked": checks, "k": k, "m": m, "segments": nseg, "fragment_bytes": F,
               "r": r, "spread_ms": {x: round(max(v) - min(v), 5) for x, v in ms.items()}}
        for x in med:
            out[x + "_GBps"] = round(held / med[x] / 1e6, 1)
        out["m0_over_p0"] = round(med["m0"] / med["p0"], 4)
        out["q0_over_p0"] = round(med["q0"] / med["p0"], 4)
        # the same alternation, repetition by repetition: the widest ratio either way
        out["m0_over_p0_range"] = [round(min(a / b for a, b in zip(ms["m0"], ms["p0"])), 4),
                                   round(max(a / b for a, b in zip(ms["m0"], ms["p0"])), 4)]
        out["q0_over_p0_range"] = [round(min(a / b for a, b in zip(ms["q0"], ms["p0"])), 4),
                                   round(max(a / b for a, b in zip(ms["q0"], ms["p0"])), 4)]
        for name in loads[1:]:
            out["m%s_over_m0" % name] = round(med["m" + name] / med["m0"], 4)
        return out

    run_legs(torch, legs, args, extra)
    enc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=sorted(SHAPES), required=True)
    ap.add_argument("--nseg", type=int, default=0)
    ap.add_argument("--frag-kib", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--legs", default="", help="comma-separated legs to time (default: all)")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    import cess_amd
    geometry(torch, cess_amd, args)


if __name__ == "__main__":
    main()
