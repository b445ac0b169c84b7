#!/usr/bin/env python3
"""Scattered-shard and required-subset rebuilds on one GPU.

  --geometry cess   64 segments of RS(2,1), F = 8 MiB, fragment (seg mod 3) lost, every fragment its
                    own device buffer. Legs, `--reps` interleaved repetitions of `--iters` calls:
                      a  what cec_dist_degraded_read does at world 1: a D2D copy of each survivor
                         into a [nseg][k][F] + [nseg][m][F] staging batch, cec_reconstruct_batch
                         there, a D2D copy of each rebuilt fragment to its destination
                         (9 F moved per segment);
                      b  cec_reconstruct_ptrs on the scattered buffers (3 F per segment);
                      c  cec_reconstruct_batch alone on a batch already in its layout (the ceiling);
                      bl cec_reconstruct_ptrs with the addresses of that batch layout (table
                         addressing without the scattered placement).
  --geometry wide   64 segments of RS(32,32), F = 512 KiB, 8 random fragments lost per segment.
                      some1  cec_reconstruct_some_batch, one lost fragment required per segment;
                      all8   cec_reconstruct_batch of the same patterns (all 8 rebuilt);
                      one1   one fragment lost and rebuilt (the k_rtb restoral case).
                    With the share of segments each leg sent to the FFT-domain decoders.

One JSON line per repetition and leg, then one summary line. Every leg's output is compared with
the codewords before the timing starts. Times are HIP events around `--iters` calls."""
import argparse
import json
import os
import sys
from ctypes import c_void_p

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def run_legs(torch, legs, args, extra):
    if args.legs:  # a profiler run of some legs only
        legs = {name: fn for name, fn in legs.items() if name in args.legs.split(",")}
    for name, fn in legs.items():  # warm every leg: code objects, plans, clocks
        for _ in range(args.warm):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for rep in range(args.reps):
        for name, fn in legs.items():
            t = timed(torch, fn, args.iters)
            ms[name].append(t)
            print(json.dumps({"geometry": args.geometry, "rep": rep, "leg": name,
                              "ms_per_call": round(t, 5)}), flush=True)
    summ = {"geometry": args.geometry, "summary": True, "reps": args.reps, "iters": args.iters}
    for name, v in ms.items():
        summ[name] = {"median_ms": round(float(np.median(v)), 5), "min_ms": round(min(v), 5),
                      "max_ms": round(max(v), 5)}
    if not args.legs:
        summ.update(extra(ms))
    print(json.dumps(summ), flush=True)


def cess_geometry(torch, cess_amd, args):
    from cess_amd import _lib
    lib = _lib.load()
    k, m, nseg, F = 2, 1, args.nseg, args.frag_kib << 10
    n = k + m
    dev = torch.device("cuda", 0)
    enc = cess_amd.New(k, m)
    ref_d = torch.empty((nseg, k, F), dtype=torch.uint8, device=dev)
    ref_p = torch.empty((nseg, m, F), dtype=torch.uint8, device=dev)
    cess_amd.fill_synthetic(ref_d, k * F, nseg, 0, 0xCE550009)
    enc.EncodeBatch(ref_d, ref_p, nseg, F)
    torch.cuda.synchronize()

    def ref(s, i):
        return ref_d[s, i] if i < k else ref_p[s, i - k]

    lost = [s % n for s in range(nseg)]
    present = np.ones((nseg, n), np.uint8)
    for s in range(nseg):
        present[s, lost[s]] = 0
    # scattered: every surviving fragment and every destination its own allocation, shuffled
    rng = np.random.default_rng(9)
    frag, out = {}, {}
    for j in rng.permutation(nseg * n):
        s, i = divmod(int(j), n)
        if i == lost[s]:
            out[s] = torch.zeros(F, dtype=torch.uint8, device=dev)
        else:
            frag[(s, i)] = ref(s, i).clone()
    st_d = torch.zeros((nseg, k, F), dtype=torch.uint8, device=dev)
    st_p = torch.zeros((nseg, m, F), dtype=torch.uint8, device=dev)

    def slot(s, i):
        return st_d[s, i] if i < k else st_p[s, i - k]

    def leg_a():
        for (s, i), t in frag.items():
            slot(s, i).copy_(t, non_blocking=True)
        enc.ReconstructBatch(st_d, st_p, nseg, F, present)
        for s in range(nseg):
            out[s].copy_(slot(s, lost[s]), non_blocking=True)

    src = (c_void_p * (nseg * n))(*[frag[(s, i)].data_ptr() if (s, i) in frag else None
                                    for s in range(nseg) for i in range(n)])
    dst = (c_void_p * (nseg * n))(*[out[s].data_ptr() if i == lost[s] else None
                                    for s in range(nseg) for i in range(n)])

    def leg_b():
        rc = lib.cec_reconstruct_ptrs(enc._h, src, dst, nseg, F, None)
        assert rc == 0, rc

    bat_d, bat_p = ref_d.clone(), ref_p.clone()

    def leg_c():
        enc.ReconstructBatch(bat_d, bat_p, nseg, F, present)

    def bat(s, i):
        return bat_d[s, i] if i < k else bat_p[s, i - k]

    # the pointer table over the batch layout's own addresses: table addressing without the
    # scattered placement (separates the two when b is slower than c)
    src_l = (c_void_p * (nseg * n))(*[bat(s, i).data_ptr() if i != lost[s] else None
                                      for s in range(nseg) for i in range(n)])
    dst_l = (c_void_p * (nseg * n))(*[bat(s, i).data_ptr() if i == lost[s] else None
                                      for s in range(nseg) for i in range(n)])

    def leg_bl():
        rc = lib.cec_reconstruct_ptrs(enc._h, src_l, dst_l, nseg, F, None)
        assert rc == 0, rc

    def outputs_exact():
        return all(torch.equal(out[s], ref(s, lost[s])) for s in range(nseg))

    checks = {}
    for name, fn in (("a", leg_a), ("b", leg_b)):
        for s in range(nseg):
            out[s].zero_()
        fn()
        torch.cuda.synchronize()
        checks[name] = outputs_exact()
    for s in range(nseg):
        (bat_d[s, lost[s]] if lost[s] < k else bat_p[s, lost[s] - k]).zero_()
    leg_c()
    torch.cuda.synchronize()
    checks["c"] = bool(torch.equal(bat_d, ref_d) and torch.equal(bat_p, ref_p))
    for s in range(nseg):
        bat(s, lost[s]).zero_()
    leg_bl()
    torch.cuda.synchronize()
    checks["bl"] = bool(torch.equal(bat_d, ref_d) and torch.equal(bat_p, ref_p))

    def extra(ms):
        med = {x: float(np.median(v)) for x, v in ms.items()}
        spread = {x: max(v) - min(v) for x, v in ms.items()}
        return {"bit_exact": checks, "segments": nseg, "fragment_bytes": F,
                "b_over_a": round(med["b"] / med["a"], 4),
                "b_over_c": round(med["b"] / med["c"], 4),
                "a_minus_b_ms": round(med["a"] - med["b"], 5),
                "b_minus_c_ms": round(med["b"] - med["c"], 5),
                "bl_minus_c_ms": round(med["bl"] - med["c"], 5),
                "spread_ms": {x: round(v, 5) for x, v in spread.items()},
                "b_GBps_3F": round(nseg * 3 * F / (med["b"] * 1e-3) / 1e9, 1),
                "c_GBps_3F": round(nseg * 3 * F / (med["c"] * 1e-3) / 1e9, 1)}

    run_legs(torch, {"a": leg_a, "b": leg_b, "c": leg_c, "bl": leg_bl}, args, extra)


def wide_geometry(torch, cess_amd, args):
    from cess_amd import _lib
    k = m = 32
    n, nseg, F = k + m, args.nseg, args.frag_kib << 10
    dev = torch.device("cuda", 0)
    # one codec per leg: a codec keeps the plan of its last per-segment pattern array only
    enc, enc_all, enc_one = (cess_amd.New(k, m) for _ in range(3))
    d_data = torch.empty((nseg, k, F), dtype=torch.uint8, device=dev)
    d_par = torch.empty((nseg, m, F), dtype=torch.uint8, device=dev)
    cess_amd.fill_synthetic(d_data, k * F, nseg, 0, 0xCE55000A)
    enc.EncodeBatch(d_data, d_par, nseg, F)
    torch.cuda.synchronize()
    ref_d, ref_p = d_data.clone(), d_par.clone()
    rng = np.random.default_rng(0xCE55)
    pres8 = np.ones((nseg, n), np.uint8)
    req1 = np.zeros((nseg, n), np.uint8)
    pres1 = np.ones((nseg, n), np.uint8)
    for s in range(nseg):
        lost = rng.choice(n, size=8, replace=False)
        pres8[s, lost] = 0
        req1[s, lost[0]] = 1
        pres1[s, lost[0]] = 0
    legs = {
        "some1": lambda: enc.ReconstructSomeBatch(d_data, d_par, nseg, F, pres8, req1),
        "all8": lambda: enc_all.ReconstructBatch(d_data, d_par, nseg, F, pres8),
        "one1": lambda: enc_one.ReconstructBatch(d_data, d_par, nseg, F, pres1),
    }
    encs = {"some1": enc, "all8": enc_all, "one1": enc_one}
    # each leg once on zeroed outputs: the required shards come back, the codeword stays whole
    checks, share = {}, {}
    for name, fn in legs.items():
        want = req1 if name != "all8" else 1 - pres8
        for s in range(nseg):
            for i in np.flatnonzero(want[s]):
                (d_data[s, i] if i < k else d_par[s, i - k]).zero_()
        fn()
        torch.cuda.synchronize()
        checks[name] = bool(torch.equal(d_data, ref_d) and torch.equal(d_par, ref_p))
        share[name] = {"fftdec": encs[name].stat(_lib.CEC_STAT_FFTDEC_SEGMENTS) / nseg,
                       "fftdec_d": encs[name].stat(_lib.CEC_STAT_FFTDEC_D_SEGMENTS) / nseg}

    def extra(ms):
        med = {x: float(np.median(v)) for x, v in ms.items()}
        return {"bit_exact": checks, "fftdec_segment_share": share, "segments": nseg,
                "fragment_bytes": F,
                "some1_over_all8": round(med["some1"] / med["all8"], 4),
                "some1_over_one1": round(med["some1"] / med["one1"], 4),
                "some1_TBps_33F": round(nseg * 33 * F / (med["some1"] * 1e-3) / 1e12, 3),
                "one1_TBps_33F": round(nseg * 33 * F / (med["one1"] * 1e-3) / 1e12, 3),
                "all8_TBps_40F": round(nseg * 40 * F / (med["all8"] * 1e-3) / 1e12, 3)}

    run_legs(torch, legs, args, extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=["cess", "wide"], required=True)
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
    (cess_geometry if args.geometry == "cess" else wide_geometry)(torch, cess_amd, args)


if __name__ == "__main__":
    main()
