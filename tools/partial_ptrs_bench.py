#!/usr/bin/env python3
"""Partial rebuild of scattered fragments in place against the staged form, and the scattered XOR
against cec_xor_batch, on one GPU.

  --geometry wide   64 segments of RS(32,32), F = 512 KiB, one fragment lost per segment, the part
                    holding 4 of the 32 survivors; the decoder receives 7 partials per fragment.
  --geometry cess   64 segments of RS(2,1), F = 8 MiB, one fragment lost, one survivor held; the
                    decoder receives 1 partial per fragment.

Legs, `--reps` interleaved repetitions of `--iters` calls:
    p   cec_reconstruct_partial_ptrs (accumulate = 0), every fragment and every output its own
        allocation, made in shuffled order;
    pa  the same with accumulate = 1 (the outputs are read too);
    s   what the gather does today, of calls that exist without the pointer-table form: a D2D copy
        of each held survivor into a [nseg][k][F] + [nseg][m][F] staging batch,
        cec_reconstruct_partial_batch there, a D2D copy of each output to its destination;
    x   the decoder side: one cec_xor_ptrs call over every lost fragment and its partials, each
        its own allocation;
    xb  a loop of cec_xor_batch calls, one per lost fragment, its partials contiguous.

The outputs of p and s, and of x and xb, are compared on the same seeded input before the timing
starts. One JSON line per repetition and leg, then one summary line. Times are HIP events around
`--iters` calls."""
import argparse
import os
import sys
from ctypes import c_uint8, c_void_p

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.ptrs_bench import run_legs  # noqa: E402  (same warm-up, interleaving and summary)


def geometry(torch, cess_amd, args):
    from cess_amd import _lib
    lib = _lib.load()
    wide = args.geometry == "wide"
    k, m = (32, 32) if wide else (2, 1)
    nheld, nrecv = (4, 7) if wide else (1, 1)
    n, nseg, F = k + m, args.nseg, args.frag_kib << 10
    dev = torch.device("cuda", 0)
    enc = cess_amd.New(k, m)
    ref_d = torch.empty((nseg, k, F), dtype=torch.uint8, device=dev)
    ref_p = torch.empty((nseg, m, F), dtype=torch.uint8, device=dev)
    cess_amd.fill_synthetic(ref_d, k * F, nseg, 0, 0xCE55000C)
    enc.EncodeBatch(ref_d, ref_p, nseg, F)
    torch.cuda.synchronize()

    def ref(s, i):
        return ref_d[s, i] if i < k else ref_p[s, i - k]

    lost = [s % n for s in range(nseg)]
    present = np.ones((nseg, n), np.uint8)
    held = np.zeros((nseg, n), np.uint8)
    surv = np.zeros(k, dtype=np.uint8)
    for s in range(nseg):
        present[s, lost[s]] = 0
        assert lib.cec_survivors(k, m, present[s].ctypes.data, surv.ctypes.data) == 0
        held[s, surv[::k // nheld][:nheld]] = 1
    # scattered: every held survivor and every output its own allocation, in shuffled order
    rng = np.random.default_rng(12)
    frag, out_p, out_s = {}, {}, {}
    for j in rng.permutation(nseg * n):
        s, i = divmod(int(j), n)
        if i == lost[s]:
            out_p[s] = torch.zeros(F, dtype=torch.uint8, device=dev)
            out_s[s] = torch.zeros(F, dtype=torch.uint8, device=dev)
        elif held[s, i]:
            frag[(s, i)] = ref(s, i).clone()
    src = (c_void_p * (nseg * n))(*[frag[(s, i)].data_ptr() if (s, i) in frag else None
                                    for s in range(nseg) for i in range(n)])
    dst = (c_void_p * (nseg * n))(*[out_p[s].data_ptr() if i == lost[s] else None
                                    for s in range(nseg) for i in range(n)])
    flags = (c_uint8 * (nseg * n))(*[int(x) for x in present.reshape(-1)])

    def leg_p():
        rc = lib.cec_reconstruct_partial_ptrs(enc._h, src, dst, flags, nseg, F, 0, None)
        assert rc == 0, rc

    def leg_pa():
        rc = lib.cec_reconstruct_partial_ptrs(enc._h, src, dst, flags, nseg, F, 1, None)
        assert rc == 0, rc

    st_d = torch.zeros((nseg, k, F), dtype=torch.uint8, device=dev)
    st_p = torch.zeros((nseg, m, F), dtype=torch.uint8, device=dev)

    def slot(s, i):
        return st_d[s, i] if i < k else st_p[s, i - k]

    def leg_s():
        for (s, i), t in frag.items():
            slot(s, i).copy_(t, non_blocking=True)
        enc.ReconstructPartialBatch(st_d, st_p, nseg, F, present, held)
        for s in range(nseg):
            out_s[s].copy_(slot(s, lost[s]), non_blocking=True)

    # the decoder side: nrecv partials per lost fragment (any bytes will do for a XOR)
    part_b = torch.empty((nseg, nrecv, F), dtype=torch.uint8, device=dev)
    cess_amd.fill_synthetic(part_b, nrecv * F, nseg, 0, 0xCE55000D)
    parts, acc_x, acc_b = {}, {}, torch.zeros((nseg, F), dtype=torch.uint8, device=dev)
    for j in rng.permutation(nseg * (nrecv + 1)):
        s, i = divmod(int(j), nrecv + 1)
        if i == nrecv:
            acc_x[s] = torch.zeros(F, dtype=torch.uint8, device=dev)
        else:
            parts[(s, i)] = part_b[s, i].clone()
    xd = (c_void_p * nseg)(*[acc_x[s].data_ptr() for s in range(nseg)])
    xs = (c_void_p * (nseg * nrecv))(*[parts[(s, i)].data_ptr() for s in range(nseg)
                                       for i in range(nrecv)])

    def leg_x():
        rc = lib.cec_xor_ptrs(enc._h, xd, xs, nseg, nrecv, F, None)
        assert rc == 0, rc

    def leg_xb():
        for s in range(nseg):
            cess_amd.xor_batch(acc_b[s], part_b[s], nrecv, F, F)

    # equality first, on the same input
    leg_p()
    leg_s()
    leg_x()
    leg_xb()
    torch.cuda.synchronize()
    checks = {"p_equals_s": all(torch.equal(out_p[s], out_s[s]) for s in range(nseg)),
              "x_equals_xb": all(torch.equal(acc_x[s], acc_b[s]) for s in range(nseg)),
              "p_nonzero": bool(out_p[0].any())}
    assert all(checks.values()), checks

    legs = {"p": leg_p, "pa": leg_pa, "s": leg_s, "x": leg_x, "xb": leg_xb}

    def extra(ms):
        med = {x: float(np.median(v)) for x, v in ms.items()}
        spread = {x: round(max(v) - min(v), 5) for x, v in ms.items()}
        tb = lambda nbytes, t: round(nbytes / (t * 1e-3) / 1e12, 3)  # noqa: E731
        return {"outputs_checked": checks, "k": k, "m": m, "segments": nseg, "fragment_bytes": F,
                "held_per_segment": nheld, "partials_received": nrecv, "spread_ms": spread,
                "p_over_s": round(med["p"] / med["s"], 4),
                "x_over_xb": round(med["x"] / med["xb"], 4),
                # algorithmic bytes: held F read, outputs F written (and read, with accumulate)
                "p_TBps": tb(nseg * (nheld + 1) * F, med["p"]),
                "pa_TBps": tb(nseg * (nheld + 2) * F, med["pa"]),
                "s_TBps_of_p_bytes": tb(nseg * (nheld + 1) * F, med["s"]),
                "x_TBps": tb(nseg * (nrecv + 2) * F, med["x"]),
                "xb_TBps": tb(nseg * (nrecv + 2) * F, med["xb"])}

    run_legs(torch, legs, args, extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=["wide", "cess"], required=True)
    ap.add_argument("--nseg", type=int, default=64)
    ap.add_argument("--frag-kib", type=int, default=0, help="fragment size (default 512 / 8192)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warm", type=int, default=30)
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
