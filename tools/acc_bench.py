#!/usr/bin/env python3
"""Parity accumulation on one GPU: EncodeIdx and Update against the full encode.

  --geometry cess   64 segments of RS(2,1), F = 8 MiB. Legs, `--reps` interleaved repetitions of
                    `--iters` calls:
                      encode    cec_encode_batch (the reference leg, 3 F per segment);
                      idx0_ow   EncodeIdx of fragment 0 overwriting (2 F);
                      idx1_acc  EncodeIdx of fragment 1 accumulating (3 F, the encode's bytes);
                      two_pass  both in a row: the streaming encode (5 F);
                      update1   Update with one of the two fragments changed (4 F).
  --geometry wide   RS(32,32), F = 512 KiB, 64 segments (1 GiB of data).
                      encode    cec_encode_batch, the FFT encode (64 F);
                      idx_acc   EncodeIdx of one fragment accumulating (65 F);
                      update<c> Update with c = 1, 2, 4, 8, 16 changed fragments ((2 c + 64) F);
                    and the number of changed fragments at which Update stops beating the encode.

Bytes per segment come from the shapes: EncodeIdx (1 + 2 m) F accumulating, (1 + m) F overwriting,
Update of c fragments (2 c + 2 m) F, encode (k + m) F. One JSON line per repetition and leg, then
one summary line with each leg's median ms and achieved bytes/s, to stdout and appended to `--out`
(default profiles/acc/<geometry>.jsonl). Every leg's result is compared bit for bit with the
encode before the timing starts. Times are HIP events around `--iters` calls."""
import argparse
import json
import os
import sys

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


def emit(out, row):
    line = json.dumps(row)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def run_legs(torch, legs, seg_bytes, args, out, extra):
    """legs: {name: fn}; seg_bytes: {name: bytes moved per segment}."""
    for fn in legs.values():  # warm every leg: code objects, clocks
        for _ in range(args.warm):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for rep in range(args.reps):
        for name, fn in legs.items():
            t = timed(torch, fn, args.iters)
            ms[name].append(t)
            emit(out, {"geometry": args.geometry, "rep": rep, "leg": name,
                       "ms_per_call": round(t, 5)})
    summ = {"geometry": args.geometry, "summary": True, "reps": args.reps, "iters": args.iters,
            "segments": args.nseg, "fragment_bytes": args.frag_kib << 10}
    med = {}
    for name, v in ms.items():
        med[name] = float(np.median(v))
        summ[name] = {"median_ms": round(med[name], 5), "min_ms": round(min(v), 5),
                      "max_ms": round(max(v), 5),
                      "bytes_per_segment": seg_bytes[name],
                      "GBps": round(args.nseg * seg_bytes[name] / (med[name] * 1e-3) / 1e9, 1),
                      "GBps_spread": round(args.nseg * seg_bytes[name] / 1e6 *
                                           (1 / min(v) - 1 / max(v)), 1)}
    summ.update(extra(med))
    emit(out, summ)


def cess_geometry(torch, cess_amd, args, out):
    k, m, nseg, F = 2, 1, args.nseg, args.frag_kib << 10
    dev = torch.device("cuda", 0)
    enc = cess_amd.New(k, m)
    d_data = torch.empty((nseg, k, F), dtype=torch.uint8, device=dev)
    d_new = torch.empty((nseg, k, F), dtype=torch.uint8, device=dev)
    ref_p = torch.empty((nseg, m, F), dtype=torch.uint8, device=dev)
    d_par = torch.empty((nseg, m, F), dtype=torch.uint8, device=dev)
    cess_amd.fill_synthetic(d_data, k * F, nseg, 0, 0xCE55000B)
    cess_amd.fill_synthetic(d_new, k * F, nseg, 0, 0xCE55000C)
    d_new[:, 0].copy_(d_data[:, 0])  # fragment 1 changed, fragment 0 as it was
    enc.EncodeBatch(d_data, ref_p, nseg, F)
    torch.cuda.synchronize()
    frag = [d_data.data_ptr() + i * F for i in range(k)]

    def idx0_ow():
        enc.EncodeIdxBatch(frag[0], k * F, 0, d_par, nseg, F, accumulate=False)

    def idx1_acc():
        enc.EncodeIdxBatch(frag[1], k * F, 1, d_par, nseg, F, accumulate=True)

    def two_pass():
        idx0_ow()
        idx1_acc()

    def update1():
        enc.UpdateBatch(d_data, d_new, d_par, nseg, F, [0, 1])

    checks = {}
    d_par.fill_(0x77)
    two_pass()
    torch.cuda.synchronize()
    checks["two_pass"] = bool(torch.equal(d_par, ref_p))
    update1()
    new_p = torch.empty_like(ref_p)
    enc.EncodeBatch(d_new, new_p, nseg, F)
    torch.cuda.synchronize()
    checks["update1"] = bool(torch.equal(d_par, new_p))
    del new_p
    assert all(checks.values()), checks
    enc_p = torch.empty_like(ref_p)
    legs = {"encode": lambda: enc.EncodeBatch(d_data, enc_p, nseg, F), "idx0_ow": idx0_ow,
            "idx1_acc": idx1_acc, "two_pass": two_pass, "update1": update1}
    seg_bytes = {"encode": (k + m) * F, "idx0_ow": (1 + m) * F, "idx1_acc": (1 + 2 * m) * F,
                 "two_pass": (2 + 3 * m) * F, "update1": (2 + 2 * m) * F}

    def extra(med):
        return {"bit_exact": checks,
                "idx1_acc_over_encode": round(med["idx1_acc"] / med["encode"], 4),
                "two_pass_over_encode": round(med["two_pass"] / med["encode"], 4)}

    run_legs(torch, legs, seg_bytes, args, out, extra)


def wide_geometry(torch, cess_amd, args, out):
    k = m = 32
    nseg, F = args.nseg, args.frag_kib << 10
    dev = torch.device("cuda", 0)
    enc = cess_amd.New(k, m)
    d_data = torch.empty((nseg, k, F), dtype=torch.uint8, device=dev)
    d_new = torch.empty((nseg, k, F), dtype=torch.uint8, device=dev)
    ref_p = torch.empty((nseg, m, F), dtype=torch.uint8, device=dev)
    d_par = torch.zeros((nseg, m, F), dtype=torch.uint8, device=dev)
    cess_amd.fill_synthetic(d_data, k * F, nseg, 0, 0xCE55000D)
    cess_amd.fill_synthetic(d_new, k * F, nseg, 0, 0xCE55000E)
    enc.EncodeBatch(d_data, ref_p, nseg, F)
    torch.cuda.synchronize()
    counts = [1, 2, 4, 8, 16]
    rng = np.random.default_rng(0xACC)
    masks = {}
    for c in counts:
        flags = np.zeros(k, np.uint8)
        flags[rng.choice(k, size=c, replace=False)] = 1
        masks[c] = flags

    checks = {}
    for i in range(k):  # every fragment once into zeroed parity
        enc.EncodeIdxBatch(d_data.data_ptr() + i * F, k * F, i, d_par, nseg, F)
    torch.cuda.synchronize()
    checks["idx_all"] = bool(torch.equal(d_par, ref_p))
    new_p = torch.empty_like(ref_p)
    mixed = torch.empty_like(d_data)
    for c in counts:
        d_par.copy_(ref_p)
        enc.UpdateBatch(d_data, d_new, d_par, nseg, F, masks[c])
        mixed.copy_(d_data)
        sel = torch.from_numpy(np.flatnonzero(masks[c])).to(dev)
        mixed[:, sel] = d_new[:, sel]
        enc.EncodeBatch(mixed, new_p, nseg, F)
        torch.cuda.synchronize()
        checks[f"update{c}"] = bool(torch.equal(d_par, new_p))
    del new_p, mixed
    assert all(checks.values()), checks
    enc_p = torch.empty_like(ref_p)
    legs = {"encode": lambda: enc.EncodeBatch(d_data, enc_p, nseg, F),
            "idx_acc": lambda: enc.EncodeIdxBatch(d_data.data_ptr() + 5 * F, k * F, 5, d_par,
                                                  nseg, F)}
    seg_bytes = {"encode": (k + m) * F, "idx_acc": (1 + 2 * m) * F}
    for c in counts:
        legs[f"update{c}"] = (lambda c=c: enc.UpdateBatch(d_data, d_new, d_par, nseg, F, masks[c]))
        seg_bytes[f"update{c}"] = (2 * c + 2 * m) * F

    def extra(med):
        slower = [c for c in counts if med[f"update{c}"] >= med["encode"]]
        return {"bit_exact": checks,
                "update_stops_beating_encode_at": slower[0] if slower else None,
                "changed_counts": counts}

    run_legs(torch, legs, seg_bytes, args, out, extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=["cess", "wide"], required=True)
    ap.add_argument("--nseg", type=int, default=64)
    ap.add_argument("--frag-kib", type=int, default=0, help="fragment size (default 8192 / 512)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--out", default="", help="JSON lines file (default profiles/acc/<geometry>.jsonl)")
    args = ap.parse_args()
    if not args.frag_kib:
        args.frag_kib = 8192 if args.geometry == "cess" else 512
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    import cess_amd
    path = args.out or os.path.join(ROOT, "profiles", "acc", f"{args.geometry}.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as out:
        (cess_geometry if args.geometry == "cess" else wide_geometry)(torch, cess_amd, args, out)


if __name__ == "__main__":
    main()
