#!/usr/bin/env python3
"""Parity accumulation on scattered shards against the batch forms, on one GPU.

Every pointer of the table forms is aimed into the batch layout the batch forms work on, so both
move the same bytes of the same buffers. Legs, `--reps` interleaved repetitions of `--iters` calls:

  --geometry cess   64 segments of RS(2,1), F = 8 MiB:
                      idx_batch / idx_ptrs   EncodeIdx of fragment 1 accumulating (3 F per segment);
                      upd_batch / upd_ptrs   Update with fragment 1 changed (4 F).
  --geometry wide   64 segments of RS(32,32), F = 512 KiB:
                      idx_batch / idx_ptrs   EncodeIdx of fragment 5 accumulating (65 F);
                      upd_batch / upd_ptrs   Update of 4 changed fragments (72 F).

A pointer-table call builds its table on the host, uploads it and waits for the upload before it
launches; the times are HIP events around `--iters` calls and include that. One JSON line per
repetition and leg, then a summary line with each leg's median ms and achieved bytes/s, to stdout
and appended to `--out` (default profiles/acc/ptrs_<geometry>.jsonl). Before the timing, a table
call's parity is compared bit for bit with the batch call's."""
import argparse
import ctypes
import json
import os
import sys
from ctypes import c_void_p

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=["cess", "wide"], required=True)
    ap.add_argument("--nseg", type=int, default=64)
    ap.add_argument("--frag-kib", type=int, default=0, help="fragment size (default 8192 / 512)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not args.frag_kib:
        args.frag_kib = 8192 if args.geometry == "cess" else 512
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    import cess_amd
    from cess_amd import _lib
    from acc_bench import emit, timed
    lib = _lib.load()
    k, m, idx, changed = (2, 1, 1, [1]) if args.geometry == "cess" else (32, 32, 5, [3, 11, 20, 29])
    nseg, F = args.nseg, args.frag_kib << 10
    dev = torch.device("cuda", 0)
    enc = cess_amd.New(k, m)
    d_data = torch.empty((nseg, k, F), dtype=torch.uint8, device=dev)
    d_new = torch.empty((nseg, k, F), dtype=torch.uint8, device=dev)
    cess_amd.fill_synthetic(d_data, k * F, nseg, 0, 0xCE55000B)
    cess_amd.fill_synthetic(d_new, k * F, nseg, 0, 0xCE55000C)
    p_batch = torch.full((nseg, m, F), 0x77, dtype=torch.uint8, device=dev)
    p_ptrs = p_batch.clone()
    torch.cuda.synchronize()
    fed, old, new = ((c_void_p * (nseg * k))() for _ in range(3))
    for s in range(nseg):
        fed[s * k + idx] = d_data.data_ptr() + (s * k + idx) * F
        for j in changed:
            old[s * k + j] = d_data.data_ptr() + (s * k + j) * F
            new[s * k + j] = d_new.data_ptr() + (s * k + j) * F
    par = (c_void_p * (nseg * m))(*[p_ptrs.data_ptr() + i * F for i in range(nseg * m)])
    flags = (ctypes.c_uint8 * k)(*[1 if j in changed else 0 for j in range(k)])
    st = torch.cuda.current_stream().cuda_stream

    def ok(rc):
        assert rc == 0, rc

    legs = {
        "idx_batch": lambda: ok(lib.cec_encode_idx_batch(
            enc._h, d_data.data_ptr() + idx * F, k * F, idx, p_batch.data_ptr(), nseg, F, 1, st)),
        "idx_ptrs": lambda: ok(lib.cec_encode_idx_ptrs(enc._h, fed, par, nseg, F, 1, st)),
        "upd_batch": lambda: ok(lib.cec_update_batch(
            enc._h, d_data.data_ptr(), d_new.data_ptr(), p_batch.data_ptr(), nseg, F, flags, st)),
        "upd_ptrs": lambda: ok(lib.cec_update_ptrs(enc._h, old, new, par, nseg, F, st)),
    }
    c = len(changed)
    seg_bytes = {"idx_batch": (1 + 2 * m) * F, "idx_ptrs": (1 + 2 * m) * F,
                 "upd_batch": (2 * c + 2 * m) * F, "upd_ptrs": (2 * c + 2 * m) * F}
    for fn in legs.values():  # every leg once: both parities took the same calls
        fn()
    torch.cuda.synchronize()
    assert torch.equal(p_batch, p_ptrs), "the table forms differ from the batch forms"
    for fn in legs.values():
        for _ in range(args.warm):
            fn()
    torch.cuda.synchronize()
    path = args.out or os.path.join(ROOT, "profiles", "acc", f"ptrs_{args.geometry}.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as out:
        ms = {name: [] for name in legs}
        for rep in range(args.reps):
            for name, fn in legs.items():
                t = timed(torch, fn, args.iters)
                ms[name].append(t)
                emit(out, {"geometry": args.geometry, "rep": rep, "leg": name,
                           "ms_per_call": round(t, 5)})
        summ = {"geometry": args.geometry, "summary": True, "reps": args.reps,
                "iters": args.iters, "segments": nseg, "fragment_bytes": F, "bit_exact": True}
        for name, v in ms.items():
            med = float(np.median(v))
            summ[name] = {"median_ms": round(med, 5), "min_ms": round(min(v), 5),
                          "max_ms": round(max(v), 5), "bytes_per_segment": seg_bytes[name],
                          "GBps": round(nseg * seg_bytes[name] / (med * 1e-3) / 1e9, 1)}
        emit(out, summ)


if __name__ == "__main__":
    main()
