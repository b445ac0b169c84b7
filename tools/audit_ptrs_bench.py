#!/usr/bin/env python3
"""A miner's storage challenge on scattered fragments against the batch form, on one GPU
(DESIGN §5): `--nfrag` fragments of `--frag-kib` KiB (1,024 of 8 MiB), 47 challenged chunks of
each (385 MB of chunks).

The pointer form's fragments are `--distinct` separate allocations (as many as HBM comfortably
holds; the pointers repeat them in a shuffled order when there are fewer than nfrag); the batch
form's batch holds the same bytes in the same order, copied there once before the timing. Legs,
`--reps` interleaved repetitions of `--iters` calls between HIP events, after `--warm` calls each:

  a  cec_audit_chunks, chunks and hashes        (what had to be done before: needs the batch)
  b  cec_audit_chunks_ptrs, chunks and hashes
  c  cec_audit_chunks_ptrs, hashes only         (chunks hashed where they lie)
  d  cec_audit_chunks, hashes only              (chunks gathered into scratch, then hashed)

A pointer call builds its tables on the host, uploads them and waits for the upload before it
launches; the times include that. Before the timing the outputs of a, b, c and d are compared
(equal). One JSON line per repetition and leg, then a summary line, to stdout and appended to
`--out` (default profiles/audit_ptrs/bench.jsonl). The GPU work runs in a child process under
`timeout`."""
import argparse
import os
import subprocess
import sys
from ctypes import POINTER, c_uint32, c_void_p

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def child(args):
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    import cess_amd
    from cess_amd import _lib
    from acc_bench import emit, timed
    lib = _lib.load()
    nfrag, F, cc = args.nfrag, args.frag_kib << 10, 1024
    chunk = F // cc
    D = min(args.distinct, nfrag)
    dev = torch.device("cuda", 0)
    enc = cess_amd.New(1, 1)  # its data-only batch [nfrag][1][F] is a plain array of fragments
    rng = np.random.default_rng(47)
    idx = np.ascontiguousarray(rng.permutation(cc)[:47].astype(np.uint32))
    nidx = int(idx.size)
    frags = []
    for i in range(D):  # separate allocations
        t = torch.empty(F, dtype=torch.uint8, device=dev)
        cess_amd.fill_synthetic(t, F, 1, i, 0xCE55A0D1)
        frags.append(t)
    order = [int(x) % D for x in rng.permutation(nfrag)]
    batch = torch.empty((nfrag, 1, F), dtype=torch.uint8, device=dev)
    for f, o in enumerate(order):
        batch[f, 0].copy_(frags[o])
    ptrs = (c_void_p * nfrag)(*[frags[o].data_ptr() for o in order])
    outs = {n: (torch.zeros(nfrag * nidx * chunk, dtype=torch.uint8, device=dev) if n in "ab"
                else None,
                torch.zeros(nfrag * nidx * 64, dtype=torch.uint8, device=dev)) for n in "abcd"}
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    ip = idx.ctypes.data_as(POINTER(c_uint32))

    def ok(rc):
        assert rc == 0, rc

    def p(t):
        return None if t is None else t.data_ptr()

    def batch_call(n):
        return lambda: ok(lib.cec_audit_chunks(enc._h, batch.data_ptr(), None, nfrag, F, cc, ip,
                                               nidx, p(outs[n][0]), p(outs[n][1]), st))

    def ptrs_call(n):
        return lambda: ok(lib.cec_audit_chunks_ptrs(enc._h, ptrs, nfrag, F, cc, ip, nidx,
                                                    p(outs[n][0]), p(outs[n][1]), st))

    legs = {"a": batch_call("a"), "b": ptrs_call("b"), "c": ptrs_call("c"), "d": batch_call("d")}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    assert torch.equal(outs["a"][0], outs["b"][0]), "gathered chunks differ"
    for n in "bcd":
        assert torch.equal(outs["a"][1], outs[n][1]), f"hashes of leg {n} differ"
    for fn in legs.values():
        for _ in range(args.warm):
            fn()
    torch.cuda.synchronize()
    path = args.out or os.path.join(ROOT, "profiles", "audit_ptrs", "bench.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    gathered = nfrag * nidx * chunk
    # algorithmic bytes: the gather reads and writes the chunks; the pointer form's hashes read
    # them once more, the batch form's read the gathered copy; 64 bytes of hex per chunk
    moved = {"a": 3 * gathered, "b": 3 * gathered, "c": gathered, "d": 3 * gathered}
    with open(path, "a") as out:
        ms = {n: [] for n in legs}
        for rep in range(args.reps):
            for n, fn in legs.items():
                t = timed(torch, fn, args.iters)
                ms[n].append(t)
                emit(out, {"rep": rep, "leg": n, "ms_per_call": round(t, 5)})
        summ = {"summary": True, "reps": args.reps, "iters": args.iters, "fragments": nfrag,
                "distinct_fragments": D, "fragment_bytes": F, "indices": nidx,
                "gathered_bytes": gathered, "outputs_equal": True,
                "device": torch.cuda.get_device_name(0)}
        for n, v in ms.items():
            med = float(np.median(v))
            summ[n] = {"median_ms": round(med, 5), "min_ms": round(min(v), 5),
                       "max_ms": round(max(v), 5),
                       "GBps": round((moved[n] + nfrag * nidx * 64) / (med * 1e-3) / 1e9, 1)}
        emit(out, summ)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nfrag", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=1024)
    ap.add_argument("--frag-kib", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--timeout", type=int, default=300, help="seconds for the GPU step")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__),
           "--child"] + [a for a in sys.argv[1:]]
    sys.exit(subprocess.run(cmd).returncode)


if __name__ == "__main__":
    main()
