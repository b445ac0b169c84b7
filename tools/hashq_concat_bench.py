#!/usr/bin/env python3
"""SegmentList hashes of scattered shards against the packed batch, on one GPU:
`--nseg` segments of RS(k, m) with `--frag-kib` KiB fragments (64 CESS segments: k = 2, m = 1,
8 MiB), every hash of their SegmentLists through one hash queue.

  a  HashQueue.add_segment_lists          the batch [nseg][k][F] + [nseg][m][F], packed
  b  HashQueue.add_segment_lists_device   the same bytes, every shard an allocation of its own
                                          (cec_hashq_add_concat_ptrs + cec_hashq_add_ptrs)
  c  HashQueue.add_segment_lists_device   the same bytes, the shards shuffled inside one
                                          allocation: scattered addresses, one mapping

Every leg then ticks `--tick` blocks at a time until the queue is empty: the same schedule; legs
b and c issue one more tick launch and a rebase launch where a fragment boundary falls inside a
tick.
The packed batch is copied from the scattered shards once before the timing, and the outputs of
the legs are compared (equal). `--reps` interleaved repetitions of `--iters` calls between HIP
events, after `--warm` calls each. One JSON line per repetition and leg, then a summary line, to
stdout and appended to `--out` (default profiles/hashq_concat/bench.jsonl). The GPU work runs in
a child process under `timeout`."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def child(args):
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    import cess_amd
    from acc_bench import emit, timed
    nseg, k, m, F = args.nseg, args.k, args.m, args.frag_kib << 10
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(61)
    shards = []
    for i in range(nseg * (k + m)):  # separate allocations
        t = torch.empty(F, dtype=torch.uint8, device=dev)
        cess_amd.fill_synthetic(t, F, 1, i, 0xCE55C0CA)
        shards.append(t)
    order = [int(x) for x in rng.permutation(len(shards))]  # a segment's shards lie anywhere
    segments = [[shards[order[s * (k + m) + j]] for j in range(k + m)] for s in range(nseg)]
    d_data = torch.empty((nseg, k, F), dtype=torch.uint8, device=dev)
    d_par = torch.empty((nseg, max(m, 1), F), dtype=torch.uint8, device=dev)
    for s, seg in enumerate(segments):
        for j in range(k):
            d_data[s, j].copy_(seg[j])
        for j in range(m):
            d_par[s, j].copy_(seg[k + j])
    arena = torch.empty(len(shards) * F, dtype=torch.uint8, device=dev)
    place = [int(x) for x in rng.permutation(len(shards))]
    shuffled = []
    for s, seg in enumerate(segments):
        row = [arena[i * F:(i + 1) * F] for i in place[s * (k + m):(s + 1) * (k + m)]]
        for v, t in zip(row, seg):
            v.copy_(t)
        shuffled.append(row)
    outs = {n: (torch.zeros((nseg, 64), dtype=torch.uint8, device=dev),
                torch.zeros((nseg, k + m, 64), dtype=torch.uint8, device=dev)) for n in "abc"}
    q = cess_amd.HashQueue(capacity=1 << 12)
    q.set_option(1, args.tick_mode)
    launches = {}

    def drain(n):
        ticks = 0
        while q.live_chains:
            q.tick(args.tick)
            ticks += 1
        launches[n] = ticks

    def packed():
        q.add_segment_lists(d_data, d_par, nseg, k, m, F, *outs["a"])
        drain("a")

    def scattered():
        q.add_segment_lists_device(segments, k, m, *outs["b"])
        drain("b")

    def one_allocation():
        q.add_segment_lists_device(shuffled, k, m, *outs["c"])
        drain("c")

    legs = {"a": packed, "b": scattered, "c": one_allocation}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    for n in "bc":
        assert torch.equal(outs["a"][0], outs[n][0]), f"segment hashes of leg {n} differ"
        assert torch.equal(outs["a"][1], outs[n][1]), f"fragment hashes of leg {n} differ"
    for fn in legs.values():
        for _ in range(args.warm):
            fn()
    torch.cuda.synchronize()
    path = args.out or os.path.join(ROOT, "profiles", "hashq_concat", "bench.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    hashed = nseg * (2 * k - 1 + m) * F  # fragment 0 once, through the prefix digest
    with open(path, "a") as out:
        ms = {n: [] for n in legs}
        for rep in range(args.reps):
            for n, fn in legs.items():
                t = timed(torch, fn, args.iters)
                ms[n].append(t)
                emit(out, {"rep": rep, "leg": n, "ms_per_call": round(t, 4)})
        summ = {"summary": True, "reps": args.reps, "iters": args.iters, "segments": nseg, "k": k,
                "m": m, "fragment_bytes": F, "tick_blocks": args.tick, "tick_mode": args.tick_mode,
                "hashed_bytes": hashed, "ticks_per_call": launches, "outputs_equal": True,
                "device": torch.cuda.get_device_name(0)}
        for n, v in ms.items():
            med = float(np.median(v))
            summ[n] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4),
                       "max_ms": round(max(v), 4),
                       "GBps": round(hashed / (med * 1e-3) / 1e9, 2)}
        emit(out, summ)
    q.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=64)
    ap.add_argument("-k", type=int, default=2)
    ap.add_argument("-m", type=int, default=1)
    ap.add_argument("--frag-kib", type=int, default=8192)
    ap.add_argument("--tick", type=int, default=5000, help="blocks per cec_hashq_tick")
    ap.add_argument("--tick-mode", type=int, default=0, help="CEC_HQOPT_TICK")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--warm", type=int, default=1)
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
