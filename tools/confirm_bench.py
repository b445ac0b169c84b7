#!/usr/bin/env python3
"""Proving a repair by hashing only what was rebuilt, against the second scrub it replaces
(DESIGN §5).

  --geometry rs21   1,024 segments of RS(2,1), F = 8 MiB: 3,072 fragments.
  --geometry wide   1,024 segments of RS(32,32), F = 512 KiB: 65,536 fragments.

Every fragment is held and has its address in the pointer table; the recorded hashes are the
fragments' own, hashed once on the GPU before anything is timed. One fragment in each of 1
segment, 1 % and 10 % of the segments counts as rebuilt: its scrub flag is 0 and its segment's
status CEC_FLAG_REBUILT. Legs, `--reps` interleaved repetitions of `--iters` calls:
    c1, c1pct, c10pct  confirm: cec_hashq_add_check_where_ptrs over the whole table, gated on the
                       statuses, cec_hashq_finish, cec_confirm_flagged;
    scrub              the proof without it, audit.scrub_device's C calls over every held
                       fragment: cec_hashq_add_check_concat_ptrs (parts == 1), cec_hashq_finish;
    l1, l1pct, l10pct  a control: the same two calls over a list of the rebuilt fragments alone,
                       built on the host beforehand (what a host that had read the flags and
                       statuses back could add; the read-back is not in the leg);
    a10pct             l10pct's count of fragments, but adjacent ones in the table: what the
                       placement of the rebuilt fragments in memory costs the ticks.
All go through the C calls with prebuilt pointer arrays, so the host's share is the library's
and not the arrays' construction. Each leg's flags are compared with what is expected before the
timing starts. One JSON line per repetition and leg, then one summary line. Times are HIP events
around `--iters` calls.

  --profile         for a run under `rocprofv3 --kernel-trace --stats --output-format csv`: every
                    leg once, warm, each ended by one k_confirm_flagged launch.
  --trace CSV       no GPU: sum the k_sha256_tick time of each leg of such a run from its
                    kernel_trace.csv, one JSON line."""
import argparse
import csv
import json
import os
import sys
from ctypes import byref, c_uint64, c_void_p

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.ptrs_bench import run_legs  # noqa: E402  (same warm-up, interleaving and summary)

LOADS = {"c1": None, "c1pct": 0.01, "c10pct": 0.10}
LEGS = list(LOADS) + ["scrub"] + ["l" + name[1:] for name in LOADS] + ["a10pct"]


def tick_time_by_leg(path):
    """{leg: ms of k_sha256_tick kernels} from the kernel trace of a --profile run: the dispatches
    in start order, cut after every k_confirm_flagged; the first len(LEGS) pieces are the
    checked warm-up."""
    with open(path) as f:
        rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"])
                       for r in csv.DictReader(f)))
    pieces, cur = [], {"tick_ns": 0, "ticks": 0, "admits": 0}
    for a, b, name in rows:  # the set-up's hashing falls into the first warm-up piece
        cur["admits"] += "k_hashq_admit" in name
        if "k_sha256_tick" in name:
            cur["tick_ns"] += b - a
            cur["ticks"] += 1
        if "k_confirm_flagged" in name:
            pieces.append(cur)
            cur = {"tick_ns": 0, "ticks": 0, "admits": 0}
    assert len(pieces) == 2 * len(LEGS), len(pieces)
    return {leg: {"tick_ms": round(p["tick_ns"] / 1e6, 4), "tick_launches": p["ticks"],
                  "admit_launches": p["admits"]}
            for leg, p in zip(LEGS, pieces[len(LEGS):])}


def geometry(torch, cess_amd, args):
    from cess_amd import _lib
    lib = _lib.load()
    wide = args.geometry == "wide"
    k, m = (32, 32) if wide else (2, 1)
    n, nseg, F = k + m, args.nseg, args.frag_kib << 10
    N = nseg * n
    dev = torch.device("cuda", 0)
    store = torch.empty((N, F), dtype=torch.uint8, device=dev)
    step = max(1, (1 << 30) // F)
    for i0 in range(0, N, step):  # any bytes will do: the legs hash, they do not decode
        cess_amd.fill_synthetic(store[i0:], F, min(step, N - i0), i0, 0xCE55001B)
    ptrs = (c_void_p * N)(*[store.data_ptr() + i * F for i in range(N)])
    q = cess_amd.HashQueue(capacity=1 << max(0, N - 1).bit_length())
    d_rec = torch.empty((N, 64), dtype=torch.uint8, device=dev)
    ticket = c_uint64()
    assert lib.cec_hashq_add_ptrs(q._h, ptrs, N, F, d_rec.data_ptr(), byref(ticket)) == 0
    q.finish()
    torch.cuda.synchronize()

    rng = np.random.default_rng(27)
    loads = {}
    for name, share in LOADS.items():
        segs = np.sort(rng.choice(nseg, 1 if share is None else max(1, round(nseg * share)),
                                  replace=False))
        fl = np.ones((nseg, n), np.uint8)
        fl[segs, rng.integers(0, n, segs.size)] = 0
        st = np.zeros(nseg, np.uint8)
        st[segs] = _lib.CEC_FLAG_REBUILT
        loads[name] = (segs, fl, torch.from_numpy(fl).to(dev), torch.from_numpy(st).to(dev))
    d_ok = torch.empty(N, dtype=torch.uint8, device=dev)
    d_confirm = torch.empty(nseg, dtype=torch.uint8, device=dev)

    def leg_confirm(name):
        _, _, d_fl, d_st = loads[name]

        def run():
            rc = lib.cec_hashq_add_check_where_ptrs(
                q._h, ptrs, N, F, d_rec.data_ptr(), d_fl.data_ptr(), n, d_st.data_ptr(),
                _lib.CEC_FLAG_REBUILT, d_ok.data_ptr(), None, None)
            assert rc == 0, rc
            assert lib.cec_hashq_finish(q._h) == 0
            assert lib.cec_confirm_flagged(d_st.data_ptr(), d_ok.data_ptr(), nseg, n,
                                           d_confirm.data_ptr(), None) == 0
        return run

    def leg_list(idx):
        """The checked add of audit.scrub_device over fragments idx (None: all of them)."""
        cnt = N if idx is None else len(idx)
        lp = ptrs if idx is None else (c_void_p * cnt)(*[ptrs[i] for i in idx])
        d_exp = d_rec if idx is None else d_rec[torch.from_numpy(idx).to(dev)].contiguous()

        def run():
            rc = lib.cec_hashq_add_check_concat_ptrs(q._h, lp, cnt, 1, 0, F, d_exp.data_ptr(),
                                                     d_ok.data_ptr(), None, None, None)
            assert rc == 0, rc
            assert lib.cec_hashq_finish(q._h) == 0
            if args.profile:  # the cut of tick_time_by_leg
                assert lib.cec_confirm_flagged(loads["c1"][3].data_ptr(), d_ok.data_ptr(), nseg,
                                               n, d_confirm.data_ptr(), None) == 0
        return run

    legs = {name: leg_confirm(name) for name in LOADS}
    legs["scrub"] = leg_list(None)
    for name in LOADS:
        legs["l" + name[1:]] = leg_list(np.flatnonzero(loads[name][1].ravel() == 0))
    cnt = loads["c10pct"][0].size
    legs["a10pct"] = leg_list(np.arange(N // 3, N // 3 + cnt))

    checks = {}
    for name, fn in legs.items():
        d_ok.fill_(0xA5)
        d_confirm.fill_(0xA5)
        fn()
        torch.cuda.synchronize()
        ok = d_ok.cpu().numpy().reshape(nseg, n)
        if name not in LOADS:  # the first `rebuilt` flags (all of them for the scrub) are 1
            cnt = N if name == "scrub" else loads["c" + name[1:]][0].size
            flat = ok.ravel()
            checks[name] = bool((flat[:cnt] == 1).all()) and bool((flat[cnt:] == 0xA5).all())
            continue
        segs, fl = loads[name][:2]
        want = np.where(fl == 0, 1, _lib.CEC_HASHQ_SKIPPED)
        conf = np.zeros(nseg, np.uint8)
        conf[segs] = _lib.CEC_CONFIRM_PROVEN
        checks[name] = bool(np.array_equal(ok, want)) and \
            bool(np.array_equal(d_confirm.cpu().numpy(), conf))
    assert all(checks.values()), checks

    if args.profile:  # the checks above were the warm-up
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"geometry": args.geometry, "profile": True, "legs": LEGS}), flush=True)
        return

    def extra(ms):
        med = {x: float(np.median(v)) for x, v in ms.items()}
        out = {"outputs_checked": checks, "k": k, "m": m, "segments": nseg, "fragment_bytes": F,
               "fragments": N, "blocks_per_chain": cess_amd.sha256_blocks(F),
               "spread_ms": {x: round(max(v) - min(v), 5) for x, v in ms.items()}}
        for name in LOADS:
            out["rebuilt_" + name] = int(loads[name][0].size)
            out[name + "_over_scrub"] = round(med[name] / med["scrub"], 4)
            out[name + "_over_list"] = round(med[name] / med["l" + name[1:]], 4)
        return out

    run_legs(torch, legs, args, extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=["wide", "rs21"])
    ap.add_argument("--nseg", type=int, default=1024)
    ap.add_argument("--frag-kib", type=int, default=0, help="fragment size (default 8192 / 512)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--legs", default="", help="comma-separated legs to time (default: all)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--trace", default="", help="kernel_trace.csv of a --profile run")
    args = ap.parse_args()
    if args.trace:
        print(json.dumps({"geometry": args.geometry, "tick_time": tick_time_by_leg(args.trace)}))
        return
    if not args.geometry:
        ap.error("--geometry is required")
    if not args.frag_kib:
        args.frag_kib = 512 if args.geometry == "wide" else 8192
    import torch
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    import cess_amd
    geometry(torch, cess_amd, args)


if __name__ == "__main__":
    main()
