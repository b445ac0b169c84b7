"""The hash queue's host bookkeeping (cess_amd/csrc/hashq_ring.h) without a GPU: the ring is built
into a small program of its own (tests/native/hashq_ring.cpp) under AddressSanitizer +
UndefinedBehaviorSanitizer and plays the script of the mixed run and hand-written edges. After
every operation its tickets, head, tail, live chains, blocks left and done flags are those of the
Python model (tests/test_hashq_script.py::Ring), and every tick's launches keep the schedule that
chains over several buffers need, which the model knows nothing of: no launch crosses a part
boundary, and every boundary but the last gets its rebase, once, right after the launch that
reaches it."""
import copy
import os
import subprocess

import pytest

from tests import test_hashq_script as hs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ring_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("hashq_ring") / "hashq_ring"
    subprocess.run(["g++", "-std=c++20", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1", "-g",
                    f"{ROOT}/tests/native/hashq_ring.cpp", "-o", str(exe)], check=True)
    return str(exe)


def add(n, blocks, parts=1, part_blocks=0):
    return {"op": "add", "n": n, "blocks": blocks, "parts": parts, "part_blocks": part_blocks}


def tick(T):
    return {"op": "tick", "T": T}


def of_script(op):
    """An operation of test_hashq_script.script in the form above."""
    if op["op"] == "tick":
        return tick(op["T"])
    return add(op["n"], hs.blocks_of(op), op.get("parts", 1), op.get("part_len", 0) // 64)


def run(exe, capacity, ops):
    """Play ops on the native ring: per operation (ticket or None, launches, state, done flags),
    launches being [(head, span, step, live, [(ticket, part), ...]), ...]."""
    text = "".join("add %(n)d %(blocks)d %(parts)d %(part_blocks)d\n" % op if op["op"] == "add"
                   else "tick %(T)d\n" % op for op in ops)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(capacity)], input=text, capture_output=True, text=True,
                       timeout=60, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    out, cur = [], None
    for line in r.stdout.splitlines():
        w = line.split()
        if cur is None:
            cur = {"ticket": None, "launches": []}
        if w[0] == "ticket":
            cur["ticket"] = int(w[1])
        elif w[0] == "refused":
            pass
        elif w[0] == "launch":
            cur["launches"].append(tuple(int(x) for x in w[1:]) + ([],))
        elif w[0] == "rebase":
            cur["launches"][-1][4].append((int(w[1]), int(w[2])))
        elif w[0] == "state":
            cur["state"] = tuple(int(x) for x in w[1:])
        else:
            assert w[0] == "done"
            cur["done"] = w[1]
            out.append(cur)
            cur = None
    assert cur is None and len(out) == len(ops), r.stdout[-2000:]
    return out


def check(exe, capacity, ops):
    """The native ring against the model, operation by operation. Returns counters of what the
    run met, for the callers to assert that it met what it was written for."""
    ring = hs.Ring(capacity)
    concat = {}         # ticket -> [parts, part_blocks, the part its chains are based on]
    seen = {"refused": 0, "rebases": 0, "cut_ticks": 0, "two_in_one_tick": 0}
    for op, got in zip(ops, run(exe, capacity, ops)):
        if op["op"] == "add":
            want = ring.add(op["n"], op["blocks"])
            assert got["ticket"] == want and not got["launches"], (op, got)
            seen["refused"] += want is None
            if want and op["parts"] > 1:
                concat[want] = [op["parts"], op["part_blocks"], 0]
        else:
            before = ring.blocks_left
            T = op["T"] or before
            whole = copy.deepcopy(ring)
            whole.tick(op["T"])
            concat_live = any(a[4] in concat for a in ring.live_adds())
            boundaries, issued, effective = set(), 0, 0
            for head, span, step, live, rebases in got["launches"]:
                assert (head, span, live) == (ring.head, ring.tail - ring.head, ring.live_chains)
                assert step >= 1
                want_rebases = []
                for a in ring.live_adds():
                    if a[4] not in concat:
                        continue
                    parts, pb, based = concat[a[4]]
                    after = a[3] + min(step, a[2] - a[3])
                    # the launch reads blocks a[3] .. after - 1: all of them in the part `based`,
                    # or past every boundary that gets a rebase (the last part, then the padding)
                    if based + 1 < parts:
                        assert after <= (based + 1) * pb, (op, a, step)
                        if after == (based + 1) * pb:
                            want_rebases.append((a[4], based + 1))
                            concat[a[4]][2] = based + 1
                            boundaries.add(a[4])
                    else:
                        assert a[3] >= based * pb
                assert rebases == want_rebases, (op, rebases, want_rebases)
                seen["rebases"] += len(rebases)
                # a launch's step is the kernel's block limit: the last one of a tick may name
                # more blocks than any chain has left, as an uncut tick always has
                effective += min(step, ring.blocks_left)
                assert step <= T - issued
                issued += step
                ring.tick(step)
            assert effective == min(T, before), (op, got)
            assert issued == T or not ring.live_adds(), (op, got)
            # a tick is cut nowhere but at a boundary that needs a rebase
            assert all(l[4] for l in got["launches"][:-1]), (op, got)
            if not concat_live:
                assert len(got["launches"]) == (1 if before else 0), (op, got)
            assert (ring.head, ring.adds) == (whole.head, whole.adds)
            seen["cut_ticks"] += len(got["launches"]) > 1
            seen["two_in_one_tick"] += len(boundaries) > 1
        assert got["state"] == (ring.head, ring.tail, ring.live_chains, ring.blocks_left), (op, got)
        want_done = "".join("1" if ring.done(t) else "0" for t in range(ring.next_ticket + 1))
        assert got["done"] == want_done, (op, got)
    return seen


def test_ring_plays_the_mixed_script(ring_exe):
    seen = check(ring_exe, hs.CAPACITY, [of_script(op) for op in hs.script(hs.SEED)])
    assert seen["refused"] >= 1 and seen["rebases"] >= 1 and seen["cut_ticks"] >= 1, seen


def test_ring_edges(ring_exe):
    ops = [
        tick(0), tick(3),                       # nothing live: no launch
        add(0, 5),                              # no chains: ticket 0, nothing listed
        add(8, 3), add(1, 1), tick(0),          # fills the ring exactly; refused; drained
        add(2, 4, 3, 1), add(1, 9), tick(7),    # three parts of one block: every block a boundary
        add(1, 2, 1, 1),                        # one part: kept as a plain add
        tick(0),
        # boundaries at different blocks of one tick: A's at block 3, B's at blocks 2 and 4
        add(2, 7, 2, 3), add(1, 7, 3, 2), add(5, 2), add(1, 1),
        tick(1), tick(5), tick(1), tick(0), tick(0),
    ]
    seen = check(ring_exe, 8, ops)
    assert seen["refused"] == 2 and seen["two_in_one_tick"] >= 1, seen
    assert seen["rebases"] == 2 + 1 + 2, seen
