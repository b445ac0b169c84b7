"""The script of the hash queue's mixed run (tests/test_gpu_hashq_resume.py) and a model of the
queue's ring, checked on the CPU: the GPU test plays script(SEED) on a queue of CAPACITY slots and
compares the queue's bookkeeping with the model's after every operation, so what this file asserts
is that the committed script is worth playing: it wraps the ring, mixes every kind of add, fills
the ring and puts resumed chains across the wrap point. Pure Python, no GPU and no library.

The model mirrors cess_amd/csrc/hashq_ring.h (tests/test_hashq_ring.py plays this script on the
ring itself and compares): adds in slot order as (slot0, n, blocks, done), a tick
of T blocks advances every add by min(T, blocks left), completed adds retire from the front only,
head is the oldest listed add's slot0 and an add of n chains is refused exactly when
tail + n - head > capacity."""

CAPACITY = 64
SEED = 6
KINDS = ("strided", "prefix", "resume", "ptrs", "concat")
TICKS = (1, 2, 3, 7)
# chain lengths: the padding edges, one to three blocks, and few long ones (at most 64 * 40 + 63)
SHORT = (0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 191, 192, 193, 247, 248, 255)
LONG = (64 * 9 + 17, 64 * 12, 64 * 20 + 56, 64 * 40 + 17, 64 * 40 + 63)


def sha256_blocks(length):
    """cess_amd.sha256_blocks, restated so that this file needs no library."""
    return (length >> 6) + (2 if (length & 63) >= 56 else 1)


class _Lcg:
    """Knuth's 64-bit LCG: the script must not change with a library's random stream."""

    def __init__(self, seed):
        self.s = (2 * seed + 1) & (2 ** 64 - 1)
        for _ in range(4):
            self.below(2)

    def below(self, k):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (self.s >> 33) % k

    def pick(self, seq):
        return seq[self.below(len(seq))]


def script(seed, nops=150):
    """The operations of the mixed run, a list of dicts: {"op": "tick", "T": T} or
    {"op": "add", "kind": kind, "n": chains, "length": bytes per chain, ...} with per (strided),
    prefix_len (prefix), start_len (resume), parts / part_len (concat; length ends in the last
    part). Whether the ring takes an add is not in the script: the model says."""
    rng = _Lcg(seed)
    ops = []
    for _ in range(nops):
        if rng.below(100) < 45:
            ops.append({"op": "tick", "T": rng.pick(TICKS)})
            continue
        kind = rng.pick(KINDS)
        n = 1 + rng.below(24) if rng.below(4) == 0 else 1 + rng.below(9)
        length = rng.pick(LONG) if rng.below(6) == 0 else rng.pick(SHORT)
        op = {"op": "add", "kind": kind, "n": n}
        if kind == "strided":
            op["per"] = 1 + rng.below(3)
        elif kind == "prefix":
            length = max(length, 64)
            op["prefix_len"] = 64 * (1 + rng.below(length >> 6))
        elif kind == "resume":
            op["start_len"] = 64 * rng.below((length >> 6) + 1)
        elif kind == "ptrs":
            length = max(length, 1)     # an empty tensor has no address to pass
        elif kind == "concat":
            parts, part_len = 1 + rng.below(3), 64 * (1 + rng.below(3))
            last = rng.pick((1, 55, 56, 63, 64, part_len))
            op["parts"], op["part_len"] = parts, part_len
            length = (parts - 1) * part_len + last
        op["length"] = length
        ops.append(op)
    return ops


def blocks_of(op):
    """Blocks the queue has to run for one chain of an add."""
    return sha256_blocks(op["length"]) - op.get("start_len", 0) // 64


class Ring:
    """The host bookkeeping of cec_hashq, without a GPU."""

    def __init__(self, capacity):
        self.cap = capacity
        self.head = self.tail = 0
        self.adds = []          # [slot0, n, blocks, done, ticket], not yet retired, in slot order
        self.next_ticket = 1

    def add(self, n, blocks):
        """The add's ticket; None where the queue refuses it (ring full), with nothing changed."""
        if n == 0:
            return 0
        if self.tail + n - self.head > self.cap:
            return None
        self.adds.append([self.tail, n, blocks, 0, self.next_ticket])
        self.tail += n
        self.next_ticket += 1
        return self.next_ticket - 1

    def tick(self, T):
        if T == 0:
            T = max((a[2] - a[3] for a in self.adds), default=0)
        for a in self.adds:
            a[3] += min(T, a[2] - a[3])
        while self.adds and self.adds[0][3] == self.adds[0][2]:
            self.adds.pop(0)
        self.head = self.adds[0][0] if self.adds else self.tail

    def done(self, ticket):
        for a in self.adds:
            if a[4] == ticket:
                return a[3] == a[2]
        return ticket < self.next_ticket

    @property
    def live_chains(self):
        return sum(a[1] for a in self.adds if a[3] < a[2])

    @property
    def blocks_left(self):
        return max((a[2] - a[3] for a in self.adds if a[3] < a[2]), default=0)

    def live_adds(self):
        return [a for a in self.adds if a[3] < a[2]]


def play(ops, capacity=CAPACITY):
    """Run the script on the model: per operation (op, ticket, ring); the ticket is None for a
    tick and for a refused add. The ring is the one live object, as it stands after the op."""
    ring = Ring(capacity)
    for op in ops:
        if op["op"] == "tick":
            ring.tick(op["T"])
            yield op, None, ring
        else:
            yield op, ring.add(op["n"], blocks_of(op)), ring


def test_ring_model_small():
    """The model on a ring of 8 by hand: a completed add behind a live one keeps its slots."""
    r = Ring(8)
    assert r.add(0, 5) == 0 and r.next_ticket == 1
    assert r.add(3, 4) == 1 and r.add(4, 1) == 2
    assert r.add(2, 1) is None and (r.tail, r.live_chains, r.blocks_left) == (7, 7, 4)
    r.tick(1)
    assert r.done(2) and not r.done(1) and not r.done(3)
    assert (r.head, r.live_chains, r.blocks_left) == (0, 3, 3)
    assert r.add(2, 1) is None        # add 2 is complete, but its slots lie behind add 1's
    assert r.add(1, 2) == 3
    r.tick(3)
    assert r.done(1) and r.done(3) and (r.head, r.tail, r.live_chains) == (8, 8, 0)
    assert r.add(8, 1) == 4 and r.add(1, 1) is None
    r.tick(0)
    assert r.done(4) and r.blocks_left == 0


def test_script_is_legal():
    """Every add of the script is one the library takes when the ring has room."""
    ops = script(SEED)
    assert ops == script(SEED)
    for op in ops:
        if op["op"] == "tick":
            assert op["T"] in TICKS
            continue
        length = op["length"]
        assert op["kind"] in KINDS and 1 <= op["n"] <= CAPACITY
        assert 0 <= length <= 64 * 40 + 63 and blocks_of(op) >= 1
        if op["kind"] == "prefix":
            assert op["prefix_len"] % 64 == 0 and 0 < op["prefix_len"] <= length
        if op["kind"] == "resume":
            assert op["start_len"] % 64 == 0 and op["start_len"] <= length & ~63
        if op["kind"] == "concat":
            assert (op["parts"] - 1) * op["part_len"] < length <= op["parts"] * op["part_len"]
            assert op["part_len"] % 64 == 0 and op["part_len"] > 0


def test_committed_script_wraps_mixes_and_fills():
    ops = script(SEED)
    assert {op["T"] for op in ops if op["op"] == "tick"} == set(TICKS)
    chains, taken, refused, straddle, mixed = 0, {k: 0 for k in KINDS}, 0, 0, 0
    kind_of = {}
    for op, ticket, ring in play(ops):
        if op["op"] == "add":
            if ticket is None:
                refused += 1
                continue
            chains += op["n"]
            taken[op["kind"]] += 1
            kind_of[ticket] = op["kind"]
            slot0 = ring.adds[-1][0]
            if op["kind"] == "resume" and slot0 % CAPACITY + op["n"] > CAPACITY:
                straddle += 1
        elif len({kind_of[a[4]] for a in ring.live_adds()}) >= 3:
            mixed += 1
    assert chains >= 4 * CAPACITY, chains           # the ring wraps at least three times
    assert min(taken.values()) >= 3, taken
    assert refused >= 1
    assert straddle >= 1
    assert mixed >= 1
