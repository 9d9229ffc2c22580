"""Pure-Python restatement of the many-keys rule of kangaroo mode (include/bsgs_hip.h, "Kangaroo, many keys"): the table of distinguished points with an owner
per entry, links between two unsolved keys, the conversion of a solved key's entries into tame ones, the assignment of wild kangaroos to keys, and a tiny
solver on the walk of tests/kangaroo_model.py.  A test model: no product code runs here."""
import kangaroo_model as K
from pybsgs.ecpy import add, mul, neg

WILD, DEAD, M128 = K.WILD, K.DEAD, K.M128
KEY_SHIFT = 8


def key_of(flags):
    return (flags >> KEY_SHIFT) & 0xFFFF


def wild_flags(key):
    return WILD | key << KEY_SHIFT


class MultiTable:
    """the host's table for a list of keys P_0 .. P_{L-1} in [a, a + W) (host_kangaroo_multi.cpp MultiKeyTable).  add() returns the events of one record:
    ('new',), ('repeat',), ('reseed', kangaroo), ('false',), ('link', j, k), ('found', k, key) -- one record can solve several keys through links."""

    def __init__(self, a, W, pubs):
        self.a, self.W, self.pubs = a, W, list(pubs)
        self.keys = [None] * len(self.pubs)
        self.map = {}                  # low 64 bits of x -> (d signed, kangaroo, owner): owner 0 tame, 1 + k wild of key k
        self.links = []                # (j, k, delta): k_j = k_k + delta
        self.false_matches = self.reseeds = self.links_kept = self.links_resolved = 0

    def solved(self):
        return sum(k is not None for k in self.keys)

    def presolve(self, k, key):
        """a key known before the search (P_k == a*G, or read from a work file)"""
        self.keys[k] = key

    def _as_tame(self, d, owner):
        """(d, owner) with a solved owner converted: tame, d' = d + (k_k - a)"""
        if owner and self.keys[owner - 1] is not None:
            return d + self.keys[owner - 1] - self.a, 0
        return d, owner

    def _verify(self, k, cand):
        return self.a <= cand < self.a + self.W and mul(cand) == self.pubs[k]

    def _found(self, k, key, ev):
        self.keys[k] = key
        ev.append(("found", k, key))
        mine = [l for l in self.links if k in (l[0], l[1])]
        self.links = [l for l in self.links if k not in (l[0], l[1])]
        for j, kk, delta in mine:
            other, cand = (kk, key - delta) if j == k else (j, key + delta)
            if self.keys[other] is not None:
                continue                                       # solved on another path meanwhile: nothing left to learn from this link
            if self._verify(other, cand):
                self.links_resolved += 1
                self._found(other, cand, ev)
            else:
                self.false_matches += 1

    def add(self, x, d, kid, flags):
        if flags & DEAD:
            self.reseeds += 1
            return [("reseed", kid)]
        k64 = x & 0xFFFFFFFFFFFFFFFF
        d = K.signed128(d)
        owner = 1 + key_of(flags) if flags & WILD else 0
        e = self.map.get(k64)
        if e is None:
            self.map[k64] = (d, kid, owner)
            return [("new",)]
        if e[1] == kid:
            return [("repeat",)]
        d1, o1 = self._as_tame(e[0], e[2])
        d2, o2 = self._as_tame(d, owner)
        if o1 == o2:
            self.reseeds += 1
            return [("reseed", kid)]
        if o1 == 0 or o2 == 0:
            k = (o1 or o2) - 1
            cand = self.a + (d1 - d2 if o1 == 0 else d2 - d1)  # d_T - d_W
            if self._verify(k, cand):
                ev = []
                self._found(k, cand, ev)
                return ev
            self.false_matches += 1
            return [("false",)]
        j, k = o1 - 1, o2 - 1                                  # stored entry's key j, the record's key k: k_j = k_k + d_k - d_j
        self.links.append((j, k, d2 - d1))
        self.links_kept += 1
        self.reseeds += 1
        return [("link", j, k), ("reseed", kid)]


class Assigner:
    """which key a wild kangaroo works on: wild kangaroo w of the run starts on the w-th key, cyclically, of the list without the keys solved up front; a
    re-seeded one keeps its key while that is unsolved, else takes the unsolved key with the fewest kangaroos, lowest list position first"""

    def __init__(self, L, presolved, n_wild):
        self.open = [k for k in range(L) if k not in presolved]
        self.count = [0] * L
        self.key = []
        for w in range(n_wild):
            k = self.open[w % len(self.open)]
            self.key.append(k)
            self.count[k] += 1

    def reseed(self, w, solved):
        """the key of wild kangaroo w from now on; solved = list position -> bool.  None when no key is open."""
        k = self.key[w]
        if not solved[k]:
            return k
        best = None
        for c in self.open:
            if not solved[c] and (best is None or self.count[c] < self.count[best]):
                best = c
        if best is not None:
            self.count[k] -= 1
            self.count[best] += 1
            self.key[w] = best
        return best


def solve_multi(pubs, a, b, seed=1, n=16, dp=None, max_steps=None):
    """tiny solver for the keys `pubs` in [a, b]: n kangaroos (half tame, half wild, the wild ones shared out by Assigner) walked one step at a time.
    -> (keys by list position, None where unsolved; steps; table)"""
    W = b - a + 1
    L = len(pubs)
    aG = mul(a)
    Qs = [add(p, neg(aG)) for p in pubs]
    sq = W ** 0.5
    if dp is None:
        dp = 0
        while n * (1 << (dp + 1)) <= sq / 8:
            dp += 1
    rng = K.Stream(seed)
    scalars, jumps = K.jump_table(rng, max(1.0, n * sq / 4))
    table = MultiTable(a, W, pubs)
    pre = {k for k in range(L) if Qs[k] is None}
    for k in pre:
        table.presolve(k, a)
    if len(pre) == L:
        return table.keys, 0, table
    asg = Assigner(L, pre, n - n // 2)
    states = [None] * n

    def solved_list():
        return [k is not None for k in table.keys]

    def on_found(k):
        """a key is solved: its kangaroos start afresh on other keys"""
        for w, kk in enumerate(asg.key):
            if kk == k:
                fresh(n // 2 + w)

    def fresh(i):
        """a new start for kangaroo i (a wild start at infinity solves its key on the spot)"""
        while True:
            wild = i >= n // 2
            key = asg.reseed(i - n // 2, solved_list()) if wild else 0
            if wild and key is None:
                states[i] = (0, 0, 0, WILD | DEAD)
                return
            d = K.herd_offset(rng, W, wild)
            p = K.start(Qs[key], d, wild) if wild else K.start(None, d, False)
            if p is None:
                if wild:
                    ev = []
                    table._found(key, a - d, ev)
                    for e in ev:
                        on_found(e[1])
                continue
            states[i] = (p[0], p[1], d & M128, wild_flags(key) if wild else 0)
            return

    for i in range(n):
        fresh(i)
    max_steps = max_steps or int(40 * L * (2 * sq + n * (1 << dp)))
    done = 0
    while done < max_steps and table.solved() < L:
        states, recs = K.walk(states, jumps, scalars, 1, dp)
        done += n
        for x, d, kid, fl, _ in recs:
            for e in table.add(x, d, kid, fl):
                if e[0] == "reseed":
                    fresh(e[1])
                elif e[0] == "found":
                    on_found(e[1])
    return table.keys, done, table
