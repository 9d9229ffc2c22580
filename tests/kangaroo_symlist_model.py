"""Pure-Python restatement of the symmetric walk for a key list (include/bsgs_hip.h, "Kangaroo, many keys, symmetric walk"), built on the symmetric walk of
tests/kangaroo_sym_model.py and the Assigner of tests/kangaroo_multi_model.py: states and records that carry a key, the table with its rule for collisions
across keys, and a tiny solver.  A test model: no product code runs here."""
import kangaroo_model as K
import kangaroo_sym_model as S
from kangaroo_multi_model import Assigner
from pybsgs.ecpy import N, add, mul, neg

WILD, DEAD, M128 = K.WILD, K.DEAD, K.M128
NEG, CYCLE = S.NEG, S.CYCLE


def walk(states, jumps, scalars, steps, dp):
    """one launch of the symmetric walk on states (x, y, d, flags, key): (final states, records (x, d, kangaroo, flags, step, key)).  The key takes no part in
    the step; a record names the key of its kangaroo."""
    keys = [s[4] for s in states]
    out, recs = S.walk([s[:4] for s in states], jumps, scalars, steps, dp)
    return [s + (k,) for s, k in zip(out, keys)], [r + (keys[r[2]],) for r in recs]


class SymListTable:
    """the table of the symmetric list search for P_0 .. P_{L-1} in [a, a + W).  An entry is (d signed, kangaroo, sigma, key).  add() returns the events of one
    record: ('new',), ('repeat',) -- always followed by a reseed --, ('reseed', kangaroo), ('false',), ('link', j, k), ('found', k, key)."""

    def __init__(self, a, W, pubs):
        self.a, self.W, self.pubs = a, W, list(pubs)
        self.mid = a + W // 2
        self.kpp = [None] * len(self.pubs)          # k''_k = key - (a + W // 2)
        self.map = {}
        self.links = []                             # (j, sigma1, d1, k, sigma2, d2)
        self.false_matches = self.reseeds = self.cycles = self.links_kept = self.links_resolved = 0

    @property
    def keys(self):
        return [None if v is None else self.mid + v for v in self.kpp]

    def solved(self):
        return sum(v is not None for v in self.kpp)

    def presolve(self, k, key):
        self.kpp[k] = key - self.mid

    def _verify(self, k, cand):
        return -(self.W // 2) <= cand < self.W - self.W // 2 and mul((self.mid + cand) % N) == self.pubs[k]

    def _as_tame(self, d, sg, k):
        if sg and self.kpp[k] is not None:
            return d + sg * self.kpp[k], 0
        return d, sg

    def _found(self, k, kpp, ev):
        self.kpp[k] = kpp
        ev.append(("found", k, self.mid + kpp))
        mine = [l for l in self.links if k in (l[0], l[3])]
        self.links = [l for l in self.links if k not in (l[0], l[3])]
        for j, s1, d1, kk, s2, d2 in mine:
            if j == k:
                other, cands = kk, [s2 * (eps * (s1 * kpp + d1) - d2) for eps in (1, -1)]
            else:
                other, cands = j, [s1 * (eps * (s2 * kpp + d2) - d1) for eps in (1, -1)]
            if self.kpp[other] is not None:
                continue                            # solved on another path meanwhile
            good = [c for c in cands if self._verify(other, c)]
            if good:
                self.links_resolved += 1
                self._found(other, good[0], ev)
            else:
                self.false_matches += 1

    def add(self, x, d, kid, flags, key):
        if flags & DEAD:
            self.reseeds += 1
            if flags & CYCLE:
                self.cycles += 1
            return [("reseed", kid)]
        k64 = x & 0xFFFFFFFFFFFFFFFF
        d, sg = K.signed128(d), S.sigma(flags)
        e = self.map.get(k64)
        if e is None:
            self.map[k64] = (d, kid, sg, key if sg else 0)
            return [("new",)]
        if e[1:] == (kid, sg, key if sg else 0) and e[0] == d:
            # its own point again with the offset and the owner it had: the walk is a function of x, so it runs a cycle longer than the window.  (A kangaroo's
            # number outlives a re-seed: on a point of its earlier life, with another offset, key or sign, it is taken as any other kangaroo below.)
            self.reseeds += 1
            self.cycles += 1
            return [("repeat",), ("reseed", kid)]
        k1, k2 = e[3], key
        d1, s1 = self._as_tame(e[0], e[2], k1)
        d2, s2 = self._as_tame(d, sg, k2)
        if not s1 and not s2:
            self.reseeds += 1
            return [("reseed", kid)]
        if not s1 or not s2:
            dt, dw, sw, k = (d1, d2, s2, k2) if not s1 else (d2, d1, s1, k1)
            for eps in (1, -1):
                cand = sw * (eps * dt - dw)
                if self._verify(k, cand):
                    ev = []
                    self._found(k, cand, ev)
                    return ev
            self.false_matches += 1
            self.reseeds += 1
            return [("false",), ("reseed", kid)]
        if k1 == k2:                                # the single-key symmetric rule: (s1 - eps s2) k'' = eps d2 - d1
            tried = False
            for eps in (1, -1):
                den = s1 - eps * s2
                if den == 0:
                    continue
                tried = True
                cand = (eps * d2 - d1) * pow(den, -1, N) % N
                if cand > N // 2:
                    cand -= N
                if self._verify(k1, cand):
                    ev = []
                    self._found(k1, cand, ev)
                    return ev
            ev = []
            if tried:
                self.false_matches += 1
                ev.append(("false",))
            self.reseeds += 1
            return ev + [("reseed", kid)]
        self.links.append((k1, s1, d1, k2, s2, d2))
        self.links_kept += 1
        self.reseeds += 1
        return [("link", k1, k2), ("reseed", kid)]


def solve_symlist(pubs, a, b, seed=1, n=16, dp=None, R=256, S_steps=32, scale=1.0, max_steps=None):
    """tiny solver for the keys `pubs` in [a, b]: n kangaroos (the first half tame, the second half wild and shared out by Assigner) walked in launches of
    S_steps steps, the records of a launch taken in step order.  -> (keys by list position, None where unsolved; steps; table)"""
    W = b - a + 1
    L = len(pubs)
    mid = a + W // 2
    nmid = neg(mul(mid))
    Qs = [add(p, nmid) for p in pubs]
    sq = W ** 0.5
    if dp is None:
        dp = 0
        while n * (1 << (dp + 1)) <= sq / 8:
            dp += 1
    rng = K.Stream(seed)
    scalars, jumps = S.jump_table(rng, max(1.0, scale * n * sq / 4), R)
    table = SymListTable(a, W, pubs)
    pre = {k for k in range(L) if Qs[k] is None}
    for k in pre:
        table.presolve(k, mid)
    if len(pre) == L:
        return table.keys, 0, table
    half = n // 2
    asg = Assigner(L, pre, n - half)
    states = [None] * n

    def solved_list():
        return [v is not None for v in table.kpp]

    def on_found(k):
        for w, kk in enumerate(asg.key):
            if kk == k:
                fresh(half + w)

    def fresh(i):
        while True:
            wild = i >= half
            key = asg.reseed(i - half, solved_list()) if wild else 0
            if wild and key is None:
                states[i] = (0, 0, 0, WILD | DEAD, 0)
                return
            d = S.herd_offset(rng, W, wild)
            p = K.start(Qs[key], d, True) if wild else K.start(None, d, False)
            if p is None:
                if wild:                            # Q_key + d G is infinity: k'' = -d
                    ev = []
                    table._found(key, -d, ev)
                    for e in ev:
                        on_found(e[1])
                continue
            states[i] = (p[0], p[1], d & M128, WILD if wild else 0, key)
            return

    for i in range(n):
        fresh(i)
    max_steps = max_steps or int(40 * L * (2 * sq + n * (1 << dp)))
    done = 0
    while done < max_steps and table.solved() < L:
        states, recs = walk(states, jumps, scalars, S_steps, dp)
        done += n * S_steps
        for x, d, kid, fl, _, key in sorted(recs, key=lambda r: r[4]):
            for e in table.add(x, d, kid, fl, key):
                if e[0] == "reseed":
                    fresh(e[1])
                elif e[0] == "found":
                    on_found(e[1])
    return table.keys, done, table
