"""Pure-Python restatement of the symmetric kangaroo walk (include/bsgs_hip.h, "Kangaroo, symmetric walk") on the integers of pybsgs/ecpy.py: the step on
the classes {P, -P} with its last-jump rule, the cycle check of a launch, records, herd starts, the collision rule of the host's table and a tiny solver.
A test model: no product code runs here."""
from kangaroo_model import DEAD, M128, WILD, Stream, is_dp, signed128, start
from pybsgs.ecpy import N, P, add, mul, neg

NEG, CYCLE = 2, 4
LAST_VALID, LAST_SHIFT, LAST_MASK = 0x100, 9, 0x1FFF << 8
WINDOW = 16
TYPE_BITS = WILD | NEG


def jump_table(stream, mean, R):
    """R scalars uniform in [1, 2 mean) and their points"""
    span = max(1, int(2 * mean) - 1)
    s = [1 + stream.u64() % span for _ in range(R)]
    return s, [mul(v) for v in s]


def herd_offset(stream, W, wild):
    """tame: uniform in [0, W/2); wild: uniform in [-W/4, W/4)"""
    r = stream.u128() % (W // 2)
    return r - W // 4 if wild else r


def jump_index(x, fl, R):
    j = x & (R - 1)
    if fl & LAST_VALID and (fl >> LAST_SHIFT) & 0xFFF == j:
        j = (j + 1) & (R - 1)
    return j


def step(state, jumps, scalars):
    """one step of (x, y, d, flags) -> (new state, kind); kinds as kangaroo_model.step.  The step works on the class representative: a state with odd y (only a
    start can be one) is taken as (x, p - y, -d, NEG toggled) first."""
    x, y, d, fl = state
    if fl & DEAD:
        return state, "dead"
    j = jump_index(x, fl, len(jumps))
    jx, jy = jumps[j]
    if y & 1:
        y, d = P - y, (-d) & M128
        if fl & WILD:
            fl ^= NEG
    if x == jx:
        if y != jy:
            return state[:3] + (state[3] | DEAD,), "dies"
        kind = "double"
    else:
        kind = "add"
    nx, ny = add((x, y), (jx, jy))
    d = (d + scalars[j]) & M128
    if ny & 1:
        ny, d = P - ny, (-d) & M128
        if fl & WILD:
            fl ^= NEG
    fl = (fl & ~LAST_MASK) | LAST_VALID | (j << LAST_SHIFT)
    return (nx, ny, d, fl), kind


def walk(states, jumps, scalars, steps, dp, history=None):
    """one launch of `steps` steps: (final states, records).  A record is (x, d, kangaroo, flags, step): a DP after a step, the point a kangaroo stood on when its
    sum was infinity, or the point on which the cycle check retired it (flags with DEAD | CYCLE)."""
    states = list(states)
    recs = []
    mark_step = steps - 1 - WINDOW if steps > WINDOW else None
    marks = {}
    for s in range(steps):
        for i, st in enumerate(states):
            new, kind = step(st, jumps, scalars)
            if kind in ("add", "double"):
                if s == mark_step:
                    marks[i] = new[0]
                elif mark_step is not None and s > mark_step and marks[i] == new[0]:
                    new = new[:3] + (new[3] | DEAD | CYCLE,)
                if new[3] & DEAD or is_dp(new[0], dp):
                    recs.append((new[0], new[2], i, new[3], s))
            elif kind == "dies":
                recs.append((new[0], new[2], i, new[3], s))
            states[i] = new
            if history is not None and i in history:
                history[i].append(new)
    return states, recs


def sigma(flags):
    return 0 if not flags & WILD else -1 if flags & NEG else 1


class SymTable:
    """the host's table in -ksym mode (host_kangaroo.cpp SymKangarooTable), keyed on the low 64 bits of x; verdicts 'new', 'found', 'reseed', 'repeat'.
    a, W, pub as given to the host; the walk's Q is pub - (a + W // 2) G."""

    def __init__(self, a, W, pub):
        self.a, self.W, self.pub = a, W, pub
        self.map = {}
        self.false_matches = self.reseeds = self.cycles = 0

    def add(self, x, d, kid, flags):
        if flags & DEAD:
            self.reseeds += 1
            if flags & CYCLE:
                self.cycles += 1
            return "reseed", None
        k64, s2, d2 = x & 0xFFFFFFFFFFFFFFFF, sigma(flags), signed128(d)
        e = self.map.get(k64)
        if e is None:
            self.map[k64] = (d & M128, kid, flags & TYPE_BITS)
            return "new", None
        ed, ekid, efl = e
        if ekid == kid:
            return "repeat", None
        s1, d1 = sigma(efl), signed128(ed)
        tried = False
        for sign in (1, -1):
            den = s1 - sign * s2
            if den == 0:
                continue
            tried = True
            k = (sign * d2 - d1) * pow(den, -1, N) % N
            cand = (self.a + self.W // 2 + k) % N
            if self.a <= cand < self.a + self.W and mul(cand) == self.pub:
                return "found", cand
        if tried:
            self.false_matches += 1
        self.reseeds += 1
        return "reseed", None


def solve(pub, a, b, seed=1, n=16, dp=None, R=256, S=32, scale=1.0, max_steps=None):
    """tiny solver: n kangaroos (half tame, half wild) walked in launches of S steps; returns (key, steps, ending, table) with ending 'tame-wild',
    'wild-wild' or 'start'; key None when the step limit was reached"""
    W = b - a + 1
    Q = add(pub, neg(mul(a + W // 2)))
    sq = W ** 0.5
    if dp is None:
        dp = 0
        while n * (1 << (dp + 1)) <= sq / 8:
            dp += 1
    rng = Stream(seed)
    scalars, jumps = jump_table(rng, max(1.0, scale * n * sq / 4), R)
    table = SymTable(a, W, pub)

    def fresh(i):
        wild = i >= n // 2
        d = herd_offset(rng, W, wild)
        return start(Q, d, wild), d, wild

    states = [None] * n
    for i in range(n):
        while states[i] is None:
            p, d, wild = fresh(i)
            if p is None and wild:
                return a + W // 2 - d, 0, "start", table
            if p is not None:
                states[i] = (p[0], p[1], d & M128, WILD if wild else 0)
    max_steps = max_steps or int(40 * (2 * sq + n * (1 << dp)))
    done = 0
    while done < max_steps:
        states, recs = walk(states, jumps, scalars, S, dp)
        done += n * S
        for x, d, kid, fl, _ in sorted(recs, key=lambda r: r[4]):
            prev = table.map.get(x & 0xFFFFFFFFFFFFFFFF)
            v, key = table.add(x, d, kid, fl)
            if v == "found":
                return key, done, "wild-wild" if prev[2] & WILD and fl & WILD else "tame-wild", table
            if v == "reseed":
                states[kid] = None
                while states[kid] is None:
                    p, d2, wild = fresh(kid)
                    if p is None and wild:
                        return a + W // 2 - d2, done, "start", table
                    if p is not None:
                        states[kid] = (p[0], p[1], d2 & M128, WILD if wild else 0)
    return None, done, None, table


def short_cycle_case(seed, R, tries=64):
    """a hand-built 2-cycle that the last-jump rule does not prevent: a table in which two DIFFERENT indices a != b hold the same jump J*, and a start P with
    index a whose successor -(P + J*) has index b: P -> -(P + J*) -> P -> ...  -> (scalars, jumps, state, a, b), state = (x, y, d, 0): a tame kangaroo, y even"""
    scalars, jumps = jump_table(Stream(seed), 1 << 40, R)
    for t in range(tries):
        d = 1000003 + 7919 * t
        p = mul(d)
        if p[1] & 1:
            p, d = neg(p), -d
        st = (p[0], p[1], d & M128, 0)
        a = jump_index(st[0], 0, R)
        s1, _ = step(st, jumps, scalars)
        b = jump_index(s1[0], 0, R)
        if b == a or s1[1] != P - add(p, jumps[a])[1]:              # the successor must be the NEGATED sum, on another index
            continue
        sc, ju = list(scalars), list(jumps)
        sc[b], ju[b] = sc[a], ju[a]
        s2, _ = step(s1, ju, sc)
        assert s2[:3] == st[:3] and jump_index(s2[0], s2[3], R) == a
        return sc, ju, st, a, b
    raise AssertionError("no short cycle among %d starts" % tries)
