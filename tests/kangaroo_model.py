"""Pure-Python restatement of the kangaroo walk (include/bsgs_hip.h, "Kangaroo") on the integers of pybsgs/ecpy.py: the step with its equal-x cases, distinguished
point records, herd starts from a seed, the collision rule of the host's table and a tiny solver.  A test model: no product code runs here."""
from pybsgs.ecpy import N, add, mul, neg

NJ = 64
WILD, DEAD = 1, 0x80000000
M128 = (1 << 128) - 1


def splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return state, z ^ (z >> 31)


class Stream:
    """the seeded stream herds and jump tables are drawn from (host_kangaroo.h; the jump table: host_kangaroo_run.cpp)"""

    def __init__(self, seed):
        self.s = seed & 0xFFFFFFFFFFFFFFFF

    def u64(self):
        self.s, z = splitmix64(self.s)
        return z

    def u128(self):
        lo = self.u64()
        return (self.u64() << 64) | lo


def herd_offset(stream, W, wild):
    """tame: t uniform in [1, W); wild: u uniform in [-W/2, W/2)"""
    r = stream.u128()
    return (r % W) - W // 2 if wild else 1 + r % (W - 1)


def jump_table(stream, mean):
    """64 scalars uniform in [1, 2 mean) and their points"""
    span = max(1, int(2 * mean) - 1)
    s = [1 + stream.u64() % span for _ in range(NJ)]
    return s, [mul(v) for v in s]


def start(Q, d, wild):
    """a kangaroo at offset d: d*G (tame) or Q + d*G (wild); None = the point at infinity"""
    p = mul(d % N)
    return add(p, Q) if wild else p


def step(state, jumps, scalars):
    """one step of a kangaroo state (x, y, d, flags) -> (new state, kind): kind 'add', 'double', 'dies' (x + J = infinity: the state keeps its point and gets
    the dead flag) or 'dead' (already dead: unchanged)"""
    x, y, d, fl = state
    if fl & DEAD:
        return state, "dead"
    j = x & (NJ - 1)
    jx, jy = jumps[j]
    if x == jx:
        if y != jy:
            return (x, y, d, fl | DEAD), "dies"
        kind = "double"
    else:
        kind = "add"
    nx, ny = add((x, y), (jx, jy))
    return (nx, ny, (d + scalars[j]) & M128, fl), kind


def is_dp(x, dp):
    return dp == 0 or (x >> (256 - dp)) == 0


def walk(states, jumps, scalars, steps, dp, history=None):
    """`steps` steps of every kangaroo, as one launch: (final states, records).  A record is (x, d, kangaroo, flags, step): a DP after a step, or the point a
    kangaroo stood on when it died.  history (optional dict kangaroo -> list) receives the state after every step."""
    states = list(states)
    recs = []
    for s in range(steps):
        for i, st in enumerate(states):
            new, kind = step(st, jumps, scalars)
            states[i] = new
            if kind == "dies":
                recs.append((new[0], new[2], i, new[3], s))
            elif kind in ("add", "double") and is_dp(new[0], dp):
                recs.append((new[0], new[2], i, new[3], s))
            if history is not None and i in history:
                history[i].append(new)
    return states, recs


def signed128(v):
    v &= M128
    return v - (1 << 128) if v >> 127 else v


class DPTable:
    """the host's table of distinguished points (host_kangaroo.cpp KangarooTable), keyed on the low 64 bits of x; verdicts 'new', 'found', 'reseed',
    'false', 'repeat'"""

    def __init__(self, a, W, pub):
        self.a, self.W, self.pub = a, W, pub
        self.map = {}
        self.false_matches = self.reseeds = 0

    def add(self, x, d, kid, flags):
        """-> (verdict, key or None)"""
        if flags & DEAD:
            self.reseeds += 1
            return "reseed", None
        k64, wild = x & 0xFFFFFFFFFFFFFFFF, bool(flags & WILD)
        e = self.map.get(k64)
        if e is None:
            self.map[k64] = (d & M128, kid, wild)
            return "new", None
        ed, ekid, ewild = e
        if ewild == wild:
            if ekid == kid:
                return "repeat", None
            self.reseeds += 1
            return "reseed", None
        k = signed128((ed - d) if wild else (d - ed))
        if 0 <= k < self.W and mul(self.a + k) == self.pub:
            return "found", self.a + k
        self.false_matches += 1
        return "false", None


def solve(pub, a, b, seed=1, n=16, dp=None, max_steps=None):
    """tiny solver: n kangaroos (half tame, half wild) walked one step at a time; returns (key, steps) or (None, steps)"""
    W = b - a + 1
    Q = add(pub, neg(mul(a)))
    sq = W ** 0.5
    if dp is None:
        dp = 0
        while n * (1 << (dp + 1)) <= sq / 8:
            dp += 1
    rng = Stream(seed)
    scalars, jumps = jump_table(rng, max(1.0, n * sq / 4))
    table = DPTable(a, W, pub)

    def fresh(i):
        wild = i >= n // 2
        d = herd_offset(rng, W, wild)
        p = start(Q, d, wild)
        return p, d, wild

    states = []
    for i in range(n):
        p, d, wild = fresh(i)
        if p is None:
            return a - d, 0
        states.append((p[0], p[1], d & M128, WILD if wild else 0))
    max_steps = max_steps or int(40 * (2 * sq + n * (1 << dp)))
    done = 0
    while done < max_steps:
        states, recs = walk(states, jumps, scalars, 1, dp)
        done += n
        for x, d, kid, fl, _ in recs:
            v, key = table.add(x, d, kid, fl)
            if v == "found":
                return key, done
            if v == "reseed":
                p, d2, wild = fresh(kid)
                if p is None:
                    return a - d2, done
                states[kid] = (p[0], p[1], d2 & M128, WILD if wild else 0)
    return None, done
