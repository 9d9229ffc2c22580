"""Degenerate kangaroo steps at every slot, wave and block of the walks (csrc/kangaroo.hip) -- the CASES, their jump tables and their expected states and
records.  TEST INFRASTRUCTURE, no GPU: pure Python on pybsgs/ecpy.py and the models tests/kangaroo_model.py, kangaroo_sym_model.py, kangaroo_symlist_model.py.

A kangaroo whose batch element J.x - x is zero (it doubles, or its sum is infinity), a dead one and one that was never uploaded get a substitute (2y or 1) in
the Montgomery batch of their thread.  A site that substitutes wrongly zeroes the product of the thread and, in blocks of four waves (fe_inv_block), of lane l
of all four waves: the damage lands on OTHER kangaroos.  So a herd here is PACKED: every kind of degenerate kangaroo at every slot of every block, each with
ordinary kangaroos around it, everything compared with the model bit for bit.

Jump tables.  A kangaroo can stand on its own jump only where x(J_j) & mask == j, so the tables are SELF-INDEXED:
  plain_table()    64 scalars s_j with x(s_j G) & 63 == j for every j;
  sym_base(64)     the same for the symmetric walk (y of both parities: an even J.y doubles, an odd one dies);
  sym_base(1024)   S.jump_table with at least six even-y and six odd-y entries replaced by self-indexed ones.
The symmetric herds walk sym_table(R): the base with TWO entries replaced, named in its `bump` -- the `bumped` kinds need a kangaroo with x & mask == m and last
index m (the walk takes m + 1) standing on the class of J_{m+1}, and x(J_{m+1}) & mask == m is what a self-indexed entry m + 1 can not give.  The cycle herd
walks cycle_table(): sym_table(64) with one more entry replaced, as S.short_cycle_case builds its 2-cycle (two indices hold one jump).

Kinds (KINDS): double@0, dies@0 (standing on J_j / -J_j), double@1, dies@1 (J_j - J_k / -J_j - J_k with index k: an ordinary step, then the degenerate one
inside the same launch), dead (DEAD set, standing on a jump point), never (never uploaded: flags 0xFFFFFFFF, state zero); symmetric only: bumped-double,
bumped-dies, odd-double, odd-dies (a start of odd y: normalised, then degenerate), and in the cycle herd `cycle`.

Geometry.  T = 1280 threads: five blocks of four waves, the leaders blockIdx & 3 = 0, 1, 2, 3, 0, and a chain scratch [g][2][T] with T > 256.  T = 320: five
one-wave blocks (the BLOCK_INV = false instantiations).  G = 1, 2, 3 kangaroos per thread: the only slot; first and last; first, middle and last.

Layout of a packed herd (layout()), the conditions tests/test_kangaroo_edge_cases.py asserts:
  * every kind at every slot of every block; every kind in every wave 0 .. 3 somewhere in the herd;
  * lanes: a block has 64 coupled sets (below) and 4 of them are the lanes 0, 31, 32, 63: five blocks give 20 such places, fewer than kinds x 4 lanes (24 plain,
    40 symmetric) -- with isolated placements every kind can NOT meet every one of the four lanes in one herd.  What holds and is asserted: every kind sits on a
    wave-edge lane (0 or 63) and on a lane at the halves' border (31 or 32) somewhere in the herd, and each of the four lanes holds a doubling and a dying kind;
  * ISOLATION.  The coupled set of kangaroo i is what shares an inversion with it: in the four-wave kernels lane l of the four waves of its block, all slots;
    in the one-wave kernels its thread, all slots.  No two placements share a coupled set; the coupled set of a placement holds at least three ordinary kangaroos
    in other threads (four-wave kernels) and at least one in its own thread when G > 1.  Ordinary = seeded, and 'add' at every step under the model;
  * three placements CROWD on purpose, in every block: (i) G > 1: a doubling at slot 0 and a death at slot G - 1 of one thread; (ii) G > 1: a thread whose G
    kangaroos are all degenerate or dead, a doubling at the LAST slot (its inverse is inv * chain[G - 2], a product of substitutes only); (iii) four-wave
    kernels: the same lane degenerate in two waves of a block.  The members of a crowd share one coupled set with nothing else degenerate in it; (i) and (ii)
    keep three ordinary threads in theirs, (iii) two.
These conditions cap what a test could hide: a wrong substitute anywhere corrupts ordinary kangaroos that the comparison covers."""
import functools
from dataclasses import dataclass

import kangaroo_model as K
import kangaroo_sym_model as S
import kangaroo_symlist_model as SL
from pybsgs.ecpy import P, add, mul, neg

M128, WILD, DEAD = K.M128, K.WILD, K.DEAD
NEVER = (0, 0, 0, 0xFFFFFFFF)          # a kangaroo kangaroo_alloc made and nobody uploaded
BLOCK_T, WAVE_T = 1280, 320            # five blocks of 256 threads / of 64
CYCLE_BLOCK_T, CYCLE_WAVE_T = 512, 128
STEPS = 3
DP = 0                                 # every step of every live kangaroo is a record: the launches are compared step by step
RECORD_CAP = 1 << 15                   # what tests/test_gpu_kangaroo_edge_positions.py gives kangaroo_setup*
EDGE_LANES, MID_LANES = (0, 63), (31, 32)

PLAIN_KINDS = ("double@0", "dies@0", "double@1", "dies@1", "dead", "never")
SYM_KINDS = PLAIN_KINDS + ("bumped-double", "bumped-dies", "odd-double", "odd-dies")
# kind -> (the step of the launch at which it is degenerate, what the model's step() says there)
INTENDED = {"double@0": (0, "double"), "dies@0": (0, "dies"), "double@1": (1, "double"), "dies@1": (1, "dies"), "dead": (0, "dead"), "never": (0, "dead"),
            "bumped-double": (0, "double"), "bumped-dies": (0, "dies"), "odd-double": (0, "double"), "odd-dies": (0, "dies")}
DOUBLING = ("double@0", "double@1", "bumped-double", "odd-double")
DYING = ("dies@0", "dies@1", "bumped-dies", "odd-dies")

FAMILIES = {"plain": (0, False), "sym64": (64, False), "sym1024": (1024, False), "keys64": (64, True)}      # -> (R, 0 = the plain walk; keyed)
PACKED = ([("plain", T, G) for T in (BLOCK_T, WAVE_T) for G in (1, 2, 3)] + [("sym64", T, G) for T in (BLOCK_T, WAVE_T) for G in (1, 2, 3)] +
          [("sym1024", T, 3) for T in (BLOCK_T, WAVE_T)] + [("keys64", T, 3) for T in (BLOCK_T, WAVE_T)])
CYCLE = [(f, T, 3) for f in ("sym64", "keys64") for T in (CYCLE_BLOCK_T, CYCLE_WAVE_T)]


def kinds_of(family):
    return PLAIN_KINDS if family == "plain" else SYM_KINDS


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Geometry:
    T: int
    G: int

    @property
    def block(self):
        return 256 if self.T % 256 == 0 else 64          # kangaroo_alloc's rule

    @property
    def N(self):
        return self.T * self.G

    @property
    def blocks(self):
        return self.T // self.block

    @property
    def waves(self):
        return self.block // 64

    def index(self, block, wave, lane, slot):
        return slot * self.T + block * self.block + wave * 64 + lane


def position(geom, i):
    """kangaroo index -> (block, wave, lane, slot): kangaroo i = slot * T + thread"""
    slot, t = divmod(i, geom.T)
    return (t // geom.block, t % geom.block // 64, t % 64, slot)


def coupled(geom, i):
    """the kangaroos that share an inversion with kangaroo i (itself included)"""
    b, w, l, _ = position(geom, i)
    waves = range(geom.waves)                             # one wave per block: the thread alone
    return sorted(geom.index(b, ww, l, g) for ww in (waves if geom.block == 256 else (w,)) for g in range(geom.G))


def where(geom, i):
    return "kangaroo %d (block %d, wave %d, lane %d, slot %d)" % ((i,) + position(geom, i))


# ---- jump tables -------------------------------------------------------------------------------------------------------------------------------------------
def _points(seed):
    """(k, k G) for k = base, base + stride, ...: one point addition each; every k is a 64-bit jump scalar"""
    rng = K.Stream(seed)
    base = 1 + rng.u64() % (1 << 61)
    stride = rng.u64() % (1 << 47) | (1 << 46) | 1
    sp, p, k = mul(stride), mul(base), base
    while True:
        yield k, p
        p, k = add(p, sp), k + stride


def _self_indexed_64(seed):
    scalars, jumps, left = [0] * 64, [None] * 64, 64
    src = _points(seed)
    while left:
        k, p = next(src)
        j = p[0] & 63
        if jumps[j] is None:
            scalars[j], jumps[j], left = k, p, left - 1
    return scalars, jumps, src


@functools.lru_cache(maxsize=None)
def plain_table():
    """(scalars, jumps): x(J_j) & 63 == j for every j"""
    scalars, jumps, _ = _self_indexed_64(0xED6E)
    return scalars, jumps


@dataclass
class SymTable:
    scalars: list
    jumps: list
    base: tuple            # (scalars, jumps) before the two bump entries went in
    even: list             # self-indexed entries with even y that the equal-x placements use
    odd: list
    bump: dict             # "even" | "odd" -> (m, m + 1): entry m + 1 holds a point with x & mask == m and that parity of y


SELF_PER_PARITY = {64: 12, 1024: 12}      # self-indexed entries per parity of y that the placements stand on


@functools.lru_cache(maxsize=None)
def sym_table(R):
    want = SELF_PER_PARITY[R]
    if R == 64:
        scalars, jumps, src = _self_indexed_64(0x5E1F)
        taken = set()
    else:
        scalars, jumps = S.jump_table(K.Stream(0x1024), 1 << 23, R)
        src = _points(0x5E1F + R)
        got = {0: [], 1: []}
        while min(len(got[0]), len(got[1])) < want:
            k, p = next(src)
            j, par = p[0] & (R - 1), p[1] & 1
            if len(got[par]) < want and j not in got[0] + got[1]:
                scalars[j], jumps[j] = k, p
                got[par].append(j)
        taken = set(got[0] + got[1])
    base = (list(scalars), list(jumps))
    bump = {}
    while len(bump) < 2:
        k, p = next(src)
        m, name = p[0] & (R - 1), ("even", "odd")[p[1] & 1]
        pair = {m, (m + 1) & (R - 1)}
        if name in bump or any(pair & set(v) for v in bump.values()) or (R > 64 and pair & taken):
            continue
        bump[name] = (m, (m + 1) & (R - 1))
        scalars[bump[name][1]], jumps[bump[name][1]] = k, p
    out = {m for v in bump.values() for m in v}
    idx = sorted(taken) if R > 64 else range(64)
    even = [j for j in idx if j not in out and jumps[j][1] & 1 == 0][:want]
    odd = [j for j in idx if j not in out and jumps[j][1] & 1][:want]
    return SymTable(scalars, jumps, base, even, odd, bump)


def sym_base(R):
    return sym_table(R).base


@functools.lru_cache(maxsize=None)
def cycle_table():
    """S.short_cycle_case's construction on sym_table(64): (scalars, jumps, state, a, b) with entry b a copy of entry a, a and b no index that an equal-x placement
    or a bump uses, and state -> -(state + J_a) -> state -> ... a tame kangaroo of even y"""
    tb = sym_table(64)
    used = set(tb.even) | set(tb.odd) | {m for v in tb.bump.values() for m in v}
    for t in range(4000):
        d = 1000003 + 7919 * t
        p = mul(d)
        if p[1] & 1:
            p, d = neg(p), -d
        st = (p[0], p[1], d & M128, 0)
        a = S.jump_index(st[0], 0, 64)
        s1, _ = S.step(st, tb.jumps, tb.scalars)
        b = S.jump_index(s1[0], 0, 64)
        if b == a or a in used or b in used or s1[1] != P - add(p, tb.jumps[a])[1]:
            continue
        sc, ju = list(tb.scalars), list(tb.jumps)
        sc[b], ju[b] = sc[a], ju[a]
        s2, _ = S.step(s1, ju, sc)
        assert s2[:3] == st[:3] and S.jump_index(s2[0], s2[3], 64) == a
        return sc, ju, st, a, b
    raise AssertionError("no short cycle")


def table_of(family):
    """(scalars, jumps) a packed herd of the family walks"""
    R = FAMILIES[family][0]
    if not R:
        return plain_table()
    tb = sym_table(R)
    return tb.scalars, tb.jumps


# ---- starts that are degenerate at step 1 ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def second_step_starts(R):
    """{"double@1": [...], "dies@1": [...]} of (x, y, j, k): a start with index k whose ordinary first step lands on the class of J_j.  Point additions only, a
    few hits per kind.  R = 0: the plain walk"""
    out = {"double@1": [], "dies@1": []}
    if not R:
        scalars, jumps = plain_table()
        js, mask = range(64), 63
    else:
        tb = sym_table(R)
        scalars, jumps, js, mask = tb.scalars, tb.jumps, tb.even + tb.odd, R - 1
    enough = 6
    for k in range(mask + 1):
        nk = neg(jumps[k])
        for j in js:
            if j == k:
                continue
            for sign in (1, -1):
                s0 = add(jumps[j] if sign > 0 else neg(jumps[j]), nk)
                if s0 is None or s0[0] & mask != k:
                    continue
                if not R:
                    kind = "double@1" if sign > 0 else "dies@1"
                elif s0[1] & 1:
                    continue                                  # (the walk would add J_k to the other point of the class)
                else:
                    kind = "double@1" if jumps[j][1] & 1 == 0 else "dies@1"
                if len(out[kind]) < enough:
                    out[kind].append((s0[0], s0[1], j, k))
        if all(len(v) >= enough for v in out.values()):
            break
    assert all(out.values()), "no start for %s" % [n for n, v in out.items() if not v]
    return out


# ---- ordinary kangaroos --------------------------------------------------------------------------------------------------------------------------------------
ORD_Q = 0xC0FFEE1234567
ORD_D0, ORD_STRIDE = (1 << 70) + 0x1D872B41, (1 << 44) + 0x6A09E667


@functools.lru_cache(maxsize=None)
def ordinary(n):
    """n seeded kangaroos by point additions: the even ones tame at d G, the odd ones wild at Q - d G with d kept as a negative 128-bit number"""
    Q, sp, cur = mul(ORD_Q), mul(ORD_STRIDE), mul(ORD_D0)
    out = []
    for i in range(n):
        d = ORD_D0 + i * ORD_STRIDE
        if i & 1:
            p = add(Q, neg(cur))
            out.append((p[0], p[1], (-d) & M128, WILD))
        else:
            out.append((cur[0], cur[1], d, 0))
        cur = add(cur, sp)
    return out


# ---- layout ----------------------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Placement:
    kind: str
    i: int                 # kangaroo
    crowd: str = None      # None: isolated; "i", "ii", "iii": a member of that crowded placement of its block


def _plain_lanes(b):
    pool = sorted((l for l in range(1, 63) if l not in MID_LANES), key=lambda l: (l * 29) % 64)
    return pool[7 * b:] + pool[:7 * b]


def layout(kinds, geom):
    """the placements of a packed herd (module docstring, "Layout")"""
    K_, G = len(kinds), geom.G
    out = []
    for b in range(geom.blocks):
        flip = b & 1
        special = {(2 * b) % K_: EDGE_LANES[flip], (2 * b + 1) % K_: EDGE_LANES[1 - flip],
                   (2 * b + K_ // 2) % K_: MID_LANES[flip], (2 * b + K_ // 2 + 1) % K_: MID_LANES[1 - flip]}
        assert len(special) == 4
        lanes = iter(_plain_lanes(b))
        for q, kind in enumerate(kinds):
            for g in range(G):
                lane = special[q] if q in special and g == b % G else next(lanes)
                wave = (q + g + b) % 4 if geom.block == 256 else 0
                out.append(Placement(kind, geom.index(b, wave, lane, g)))
        w = (lambda v: v % 4) if geom.block == 256 else (lambda v: 0)
        if G > 1:
            lane = next(lanes)
            out.append(Placement("double@0", geom.index(b, w(b + 1), lane, 0), "i"))
            out.append(Placement("dies@0", geom.index(b, w(b + 1), lane, G - 1), "i"))
            lane = next(lanes)
            for g, kind in enumerate((("dead", "double@0") if G == 2 else ("dies@0", "dead", "double@0"))):
                out.append(Placement(kind, geom.index(b, w(b + 2), lane, g), "ii"))
        if geom.block == 256:
            lane = next(lanes)
            out.append(Placement("double@0", geom.index(b, b % 4, lane, b % G), "iii"))
            out.append(Placement("dies@1", geom.index(b, (b + 2) % 4, lane, (b + 1) % G), "iii"))
    return out


def cycle_layout(geom):
    """the cycle kangaroo at each slot, in wave 0 and wave 3 (one-wave blocks: wave 0), in every block of the cycle herd: each in a coupled set of its own"""
    out = []
    for b in range(geom.blocks):
        lanes = iter(_plain_lanes(b))
        for g in range(geom.G):
            for wave in ((0, 3) if geom.block == 256 else (0,)):
                out.append(Placement("cycle", geom.index(b, wave, next(lanes), g)))
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    family: str
    geom: Geometry
    scalars: list
    jumps: list
    states: list           # [N] (x, y, d, flags) or, keyed, (x, y, d, flags, key); a `never` kangaroo: NEVER (keyed: key 0)
    placements: list
    steps: int

    @property
    def keyed(self):
        return FAMILIES[self.family][1]

    @property
    def R(self):
        return FAMILIES[self.family][0]

    @property
    def uploaded(self):
        never = {p.i for p in self.placements if p.kind == "never"}
        return [i for i in range(self.geom.N) if i not in never]

    @property
    def name(self):
        return "%s-T%d-G%d" % (self.family, self.geom.T, self.geom.G)


def _d_and_flags(n):
    """offsets that carry through all four words, of 64 and of 128 bits; tame and wild"""
    return (M128 - 5 - n, (n + 1) * 0x9E3779B97F4A7C15, ((n + 1) * 0x9E3779B97F4A7C15 << 50) & M128)[n % 3], (WILD if n & 1 else 0)


def _placed_state(R, kind, n):
    """the n-th state of a kind on the family's table"""
    d, fl = _d_and_flags(n)
    if kind == "never":
        return NEVER
    if kind in ("double@1", "dies@1"):
        hits = second_step_starts(R)[kind]
        x, y, _, _ = hits[n % len(hits)]
        return (x, y, d, fl)
    if not R:
        scalars, jumps = plain_table()
        jx, jy = jumps[(n * 11 + 5) % 64]
        minus = {"double@0": False, "dies@0": True, "dead": bool(n & 2)}[kind]
        return (jx, P - jy if minus else jy, d, fl | (DEAD if kind == "dead" else 0))
    tb = sym_table(R)
    if kind in ("bumped-double", "bumped-dies"):
        m, m1 = tb.bump["even" if kind == "bumped-double" else "odd"]
        jx, jy = tb.jumps[m1]
        assert jx & (R - 1) == m
        y = P - jy if (jy & 1) ^ (n & 1) else jy                  # starts of both parities
        return (jx, y, d, fl | S.LAST_VALID | m << S.LAST_SHIFT)
    even_j = kind in ("double@0", "odd-double") or (kind == "dead" and n & 2)
    pool = tb.even if even_j else tb.odd
    jx, jy = tb.jumps[pool[n % len(pool)]]
    odd_start = kind in ("odd-double", "odd-dies") or (kind == "dead" and n & 1)
    return (jx, jy if (jy & 1) == odd_start else P - jy, d, fl | (DEAD if kind == "dead" else 0))


def _key(i):
    return i + 1           # every kangaroo another key word: a record that names the wrong kangaroo's key shows


@functools.lru_cache(maxsize=None)
def packed_case(family, T, G):
    R, keyed = FAMILIES[family]
    if keyed:              # the keyed herd walks the states of the symmetric one, a key beside each: one model run serves both
        c = packed_case("sym64", T, G)
        states = [s + (0 if s == NEVER else _key(i),) for i, s in enumerate(c.states)]
        return Case(family, c.geom, c.scalars, c.jumps, states, c.placements, STEPS)
    geom = Geometry(T, G)
    scalars, jumps = table_of(family)
    states = list(ordinary(BLOCK_T * 3)[:geom.N])
    placements = layout(kinds_of(family), geom)
    count = {}
    for p in placements:
        n = count.get(p.kind, 0)
        count[p.kind] = n + 1
        states[p.i] = _placed_state(R, p.kind, n)
    return Case(family, geom, scalars, jumps, states, placements, STEPS)


@functools.lru_cache(maxsize=None)
def cycle_case(family, T, G):
    R, keyed = FAMILIES[family]
    assert R == 64
    geom = Geometry(T, G)
    sc, ju, st, _, _ = cycle_table()
    states = list(ordinary(BLOCK_T * 3)[:geom.N])
    placements = cycle_layout(geom)
    for p in placements:
        states[p.i] = st
    if keyed:
        states = [s + (_key(i),) for i, s in enumerate(states)]
    return Case(family, geom, sc, ju, states, placements, S.WINDOW + 1)


# ---- expected states and records, from the model ---------------------------------------------------------------------------------------------------------------
@dataclass
class Expected:
    after: list            # the herd after each launch of one step (packed) / after the launch (cycle)
    recs: list             # the records of each of those launches: (x, d, kangaroo, flags, step[, key])
    one_launch: list       # packed: the records of ONE launch of STEPS steps


def model_walk(case, states, steps):
    """one launch under the family's model: K.walk, S.walk or, with keys, SL.walk"""
    walk = SL.walk if states and len(states[0]) == 5 else S.walk if case.R else K.walk
    return walk(states, case.jumps, case.scalars, steps, DP)


@functools.lru_cache(maxsize=None)
def _expected_unkeyed(which, family, T, G):
    case = (packed_case if which == "packed" else cycle_case)(family, T, G)
    if which == "cycle":
        after, recs = model_walk(case, case.states, case.steps)
        return Expected([after], [recs], recs)
    # a launch of at most S.WINDOW steps has no cycle check: its steps are those of launches of one step (test_kangaroo_edge_cases.py runs the model both ways
    # on the small herds), and its records are theirs with the launch number as the step
    states, after, recs = case.states, [], []
    for _ in range(case.steps):
        states, r = model_walk(case, states, 1)
        after.append(states)
        recs.append(r)
    return Expected(after, recs, [r[:4] + (s,) for s, rs in enumerate(recs) for r in rs])


def expected(which, family, T, G):
    """Expected of packed_case / cycle_case (which = "packed" | "cycle"), computed once per process"""
    if not FAMILIES[family][1]:
        return _expected_unkeyed(which, family, T, G)
    return _expected_keyed(which, family, T, G)


@functools.lru_cache(maxsize=None)
def _expected_keyed(which, family, T, G):
    case = (packed_case if which == "packed" else cycle_case)(family, T, G)
    e = _expected_unkeyed(which, "sym64", T, G)
    keys = [s[4] for s in case.states]
    assert [s[:4] for s in case.states] == (packed_case if which == "packed" else cycle_case)("sym64", T, G).states
    # as SL.walk: the key takes no part in the step; a record names the key of its kangaroo (test_kangaroo_edge_cases.py runs SL.walk itself on the small herd)
    return Expected([[s + (k,) for s, k in zip(a, keys)] for a in e.after], [[r + (keys[r[2]],) for r in rs] for rs in e.recs],
                    [r + (keys[r[2]],) for r in e.one_launch])


def dead_records(case, exp):
    """the dead records the placements alone demand, as (launch of one step, record): a `dies` kind leaves exactly one, of the state it stood in, DEAD set"""
    out = []
    for p in case.placements:
        if p.kind in DYING:
            step = INTENDED[p.kind][0]
            st = case.states[p.i] if step == 0 else exp.after[step - 1][p.i]
            out.append((step, (st[0], st[2], p.i, st[3] | DEAD, 0) + tuple(st[4:])))
    return sorted(out)


# ---- helpers of the tests ----------------------------------------------------------------------------------------------------------------------------------------
def is_ordinary_step(case, state):
    """the next step of a live state is a plain addition: its x is not the x of the jump it takes (integers only, no curve arithmetic)"""
    x, fl = state[0], state[3]
    if fl & DEAD:
        return False
    j = S.jump_index(x, fl, case.R) if case.R else x & 63
    return case.jumps[j][0] != x


def mismatch(case, got, want, limit=6):
    """'' when the herds are equal; else the first differing kangaroos by position, each with the placements of its coupled set"""
    placed = {p.i: p for p in case.placements}
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    if not bad and len(got) == len(want):
        return ""
    lines = ["%s: %d of %d kangaroos differ (herd of %d downloaded)" % (case.name, len(bad), len(want), len(got))]
    for i in bad[:limit]:
        near = ["%s%s at %s" % (placed[c].kind, "/" + placed[c].crowd if placed[c].crowd else "", position(case.geom, c)) for c in coupled(case.geom, i) if c in placed]
        lines.append("  %s%s; degenerate in its coupled set: %s" % (where(case.geom, i), " [%s]" % placed[i].kind if i in placed else "", ", ".join(near) or "none"))
    return "\n".join(lines)
