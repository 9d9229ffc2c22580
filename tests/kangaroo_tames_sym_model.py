"""Pure-Python restatement of the tame table for the symmetric walk (include/bsgs_hip.h, "Kangaroo, tame table for the symmetric walk"), built on the symmetric
walk of tests/kangaroo_sym_model.py and the tame table of tests/kangaroo_tames_model.py: what the match hands back for a herd whose records carry a key, the
version-2 table file, the planning defaults, generation on the curve and the search rule.  A test model: no product code runs here."""
import math
import struct

import kangaroo_model as K
import kangaroo_sym_model as S
import kangaroo_tames_model as TM

M64 = TM.M64
MAGIC, VERSION, FIXED, ENTRY = TM.MAGIC, 2, 128, 24


def match(recs, tags):
    """what the match hands back of a launch's records (x, d, kangaroo, flags, step, key): those whose low 64 bits of x are a tag, and the DEAD ones, each as
    the walk wrote it, with the entry number or None beside it -> sorted list of (x, d, kangaroo, flags, step, key, entry)"""
    L = TM.build(tags)
    out = []
    for r in recs:
        e = TM.lookup(L, r[0] & M64)
        if e is not None or r[3] & K.DEAD:
            out.append(tuple(r) + (e,))
    return sorted(out, key=lambda r: r[:6])


# ---- the planning defaults ----------------------------------------------------------------------------------------------------------------------------
def plan(W, T, dp, kn):
    """-> (m, E, U, A): mean jump, how far past ceil(W/2) tame starts reach, wild starts are spread over [-U, U), the age limit in steps; kn = the kangaroos
    of the generating herd, all engines together.  The walk on classes diffuses: after n steps a kangaroo is about m sqrt(n) from its start and has n points
    within that distance, so it meets its own trail with probability about n^1.5 / m.  m is therefore the largest that keeps the herd inside the covered
    region, m sqrt(n) = E / 2 with n = K / kn the steps of a generating kangaroo, and never below the plain table's W / 2K."""
    Kp = T << dp
    m0 = max(2, min((1 << 62) - 1, W // (2 * Kp)))
    E = max(1, W // 16)
    n = max(1, Kp // kn)
    m = max(m0, min((1 << 62) - 1, E // (2 * math.isqrt(n))))
    return m, E, max(1, min(1 << 32, E // 4)), 8 * (W // Kp + (1 << dp))


# ---- the table file, version 2 ----------------------------------------------------------------------------------------------------------------------------
def header_bytes(R):
    return FIXED + 8 * R


def pack_file(dp, pk, pke, steps, seed, m, R, scale, scalars, entries, version=VERSION, magic=MAGIC):
    """entries = [(low 64 bits of x, d)], written in the order given (a valid file has them strictly ascending by x); len(scalars) words follow the fixed part,
    whatever R says"""
    out = magic + struct.pack("<II", version, dp) + pk.to_bytes(32, "little") + pke.to_bytes(32, "little") + struct.pack("<QQQQ", len(entries), steps, seed, m)
    out += struct.pack("<IId", R, 0, scale)
    assert len(out) == FIXED
    out += struct.pack("<%dQ" % len(scalars), *scalars)
    for x, d in entries:
        out += struct.pack("<Q", x) + (d & K.M128).to_bytes(16, "little")
    return out


def parse_file(b):
    """-> dict of the fields; ValueError names the first thing wrong, in the reader's order: magic, version, jumps (R), length, zero scalar, ordering"""
    if b[:8] != MAGIC:
        raise ValueError("magic")
    if len(b) < 12 or struct.unpack_from("<I", b, 8)[0] != VERSION:
        raise ValueError("version")
    if len(b) < FIXED:
        raise ValueError("length")
    R, _, scale = struct.unpack_from("<IId", b, 112)
    if R < 64 or R > 4096 or R & (R - 1):
        raise ValueError("jumps")
    T = struct.unpack_from("<Q", b, 80)[0]
    H = header_bytes(R)
    if not T or len(b) != H + ENTRY * T:
        raise ValueError("length")
    f = {"dp": struct.unpack_from("<I", b, 12)[0], "pk": int.from_bytes(b[16:48], "little"), "pke": int.from_bytes(b[48:80], "little"), "R": R, "scale": scale}
    f["steps"], f["seed"], f["m"] = struct.unpack_from("<QQQ", b, 88)
    f["scalars"] = list(struct.unpack_from("<%dQ" % R, b, FIXED))
    if 0 in f["scalars"]:
        raise ValueError("zero scalar")
    f["entries"] = [(struct.unpack_from("<Q", b, H + ENTRY * i)[0], K.signed128(int.from_bytes(b[H + ENTRY * i + 8:H + ENTRY * (i + 1)], "little"))) for i in range(T)]
    if any(f["entries"][i][0] <= f["entries"][i - 1][0] for i in range(1, T)):
        raise ValueError("ordering")
    return f


LAUNCH = 32                                                           # steps per launch of the model's generator: longer than the cycle window


def generate(a, W, T, dp, n, seed, R=64, scale=1.0):
    """an all-tame herd of n kangaroos of the symmetric walk, in launches of LAUNCH steps, until the map holds T distinguished points -> (the file's fields,
    steps, merges).  The stored d is the offset of the representative: signed."""
    m, E, _, _ = plan(W, T, dp, n)
    rng = K.Stream(seed)
    scalars, jumps = S.jump_table(rng, m * scale, R)
    span = (W + 1) // 2 + E - 1

    def fresh():
        t = 1 + rng.u128() % span
        p = K.start(None, t, False)
        return (p[0], p[1], t, 0)

    states = [fresh() for _ in range(n)]
    table, steps, merges = {}, 0, 0
    while len(table) < T:
        states, recs = S.walk(states, jumps, scalars, LAUNCH, dp)
        steps += n * LAUNCH
        for x, d, kid, fl, _ in sorted(recs, key=lambda r: r[4]):
            if len(table) >= T:
                break
            if fl & K.DEAD or (x & M64) in table:
                merges += 0 if fl & K.DEAD else 1
                states[kid] = fresh()
            else:
                table[x & M64] = K.signed128(d)
    f = {"dp": dp, "pk": a, "pke": a + W - 1, "steps": steps, "seed": seed, "m": max(1, int(m * scale)), "R": R, "scale": scale, "scalars": scalars, "entries": sorted(table.items())}
    return f, steps, merges


class SearchRule(TM.SearchRule):
    """what a record the device hands back means to the search with a table of the symmetric walk; every method returns the lines
    -selftest kangaroo-tames-search sym prints for the same item"""

    def __init__(self, f, pubs, n_wild, limit):
        import kangaroo_multi_model as M
        super().__init__(f, pubs, n_wild, limit)
        self.mid = self.a + self.W // 2
        mG = self.mul(self.mid)
        self.solved = [p == mG for p in pubs]
        self.key = [self.mid if s else None for s in self.solved]
        self.asg = M.Assigner(len(pubs), {k for k, s in enumerate(self.solved) if s}, n_wild)
        self.cycles = 0

    def cycle(self, w):
        self.cycles += 1
        return self.dead(w)

    def record(self, x, d, w, neg=False):
        e = self.index.get(x & M64)
        if e is None:
            return ["miss"]
        self.matches += 1
        k = self.asg.key[w]
        if self.solved[k]:
            return ["stale"]
        sg, dT, dW = -1 if neg else 1, self.f["entries"][e][1], K.signed128(d)
        for eps in (1, -1):
            kpp = sg * (eps * dT - dW)
            if -(self.W // 2) <= kpp < self.W - self.W // 2 and self.mul(self.mid + kpp) == self.pubs[k]:
                same = [o for o, p in enumerate(self.pubs) if p == self.pubs[k] and not self.solved[o]]      # equal points of the list are solved with it
                for o in same:
                    self.solved[o], self.key[o] = True, self.mid + kpp
                out = []
                for o in same:
                    out.append("found %d %064x" % (o, self.mid + kpp))
                    out += [self._afresh("reassign", v) for v, kv in enumerate(list(self.asg.key)) if kv == o]
                return out
        self.false += 1
        return ["false"]

    def summary(self):
        return "summary %d %d %d %d %d" % (self.matches, self.false, self.reseeds, sum(self.solved), self.cycles)
