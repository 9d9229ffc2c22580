"""Pure-Python restatement of the tame table (include/bsgs_hip.h, "Kangaroo, tame table"): the image in device memory, the lookup, what the match of a launch
hands back, and the table file.  A test model: no product code runs here."""
import struct

import kangaroo_model as K

SLOTS, MIN_LINES, LINE = 4, 64, 64
M64 = (1 << 64) - 1
MAGIC, VERSION, HEADER, ENTRY = b"KANGTAME", 1, 624, 24


def n_lines(n):
    """the power of two at or above n / 2, at least 64"""
    lines = MIN_LINES
    while lines * 2 < n:
        lines *= 2
    return lines


def home(tag, lines):
    return (tag >> 6) & (lines - 1)


def build(tags):
    """-> lines as lists [tags, entries, overflowed]; entries in the order given; ValueError for a tag that occurs twice"""
    lines = n_lines(len(tags))
    L = [[[], [], 0] for _ in range(lines)]
    for e, tag in enumerate(tags):
        assert 0 <= tag <= M64
        ln = home(tag, lines)
        while True:
            if tag in L[ln][0]:
                raise ValueError("tag %016x twice" % tag)
            if len(L[ln][0]) < SLOTS:
                L[ln][0].append(tag)
                L[ln][1].append(e)
                break
            L[ln][2] = 1
            ln = (ln + 1) & (lines - 1)
    return L


def image(tags):
    """the bytes of the image: per line four u64 tags, four u32 entry numbers, u32 count, u32 overflowed, 8 bytes of zero"""
    out = bytearray()
    for t, e, ovf in build(tags):
        out += struct.pack("<4Q4IIIQ", *(t + [0] * (SLOTS - len(t))), *(e + [0] * (SLOTS - len(e))), len(t), ovf, 0)
    return bytes(out)


def lookup(L, tag):
    """entry number or None; reads at most len(L) lines"""
    ln = home(tag, len(L))
    for _ in range(len(L)):
        t, e, ovf = L[ln]
        if tag in t:
            return e[t.index(tag)]
        if not ovf:
            return None
        ln = (ln + 1) & (len(L) - 1)
    return None


def match(recs, tags):
    """what the match hands back of a launch's records (x, d, kangaroo, flags, step): those whose low 64 bits of x are a tag, and the DEAD ones, each with the
    entry number or None -> sorted list of (x, d, kangaroo, flags, step, entry)"""
    L = build(tags)
    out = []
    for x, d, kid, fl, step in recs:
        e = lookup(L, x & M64)
        if e is not None or fl & K.DEAD:
            out.append((x, d, kid, fl, step, e))
    return sorted(out, key=lambda r: (r[0], r[1], r[2], r[3], r[4]))


def chain_tags(first_line, lines=64, n=64, salt=1):
    """n tags with the same home line `first_line` of an image of `lines` lines, their bits 0..5 running through 0..63 (so each can be planted as the x of one
    jump point, include/bsgs_hip.h "Kangaroo": j = x & 63) and pairwise different above the home bits"""
    bits = lines.bit_length() - 1
    return [(j & 63) | (first_line << 6) | (((salt * 0x9E3779B1 + j * 0x85EBCA6B) & ((1 << (58 - bits)) - 1)) << (6 + bits)) for j in range(n)]


# ---- the table file, the plan, generation and the search rule (host/host_kangaroo_tames.cpp) ------------------------------------------------------------
def plan(W, T, dp):
    """the planning defaults -> (m, E, U, A): mean jump, how far past the range tame starts reach, the spread of wild starts, the age limit in steps"""
    Kp = T << dp
    m = max(2, min((1 << 62) - 1, W // (2 * Kp)))
    E = max(1, 4 * m * W // Kp, W // 8)                                              # (at least W / 8: a share of the trails starts beyond the top of the range)
    return m, E, min(1 << 32, max(W // 4, 1), E), 8 * (W // Kp + (1 << dp))          # (U within E: a wild start beyond the tame starts meets no trail)


def pack_file(dp, pk, pke, steps, seed, m, scalars, entries, version=VERSION, magic=MAGIC):
    """entries = [(low 64 bits of x, d)], written in the order given (a valid file has them strictly ascending by x)"""
    out = magic + struct.pack("<II", version, dp) + pk.to_bytes(32, "little") + pke.to_bytes(32, "little") + struct.pack("<QQQQ", len(entries), steps, seed, m)
    out += struct.pack("<64Q", *scalars)
    assert len(out) == HEADER
    for x, d in entries:
        out += struct.pack("<Q", x) + (d & K.M128).to_bytes(16, "little")
    return out


def parse_file(b):
    """-> dict of the fields; ValueError names the first thing wrong, in the reader's order: magic, version, length, zero scalar, ordering"""
    if b[:8] != MAGIC:
        raise ValueError("magic")
    if len(b) < 12 or struct.unpack_from("<I", b, 8)[0] != VERSION:
        raise ValueError("version")
    T = struct.unpack_from("<Q", b, 80)[0] if len(b) >= HEADER else 0
    if not T or len(b) != HEADER + ENTRY * T:
        raise ValueError("length")
    f = {"dp": struct.unpack_from("<I", b, 12)[0], "pk": int.from_bytes(b[16:48], "little"), "pke": int.from_bytes(b[48:80], "little")}
    f["steps"], f["seed"], f["m"] = struct.unpack_from("<QQQ", b, 88)
    f["scalars"] = list(struct.unpack_from("<64Q", b, 112))
    if 0 in f["scalars"]:
        raise ValueError("zero scalar")
    f["entries"] = [(struct.unpack_from("<Q", b, HEADER + ENTRY * i)[0], K.signed128(int.from_bytes(b[HEADER + ENTRY * i + 8:HEADER + ENTRY * (i + 1)], "little"))) for i in range(T)]
    if any(f["entries"][i][0] <= f["entries"][i - 1][0] for i in range(1, T)):
        raise ValueError("ordering")
    return f


def generate(a, W, T, dp, n, seed):
    """an all-tame herd of n kangaroos walked one step at a time until the map holds T distinguished points -> (the file's fields, steps, merges)"""
    m, E, _, _ = plan(W, T, dp)
    rng = K.Stream(seed)
    scalars, jumps = K.jump_table(rng, m)

    def fresh():
        t = 1 + rng.u128() % (W + E - 1)
        p = K.start(None, t, False)
        return (p[0], p[1], t, 0)

    states = [fresh() for _ in range(n)]
    table, steps, merges = {}, 0, 0
    while len(table) < T:
        states, recs = K.walk(states, jumps, scalars, 1, dp)
        steps += n
        for x, d, kid, fl, _ in recs:
            if len(table) >= T:
                break
            if fl & K.DEAD or (x & M64) in table:
                merges += 0 if fl & K.DEAD else 1
                states[kid] = fresh()
            else:
                table[x & M64] = d
    f = {"dp": dp, "pk": a, "pke": a + W - 1, "steps": steps, "seed": seed, "m": m, "scalars": scalars, "entries": sorted(table.items())}
    return f, steps, merges


class SearchRule:
    """what a record the device hands back means to the search (all kangaroos wild, keys shared out by the list search's Assigner); every method returns the
    lines -selftest kangaroo-tames-search prints for the same item"""

    def __init__(self, f, pubs, n_wild, limit):
        import kangaroo_multi_model as M
        from pybsgs.ecpy import mul
        self.mul = mul
        self.f, self.pubs, self.a, self.W = f, pubs, f["pk"], f["pke"] - f["pk"] + 1
        self.index = {x: i for i, (x, _) in enumerate(f["entries"])}
        aG = mul(self.a)
        self.solved = [p == aG for p in pubs]
        self.key = [self.a if s else None for s in self.solved]
        self.asg = M.Assigner(len(pubs), {k for k, s in enumerate(self.solved) if s}, n_wild)
        self.age = [0] * n_wild
        self.limit = limit
        self.matches = self.false = self.reseeds = 0

    def presolved_lines(self):
        return ["presolved %d" % k for k, s in enumerate(self.solved) if s]

    def _afresh(self, word, w):
        self.age[w] = 0
        k = self.asg.reseed(w, self.solved)
        return "rest %d" % w if k is None else "%s %d %d" % (word, w, k)

    def dead(self, w):
        self.reseeds += 1
        return [self._afresh("reseed", w)]

    def record(self, x, d, w):
        e = self.index.get(x & M64)
        if e is None:
            return ["miss"]
        self.matches += 1
        k = self.asg.key[w]
        if self.solved[k]:
            return ["stale"]
        off = self.f["entries"][e][1] - K.signed128(d)
        if 0 <= off < self.W and self.mul(self.a + off) == self.pubs[k]:
            same = [o for o, p in enumerate(self.pubs) if p == self.pubs[k] and not self.solved[o]]      # equal points of the list are solved with it
            for o in same:
                self.solved[o], self.key[o] = True, self.a + off
            out = []
            for o in same:
                out.append("found %d %064x" % (o, self.a + off))
                out += [self._afresh("reassign", v) for v, kv in enumerate(list(self.asg.key)) if kv == o]
            return out
        self.false += 1
        return ["false"]

    def launch(self):
        out = []
        for w in range(len(self.age)):
            self.age[w] += 1
            if self.age[w] > self.limit:
                self.reseeds += 1
                out.append(self._afresh("aged", w))
        return out

    def summary(self):
        return "summary %d %d %d %d" % (self.matches, self.false, self.reseeds, sum(self.solved))
