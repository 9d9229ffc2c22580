"""Equal-x giants at every batch position of the tile kernels -- the CASES, their tables and their expected hit lists.  TEST INFRASTRUCTURE, no GPU.

A centre P with P.x == G2[i].x (P = +-G2[i]) makes the batch element Px - Gx zero, so every tile kernel (csrc/giant_kernel.hip.h) puts 2 Py into the Montgomery
batch in its place and probes x(2P), code 4.  The substitution is made separately at every unrolled position of a chain, and most positions re-derive their
neighbours' d and must substitute there as well.  This module enumerates those positions per kernel (`positions`), lists the cases that put an equal-x giant on
each of them (`single_cases`, `walk_cases`, `clamped_cases`, `narrow_cases`), and builds for a case (`build`)
  * a table of EVERY 64-bit key that every thread of each 256-thread block holding an equal-x giant probes (o_tile_ref_slice_keys), for every tile of the case,
    plus x(P) of one centre (code 5): a wrong inverse anywhere in such a block -- the equal-x thread's other giants, the lanes that share its block inversion
    (fe_inv_block: lane l of each of the four waves) -- is a missing record;
  * the expected hit list (o_tile_ref / o_tile_ref_ext over that table, per tile);
  * the completeness set that follows from the geometry alone: (tile, 2, i) for every giant i of those blocks, (tile, 1, i) for the ordinary ones and
    (tile, 4, i) for the equal-x one.
tests/test_equal_x_cases.py checks the lists against the kernels' position classes and the keys against Python integers; tests/test_gpu_equal_x_positions.py
runs them on the GPU."""
import functools
from dataclasses import dataclass

import numpy as np

import oracle_lib as O

BLOCK = 256                    # threads per block of the tile kernels (four waves: one fe_inv_block)
HIT_BUFFER = 1 << 16           # records the device hit buffer holds (csrc/bsgs_internal.h max_hits)
W = 1 << 16                    # the giants are G2[i] = (i + 1) * ADDPUBG, ADDPUBG = -(2 W) G
HTSZ = 14                      # buckets of the reference-format tables: load <= 3 with the 49 152 keys of the largest case
MASK64 = (1 << 64) - 1
BASE = (64, 8, 12)             # T = 512: two blocks; three quads of the quad chain, six pairs of the pair chain, six quads of the pair walk


def _phase(g, n):
    return "first" if g == 0 else ("last" if g == n - 1 else "middle")


def positions(kernel, p):
    """the class of each chain slot j in 0 .. p-1, as the kernel's source distinguishes them:
    giant  giant_tile_kernel: (first | middle | last,) -- j == 0 takes s = inv, the others read the chain
    pair   giant_pair2_kernel<.., false>: (a | b, first | middle | last) over m = j >> 1 -- m == 0 has no stash S
    quad   giant_pair2_kernel<.., true>: (a | b | c | d, ..) over Q = j >> 2
    walk   tile_pair_walk: (jl | jh, ..) over Q = j >> 1; the full class of an element is (A | B,) + this (see `classes`)"""
    if kernel == "giant":
        return [(_phase(j, p),) for j in range(p)]
    if kernel == "pair":
        assert p % 2 == 0
        return [("ab"[j & 1], _phase(j >> 1, p >> 1)) for j in range(p)]
    if kernel == "quad":
        assert p % 4 == 0
        return [("abcd"[j & 3], _phase(j >> 2, p >> 2)) for j in range(p)]
    if kernel == "walk":
        assert p % 2 == 0
        return [(("jl", "jh")[j & 1], _phase(j >> 1, p >> 1)) for j in range(p)]
    raise ValueError(kernel)


def classes(kernel, p):
    """every position class of a kernel at batch length p"""
    s = set(positions(kernel, p))
    return {(tl,) + c for tl in "AB" for c in s} if kernel == "walk" else s


@dataclass
class Case:
    name: str
    geom: tuple                                   # (t, b, p) of the giants
    centres: list                                 # one (x, y) per tile
    eq: list                                      # [(tile, giant index, sign)]: centre of `tile` = sign * G2[index]
    engine: tuple = None                          # (threads, giants per thread) of the launch when it is not (t * b, p): the narrow batching
    waves: tuple = None                           # narrow batching: the waves of the affected block whose keys the table holds (None: the whole block)

    @property
    def batching(self):
        t, b, p = self.geom
        return self.engine or (t * b, p)

    def slot(self, i):
        return i % self.batching[1]

    def thread(self, i):
        return i // self.batching[1]


def case_classes(case, kernel):
    """{(position class, sign)} the case exercises in `kernel`; the pair walk takes tiles 2u, 2u + 1 as A, B"""
    pos = positions(kernel, case.batching[1])
    out = set()
    for tile, i, sign in case.eq:
        c = pos[case.slot(i)]
        out.add((("AB"[tile & 1],) + c if kernel == "walk" else c, sign))
    return out


@functools.lru_cache(maxsize=None)
def giants(geom):
    """(image bytes, the same as numpy uint8) of the giants of a geometry"""
    g2 = O.build_g2(geom[0], geom[1], geom[2], W)
    return g2, np.frombuffer(g2, dtype=np.uint8)


def eq_centre(geom, i, sign):
    gx, gy = O.g2_unpack(giants(geom)[0], geom[0], geom[1], geom[2], i)
    return (gx, gy) if sign > 0 else (gx, O.P_INT - gy)


def random_centre(tag):
    import random
    return O.pt_mul(random.Random("equal-x/%s" % (tag,)).randrange(1, 2**128))


def spread_threads(T):
    """lane 0, a wave edge, a block edge and the last thread"""
    return sorted({x for x in (0, 63, 64, 255, 256, T - 1) if x < T})


def _thread_for(T, j, sign, kind=0):
    th = spread_threads(T)
    return th[(j + (3 if sign < 0 else 0) + kind) % len(th)]


# ---- the case lists -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def single_cases(geom=BASE):
    """one tile, the equal-x giant at every slot j with both signs of the centre; the thread walks over spread_threads"""
    t, b, p = geom
    out = []
    for j in range(p):
        for sign in (1, -1):
            th = _thread_for(t * b, j, sign)
            i = th * p + j
            out.append(Case("j%d%st%d" % (j, "+" if sign > 0 else "-", th), geom, [eq_centre(geom, i, sign)], [(0, i, sign)]))
    return out


WALK_KINDS = ("eq_random", "random_eq", "same_twice", "plus_minus", "two_slots", "two_threads")


@functools.lru_cache(maxsize=None)
def walk_cases(kind, geom=BASE):
    """pairs of tiles for tile_pair_walk, the equal-x giant at every slot j:
    eq_random    (equal-x at j, random centre)                       both signs
    random_eq    (random, equal-x at j)                               both signs
    same_twice   the same equal-x centre in both tiles: a & b, or c & d, substitute together      both signs
    plus_minus   (G2[i], -G2[i]) and (-G2[i], G2[i])
    two_slots    A and B equal-x at different slots of ONE thread: the other slot of the same quad, and a slot of another quad     signs (+, -) and (-, +)
    two_threads  A and B equal-x in different threads of one block    signs (+, -) and (-, +)"""
    t, b, p = geom
    T = t * b
    kn = WALK_KINDS.index(kind)
    out = []
    for j in range(p):
        for sign in (1, -1):
            th = _thread_for(T, j, sign, kn)
            i = th * p + j
            E = eq_centre(geom, i, sign)
            tag = "%s-j%d%st%d" % (kind, j, "+" if sign > 0 else "-", th)
            if kind == "eq_random":
                out.append(Case(tag, geom, [E, random_centre(tag)], [(0, i, sign)]))
            elif kind == "random_eq":
                out.append(Case(tag, geom, [random_centre(tag), E], [(1, i, sign)]))
            elif kind == "same_twice":
                out.append(Case(tag, geom, [E, E], [(0, i, sign), (1, i, sign)]))
            elif kind == "plus_minus":
                out.append(Case(tag, geom, [E, eq_centre(geom, i, -sign)], [(0, i, sign), (1, i, -sign)]))
            elif kind == "two_slots":
                for j2 in (j ^ 1, (j + 2 + (j & 1)) % p):             # the partner in the quad (2Q, 2Q + 1); a slot of the next quad, of the other half
                    i2 = th * p + j2
                    out.append(Case("%s/%d" % (tag, j2), geom, [E, eq_centre(geom, i2, -sign)], [(0, i, sign), (1, i2, -sign)]))
            elif kind == "two_threads":
                blk = th // BLOCK
                th2 = blk * BLOCK + (th % BLOCK + 64 + 7) % min(BLOCK, T - blk * BLOCK)       # another wave and another lane of the same block
                i2 = th2 * p + (j + 5) % p
                out.append(Case("%s/t%d" % (tag, th2), geom, [E, eq_centre(geom, i2, -sign)], [(0, i, sign), (1, i2, -sign)]))
            else:
                raise ValueError(kind)
    return out


CLAMPED = (96, 3, 12)          # T = 288: the second block has 32 live threads and 224 lanes clamped to thread 287
WAVE32 = (32, 1, 12)           # T = 32: a single partial wave


@functools.lru_cache(maxsize=None)
def clamped_cases(pair):
    """the tail block's clamped lanes shadow thread T - 1: the equal-x giant in thread 287 at a first, a middle and a last slot, in thread 0, and in the last
    thread of a single partial wave.  pair: two tiles (equal-x, random) and (random, equal-x) for the pair walk; else one tile."""
    out = []
    for geom, th, j, sign in [(CLAMPED, 287, 0, 1), (CLAMPED, 287, 5, -1), (CLAMPED, 287, 11, 1), (CLAMPED, 287, 6, -1), (CLAMPED, 0, 10, -1), (WAVE32, 31, 7, 1), (WAVE32, 31, 0, -1)]:
        i = th * geom[2] + j
        E = eq_centre(geom, i, sign)
        tag = "T%d-t%d-j%d%s" % (geom[0] * geom[1], th, j, "+" if sign > 0 else "-")
        if not pair:
            out.append(Case(tag, geom, [E], [(0, i, sign)]))
        else:
            out.append(Case(tag + "-A", geom, [E, random_centre(tag)], [(0, i, sign)]))
            out.append(Case(tag + "-B", geom, [random_centre(tag), E], [(1, i, sign)]))
    return out


NARROW = (128, 2, 256)         # a one-tile launch of this geometry takes the narrow copy of the giants: 512 threads x 128 giants (bsgs_hip.hip pick_batching)
NARROW_ENGINE = (512, 128)
NARROW_THREAD = 5              # wave 0, lane 5 of block 0


@functools.lru_cache(maxsize=None)
def narrow_cases():
    """slots 0 .. 3 and 124 .. 127 of narrow thread 5.  A whole block would be 65 536 records, the hit buffer's size, so the table holds three of the block's
    four waves (49 152 keys): always wave 0, the equal-x thread's, and the case number decides which of waves 1, 2, 3 is left out -- over the list, lane 5 of
    every wave (threads 5, 69, 133, 197: the four that share one inversion in fe_inv_block) is covered.
    The thread must be a low one.  With P = +-G2[i] every key is x(m * ADDPUBG) for a small m (|i - k| or i + k + 2 for giant k), so giants OUTSIDE the table's
    waves hit as well wherever their m is some covered giant's (the oracle lists them: they are expected records), and those records plus the table's 49 152
    must stay at or below 65 536: with i in wave 0 they are 1 300 to 4 600.  So in the narrow batching only wave 0, lane 5 HOSTS the equal-x giant; the other
    three threads of the shared inversion are covered as its victims only."""
    out = []
    for n, j in enumerate((0, 1, 2, 3, 124, 125, 126, 127)):
        sign = 1 if n % 2 == 0 else -1
        i = NARROW_THREAD * NARROW_ENGINE[1] + j
        waves = tuple(w for w in range(4) if w != (1, 2, 3)[n % 3])
        out.append(Case("narrow-j%d%s" % (j, "+" if sign > 0 else "-"), NARROW, [eq_centre(NARROW, i, sign)], [(0, i, sign)], engine=NARROW_ENGINE, waves=waves))
    return out


# ---- table, expected hits, completeness -----------------------------------------------------------------------------------------------------------------
def thread_ranges(case):
    """engine-thread ranges [lo, hi) whose keys the table holds: every block with an equal-x giant (any tile of the case), clipped to the live threads; or the
    chosen waves of it"""
    T = case.batching[0]
    out = []
    for blk in sorted({case.thread(i) // BLOCK for _, i, _ in case.eq}):
        if case.waves is None:
            out.append((blk * BLOCK, min((blk + 1) * BLOCK, T)))
        else:
            assert any(case.thread(i) % BLOCK // 64 in case.waves for _, i, _ in case.eq), "the equal-x thread's wave must be in the table"
            out += [(blk * BLOCK + 64 * w, blk * BLOCK + 64 * w + 64) for w in case.waves]
    return out


def slice_keys(case, tile, lo, hi):
    """(first giant, uint64[giants, 2]) of engine threads [lo, hi) of a tile, from the oracle's per-key listing"""
    t, b, p = case.geom
    pe = case.batching[1]
    g0, g1 = lo * pe, hi * pe
    assert g0 % p == 0 and g1 % p == 0
    return g0, O.tile_slice_keys(case.centres[tile], giants(case.geom)[1], t, b, p, g0 // p, g1 // p).reshape(-1, 2)


@dataclass
class Built:
    case: Case
    keys: np.ndarray              # the table: ascending distinct 64-bit keys
    slices: dict                  # (tile, first giant) -> uint64[giants, 2]
    complete: set                 # {(tile, code, idx)} that the geometry alone demands
    code5: int                    # the tile whose x(P) is in the table


@functools.lru_cache(maxsize=None)
def _build(list_name, args, n):
    case = CASE_LISTS[list_name](*args)[n]
    eqs = {(tile, i) for tile, i, _ in case.eq}
    slices, complete, allk = {}, set(), []
    for tile in range(len(case.centres)):
        for lo, hi in thread_ranges(case):
            g0, k = slice_keys(case, tile, lo, hi)
            slices[(tile, g0)] = k
            allk.append(k.reshape(-1))
            for i in range(g0, g0 + len(k)):
                complete.add((tile, 2, i))
                complete.add((tile, 4 if (tile, i) in eqs else 1, i))
    code5 = case.eq[0][0]
    allk.append(np.array([case.centres[code5][0] & MASK64], dtype=np.uint64))
    complete.add((code5, 5, 0xFFFFFFFF))
    return Built(case, np.unique(np.concatenate(allk)), slices, complete, code5)


CASE_LISTS = {"single": single_cases, "walk": walk_cases, "clamped": clamped_cases, "narrow": narrow_cases}


def build(list_name, args, n):
    """the n-th case of CASE_LISTS[list_name](*args), built once per process"""
    return _build(list_name, tuple(args), n)


def built_list(list_name, *args):
    return [build(list_name, args, n) for n in range(len(CASE_LISTS[list_name](*args)))]


@functools.lru_cache(maxsize=None)
def _expected_ref(list_name, args, n):
    bt = _build(list_name, args, n)
    t, b, p = bt.case.geom
    gpu, _ = O.pack_tables_from_keys(bt.keys, HTSZ)
    want = []
    for tile, P in enumerate(bt.case.centres):
        ref, nref = O.tile_ref(P, giants(bt.case.geom)[0], t, b, p, gpu, HTSZ, 0, HIT_BUFFER)
        assert nref == len(ref)
        want += [(tile, c, i) for c, i in ref]
    return gpu, want


def expected(list_name, args, n):
    """(htGPU image of the case's table with 2^HTSZ buckets, the oracle's hit list [(tile, code, idx)] in the library's order)"""
    return _expected_ref(list_name, tuple(args), n)


def expected_ext(bt, ck, M):
    """the oracle's hit list over an any-bucket table given as its composite keys (tests/ext_table_model.py)"""
    t, b, p = bt.case.geom
    want = []
    for tile, P in enumerate(bt.case.centres):
        ref, nref = O.tile_ref_ext(P, giants(bt.case.geom)[0], t, b, p, ck, M, 0, 0, t * b, True, HIT_BUFFER)
        assert nref == len(ref)
        want += [(tile, c, i) for c, i in ref]
    return want


def thread_digests(bt):
    """{(tile, engine thread): (xor, wrapping sum)} of the keys of every thread the table covers: what debug_flags & 8 must report for it"""
    pe = bt.case.batching[1]
    out = {}
    for (tile, g0), k in bt.slices.items():
        per = k.reshape(-1, pe * 2)
        x = np.bitwise_xor.reduce(per, axis=1)
        with np.errstate(over="ignore"):
            s = per.sum(axis=1, dtype=np.uint64)
        for r in range(len(per)):
            out[(tile, g0 // pe + r)] = (int(x[r]), int(s[r]))
    return out


# ---- what a slipped substitution would do: tile_pair_walk's chain on Python integers ---------------------------------------------------------------------
WALK_SITES = ("p1A", "p1B", "d.dd", "d.da", "d.db", "d.dc", "c.dc", "b.db", "a.da")     # phase 1 (both tiles); element d: its own dd and da, db, dc re-derived; c, b, a: their own
WALK_SLIPS = ("forget", "other")                                                        # the substitution is not made | it takes the other tile's Py


def walk_chain_wrong(case, thread, slip=None):
    """The s-chain of tile_pair_walk (csrc/giant_kernel.hip.h: phase 1, the inversion, the walk d, c, b, a of every quad with its recurrences q1, q2, q3, u and
    the stash S) restated for ONE thread of a two-tile case, with the equal-x substitution of one site slipped: slip = (site, "forget" | "other").
    -> the elements (tile, slot) whose s is not 1 / d: their keys are wrong, their records missing.  An analysis tool for the case matrix
    (tests/test_equal_x_cases.py: every site, slipped either way, must fail cases); no kernel is compared with it."""
    t, b, p = case.geom
    P = O.P_INT
    g2 = giants(case.geom)[0]
    gx = [O.g2_unpack(g2, t, b, p, thread * p + j)[0] for j in range(p)]
    two = [2 * case.centres[k][1] % P for k in (0, 1)]
    raw = [[(case.centres[k][0] - gx[j]) % P for j in range(p)] for k in (0, 1)]
    true = [[raw[k][j] or two[k] for j in range(p)] for k in (0, 1)]

    def d_at(site, k, j):
        if raw[k][j]:
            return raw[k][j]
        if slip == (site, "forget"):
            return 0
        return two[1 - k] if slip == (site, "other") else two[k]

    acc, S = 1, {}
    for j in range(p):
        acc = acc * d_at("p1A", 0, j) * d_at("p1B", 1, j) % P
        if (j & 1) and j + 1 < p:
            S[(j + 1) >> 1] = acc
    inv = pow(acc, P - 2, P)                                     # Fermat, as fe_inv: 0 for 0
    s = {}
    for Q in range(p // 2 - 1, -1, -1):
        jl, jh = 2 * Q, 2 * Q + 1
        dd, da = d_at("d.dd", 1, jh), d_at("d.da", 0, jl)
        q1 = S[Q] * da % P if Q > 0 else da
        q2 = q1 * d_at("d.db", 1, jl) % P
        q3 = q2 * d_at("d.dc", 0, jh) % P
        s[(1, jh)], u = inv * q3 % P, inv * dd % P
        s[(0, jh)], u = u * q2 % P, u * d_at("c.dc", 0, jh) % P
        s[(1, jl)], u = u * q1 % P, u * d_at("b.db", 1, jl) % P
        s[(0, jl)] = u * S[Q] % P if Q > 0 else u
        inv = u * d_at("a.da", 0, jl) % P
    return sorted(e for e in s if s[e] * true[e[0]][e[1]] % P != 1)


def walk_slip_caught(case, slip):
    """would the case fail with that slip: some element of a thread that holds an equal-x giant gets a wrong s (its two records are in the completeness set)"""
    return any(walk_chain_wrong(case, th, slip) for th in sorted({case.thread(i) for _, i, _ in case.eq}))
