"""CPU checks of tests/kangaroo_edge_cases.py, the inputs of tests/test_gpu_kangaroo_edge_positions.py:
  * the jump tables are self-indexed as the module says, and the herds' tables differ from them at the named entries only;
  * every placement has the kind and the step it claims under the model's step();
  * the coverage matrix, ENUMERATED HERE and not derived from the cases: kind x slot x block, kind x wave, kind x lane set, the three crowded placements, per
    herd and geometry; both block sizes, all four leaders, G = 1, 2, 3;
  * the isolation conditions: with a substitute missing (kang_element returning kind 0 on a zero element) the thread's product is zero, so every kangaroo of
    the coupled set gets a wrong inverse -- and every coupled set of a placement holds ordinary kangaroos, whose states and records the GPU test compares;
  * no expected record list exceeds the record capacity the GPU test sets."""
import pytest

import kangaroo_edge_cases as E
import kangaroo_model as K
import kangaroo_sym_model as S
from pybsgs.ecpy import mul

# the matrix, written out
HERDS = [("plain", 1280, 1), ("plain", 1280, 2), ("plain", 1280, 3), ("plain", 320, 1), ("plain", 320, 2), ("plain", 320, 3),
         ("sym64", 1280, 1), ("sym64", 1280, 2), ("sym64", 1280, 3), ("sym64", 320, 1), ("sym64", 320, 2), ("sym64", 320, 3),
         ("sym1024", 1280, 3), ("sym1024", 320, 3), ("keys64", 1280, 3), ("keys64", 320, 3)]
CYCLE_HERDS = [("sym64", 512, 3), ("sym64", 128, 3), ("keys64", 512, 3), ("keys64", 128, 3)]
KINDS = {"plain": ["double@0", "dies@0", "double@1", "dies@1", "dead", "never"],
         "sym": ["double@0", "dies@0", "double@1", "dies@1", "dead", "never", "bumped-double", "bumped-dies", "odd-double", "odd-dies"]}
BLOCKS = 5                                                       # T = 1280 = 5 x 256 (leaders 0, 1, 2, 3, 0) and T = 320 = 5 x 64
LANES = (0, 31, 32, 63)
IDS = ["%s-T%d-G%d" % h for h in HERDS]


def kinds(family):
    return KINDS["plain" if family == "plain" else "sym"]


def step_of(case):
    return S.step if case.R else K.step


def test_the_herd_lists_are_the_issue_s():
    assert E.PACKED == HERDS and E.CYCLE == CYCLE_HERDS
    assert max(T * G for _, T, G in HERDS) == 3840
    for family, T, G in HERDS:
        g = E.packed_case(family, T, G).geom
        assert (g.block, g.blocks) == ((256, 5) if T == 1280 else (64, 5))
        assert [b & 3 for b in range(g.blocks)] == [0, 1, 2, 3, 0]                 # fe_inv_block's leader, blockIdx & 3
    for fam in ("plain", "sym64"):
        assert {(T, G) for f, T, G in HERDS if f == fam} == {(T, G) for T in (1280, 320) for G in (1, 2, 3)}
    for fam in ("sym1024", "keys64"):
        assert {(T, G) for f, T, G in HERDS if f == fam} == {(1280, 3), (320, 3)}


def test_position_and_coupled():
    g = E.Geometry(1280, 3)
    assert E.position(g, 0) == (0, 0, 0, 0) and E.position(g, 1280 + 256 + 64 + 5) == (1, 1, 5, 1) and E.position(g, 3839) == (4, 3, 63, 2)
    assert all(g.index(*E.position(g, i)) == i for i in range(0, g.N, 37))
    assert E.coupled(g, 1280 + 256 + 64 + 5) == sorted(s * 1280 + 256 + w * 64 + 5 for s in range(3) for w in range(4))
    w = E.Geometry(320, 2)
    assert w.block == 64 and E.position(w, 320 + 64 * 4 + 63) == (4, 0, 63, 1)
    assert E.coupled(w, 70) == [70, 390]


def test_tables_are_self_indexed():
    scalars, jumps = E.plain_table()
    assert len(jumps) == 64 and all(p[0] & 63 == j for j, p in enumerate(jumps))
    assert all(0 < s < 1 << 64 and mul(s) == p for s, p in zip(scalars, jumps))
    for R in (64, 1024):
        tb = E.sym_table(R)
        bs, bj = E.sym_base(R)
        assert len(bj) == len(tb.jumps) == R and all(0 < s < 1 << 64 for s in tb.scalars)
        self_even = [j for j, p in enumerate(bj) if p[0] & (R - 1) == j and p[1] & 1 == 0]
        self_odd = [j for j, p in enumerate(bj) if p[0] & (R - 1) == j and p[1] & 1]
        if R == 64:
            assert len(self_even) + len(self_odd) == 64                              # every entry
            assert all(mul(s) == p for s, p in zip(bs, bj))
        else:
            rs, rj = S.jump_table(K.Stream(0x1024), 1 << 23, R)
            replaced = [j for j in range(R) if bj[j] != rj[j]]
            assert all(bs[j] == rs[j] for j in range(R) if j not in replaced) and set(replaced) <= set(self_even + self_odd)
            assert all(mul(bs[j]) == bj[j] for j in replaced)
        assert len(self_even) >= 6 and len(self_odd) >= 6
        assert len(tb.even) >= 6 and len(tb.odd) >= 6 and set(tb.even) <= set(self_even) and set(tb.odd) <= set(self_odd)
        # the herd's table: the base but for the two bump entries, which hold a point whose x names the index BEFORE theirs
        changed = [j for j in range(R) if (tb.scalars[j], tb.jumps[j]) != (bs[j], bj[j])]
        assert sorted(changed) == sorted(m1 for _, m1 in tb.bump.values()) and len(changed) == 2
        for name, (m, m1) in tb.bump.items():
            x, y = tb.jumps[m1]
            assert m1 == (m + 1) & (R - 1) and x & (R - 1) == m and y & 1 == (name == "odd") and mul(tb.scalars[m1]) == (x, y)
            assert not {m, m1} & set(tb.even + tb.odd)
    sc, ju, st, a, b = E.cycle_table()
    tb = E.sym_table(64)
    assert [j for j in range(64) if (sc[j], ju[j]) != (tb.scalars[j], tb.jumps[j])] == [b] and (sc[b], ju[b]) == (sc[a], ju[a]) and a != b
    assert not {a, b} & (set(tb.even + tb.odd) | {m for v in tb.bump.values() for m in v})      # two indices no equal-x placement uses


@pytest.mark.parametrize("herd", HERDS, ids=IDS)
def test_every_placement_has_its_kind_and_step(herd):
    case = E.packed_case(*herd)
    exp = E.expected("packed", *herd)
    step, mask = step_of(case), (case.R or 64) - 1
    assert set(E.INTENDED) == set(KINDS["sym"]) and {p.kind for p in case.placements} == set(kinds(herd[0]))
    for p in case.placements:
        st = case.states[p.i][:4]
        at, kind = E.INTENDED[p.kind]
        msg = (p, E.position(case.geom, p.i))
        if at == 1:
            st, first = step(st, case.jumps, case.scalars)
            assert first == "add", msg
            assert st == exp.after[0][p.i][:4], msg
        new, got = step(st, case.jumps, case.scalars)
        assert got == kind, msg
        if p.kind == "never":
            assert st == E.NEVER and p.i not in case.uploaded, msg
        else:
            assert p.i in case.uploaded, msg
            j = S.jump_index(st[0], st[3], case.R) if case.R else st[0] & 63
            assert case.jumps[j][0] == st[0], msg                                   # it stands on the x of the jump it takes
        if p.kind == "dead":
            assert st[3] & K.DEAD and st[3] != 0xFFFFFFFF, msg
        if p.kind.startswith("bumped"):
            assert st[3] & S.LAST_VALID and (st[3] >> S.LAST_SHIFT) & 0xFFF == st[0] & mask and j == (st[0] & mask) + 1, msg
        elif case.R and p.kind != "never":
            assert not st[3] & S.LAST_VALID or at == 1, msg
        if p.kind.startswith("odd"):
            assert st[1] & 1, msg
        if kind == "dies":                                                          # it keeps its state, rests inside the launch, and the model's dead record is the one demanded
            assert new == st[:3] + (st[3] | K.DEAD,), msg
            assert all(exp.after[s][p.i][:4] == new for s in range(at, E.STEPS)), msg
        if kind == "double":
            assert (new[0], new[1]) != (st[0], st[1]) and all(not exp.after[s][p.i][3] & K.DEAD for s in range(E.STEPS)), msg
        if kind == "dead":
            assert all(exp.after[s][p.i][:4] == st for s in range(E.STEPS)), msg
    # the dead records of the model are those the placements demand, each once, and nothing else of a placement's kangaroo comes after its death
    for launch in range(E.STEPS):
        model_dead = sorted(r for r in exp.recs[launch] if r[3] & K.DEAD)
        assert model_dead == [r for s, r in E.dead_records(case, exp) if s == launch]
    if case.R:                                                                      # both y parities among the bumped starts
        assert {case.states[p.i][1] & 1 for p in case.placements if p.kind == "bumped-double"} == {0, 1}
    if case.keyed:
        assert all(r[5] == r[2] + 1 for r in exp.one_launch) and len({s[4] for s in case.states}) == len(case.uploaded) + 1


@pytest.mark.parametrize("herd", HERDS, ids=IDS)
def test_coverage_matrix(herd):
    family, T, G = herd
    case = E.packed_case(*herd)
    geom = case.geom
    waves = (0, 1, 2, 3) if T == 1280 else (0,)
    pos = [(p, E.position(geom, p.i)) for p in case.placements]
    lone = [(p.kind, w) for p, w in pos if p.crowd is None]
    # kind x slot x block: the isolated placements, exactly once each
    assert sorted((k, s, b) for k, (b, _, _, s) in lone) == sorted((k, s, b) for k in kinds(family) for s in range(G) for b in range(BLOCKS))
    # kind x wave
    assert {(k, w) for k, (_, w, _, _) in lone} == {(k, w) for k in kinds(family) for w in waves}
    # kind x lane set: a wave-edge lane and a lane at the border of the halves, for every kind; every one of the four lanes under a doubling and a dying kind
    sets = {(k, "edge" if l in (0, 63) else "mid") for k, (_, _, l, _) in lone if l in LANES}
    assert sets == {(k, s) for k in kinds(family) for s in ("edge", "mid")}
    doubling, dying = [k for k in kinds(family) if "double" in k], [k for k in kinds(family) if "dies" in k]
    for lane in LANES:
        here = {k for k, (_, _, l, _) in lone if l == lane}
        assert here & set(doubling) and here & set(dying), (lane, here)
    # the crowded placements, in every block
    for b in range(BLOCKS):
        crowd = {c: sorted((p.kind, w, l, s) for p, (bb, w, l, s) in pos if p.crowd == c and bb == b) for c in ("i", "ii", "iii")}
        if G > 1:
            (k0, w0, l0, s0), (k1, w1, l1, s1) = sorted(crowd["i"], key=lambda v: v[3])
            assert (k0, s0, k1, s1) == ("double@0", 0, "dies@0", G - 1) and (w0, l0) == (w1, l1)
            two = sorted(crowd["ii"], key=lambda v: v[3])
            assert [v[3] for v in two] == list(range(G)) and len({v[1:3] for v in two}) == 1           # one thread, every slot
            assert two[-1][0] == "double@0" and {v[0] for v in two[:-1]} <= {"dies@0", "dead"}
        else:
            assert not crowd["i"] and not crowd["ii"]
        if T == 1280:
            (ka, wa, la, _), (kb, wb, lb, _) = crowd["iii"]
            assert la == lb and wa != wb and "double" in ka + kb and "dies" in ka + kb
        else:
            assert not crowd["iii"]


@pytest.mark.parametrize("herd", HERDS, ids=IDS)
def test_isolation(herd):
    family, T, G = herd
    case = E.packed_case(*herd)
    exp = E.expected("packed", *herd)
    geom = case.geom
    placed = {p.i: p for p in case.placements}
    assert len(placed) == len(case.placements)
    # ordinary: seeded, a plain addition at every step of the launch
    ordinary = [i for i in range(geom.N) if i not in placed]
    for i in ordinary:
        assert all(E.is_ordinary_step(case, s[i]) for s in [case.states] + exp.after[:-1]), E.where(geom, i)
    assert len(ordinary) > geom.N * 3 // 4
    assert sum(1 for i in ordinary if case.states[i][3] & K.WILD) > len(ordinary) // 3 and sum(1 for i in ordinary if not case.states[i][3] & K.WILD) > len(ordinary) // 3
    if case.R:
        assert sum(case.states[i][1] & 1 for i in ordinary) > len(ordinary) // 3 and sum(1 - (case.states[i][1] & 1) for i in ordinary) > len(ordinary) // 3
    sets_seen = {}
    for p in case.placements:
        cs = E.coupled(geom, p.i)
        assert p.i in cs and len(cs) == (4 * G if T == 1280 else G)
        inside = [placed[c] for c in cs if c in placed]
        _, w, l, _ = E.position(geom, p.i)
        other_threads = {E.position(geom, c)[1] for c in cs} - {E.position(geom, c)[1] for c in cs if c in placed}
        if p.crowd is None:
            assert inside == [p], (p, inside)                                          # nothing else degenerate shares its inversion
            if G > 1:
                assert sum(1 for c in cs if E.position(geom, c)[1:3] == (w, l) and c not in placed) >= 1
            if T == 1280:
                assert len(other_threads) == 3 and sum(1 for c in cs if E.position(geom, c)[1] != w and c not in placed) >= 3
        else:
            assert {q.crowd for q in inside} == {p.crowd}, (p, inside)
            if T == 1280:
                assert len(other_threads) == (2 if p.crowd == "iii" else 3)            # whole threads of ordinary kangaroos beside the crowd
        sets_seen.setdefault(tuple(cs), set()).add(p.crowd or p.i)
    assert all(len(v) == 1 for v in sets_seen.values())                                # no coupled set holds two placements, or a crowd and anything else


def test_record_lists_fit_the_capacity():
    for herd in HERDS:
        exp = E.expected("packed", *herd)
        assert len(exp.one_launch) <= E.RECORD_CAP and all(len(r) <= E.RECORD_CAP for r in exp.recs)
        assert len(exp.one_launch) == sum(len(r) for r in exp.recs)
    for herd in CYCLE_HERDS:
        assert len(E.expected("cycle", *herd).one_launch) <= E.RECORD_CAP


@pytest.mark.parametrize("herd", [h for h in HERDS if h[1] == 320], ids=[i for i, h in zip(IDS, HERDS) if h[1] == 320])
def test_one_launch_of_three_steps_is_three_launches_of_one(herd):
    """the expectation of the long launch is derived from the short ones: the model itself, run as one launch, agrees (the small herds; with keys SL.walk)"""
    case = E.packed_case(*herd)
    exp = E.expected("packed", *herd)
    states, recs = E.model_walk(case, case.states, E.STEPS)
    assert states == exp.after[-1] and sorted(recs) == sorted(exp.one_launch)
    assert len(states[0]) == (5 if case.keyed else 4)


@pytest.mark.parametrize("herd", CYCLE_HERDS, ids=["%s-T%d-G%d" % h for h in CYCLE_HERDS])
def test_cycle_herd(herd):
    family, T, G = herd
    case = E.cycle_case(*herd)
    exp = E.expected("cycle", *herd)
    geom = case.geom
    assert case.steps == S.WINDOW + 1 and case.steps - 1 - S.WINDOW == 0                 # the mark falls at step 0
    want = [(b, w, s) for b in range(2) for s in range(3) for w in ((0, 3) if T == 512 else (0,))]
    got = [(b, w, s) for b, w, _, s in (E.position(geom, p.i) for p in case.placements)]
    assert sorted(got) == sorted(want) and (geom.block, geom.blocks) == ((256, 2) if T == 512 else (64, 2))
    placed = {p.i for p in case.placements}
    for p in case.placements:
        assert [q.i for q in case.placements if q.i in E.coupled(geom, p.i)] == [p.i]
    # one CYCLE record per placed kangaroo (an ordinary one may run into a short cycle of its own on 64 jumps: the model says which, and they are few)
    cyc = [r for r in exp.one_launch if r[3] & S.CYCLE and r[2] in placed]
    assert sorted(r[2] for r in cyc) == sorted(placed)
    # marked after step 0, back on the mark two steps later: retired at step 2, on the marked point
    first, _ = S.step(case.states[case.placements[0].i][:4], case.jumps, case.scalars)
    for r in cyc:
        assert r[4] == 2 and r[3] & (K.DEAD | S.CYCLE) == K.DEAD | S.CYCLE and r[0] == first[0]
        assert exp.after[0][r[2]][3] & K.DEAD and (not case.keyed or r[5] == r[2] + 1)
    dead = {i for i, s in enumerate(exp.after[0]) if s[3] & K.DEAD}
    assert placed <= dead and len(dead - placed) <= geom.N // 64                           # the neighbours walk on
    if case.keyed:
        assert [s[:4] for s in exp.after[0]] == E.expected("cycle", "sym64", T, G).after[0]
