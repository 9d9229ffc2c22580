"""CPU checks of tests/equal_x_cases.py, the inputs of tests/test_gpu_equal_x_positions.py:
  * the case lists put an equal-x giant on EVERY position class of every tile kernel with both signs of the centre (a condition on the inputs: a later edit of
    the matrix cannot quietly drop a position);
  * the oracle's hit list over each case's table contains the completeness set the geometry demands;
  * a slipped substitution at any site of tile_pair_walk, in an integer restatement of its chain, fails cases of the lists;
  * the oracle's keys of the equal-x thread equal x(P - G), x(P + G) and x(2P) recomputed with pybsgs.ecpy on Python integers (the minus key of the equal-x
    giant is reference-defined garbage -- s = 1 / (2 Py) used as if it were 1 / (Px - Gx) -- and is taken from o_tile_xs only)."""
import numpy as np
import pytest

import equal_x_cases as E
import oracle_lib as O
from pybsgs import ecpy

P10, P7 = (64, 8, 10), (64, 8, 7)          # the pair chain by batch length, the per-giant kernel by an odd one

ALL_LISTS = ([("single", (g,)) for g in (E.BASE, P10, P7)] + [("walk", (k,)) for k in E.WALK_KINDS] +
             [("clamped", (False,)), ("clamped", (True,)), ("narrow", ())])


def _covered(cases, kernel):
    out = set()
    for c in cases:
        out |= E.case_classes(c, kernel)
    return out


def _all(kernel, p):
    return {(c, s) for c in E.classes(kernel, p) for s in (1, -1)}


def test_positions_are_the_kernels_classes():
    assert E.positions("giant", 7) == [("first",)] + [("middle",)] * 5 + [("last",)]
    assert E.positions("pair", 6) == [("a", "first"), ("b", "first"), ("a", "middle"), ("b", "middle"), ("a", "last"), ("b", "last")]
    assert E.positions("quad", 12) == [(e, ph) for ph in ("first", "middle", "last") for e in "abcd"]
    assert E.positions("walk", 12)[:4] == [("jl", "first"), ("jh", "first"), ("jl", "middle"), ("jh", "middle")] and E.positions("walk", 12)[10:] == [("jl", "last"), ("jh", "last")]
    assert len(E.classes("giant", 12)) == 3 and len(E.classes("pair", 12)) == 6 and len(E.classes("quad", 12)) == 12 and len(E.classes("walk", 12)) == 12
    assert len(E.classes("quad", 128)) == 12                       # the narrow batching: 32 quads


def test_case_lists_cover_every_class_of_every_kernel_with_both_signs():
    base = E.single_cases(E.BASE)
    for kernel in ("quad", "pair", "giant"):                        # variants 13, 10 and 0 at p = 12
        assert _covered(base, kernel) == _all(kernel, 12), kernel
    assert _covered(E.single_cases(P10), "pair") == _all("pair", 10)
    assert _covered(E.single_cases(P7), "giant") == _all("giant", 7)
    for kind in ("eq_random", "random_eq"):                         # each side of the pair on its own: half of the walk's classes each
        tl = "A" if kind == "eq_random" else "B"
        assert _covered(E.walk_cases(kind), "walk") == {(c, s) for c, s in _all("walk", 12) if c[0] == tl}, kind
    for kind in ("same_twice", "plus_minus", "two_slots", "two_threads"):
        assert _covered(E.walk_cases(kind), "walk") == _all("walk", 12), kind
    # the thread of the equal-x giant: lane 0, a wave edge, a block edge, the last thread -- all of them occur, in both blocks
    for cases in (base, E.walk_cases("eq_random"), E.walk_cases("random_eq")):
        assert {c.thread(i) for c in cases for _, i, _ in c.eq} == {0, 63, 64, 255, 256, 511}
    # two_slots: both the partner slot of the same quad and a slot of another quad; two_threads: same block, another wave and lane
    same = [c for c in E.walk_cases("two_slots") if c.slot(c.eq[0][1]) >> 1 == c.slot(c.eq[1][1]) >> 1]
    assert len(same) == 24 and len(E.walk_cases("two_slots")) == 48
    assert all(c.thread(c.eq[0][1]) == c.thread(c.eq[1][1]) and c.eq[0][1] != c.eq[1][1] for c in E.walk_cases("two_slots"))
    for c in E.walk_cases("two_threads"):
        ta, tb = c.thread(c.eq[0][1]), c.thread(c.eq[1][1])
        assert ta != tb and ta // 256 == tb // 256 and ta % 64 != tb % 64 and ta // 64 != tb // 64
    # clamped lanes: thread 287 at a first, a middle and a last slot of both chains, thread 0, and the single partial wave
    for pair, kernel in ((False, "quad"), (True, "walk")):
        cl = [c for c in E.clamped_cases(pair) if c.geom == E.CLAMPED]
        assert {ph for c in cl for _, i, _ in c.eq if c.thread(i) == 287 for ph in [E.positions(kernel, 12)[c.slot(i)][-1]]} == {"first", "middle", "last"}
        assert any(c.thread(i) == 0 for c in cl for _, i, _ in c.eq)
        assert any(c.geom == E.WAVE32 for c in E.clamped_cases(pair))
    # narrow batching: the first and the last quad of 32, every element of each; every wave of the block is in some case's table
    nr = E.narrow_cases()
    assert {E.positions("quad", 128)[c.slot(c.eq[0][1])] for c in nr} == {(e, ph) for e in "abcd" for ph in ("first", "last")}
    assert {w for c in nr for w in c.waves} == {0, 1, 2, 3} and all(0 in c.waves and len(c.waves) == 3 for c in nr)
    assert all(c.thread(c.eq[0][1]) == E.NARROW_THREAD and c.batching == E.NARROW_ENGINE for c in nr)


@pytest.mark.parametrize("name,args", ALL_LISTS, ids=lambda v: str(v).replace(" ", ""))
def test_oracle_lists_contain_the_completeness_set(name, args):
    for n, bt in enumerate(E.built_list(name, *args)):
        case = bt.case
        T, pe = case.batching
        blocks = {case.thread(i) // E.BLOCK for _, i, _ in case.eq}
        live = sum(min((blk + 1) * E.BLOCK, T) - blk * E.BLOCK for blk in blocks) if case.waves is None else 64 * len(case.waves)
        assert len(bt.complete) == 2 * live * pe * len(case.centres) + 1, case.name
        assert sum(1 for _, c, _ in bt.complete if c == 4) == len(case.eq)
        _, want = E.expected(name, args, n)
        assert len(want) <= E.HIT_BUFFER, case.name
        assert len(set(want)) == len(want) and bt.complete <= set(want), (case.name, sorted(bt.complete - set(want))[:8])
        assert want == sorted(want, key=lambda h: (h[0], h[2], h[1]))                # the order bsgs_collect reports in
        for tile, i, _ in case.eq:
            assert (tile, 4, i) in want and (tile, 1, i) not in want


def _giants_int(first, count):
    """G2[first .. first + count) = (i + 1) * ADDPUBG on Python integers"""
    A = ecpy.addpubg(E.W)
    g = ecpy.mul(first + 1, A)
    out = []
    for _ in range(count):
        out.append(g)
        g = ecpy.add(g, A)
    return out


@pytest.mark.parametrize("name,args", ALL_LISTS, ids=lambda v: str(v).replace(" ", ""))
def test_keys_of_the_equal_x_thread_equal_python_integers(name, args):
    for bt in E.built_list(name, *args):
        case = bt.case
        t, b, p = case.geom
        pe = case.batching[1]
        for tile, ieq, sign in case.eq:
            P = case.centres[tile]
            th = case.thread(ieq)
            (g0, keys), = [(g, k) for (tl, g), k in bt.slices.items() if tl == tile and g <= ieq < g + len(k)]
            G = _giants_int(th * pe, pe)
            assert G[ieq - th * pe] == (P if sign > 0 else ecpy.neg(P)), case.name
            for r, Gi in enumerate(G):
                i = th * pe + r
                assert O.g2_unpack(E.giants(case.geom)[0], t, b, p, i) == Gi
                eq, xm, xp, xd = O.tile_xs(P, Gi, 0)
                km, kp = (int(v) for v in keys[i - g0])
                if i == ieq:
                    assert eq == 1 and xd == ecpy.add(P, P)[0], (case.name, i)
                    assert (km, kp) == (xm & E.MASK64, xd & E.MASK64), (case.name, i)
                else:
                    assert eq == 0 and xm == ecpy.add(P, ecpy.neg(Gi))[0] and xp == ecpy.add(P, Gi)[0], (case.name, i)
                    assert (km, kp) == (xm & E.MASK64, xp & E.MASK64), (case.name, i)


def test_thread_digests_are_xor_and_sum_of_the_listed_keys():
    bt = E.build("walk", ("plus_minus",), 3)
    dg = E.thread_digests(bt)
    assert len(dg) == 2 * 256
    for (tile, th), (x, s) in list(dg.items())[::37]:
        (g0, keys), = [(g, k) for (tl, g), k in bt.slices.items() if tl == tile]
        mine = [int(v) for v in keys[th * 12 - g0:th * 12 - g0 + 12].reshape(-1)]
        xx = 0
        for v in mine:
            xx ^= v
        assert (x, s) == (xx, sum(mine) & E.MASK64)
    assert np.array_equal(bt.keys, np.unique(bt.keys)) and len(bt.keys) <= 2 * 2 * 256 * 12 + 1


def test_every_slipped_site_of_the_pair_walk_fails_cases():
    """E.walk_chain_wrong restates tile_pair_walk's chain on Python integers with ONE substitution site slipped (forgotten, or given the other tile's Py) and
    lists the elements whose s is then wrong: their records, which the completeness set demands, would be missing.  Every one of the nine sites, slipped either
    way, must fail cases of the walk lists; the one-sided lists catch the sites of their own tile."""
    lists = {k: E.walk_cases(k) for k in E.WALK_KINDS}
    allc = [c for k in E.WALK_KINDS for c in lists[k]]
    assert len(allc) == 168
    assert not any(E.walk_chain_wrong(c, c.thread(i)) for c in allc for _, i, _ in c.eq)          # nothing slipped: every s is 1 / d
    for site in E.WALK_SITES:
        own = "eq_random" if site in ("p1A", "d.da", "d.dc", "c.dc", "a.da") else "random_eq"     # the tile whose element the site substitutes
        for how in E.WALK_SLIPS:
            caught = {k: sum(E.walk_slip_caught(c, (site, how)) for c in lists[k]) for k in E.WALK_KINDS}
            assert sum(caught.values()) >= 48, (site, how, caught)
            assert caught[own] >= 10 and caught["plus_minus"] >= 10 and caught["two_slots"] >= 12, (site, how, caught)
            if how == "other":
                assert caught["same_twice"] == 0                 # both tiles have the same Py there: that slip changes nothing
    # phase 1 is caught at every slot; a site of the probe loop at the slots of its own element (every other one)
    assert sum(E.walk_slip_caught(c, ("p1A", "forget")) for c in lists["eq_random"]) == 24
    assert sum(E.walk_slip_caught(c, ("d.dd", "forget")) for c in lists["random_eq"]) == 12
    # element a forgotten: inv = u * 0, every quad BELOW is spoilt in both tiles -- at Q = 0 the value is dead, so 10 of the 12 jl cases fail
    a_caught = [c.name for c in lists["eq_random"] if E.walk_slip_caught(c, ("a.da", "forget"))]
    assert len(a_caught) == 10 and not any(n.startswith("eq_random-j0") for n in a_caught)
    c = next(c for c in lists["eq_random"] if c.name.startswith("eq_random-j4+"))
    assert E.walk_chain_wrong(c, c.thread(c.eq[0][1]), ("a.da", "forget")) == [(tl, j) for tl in (0, 1) for j in range(4)]
