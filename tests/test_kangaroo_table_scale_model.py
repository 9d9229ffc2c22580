"""CPU: tests/kangaroo_table_scale_cases.py pinned before a GPU test relies on it.  Its set reference and its checks against the slot-level models
(tests/kangaroo_tames_gen_model.py, kangaroo_tames_extend_model.py, kangaroo_dptable_model.py) on a few hundred random small launches answered by a
slot-by-slot device simulated here, which takes the records in a random order; every check refuses an answer that is wrong in one record; the occupancy
rule against the slots of the models; and the generators of the scale launches hold what they claim."""
import random
from collections import Counter

import numpy as np
import pytest

import kangaroo_dptable_model as DM
import kangaroo_model as K
import kangaroo_table_scale_cases as SC
import kangaroo_tames_extend_model as XM
import kangaroo_tames_gen_model as GM

CAPACITY, CAP = 64, 192                                               # 512 slots; a sequence of launches leaves at most 300 tags in them: never FULL
SLOTS = GM.n_slots(CAPACITY, CAP)


def test_constants_are_the_models():
    assert SLOTS == 512 == SC.n_slots(CAPACITY, CAP) == DM.n_slots(CAPACITY, CAP)
    assert SC.SLOTS == GM.n_slots(SC.CAPACITY, SC.CAP) == DM.n_slots(SC.CAPACITY, SC.CAP) == 1 << 21
    assert (SC.R_DEAD, SC.R_DUPLICATE, SC.R_TAG_ZERO, SC.R_FULL) == (GM.GEN_DEAD, GM.GEN_DUPLICATE, GM.GEN_TAG_ZERO, GM.GEN_FULL)
    assert (SC.R_DEAD, SC.R_DUPLICATE, SC.R_TAG_ZERO, SC.R_FULL, SC.R_STORED) == (DM.DPT_DEAD, DM.DPT_DUPLICATE, DM.DPT_TAG_ZERO, DM.DPT_FULL, DM.DPT_STORED)
    assert (SC.WILD, SC.NEG, SC.DEAD) == (DM.WILD, DM.NEG, K.DEAD) and SC.LOAD_CHUNK == XM.LOAD_CHUNK
    fl = [0, 1, 2, 3, 1 | 1 << 8 | 37 << 9, 2 | 1 << 8, K.DEAD | 3]
    assert list(SC.entry_type(np.array(fl, np.uint32))) == [DM.type_of(f) for f in fl]
    for t in (1, 63, 64, (1 << 64) - 1, 0x123456789ABCDEF0):
        assert int(SC.home(np.array([t], np.uint64), SLOTS)[0]) == GM.home(t, SLOTS) == DM.home(t, SLOTS)


def test_the_record_layout_is_the_binding_s():
    """REC is pybsgs.KangarooRecord field by field, and the raw forms of the wrappers take its bytes (importing pybsgs needs no GPU)"""
    import ctypes
    import pybsgs
    assert ctypes.sizeof(pybsgs.KangarooRecord) == SC.REC.itemsize == 64
    for name in ("x", "d", "kangaroo", "flags", "step", "reserved"):
        assert getattr(pybsgs.KangarooRecord, name).offset == SC.REC.fields[name][1]
    recs = SC.make_records(np.random.default_rng(1), np.array([5, 6], np.uint64), np.array([1, 3], np.uint32), 2)
    ptr, m, keep = pybsgs.Device._raw_records_in(recs.tobytes())
    assert m == 2 and ptr[1].kangaroo == int(recs["kangaroo"][1]) and bytes(ptr[1].d) == recs["d"][1].tobytes() and ptr[0].flags == 1
    assert pybsgs.Device._raw_records_in(recs)[1] == 2                # anything with the buffer protocol
    with pytest.raises(pybsgs.BsgsError, match="no multiple of 64"):
        pybsgs.Device._raw_records_in(b"\0" * 65)


def small_launch(rnd, universe, launch):
    """up to 100 records whose tags come from a small universe (so tags repeat in the launch and across launches), with tag 0 and DEAD among them"""
    n = rnd.randrange(1, 101)
    tags = [rnd.choice(universe) if rnd.random() < 0.9 else 0 for _ in range(n)]
    flags = [rnd.choice([0, 1, 3, 1 | 1 << 8 | 37 << 9]) | (K.DEAD if rnd.random() < 0.08 else 0) | (4 if rnd.random() < 0.02 else 0) for _ in range(n)]
    return SC.make_records(np.random.default_rng(rnd.randrange(1 << 30)), np.array(tags, np.uint64), np.array(flags, np.uint32), launch)


def as_tuples(recs):
    """(tag, d, flags, kangaroo) as the models take them"""
    return [(int(r["x"][0]), int(r["d"][0]) | int(r["d"][1]) << 64, int(r["flags"]), int(r["kangaroo"])) for r in recs]


def simulated_device(rnd, slots_tag, slots_entry, recs):
    """the insert slot by slot, the records taken in a random order: the table's slots are updated in place -> the hand-backs as a REC array in the layout of
    the distinguished-point table (a duplicate behind its STORED record, which is written from the slot after all inserts, as the resolve does)"""
    n_slots = len(slots_tag)
    out = []                                                          # (record index, reason, slot)
    for i in rnd.sample(range(len(recs)), len(recs)):
        tag, fl = int(recs["x"][i, 0]), int(recs["flags"][i])
        if fl & K.DEAD:
            out.append((i, SC.R_DEAD, None))
        elif tag == 0:
            out.append((i, SC.R_TAG_ZERO, None))
        else:
            s = GM.home(tag, n_slots)
            while slots_tag[s] not in (0, tag):
                s = (s + 1) & (n_slots - 1)
            if slots_tag[s] == 0:
                slots_tag[s] = tag
                slots_entry[s] = (tag, int(recs["d"][i, 0]), int(recs["d"][i, 1]), int(recs["kangaroo"][i]), int(SC.entry_type(recs["flags"][i:i + 1])[0]))
            else:
                out.append((i, SC.R_DUPLICATE, s))
    rnd.shuffle(out)
    got = np.zeros(len(out) + sum(1 for _, r, _ in out if r == SC.R_DUPLICATE), SC.REC)
    k = 0
    for i, reason, s in out:
        if reason == SC.R_DUPLICATE:
            t, d0, d1, kid, ty = slots_entry[s]
            got["x"][k, 0], got["d"][k], got["kangaroo"][k], got["flags"][k], got["reserved"][k] = t, (d0, d1), kid, ty, SC.R_STORED
            k += 1
        got[k] = recs[i]
        got["reserved"][k] = reason
        k += 1
    return got


def table_rows(slots_entry):
    return np.array([e for e in slots_entry if e is not None], np.uint64).reshape(-1, 5)


def as_dicts(got):
    """hand-backs as pybsgs gives them to DM.check_device (x = the tag: the model compares the whole x with what it sent)"""
    return [{"x": int(r["x"][0]), "d": int(r["d"][0]) | int(r["d"][1]) << 64, "kangaroo": int(r["kangaroo"]), "flags": int(r["flags"]), "step": int(r["step"]),
             "reason": int(r["reserved"])} for r in got]


def wrong_answers(rnd, ref, recs, walk, stored, dup, n_entries, table):
    """(what is wrong, the arguments of check_launch / check_pairs with one thing wrong) for everything this answer allows"""
    def launch(**kw):
        a = {"back": walk, "n_entries": n_entries, "table": table}
        a.update(kw)
        return a
    yield "entry count", launch(n_entries=n_entries + 1), None
    extra = np.zeros(1, SC.REC)                                       # what a lane past the last record of a ragged wave would make of zeros behind the records
    extra["reserved"] = SC.R_TAG_ZERO
    yield "a record that was never sent", launch(back=np.concatenate([walk, extra])), None
    if len(table):
        yield "a tag missing from the table", launch(table=table[1:]), None
        t = table.copy()
        t[rnd.randrange(len(t)), 1] ^= np.uint64(1)
        yield "an offset of the table changed", launch(table=t), None
    if len(walk):
        k = rnd.randrange(len(walk))
        yield "a record lost", launch(back=np.delete(walk, k)), None
        w = walk.copy()
        w["d"][k, 1] ^= np.uint64(1 << 40)
        yield "a bit of a record", launch(back=w), None
        w = walk.copy()
        w["step"][k] += 1
        yield "the step of a record", launch(back=w), None
    if len(walk) > 1 and len({(int(r["x"][0]), int(r["reserved"])) for r in walk}) < len(walk):
        by = Counter((int(r["x"][0]), int(r["reserved"])) for r in walk)
        key = next(k for k, c in by.items() if c > 1)
        i, j = [k for k, r in enumerate(walk) if (int(r["x"][0]), int(r["reserved"])) == key][:2]
        w = walk.copy()
        w[j] = w[i]
        yield "one record twice in the place of another of its tag", launch(back=w), None
    fresh_dups = [k for k, r in enumerate(walk) if r["reserved"] == SC.R_DUPLICATE and SC.is_in(r["x"][:1], ref["new_tags"])[0]]
    if fresh_dups:                                                    # the table claims a copy that also came back
        r = walk[rnd.choice(fresh_dups)]
        t = table.copy()
        row = int(np.flatnonzero(t[:, 0] == r["x"][0])[0])
        t[row] = (r["x"][0], r["d"][0], r["d"][1], r["kangaroo"], SC.entry_type(r["flags"]))
        yield "the stored copy also handed back", launch(table=t), None
    if len(stored) > 1 and len(set(stored["x"][:, 0].tolist())) > 1:
        j = next(k for k in range(1, len(stored)) if stored["x"][k, 0] != stored["x"][0, 0])
        s = stored.copy()
        for f in ("d", "kangaroo", "flags"):
            s[f][[0, j]] = stored[f][[j, 0]]
        yield "a pair names another tag's entry", None, (s, dup, table)


@pytest.mark.parametrize("seed", range(100))
def test_reference_and_checks_against_the_slot_models(seed):
    """three launches in a row on one small table: the set reference says what the three slot-level models say, the simulated device passes the models' check
    and this file's, and an answer with one thing wrong does not"""
    rnd = random.Random(seed)
    universe = [rnd.getrandbits(64) | 1 for _ in range(40)] + GM.chain_tags(rnd.randrange(SLOTS), SLOTS, 25, salt=seed + 1) + GM.chain_tags(SLOTS - 1, SLOTS, 25, salt=seed + 2)
    universe = list(dict.fromkeys(universe))
    gm, dm = GM.new_table(CAPACITY, CAP), DM.new_table(CAPACITY, CAP)
    slots_tag, slots_entry = [0] * SLOTS, [None] * SLOTS
    held = np.zeros(0, np.uint64)
    refused = Counter()
    for launch in range(1, 4):
        recs = small_launch(rnd, universe, launch)
        tup = as_tuples(recs)
        ref = SC.reference(held, recs)
        # the growing tame table's model
        gm_new, gm_back = GM.insert(gm, [(t, d, fl) for t, d, fl, _ in tup])
        assert not any(r == GM.GEN_FULL for _, r in gm_back)
        assert Counter((int(t), int(r)) for t, r in ref["back"]) == gm_back
        assert ref["tags"].tolist() == sorted(gm_new["cand"]) and ref["entries"] == GM.entries(gm_new)
        assert ref["new_tags"].tolist() == sorted(set(gm_new["cand"]) - set(gm["cand"]))
        for t in ref["new_tags"].tolist():
            mine = ref["cand"][ref["cand"][:, 0] == t]
            assert {int(r[1]) | int(r[2]) << 64 for r in mine} == gm_new["cand"][t]
        # the distinguished-point table's model
        dm_new, dm_back = DM.insert(dm, tup)
        assert Counter((int(t), int(r)) for t, r in ref["back"]) == Counter((rec[0], reason) for reason, rec, _ in dm_back)
        assert ref["tags"].tolist() == sorted(dm_new["cand"]) and ref["entries"] == DM.entries(dm_new)
        for t in ref["new_tags"].tolist():
            mine = ref["cand"][ref["cand"][:, 0] == t]
            assert {(int(r[0]), int(r[1]) | int(r[2]) << 64, int(r[3]), int(r[4])) for r in mine} == dm_new["cand"][t]
        # occupancy without probing order = the slots of both models, however the device ordered the records
        before = table_rows(slots_entry)
        got = simulated_device(rnd, slots_tag, slots_entry, recs)
        occ = SC.occupied(ref["tags"], SLOTS)
        assert occ.tolist() == [t != 0 for t in gm_new["tags"]] == [t != 0 for t in dm_new["tags"]] == [t != 0 for t in slots_tag]
        runs = "".join("x" if o else " " for o in occ.tolist())
        runs = (runs + runs).split() if " " in runs else [runs]
        assert SC.longest_run(occ) == min(SLOTS, max((len(r) for r in runs), default=0))
        # the simulated device: right by the model's check and by this file's
        table = table_rows(slots_entry)
        dm, _ = DM.check_device(dm, tup, as_dicts(got), len(table))
        walk, stored, dup = SC.split_pairs(got)
        assert len(got) == len(ref["back"]) + int((ref["back"][:, 1] == SC.R_DUPLICATE).sum())
        SC.check_launch(ref, recs, walk, len(table), table, before)
        SC.check_pairs(stored, dup, table)
        SC.check_launch(ref, recs, walk, len(table), table[:, :3], before[:, :3])      # the table without owners
        for what, a, p in wrong_answers(rnd, ref, recs, walk, stored, dup, len(table), table):
            with pytest.raises(AssertionError):
                if a is not None:
                    SC.check_launch(ref, recs, a["back"], a["n_entries"], a["table"], before)
                else:
                    SC.check_pairs(*p)
            refused[what] += 1
        if len(stored):                                               # a pair torn apart
            torn = np.concatenate([got[got["reserved"] != SC.R_STORED], got[got["reserved"] == SC.R_STORED]])
            with pytest.raises(AssertionError):
                SC.split_pairs(torn)
        # the loads: the same tags as (tag, d) pairs and as entries, on the table as it stands
        counts, tags = SC.reference_load(held, recs["x"][:, 0])
        _, n = XM.load(gm, [(t, d) for t, d, _, _ in tup])
        assert counts == (n["stored"], n["duplicate"], n["zero"], n["full"])
        dm_loaded, n = DM.load({"slots": SLOTS, "tags": list(gm["tags"]), "cand": {}}, [(t, d, k, DM.type_of(fl)) for t, d, fl, k in tup])
        assert counts == n and tags.tolist() == sorted(t for t in dm_loaded["tags"] if t)
        gm, held = gm_new, ref["tags"]
    assert refused["entry count"] == 3


def test_every_kind_of_wrong_answer_was_tried():
    """over the seeds above every corruption of wrong_answers finds a launch it applies to (so each of the checks is known to bite)"""
    seen = Counter()
    for seed in range(12):
        rnd = random.Random(seed)
        universe = [rnd.getrandbits(64) | 1 for _ in range(30)]
        recs = small_launch(rnd, universe, 1)
        slots_tag, slots_entry = [0] * SLOTS, [None] * SLOTS
        got = simulated_device(rnd, slots_tag, slots_entry, recs)
        table = table_rows(slots_entry)
        walk, stored, dup = SC.split_pairs(got)
        for what, _, _ in wrong_answers(rnd, SC.reference(np.zeros(0, np.uint64), recs), recs, walk, stored, dup, len(table), table):
            seen[what] += 1
    assert set(seen) == {"entry count", "a record that was never sent", "a tag missing from the table", "an offset of the table changed", "a record lost", "a bit of a record", "the step of a record",
                         "one record twice in the place of another of its tag", "the stored copy also handed back", "a pair names another tag's entry"}


@pytest.mark.parametrize("seed", range(20))
def test_reference_match_against_the_tame_table_model(seed):
    import kangaroo_tames_model as TM
    rnd = random.Random(1000 + seed)
    universe = [rnd.getrandbits(64) for _ in range(60)] + TM.chain_tags(rnd.randrange(64), n=30, salt=seed + 1)
    recs = small_launch(rnd, universe, 1)
    table = np.unique(np.array(rnd.sample(universe, 30) + ([0] if seed % 2 else []), np.uint64))
    keep, word = SC.reference_match(recs, table)
    kept = recs[keep]
    mine = sorted((int(r["x"][0]), int(r["d"][0]) | int(r["d"][1]) << 64, int(r["kangaroo"]), int(r["flags"]), int(r["step"]), int(w) - 1 if w else None)
                  for r, w in zip(kept, word))
    want = TM.match([(t, d, k, fl, int(s)) for (t, d, fl, k), s in zip(as_tuples(recs), recs["step"])], table.tolist())
    assert mine == want and len(want) > 0
    # sorted_words: equal for equal multisets, different when one word differs
    p = np.random.default_rng(seed).permutation(len(kept))
    assert np.array_equal(SC.sorted_words(kept, word), SC.sorted_words(kept[p], word[p]))
    other = word.copy()
    other[0] ^= 1
    assert not np.array_equal(SC.sorted_words(kept, word), SC.sorted_words(kept, other))


# ---- the generators of the scale launches ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    return SC.scale_case()


def test_the_main_launch_holds_what_it_claims(case):
    (name, recs), ref, plan = case["launches"][0], case["refs"][0], case["plan"]
    assert name == "main" and len(recs) == SC.N1 == SC.CAP and recs.dtype == SC.REC and recs.nbytes == 64 * SC.N1
    tag, fl = recs["x"][:, 0], recs["flags"]
    dead = (fl & SC.DEAD) != 0
    live = ~dead & (tag != 0)
    assert dead.sum() == SC.N_DEAD and (~dead & (tag == 0)).sum() == SC.N_ZERO
    tail = np.arange(SC.N1 - 37, SC.N1)
    assert (~dead & (tag == 0))[tail].sum() == 3 and dead[tail].sum() == 3        # both kinds in the ragged third iteration
    # multiplicities of the live tags
    uniq, counts = np.unique(tag[live], return_counts=True)
    singles = len(plan["singles"])
    assert Counter(counts.tolist()) == Counter({1: singles + SC.CHAIN_A_LEN + SC.CHAIN_B_LEN, 2: 30000, 3: 3000, 64: 64 + 1, 512: 1, 4096: 8})
    assert singles > 300000 and len(uniq) == ref["entries"] == len(ref["new_tags"])
    # positions: the copies of a group spread over the whole launch -- both full iterations, many blocks, all eight XCDs (blocks are dealt out round robin)
    stride = SC.INSERT_GRID_MAX * SC.BLOCK
    for t in plan["groups"][4096]:
        at = np.flatnonzero(tag == t)
        assert len(at) == 4096 and set((at // stride).tolist()) >= {0, 1}
        blocks = (at % stride) // SC.BLOCK
        assert len(np.unique(blocks)) > 900 and set((blocks % 8).tolist()) == set(range(8)) and len(np.unique(at // 64)) > 3000
    two = plan["groups"][2][:300]
    first = np.array([np.flatnonzero(tag == t) for t in two])
    assert first.shape == (300, 2) and 100 < ((first[:, 0] // stride) != (first[:, 1] // stride)).sum() < 200      # about half of the pairs span the two iterations
    t, w = plan["whole"]
    assert np.flatnonzero(tag == t).tolist() == list(range(64 * w, 64 * w + 64)) and 64 * w + 64 <= SC.N1 - 37
    t, waves = plan["lane5"]
    assert np.array_equal(np.flatnonzero(tag == t), 64 * waves + 5) and len(np.unique(waves)) == 512 and w not in waves
    # the chains
    for chain, h, n in ((plan["chain_a"], SC.CHAIN_A_HOME, 4096), (plan["chain_b"], SC.SLOTS - 1, 2048)):
        assert len(np.unique(chain)) == n and (SC.home(chain, SC.SLOTS) == h).all() and SC.is_in(chain, uniq).all()
        at = np.flatnonzero(SC.is_in(tag, np.sort(chain)))
        assert len(at) == n and len(np.unique(at // stride)) >= 2 and len(np.unique((at % stride) // SC.BLOCK % 8)) == 8
    # the DEAD records: tags of their own, tags that also live in this launch, tag 0
    dt = tag[dead]
    assert (dt == 0).sum() > 300 and SC.is_in(dt, uniq).sum() > 300 and (~SC.is_in(dt, uniq) & (dt != 0)).sum() > 300
    assert (fl[dead] & SC.CYCLE).any()
    # flags and the words that tell records apart
    assert set(np.unique(fl[live]).tolist()) == set(SC.FLAG_CHOICES.tolist()) and {0, 1, 3} == set(np.unique(SC.entry_type(fl[live])).tolist())
    d = recs["d"]
    assert len(np.unique(d[:, 0])) == len(np.unique(recs["kangaroo"])) == len(np.unique(recs["step"])) == SC.N1
    assert (recs["reserved"] > SC.R_STORED).all() and recs["x"][:, 1:].any(axis=1).all()


def test_the_launches_stay_far_from_full(case):
    names = [n for n, _ in case["launches"]]
    assert names == ["main", "again", "fresh", "mixed"] and case["launches"][1][1] is case["launches"][0][1]
    main, again, fresh, mixed = case["refs"]
    assert all(r["load"] <= 0.70 and r["chain"] <= 4096 for r in case["refs"])
    assert main["chain"] == 4096                                      # the chain of 4096 tags is the longest run, and no random tag made it longer
    occ = SC.occupied(main["tags"], SC.SLOTS)
    assert occ[SC.CHAIN_A_HOME:SC.CHAIN_A_HOME + 4096].all() and not occ[SC.CHAIN_A_HOME - 1] and not occ[SC.CHAIN_A_HOME + 4096]
    assert occ[SC.SLOTS - 1] and occ[:2047].all() and not occ[2047] and not occ[SC.SLOTS - 2]
    # the same launch again: nothing new, every live record of a non-zero tag a duplicate -- the hand-back buffer of the distinguished-point table at its bound
    n_single = SC.N_DEAD + SC.N_ZERO
    assert again["entries"] == main["entries"] and len(again["new_tags"]) == 0 and len(again["back"]) == SC.N1
    assert (again["back"][:, 1] == SC.R_DUPLICATE).sum() == SC.N1 - n_single and 2 * SC.N1 - n_single > SC.CAP
    # fresh: N1 new tags, about 45 %; mixed: half new, half held, at most 60 %
    assert len(fresh["new_tags"]) == SC.N1 and len(fresh["back"]) == 0 and 0.40 < fresh["load"] < 0.50
    recs = case["launches"][3][1]
    held = SC.is_in(recs["x"][:, 0], fresh["tags"])
    assert held.sum() == SC.N1 // 2 and len(mixed["new_tags"]) == SC.N1 - SC.N1 // 2 and mixed["load"] <= 0.60
    assert len(np.unique(recs["x"][:, 0][held])) < held.sum()         # some held tags twice in the launch
    assert abs(int(held[:SC.N1 // 2].sum()) - SC.N1 // 4) < 5000      # at random positions


def test_the_load_holds_what_it_claims(case):
    e, plan = case["entries"], case["load_plan"]
    assert len(e) == SC.LOAD_PAIRS == (1 << 20) + (1 << 18) and e.nbytes == 32 * SC.LOAD_PAIRS
    c1, c2 = e["tag"][:SC.LOAD_CHUNK], e["tag"][SC.LOAD_CHUNK:]
    u1, n1 = np.unique(c1[c1 != 0], return_counts=True)
    u2, n2 = np.unique(c2[c2 != 0], return_counts=True)
    assert (c1 == 0).sum() == 576 and (c2 == 0).sum() == 144
    assert np.array_equal(u1[n1 == 2], np.sort(plan["twice_in_1"])) and np.array_equal(u2[n2 == 2], np.sort(plan["twice_in_2"]))      # duplicates inside a chunk
    across = np.intersect1d(u1, u2)
    assert np.array_equal(across, np.sort(np.concatenate([plan["both_chunks"], plan["again_in_2"]]))) and len(across) == 88000          # and across the two
    assert case["load_counts"] == (1172000, SC.LOAD_PAIRS - 720 - 1172000, 720, 0) and len(case["load_tags"]) == 1172000
    assert len(case["load_tags"]) <= 0.70 * SC.SLOTS and np.array_equal(e["d"][:, 0], np.arange(SC.LOAD_PAIRS, dtype=np.uint64))
    assert set(np.unique(e["type"]).tolist()) == {0, 1, 3}
