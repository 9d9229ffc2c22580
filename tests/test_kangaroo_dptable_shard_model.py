"""CPU: the model of the distinguished-point table divided over engines (tests/kangaroo_dptable_shard_model.py) against the model of the one table
(tests/kangaroo_dptable_model.py): the shard function stays below E, E shard tables fed through the routing hold what one table fed the whole stream holds,
the duplicates pair up the same way, and DEAD and tag-0 records never travel."""
from collections import Counter

import pytest

import kangaroo_model as K
import kangaroo_dptable_model as DM
import kangaroo_dptable_shard_model as SM

ENGINES = [1, 2, 3, 5, 8, 16]
KN = 96                                                               # kangaroos per engine


def test_shard_is_below_the_number_of_shards():
    rng = K.Stream(7)
    tags = [0, 1, SM.M64, SM.M64 - 1, 0xFFFF << 48, (0xFFFF << 48) - 1, 1 << 48, (1 << 48) - 1] + [rng.u64() for _ in range(2000)]
    for e in range(1, SM.MAX_SHARDS + 1):
        got = [SM.shard(t, e) for t in tags]
        assert max(got) == e - 1 == SM.shard(SM.M64, e) and min(got) == 0
        assert all(SM.shard(t, e) == (t >> 48) * e // 65536 for t in tags)
        # every shard gets its share of uniformly drawn tags: within a third of 1/E
        share = Counter(got[8:])
        assert all(abs(share[s] - 2000 / e) < 2000 / e / 3 + 12 for s in range(e)), (e, share)
    assert SM.shard(SM.M64, 1) == 0
    with pytest.raises(AssertionError):
        SM.shard(1, 17)


def launches_for(engines, seed, earlier=()):
    """one launch per engine: fresh tags, tags of `earlier` launches (certain duplicates), one tag in several engines' launches, DEAD records and tag-0
    records whose `d` is all the model has to tell them apart"""
    rng = K.Stream(seed)
    shared = [rng.u64() | 1 for _ in range(6)]
    out = []
    for e in range(engines):
        recs = []
        for i in range(KN):
            fl = K.WILD if i >= KN // 2 else 0
            tag = rng.u64() | 1
            if i % 7 == 3 and earlier:
                tag = earlier[(i * 31 + e) % len(earlier)]
            elif i % 11 == 5:
                tag = shared[(i + e) % len(shared)]
            elif i % 13 == 6:
                fl |= K.DEAD
            elif i % 17 == 8:
                tag = 0
            recs.append((tag, rng.u128(), fl, i))
        out.append(recs)
    return out


@pytest.mark.parametrize("engines", ENGINES)
def test_the_shards_hold_together_what_one_table_holds(engines):
    bases = [e * KN for e in range(engines)]
    one = DM.new_table(4096, 1024)
    shards = [DM.new_table(4096, 1024) for _ in range(engines)]
    earlier = []
    for seed in (1, 2, 3):
        launches = launches_for(engines, 100 * engines + seed, earlier)
        stream = [SM.with_base(r, bases[e]) for e, recs in enumerate(launches) for r in recs]
        before = set(one["cand"])
        one, back_one = DM.insert(one, stream)
        shards, backs = SM.relay(shards, launches, bases)
        back_sh = [b for per in backs for b in per]
        # the tags: jointly the one table's, every tag on the shard its bits name, and as many entries
        assert set().union(*[set(t["cand"]) for t in shards]) == set(one["cand"])
        assert sum(DM.entries(t) for t in shards) == DM.entries(one)
        for s, t in enumerate(shards):
            assert all(SM.shard(tag, engines) == s for tag in t["cand"])
        # every record ended the same way, under its global id ...
        how = lambda back: Counter((reason, rec[0], rec[3]) for reason, rec, _ in back if reason != DM.DPT_DUPLICATE)
        assert how(back_sh) == how(back_one)
        # ... and the duplicates pair up the same way: a tag that stood in the table meets the same stored entry; of a tag new in this launch one copy is
        # stored and the others each come back with it, whichever copy that is -- the pairs together name the same kangaroos
        known = {tag for tag in before if len(one["cand"][tag]) == 1}      # (the models know the stored copy only where one copy came)
        exact = lambda back: Counter((rec[0], rec[3], tuple(st) if rec[0] in known else None) for reason, rec, st in back
                                     if reason == DM.DPT_DUPLICATE and rec[0] in before)
        assert exact(back_sh) == exact(back_one) and (not earlier or any(st for _, _, st in exact(back_one)))
        fresh = lambda back: Counter(rec[0] for reason, rec, _ in back if reason == DM.DPT_DUPLICATE and rec[0] not in before)
        assert fresh(back_sh) == fresh(back_one) and (engines == 1 or fresh(back_one))
        senders = {}
        for tag, _, fl, kang in stream:
            if not fl & K.DEAD and tag and tag not in before:
                senders.setdefault(tag, Counter())[kang] += 1
        for back, tables in ((back_sh, shards), (back_one, [one])):
            came = {}
            for reason, rec, _ in back:
                if reason == DM.DPT_DUPLICATE and rec[0] not in before:
                    came.setdefault(rec[0], Counter())[rec[3]] += 1
            cand = {tag: c for t in tables for tag, c in t["cand"].items() if tag not in before}
            for tag, sent in senders.items():
                left = sent - came.get(tag, Counter())               # the one copy that did not come back is the stored one
                assert sum(left.values()) == 1 and next(iter(left)) in {c[2] for c in cand[tag]}, (tag, sent, came.get(tag))
        assert len(SM.duplicate_pairs(back_sh)) == len(SM.duplicate_pairs(back_one))
        earlier = sorted(one["cand"])[::5]


@pytest.mark.parametrize("engines", [2, 3, 16])
def test_dead_and_tag_zero_records_are_never_routed(engines):
    rng = K.Stream(5)
    recs = []
    for i in range(64 * engines):
        tag = (i % engines * 65536 // engines + 65536 // engines // 2) << 48 | rng.u64() >> 16      # shard i % engines
        assert SM.shard(tag, engines) == i % engines
        recs.append((tag, rng.u128(), (K.WILD if i & 1 else 0) | (K.DEAD if i % 3 == 0 else 0), i))
    recs += [(0, rng.u128(), K.WILD, 9000 + j) for j in range(5)]
    for own in range(engines):
        mine, groups = SM.split(recs, own, engines, base=1000)
        assert not groups[own]
        assert all(SM.routable(SM.with_base(r, -1000)) and SM.shard(r[0], engines) == to for to, g in enumerate(groups) for r in g)
        dead_or_zero = [SM.with_base(r, 1000) for r in recs if not SM.routable(r)]
        assert [r for r in mine if not SM.routable(r)] == dead_or_zero and len(dead_or_zero) > 64 * engines // 3
        assert len(mine) + sum(map(len, groups)) == len(recs)
        table, back, _ = SM.insert(DM.new_table(1024, 1024), recs, own, engines, 1000)
        assert Counter(reason for reason, _, _ in back) == Counter({DM.DPT_DEAD: len(dead_or_zero) - 5, DM.DPT_TAG_ZERO: 5})
        assert DM.entries(table) == len(mine) - len(dead_or_zero)
