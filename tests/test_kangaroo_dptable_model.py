"""CPU: the rule of the distinguished-point table in device memory as tests/kangaroo_dptable_model.py restates it (include/bsgs_hip.h, "Kangaroo,
distinguished-point table in device memory"): insert with resolve, load and read on hand-made record sets -- one tag many times, tag 0, DEAD, a home at the
last slot, a table begun too small -- and the invariants: stored + handed back = records in, exactly one stored per distinct non-zero tag, every duplicate
paired with the entry of its tag.  The header and the Python binding carry the same reasons and the same 32-byte entry."""
import os
import re
from collections import Counter

import kangaroo_model as K
import kangaroo_dptable_model as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CYCLE = 4


def tags_of(rng, n, avoid=()):
    out, seen = [], set(avoid) | {0}
    while len(out) < n:
        t = rng.u64()
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


def invariants(before, after, records, back):
    """stored + handed back = records in; one entry per distinct live non-zero tag; every duplicate is paired with the entry of its tag"""
    assert DM.entries(after) - DM.entries(before) + len(back) == len(records)
    live = {r[0] for r in records if r[0] and not r[2] & K.DEAD}
    if not any(reason == DM.DPT_FULL for reason, _, _ in back):
        assert set(after["cand"]) == set(before["cand"]) | live
    assert sorted(t for t in after["tags"] if t) == sorted(after["cand"])        # one slot per tag
    for reason, rec, stored in back:
        assert (stored is not None) == (reason == DM.DPT_DUPLICATE)
        if stored is not None:
            assert stored and all(e[0] == rec[0] for e in stored)
            if rec[0] in before["cand"]:
                assert stored == before["cand"][rec[0]]              # what was stored before the launch stays


def test_slots():
    assert DM.n_slots(1, 1) == 128 and DM.n_slots(63, 1) == 128 and DM.n_slots(64, 1) == 256
    assert DM.n_slots(2048, 1024) == 8192 and DM.n_slots(1 << 27, 1 << 22) == 1 << 29
    assert DM.home(0xFFFFFFFFFFFFFFFF, 128) == 127 and DM.home(0x3F, 128) == 0 and DM.home(0x40, 128) == 1


def test_types():
    assert [DM.type_of(f) for f in (0, 1, 3, 2, 1 | 1 << 8 | 5 << 9, 3 | 1 << 8)] == [0, 1, 3, 0, 1, 3]      # the symmetric walk's last-jump bits are not the type


def test_one_tag_many_times():
    rng = K.Stream(1)
    t0 = DM.new_table(64, 64)
    x, y = tags_of(rng, 2)
    recs = [(x, 100 + k, k & 1, k) for k in range(64)] + [(y, 7, 3, 64)]
    t1, back = DM.insert(t0, recs)
    invariants(t0, t1, recs, back)
    assert DM.entries(t1) == 2 and Counter(r for r, _, _ in back) == Counter({DM.DPT_DUPLICATE: 63})
    assert t1["cand"][x] == {(x, 100 + k, k, k & 1) for k in range(64)}          # any of them may be the stored one
    assert t1["cand"][y] == {(y, 7, 64, 3)}
    # a later launch meets what is stored: the pair names the candidates of the first launch, and the new record is none of them
    again = [(x, 5, 1, 9), (y, 6, 0, 10)]
    t2, back = DM.insert(t1, again)
    invariants(t1, t2, again, back)
    assert [(r, rec) for r, rec, _ in back] == [(DM.DPT_DUPLICATE, again[0]), (DM.DPT_DUPLICATE, again[1])]
    assert back[0][2] == t1["cand"][x] and back[1][2] == {(y, 7, 64, 3)} and t2["cand"] == t1["cand"]


def test_tag_zero_and_dead_are_never_stored():
    rng = K.Stream(2)
    a, b, c = tags_of(rng, 3)
    t0 = DM.new_table(64, 64)
    recs = [(c, 9, 1, 0), (a, 1, K.DEAD, 1), (b, 2, K.DEAD | CYCLE | 1, 2), (0, 3, 0, 3), (0, 4, K.DEAD, 4)]
    t1, back = DM.insert(t0, recs)
    invariants(t0, t1, recs, back)
    assert [(r, rec[3]) for r, rec, _ in back] == [(DM.DPT_DEAD, 1), (DM.DPT_DEAD, 2), (DM.DPT_TAG_ZERO, 3), (DM.DPT_DEAD, 4)]
    assert DM.read(t1) == {(c, 9, 0, 1)}
    t2, back = DM.insert(t1, [(a, 5, 0, 1), (b, 6, 3, 2)])          # none of them was stored: their tags are still free
    assert back == [] and DM.read(t2) == {(c, 9, 0, 1), (a, 5, 1, 0), (b, 6, 2, 3)}


def test_a_home_at_the_last_slot_wraps():
    t0 = DM.new_table(64, 64)
    slots = t0["slots"]
    tags = DM.chain_tags(slots - 1, slots, 5)
    recs = [(t, k, 1, k) for k, t in enumerate(tags)]
    t1, back = DM.insert(t0, recs)
    invariants(t0, t1, recs, back)
    assert back == [] and [s for s, t in enumerate(t1["tags"]) if t] == [0, 1, 2, 3, slots - 1]
    t2, back = DM.insert(t1, [(tags[4], 77, 0, 9)])                 # found again behind the wrap
    assert [(r, st) for r, _, st in back] == [(DM.DPT_DUPLICATE, {(tags[4], 4, 4, 1)})]


def test_a_table_begun_too_small_reaches_full():
    rng = K.Stream(3)
    t0 = DM.new_table(0, 0, slots=128)
    tags = tags_of(rng, 160)
    recs = [(t, k, 0, k) for k, t in enumerate(tags)]
    t1, back = DM.insert(t0, recs)
    invariants(t0, t1, recs, back)
    assert DM.entries(t1) == 128 and [(r, rec[3]) for r, rec, _ in back] == [(DM.DPT_FULL, k) for k in range(128, 160)]
    # on the full table a tag that is there is still found, a new one is FULL, and nothing spins
    t2, back = DM.insert(t1, [(tags[3], 1, 1, 0), (tags[150], 2, 1, 1)])
    assert [(r, st) for r, _, st in back] == [(DM.DPT_DUPLICATE, {(tags[3], 3, 3, 0)}), (DM.DPT_FULL, None)]
    assert t2["cand"] == t1["cand"]


def test_load_and_read():
    rng = K.Stream(4)
    t0 = DM.new_table(256, 64)
    tags = tags_of(rng, 200)
    ent = [(t, rng.u128(), k, (0, 1, 3)[k % 3]) for k, t in enumerate(tags)]
    t1, counts = DM.load(t0, ent + [(0, 1, 2, 0), (tags[5], 9, 9, 1), (0, 3, 4, 1)])
    assert counts == (200, 1, 2, 0) and sum(counts) == 203 and DM.entries(t1) == 200
    assert t1["cand"][tags[5]] == {ent[5], (tags[5], 9, 9, 1)}       # two entries of one call with one tag: either may be the stored one
    t1["cand"][tags[5]] = {ent[5]}
    assert DM.read(t1) == set(ent)
    # a record whose tag was loaded comes back paired with the loaded entry
    t2, back = DM.insert(t1, [(tags[7], 1, 0, 3)])
    assert [(r, st) for r, _, st in back] == [(DM.DPT_DUPLICATE, {ent[7]})]
    # loading the same entries again: all duplicates
    t3, counts = DM.load(t2, ent)
    assert counts == (0, 200, 0, 0) and t3["cand"] == t2["cand"]
    small, counts = DM.load(DM.new_table(0, 0, slots=128), ent)
    assert counts == (128, 0, 0, 72)


def test_the_device_check_accepts_any_order_and_nothing_else():
    """check_device, which the GPU tests judge the device with, against a device played by the model itself with the records taken in another order"""
    rng = K.Stream(5)
    x, *rest = tags_of(rng, 9)
    recs = [(x, 10 + k, 1, k) for k in range(4)] + [(t, 1, 0, 4 + k) for k, t in enumerate(rest)] + [(0, 2, 0, 20), (rest[0], 3, K.DEAD, 21)]

    def play(order):
        table, out = DM.new_table(64, 64), []
        table, back = DM.insert(table, [recs[k] for k in order])
        for reason, rec, stored in back:
            if stored is not None:
                st = next(iter(table["cand"][rec[0]] - {(r[0], r[1], r[3], DM.type_of(r[2])) for r2, r, _ in back if r2 == DM.DPT_DUPLICATE}))
                out.append({"x": st[0], "d": st[1], "kangaroo": st[2], "flags": st[3], "step": 0, "reason": DM.DPT_STORED})
            out.append({"x": rec[0], "d": rec[1], "kangaroo": rec[3], "flags": rec[2], "step": 0, "reason": reason})
        return out, DM.entries(table)

    for order in (list(range(len(recs))), list(reversed(range(len(recs))))):
        got, n = play(order)
        new, pairs = DM.check_device(DM.new_table(64, 64), recs, got, n)
        assert len(new["cand"][x]) == 1 and len(pairs) == 5
    got, n = play(list(range(len(recs))))
    stored = [g for g in got if g["reason"] == DM.DPT_STORED]
    stored[0]["d"] ^= 1                                               # a pair that names something the table cannot hold
    try:
        DM.check_device(DM.new_table(64, 64), recs, got, n)
    except AssertionError:
        pass
    else:
        raise AssertionError("a wrong stored entry passed")


def test_header_and_binding_state_the_same_rule():
    import pybsgs
    with open(os.path.join(ROOT, "include", "bsgs_hip.h")) as f:
        text = f.read()
    assert "Kangaroo, distinguished-point table in device memory" in text
    for k, name in enumerate(["DEAD", "DUPLICATE", "TAG_ZERO", "FULL", "STORED"]):
        assert "#define BSGS_KANGAROO_DPT_%s %du" % (name, k) in text
        assert getattr(pybsgs, "KANGAROO_DPT_" + name) == k == getattr(DM, "DPT_" + name)
    assert re.search(r"typedef struct \{ uint64_t x_lo64; uint8_t d\[16\]; uint32_t kangaroo, type; \} bsgs_kangaroo_dp_entry;", text)
    assert (pybsgs.KANGAROO_WILD, pybsgs.KANGAROO_NEG) == (DM.WILD, DM.NEG)
