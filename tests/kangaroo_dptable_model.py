"""Pure-Python restatement of the distinguished-point table in device memory (include/bsgs_hip.h, "Kangaroo, distinguished-point table in device memory"):
the number of slots, insert with resolve, load and read.  A test model: no product code runs here.

A record is (tag, d, flags, kangaroo); an entry is (tag, d mod 2^128, kangaroo, type).  The records of a launch are inserted in no particular order, so of
equal tags that are new to the table the stored one is "one of the candidates": cand[tag] holds every entry that may stand in the slot."""
import kangaroo_model as K

MIN_SLOTS = 128
M64 = (1 << 64) - 1
DPT_DEAD, DPT_DUPLICATE, DPT_TAG_ZERO, DPT_FULL, DPT_STORED = range(5)
WILD, NEG = 1, 2


def n_slots(capacity, record_cap):
    """the power of two at or above 2 * (capacity + record_cap), at least 128"""
    slots = MIN_SLOTS
    while slots < 2 * (capacity + record_cap):
        slots *= 2
    return slots


def home(tag, slots):
    return (tag >> 6) & (slots - 1)


def type_of(flags):
    """0 tame, 1 wild, 3 wild with NEG"""
    return flags & (WILD | NEG) if flags & WILD else 0


def new_table(capacity, record_cap, slots=None):
    """tags: one per slot, 0 = empty; cand: tag -> the entries one of which is stored with it.  slots: a table begun with another size than the rule's (the
    model's way to a full table)"""
    slots = n_slots(capacity, record_cap) if slots is None else slots
    return {"slots": slots, "tags": [0] * slots, "cand": {}}


def _place(tags, slots, tag):
    """-> (slot, True) the tag was put into an empty slot; (slot, False) it stands there already; (None, False) no slot after `slots` probes"""
    s = home(tag, slots)
    for _ in range(slots):
        if tags[s] == 0:
            tags[s] = tag
            return s, True
        if tags[s] == tag:
            return s, False
        s = (s + 1) & (slots - 1)
    return None, False


def insert(table, records):
    """one launch -> (the new table, the hand-backs).  A hand-back is (reason, record, stored): stored is None unless the reason is DPT_DUPLICATE, and then
    the set of entries one of which the device pairs with the record (one entry unless the tag came into the table in this very launch)."""
    slots = table["slots"]
    tags, cand = list(table["tags"]), {t: set(c) for t, c in table["cand"].items()}
    back, fresh = [], {}
    for rec in records:
        tag, d, fl, kang = rec
        assert 0 <= tag <= M64
        if fl & K.DEAD:                                               # a CYCLE record has DEAD too
            back.append((DPT_DEAD, rec, None))
            continue
        if tag == 0:                                                   # the one tag the table cannot hold: 0 marks an empty slot
            back.append((DPT_TAG_ZERO, rec, None))
            continue
        entry = (tag, d & K.M128, kang, type_of(fl))
        s, new = _place(tags, slots, tag)
        if s is None:
            back.append((DPT_FULL, rec, None))
        elif new:
            cand[tag] = {entry}
            fresh[tag] = [entry]
        else:
            if tag in fresh:                                           # one of this launch's records with the tag is stored, which one is unspecified
                cand[tag].add(entry)
                fresh[tag].append(entry)
            back.append((DPT_DUPLICATE, rec, cand[tag]))
    return {"slots": slots, "tags": tags, "cand": cand}, back


def load(table, entries):
    """entries (tag, d, kangaroo, type) by the insert's rule -> (the new table, (stored, duplicate, zero, full))"""
    slots = table["slots"]
    tags, cand = list(table["tags"]), {t: set(c) for t, c in table["cand"].items()}
    stored = dup = zero = full = 0
    fresh = set()
    for tag, d, kang, typ in entries:
        if tag == 0:
            zero += 1
            continue
        s, new = _place(tags, slots, tag)
        if s is None:
            full += 1
        elif new:
            cand[tag] = {(tag, d & K.M128, kang, typ)}
            fresh.add(tag)
            stored += 1
        else:
            if tag in fresh:
                cand[tag].add((tag, d & K.M128, kang, typ))
            dup += 1
    return {"slots": slots, "tags": tags, "cand": cand}, (stored, dup, zero, full)


def entries(table):
    return len(table["cand"])


def read(table):
    """the table as a set of entries -- exact when no tag has more than one candidate"""
    assert all(len(c) == 1 for c in table["cand"].values())
    return {next(iter(c)) for c in table["cand"].values()}


def check_device(table, records, got, n_entries):
    """what a device returned for the launch `records` on `table`, against the rule, whichever order it took the records in -> (the model's new table, the
    device's hand-backs as [(reason, record, stored entry or None)]).  got: the handed-back records as pybsgs gives them ({x, d, kangaroo, flags, reason}).
      every record is stored or handed back; DEAD / TAG_ZERO / FULL as the model has them; a DUPLICATE directly follows a STORED record that holds an entry of
      its tag, one of the model's candidates; of the records of one fresh tag exactly one is missing from the hand-backs, and it is the entry every pair names."""
    from collections import Counter
    new, want = insert(table, records)
    assert n_entries == entries(new)
    pairs, k = [], 0
    while k < len(got):
        r = got[k]
        if r["reason"] == DPT_STORED:
            assert k + 1 < len(got) and got[k + 1]["reason"] == DPT_DUPLICATE, "a stored entry stands in front of its duplicate"
            assert r["x"] <= M64 and r["step"] == 0
            w = got[k + 1]
            pairs.append((DPT_DUPLICATE, (w["x"], w["d"], w["flags"], w["kangaroo"]), (r["x"], r["d"], r["kangaroo"], r["flags"])))
            k += 2
        else:
            assert r["reason"] in (DPT_DEAD, DPT_TAG_ZERO, DPT_FULL), r
            pairs.append((r["reason"], (r["x"], r["d"], r["flags"], r["kangaroo"]), None))
            k += 1
    norm = lambda rec: (rec[0], rec[1] & K.M128, rec[2], rec[3])
    assert Counter((reason, norm(rec)[0] & M64) for reason, rec, _ in pairs) == Counter((reason, rec[0]) for reason, rec, _ in want)
    sent = Counter(norm(r) for r in records)
    assert not Counter(rec for _, rec, _ in pairs) - sent             # the records as they were sent
    chosen = {}
    for reason, rec, st in pairs:
        if reason != DPT_DUPLICATE:
            continue
        tag = rec[0] & M64
        assert st[0] == tag and st in new["cand"][tag], (rec, st)
        assert chosen.setdefault(tag, st) == st                       # every pair of a tag names the one stored entry
    # a fresh tag: the records that came back and the stored one are together the records sent
    for tag, st in chosen.items():
        if tag in table["cand"]:
            continue
        mine = Counter((r[0], r[1] & K.M128, r[3], type_of(r[2])) for r in records if r[0] == tag and not r[2] & K.DEAD)
        came = Counter((rec[0], rec[1], rec[3], type_of(rec[2])) for reason, rec, _ in pairs if reason == DPT_DUPLICATE and rec[0] == tag)
        assert came + Counter([st]) == mine
        new["cand"][tag] = {st}                                       # now known
    return new, pairs


def chain_tags(home_slot, slots, n, salt=1):
    """n different non-zero tags with the one home slot `home_slot` of a table of `slots` slots"""
    bits = slots.bit_length() - 1
    out = [(j & 63) | (home_slot << 6) | ((1 + ((salt * 0x9E3779B1 + j * 0x85EBCA6B) % ((1 << (58 - bits)) - 1))) << (6 + bits)) for j in range(n)]
    assert len(set(out)) == n and 0 not in out and {home(t, slots) for t in out} == {home_slot}
    return out
