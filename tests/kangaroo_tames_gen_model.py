"""Pure-Python restatement of the tame table grown on the device (include/bsgs_hip.h, "Kangaroo, tame table grown on the device"): the number of slots, the
insert of a launch's records with its hand-backs, and the host's rule for what comes back (host/host_kangaroo_tames.cpp GenRule).  A test model: no product
code runs here."""
from collections import Counter

import kangaroo_model as K

MIN_SLOTS = 128
M64 = (1 << 64) - 1
GEN_DEAD, GEN_DUPLICATE, GEN_TAG_ZERO, GEN_FULL = range(4)


def n_slots(capacity, record_cap):
    """the power of two at or above 2 * (capacity + record_cap), at least 128"""
    slots = MIN_SLOTS
    while slots < 2 * (capacity + record_cap):
        slots *= 2
    return slots


def home(tag, slots):
    return (tag >> 6) & (slots - 1)


def new_table(capacity, record_cap):
    """tags: one per slot, 0 = empty; cand: tag -> the offsets one of which is stored with it"""
    return {"slots": n_slots(capacity, record_cap), "tags": [0] * n_slots(capacity, record_cap), "cand": {}}


def insert(table, records):
    """one launch: records = [(tag, d, flags)] -> (the new table, the hand-backs as a Counter of (tag, reason)).  The records of a launch are inserted in no
    particular order: of equal tags that are new to the table exactly ONE is stored and the others come back as duplicates, so the stored d is "one of the
    candidates" (cand[tag] holds them all).  Which slot a tag ends up in depends on that order, but which slots are occupied does not (linear probing), and
    neither does anything the device reports as long as no record of the launch is FULL."""
    slots = table["slots"]
    tags, cand = list(table["tags"]), {t: set(c) for t, c in table["cand"].items()}
    back, fresh = Counter(), set()
    for tag, d, fl in records:
        assert 0 <= tag <= M64
        if fl & K.DEAD:                                               # a CYCLE record has DEAD too
            back[(tag, GEN_DEAD)] += 1
            continue
        if tag == 0:                                                   # the one tag the table cannot hold: 0 marks an empty slot
            back[(0, GEN_TAG_ZERO)] += 1
            continue
        if len(cand) == slots:                                         # (a full table, the short way: a tag that is there is found, any other sees every slot)
            back[(tag, GEN_DUPLICATE if tag in cand else GEN_FULL)] += 1
            continue
        s = home(tag, slots)
        for _ in range(slots):
            if tags[s] == 0:
                tags[s] = tag
                cand[tag] = {d & K.M128}
                fresh.add(tag)
                break
            if tags[s] == tag:
                back[(tag, GEN_DUPLICATE)] += 1
                if tag in fresh:
                    cand[tag].add(d & K.M128)
                break
            s = (s + 1) & (slots - 1)
        else:
            back[(tag, GEN_FULL)] += 1
    return {"slots": slots, "tags": tags, "cand": cand}, back


def entries(table):
    return len(table["cand"])


def chain_tags(home_slot, slots, n, salt=1):
    """n different non-zero tags with the one home slot `home_slot` of a table of `slots` slots"""
    bits = slots.bit_length() - 1
    out = [(j & 63) | (home_slot << 6) | ((1 + ((salt * 0x9E3779B1 + j * 0x85EBCA6B) % ((1 << (58 - bits)) - 1))) << (6 + bits)) for j in range(n)]
    assert len(set(out)) == n and 0 not in out and {home(t, slots) for t in out} == {home_slot}
    return out


class GenRule:
    """what a handed-back record means to the generator; every method returns the lines -selftest kangaroo-tames-gen prints for the same item"""

    def __init__(self, T):
        self.T, self.dev, self.held = T, 0, {}
        self.reseeds = self.merges = self.dropped = 0
        self.said = False

    def done(self):
        return self.dev + len(self.held) >= self.T

    def _done_line(self, out):
        if self.done() and not self.said:
            self.said = True
            out.append("done")
        return out

    def entries(self, n):
        self.dev = n
        return self._done_line(["entries %d" % (self.dev + len(self.held))])

    def record(self, reason, x, d, kangaroo):
        if self.done():
            return ["ignored"]
        if reason == GEN_DEAD:
            self.reseeds += 1
            out = ["reseed %d" % kangaroo]
        elif reason == GEN_DUPLICATE or (reason == GEN_TAG_ZERO and (x & M64) in self.held):
            self.merges += 1
            self.reseeds += 1
            out = ["merge %d" % kangaroo]
        elif reason == GEN_TAG_ZERO:
            self.held[x & M64] = d
            out = ["held %d" % kangaroo]
        else:
            self.dropped += 1
            out = ["dropped"]
        return self._done_line(out)

    def summary(self):
        return "summary %d %d %d %d %d" % (self.reseeds, self.merges, len(self.held), self.dropped, 1 if self.done() else 0)
