"""Pure-Python restatement of the distinguished-point table for a key list (include/bsgs_hip.h, "Kangaroo, distinguished-point table for a key list"), on
the model of the table it extends (kangaroo_dptable_model.py): the owner word, what a hand-back's `reserved` holds, and the pair rule.  A test model: no
product code runs here.

A record is (tag, d, flags, kangaroo, reserved); an entry is (tag, d mod 2^128, kangaroo, owner).  sym: the herd of bsgs_kangaroo_setup_sym_keys, whose
records name their key in `reserved` and may carry NEG; else the herd of bsgs_kangaroo_setup with a key list, whose records name it in flag bits 8..23."""
from collections import Counter

import kangaroo_model as K
import kangaroo_dptable_model as DM

KEY_SHIFT = 8                 # BSGS_KANGAROO_KEY_SHIFT: the key in the flags of the plain walk's herd
DPT_KEY_SHIFT = 8             # BSGS_KANGAROO_DPT_KEY_SHIFT: the key in a hand-back's `reserved`
NEG_OWNER = 1 << 31
M64, WILD, NEG = DM.M64, DM.WILD, DM.NEG
DPT_DEAD, DPT_DUPLICATE, DPT_TAG_ZERO, DPT_FULL, DPT_STORED = DM.DPT_DEAD, DM.DPT_DUPLICATE, DM.DPT_TAG_ZERO, DM.DPT_FULL, DM.DPT_STORED


def key_of(flags, reserved, sym):
    return (reserved if sym else flags >> KEY_SHIFT) & 0xFFFF


def owner_of(flags, reserved, sym):
    """the work file's owner word: 0 tame, 1 + key wild, bit 31 for NEG in the symmetric list's herd"""
    if not flags & WILD:
        return 0
    return (1 + key_of(flags, reserved, sym)) | (NEG_OWNER if sym and flags & NEG else 0)


def owner_parts(owner):
    """-> (wild, key or None, neg)"""
    return (False, None, False) if owner == 0 else (True, (owner & ~NEG_OWNER) - 1, bool(owner & NEG_OWNER))


def encode_reserved(reason, key):
    assert 0 <= reason < DPT_STORED and 0 <= key <= 0xFFFF
    return reason | key << DPT_KEY_SHIFT


def decode_reserved(word):
    """-> (reason, key); the stored half of a pair is DPT_STORED exactly and has no key"""
    return (DPT_STORED, None) if word == DPT_STORED else (word & ((1 << DPT_KEY_SHIFT) - 1), word >> DPT_KEY_SHIFT)


def entry_of(rec, sym):
    tag, d, fl, kang, res = rec
    return (tag, d & K.M128, kang, owner_of(fl, res, sym))


def insert(table, records, sym):
    """one launch -> (the new table, the hand-backs) as kangaroo_dptable_model.insert, a hand-back (reason, record, stored, reserved word): the entries hold
    the owner word, and `reserved` of what comes back is reason | key << 8"""
    slots = table["slots"]
    tags, cand = list(table["tags"]), {t: set(c) for t, c in table["cand"].items()}
    back, fresh = [], set()
    for rec in records:
        tag, d, fl, kang, res = rec
        word = lambda reason: encode_reserved(reason, key_of(fl, res, sym))
        if fl & K.DEAD:
            back.append((DPT_DEAD, rec, None, word(DPT_DEAD)))
            continue
        if tag == 0:
            back.append((DPT_TAG_ZERO, rec, None, word(DPT_TAG_ZERO)))
            continue
        s, new = DM._place(tags, slots, tag)
        if s is None:
            back.append((DPT_FULL, rec, None, word(DPT_FULL)))
        elif new:
            cand[tag] = {entry_of(rec, sym)}
            fresh.add(tag)
        else:
            if tag in fresh:                                           # one of this launch's records with the tag is stored, which one is unspecified
                cand[tag].add(entry_of(rec, sym))
            back.append((DPT_DUPLICATE, rec, cand[tag], word(DPT_DUPLICATE)))
    return {"slots": slots, "tags": tags, "cand": cand}, back


def pairs_of(got):
    """the device's hand-backs ({x, d, kangaroo, flags, step, reason, key}) -> [(reason, the record as (tag or x, d, flags, kangaroo, key), stored entry or
    None)]: a stored half stands directly in front of its duplicate"""
    out, k = [], 0
    while k < len(got):
        r = got[k]
        if r["reason"] == DPT_STORED:
            assert k + 1 < len(got) and got[k + 1]["reason"] == DPT_DUPLICATE, "a stored entry stands in front of its duplicate"
            assert r["x"] <= M64 and r["step"] == 0 and r["key"] is None
            w = got[k + 1]
            assert w["x"] & M64 == r["x"]
            out.append((DPT_DUPLICATE, (w["x"], w["d"], w["flags"], w["kangaroo"], w["key"]), (r["x"], r["d"], r["kangaroo"], r["flags"])))
            k += 2
        else:
            assert r["reason"] in (DPT_DEAD, DPT_TAG_ZERO, DPT_FULL), r
            out.append((r["reason"], (r["x"], r["d"], r["flags"], r["kangaroo"], r["key"]), None))
            k += 1
    return out


def check_device(table, records, got, n_entries, sym):
    """what a device returned for the launch `records` on `table` against the rule, whichever order it took the records in -> (the model's new table, the
    pairs).  Every record is stored or handed back; a handed-back record is one of those sent, with its own key and reason; every pair of a tag names one
    stored entry, a candidate of the model's with its owner word exact; for a tag new to the table the stored entry plus the copies handed back are the copies
    sent."""
    new, want = insert(table, records, sym)
    assert n_entries == DM.entries(new)
    pairs = pairs_of(got)
    sent = lambda rec: (rec[0], rec[1] & K.M128, rec[2], rec[3], key_of(rec[2], rec[4], sym))
    assert Counter((reason, rec[0] & M64) for reason, rec, _ in pairs) == Counter((reason, rec[0]) for reason, rec, _, _ in want)
    assert not Counter(rec for _, rec, _ in pairs) - Counter(sent(r) for r in records)      # the records as they were sent, the key they named
    chosen = {}
    for reason, rec, st in pairs:
        if reason != DPT_DUPLICATE:
            continue
        tag = rec[0] & M64
        assert st[0] == tag and st in new["cand"][tag], (rec, st)
        assert chosen.setdefault(tag, st) == st                       # every pair of a tag names the one stored entry
    for tag, st in chosen.items():
        if tag in table["cand"]:
            continue
        mine = Counter(entry_of(r, sym) for r in records if r[0] == tag and not r[2] & K.DEAD)
        came = Counter(entry_of((rec[0], rec[1], rec[2], rec[3], rec[4] if sym else 0), sym) for reason, rec, _ in pairs if reason == DPT_DUPLICATE and rec[0] == tag)
        assert came + Counter([st]) == mine                           # stored entry plus handed-back copies = copies sent
        new["cand"][tag] = {st}
    return new, pairs
