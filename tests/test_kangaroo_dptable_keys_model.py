"""CPU: the model of the distinguished-point table for a key list (tests/kangaroo_dptable_keys_model.py) -- the owner word, the `reserved` word of a
hand-back, and the pair rule: of equal tags one is stored and every other one comes back paired with it."""
from collections import Counter

import pytest

import kangaroo_model as K
import kangaroo_dptable_model as DM
import kangaroo_dptable_keys_model as KM


def test_the_model_stands_on_the_unkeyed_one():
    assert KM.DM is DM and KM.DPT_STORED == DM.DPT_STORED == 4 and KM.DPT_KEY_SHIFT == 8


@pytest.mark.parametrize("sym", [False, True])
def test_owner_words(sym):
    rec = lambda key, fl: (fl | (0 if sym else key << KM.KEY_SHIFT), key if sym else 0)
    assert KM.owner_of(*rec(0, 0), sym) == 0                                                  # tame
    assert KM.owner_of(*rec(0, KM.WILD), sym) == 1                                            # wild, key 0
    assert KM.owner_of(*rec(65534, KM.WILD), sym) == 65535                                    # the last key a list can hold
    assert KM.owner_of(*rec(7, KM.WILD | KM.NEG), sym) == (8 | 1 << 31 if sym else 8)         # NEG counts in the symmetric list's herd only
    assert KM.owner_of(*rec(65534, KM.WILD | KM.NEG), True if sym else False) == (65535 | (1 << 31 if sym else 0))
    assert KM.owner_parts(0) == (False, None, False) and KM.owner_parts(1) == (True, 0, False) and KM.owner_parts(65535 | 1 << 31) == (True, 65534, True)


def test_the_symmetric_herd_ignores_the_jump_index_in_the_flags_and_the_plain_herd_ignores_reserved():
    assert KM.owner_of(KM.WILD | 0x1FFF << 8, 3, True) == 4              # flag bits 8..20 hold the last jump index there
    assert KM.owner_of(KM.WILD | 3 << 8, 0xABCD, False) == 4
    assert KM.owner_of(0x1FFF << 8, 9, True) == 0 and KM.owner_of(9 << 8, 9, False) == 0      # a tame record has no owner whatever the words hold


def test_reserved_round_trips():
    for reason in (KM.DPT_DEAD, KM.DPT_DUPLICATE, KM.DPT_TAG_ZERO, KM.DPT_FULL):
        for key in (0, 1, 255, 256, 65534, 65535):
            word = KM.encode_reserved(reason, key)
            assert word != KM.DPT_STORED and word < 1 << 24 and KM.decode_reserved(word) == (reason, key)
    assert KM.decode_reserved(KM.DPT_STORED) == (KM.DPT_STORED, None)
    with pytest.raises(AssertionError):
        KM.encode_reserved(KM.DPT_STORED, 0)                             # the stored half is not a reason


@pytest.mark.parametrize("sym", [False, True])
def test_of_equal_tags_one_is_stored_and_the_others_pair_with_it(sym):
    mk = lambda tag, d, key, kang, fl=KM.WILD: (tag, d, fl | (0 if sym else key << KM.KEY_SHIFT), kang, key if sym else 0)
    table = DM.new_table(64, 64)
    recs = [mk(5, 1, 0, 10), mk(5, 2, 1, 11), mk(5, 3, 65534, 12), mk(9, 4, 2, 13, 0), mk(0, 5, 3, 14), mk(7, 6, 4, 15, KM.WILD | K.DEAD)]
    table, back = KM.insert(table, recs, sym)
    assert DM.entries(table) == 2 and len(table["cand"][5]) == 3 and table["cand"][9] == {(9, 4, 13, 0)}
    assert Counter((r, rec[3], word) for r, rec, _, word in back) == Counter({
        (KM.DPT_DUPLICATE, 11, 1 | 1 << 8): 1, (KM.DPT_DUPLICATE, 12, 1 | 65534 << 8): 1, (KM.DPT_TAG_ZERO, 14, 2 | 3 << 8): 1, (KM.DPT_DEAD, 15, 0 | 4 << 8): 1})
    assert all(st == table["cand"][5] for r, _, st, _ in back if r == KM.DPT_DUPLICATE)
    # whichever copy the device stored, its answer passes: the stored entry plus the copies handed back are the copies sent
    for stored in range(3):
        got = []
        for k in range(3):
            if k == stored:
                continue
            t, d, fl, kang, res = recs[stored]
            got.append({"x": t, "d": d, "kangaroo": kang, "flags": KM.owner_of(fl, res, sym), "step": 0, "reason": KM.DPT_STORED, "key": None})
            t, d, fl, kang, res = recs[k]
            got.append({"x": t, "d": d, "kangaroo": kang, "flags": fl, "step": 0, "reason": KM.DPT_DUPLICATE, "key": KM.key_of(fl, res, sym)})
        for t, d, fl, kang, res in recs[4:]:
            got.append({"x": t, "d": d, "kangaroo": kang, "flags": fl, "step": 0, "reason": KM.DPT_DEAD if fl & K.DEAD else KM.DPT_TAG_ZERO, "key": KM.key_of(fl, res, sym)})
        new, pairs = KM.check_device(DM.new_table(64, 64), recs, got, 2, sym)
        assert new["cand"][5] == {KM.entry_of(recs[stored], sym)}
        bad = [dict(g) for g in got]
        bad[0]["flags"] ^= 2                                             # a stored half with another owner than the stored copy's
        with pytest.raises(AssertionError):
            KM.check_device(DM.new_table(64, 64), recs, bad, 2, sym)
        bad = [dict(g) for g in got]
        bad[1]["key"] ^= 1                                               # a record that lost its key
        with pytest.raises(AssertionError):
            KM.check_device(DM.new_table(64, 64), recs, bad, 2, sym)
    # a second launch meets the stored entry alone
    table["cand"][5] = {KM.entry_of(recs[0], sym)}
    table, back = KM.insert(table, [mk(5, 8, 9, 20)], sym)
    assert [(r, st, word) for r, _, st, word in back] == [(KM.DPT_DUPLICATE, {KM.entry_of(recs[0], sym)}, 1 | 9 << 8)]
