"""GPU: the growing tame table (csrc/kangaroo_tames_gen.hip) and the distinguished-point table (csrc/kangaroo_dptable.hip) place and refuse by one rule
(csrc/kangaroo_table.hip.h): the same records through both inserts on one herd -- two probe chains that collide behind the table's end, one tag three
times, tag 0, a DEAD record, fillers -- come back with the same reasons, and both tables then hold the same tags with the same offsets."""
from collections import Counter

import pytest

import kangaroo_model as K
import kangaroo_dptable_model as DM
import kangaroo_tames_gen_model as GM

pytestmark = pytest.mark.gpu

HERD = CAP = CAPACITY = 64
SLOTS = 256


def test_both_tables_place_and_refuse_alike():
    import pybsgs
    assert DM.n_slots(CAPACITY, CAP) == GM.n_slots(CAPACITY, CAP) == SLOTS
    assert (GM.GEN_DEAD, GM.GEN_DUPLICATE, GM.GEN_TAG_ZERO, GM.GEN_FULL) == (DM.DPT_DEAD, DM.DPT_DUPLICATE, DM.DPT_TAG_ZERO, DM.DPT_FULL) == (0, 1, 2, 3)
    rng = K.Stream(31)
    last = DM.chain_tags(SLOTS - 1, SLOTS, 5)                         # home at the last slot: the chain runs on from slot 0 ...
    first = DM.chain_tags(0, SLOTS, 5, salt=3)                        # ... into the tags whose home is slot 0
    thrice, dead = DM.chain_tags(77, SLOTS, 1, salt=5)[0], DM.chain_tags(99, SLOTS, 1, salt=9)[0]
    fillers = []
    while len(fillers) < 28:
        t = rng.u64()
        if t and t not in last + first + [thrice, dead] + fillers:
            fillers.append(t)
    tags = ([last[0], first[0], thrice, last[1], first[1]] + fillers[:10] + [thrice, last[2], 0, first[2], last[3]] + fillers[10:20]
            + [dead, first[3], thrice, last[4], first[4]] + fillers[20:])
    recs = [(t, 1000 + k, K.DEAD if t == dead else 0, k) for k, t in enumerate(tags)]
    assert 40 < len(recs) <= CAP
    once = {t: d for t, d, _, _ in recs if t not in (thrice, dead, 0)}
    scalars, jumps = K.jump_table(K.Stream(11), 1 << 30)
    d = pybsgs.Device(0)
    try:
        d.kangaroo_setup(jumps, scalars, 0, HERD, 1, CAP)
        d.kangaroo_tames_gen_begin(CAPACITY)
        d.kangaroo_dptable_begin(CAPACITY)
        gen_back, gen_entries = d.kangaroo_tames_gen_insert(recs)
        dpt_back, dpt_entries, dropped = d.kangaroo_dptable_insert(recs)
        assert dropped == 0
        gen_reasons = Counter((r["reason"], r["x"]) for r in gen_back)
        dpt_reasons = Counter((r["reason"], r["x"]) for r in dpt_back if r["reason"] != DM.DPT_STORED)
        print(sorted(gen_reasons.items()), sorted(dpt_reasons.items()), gen_entries, dpt_entries)
        assert gen_reasons == dpt_reasons == Counter({(GM.GEN_DUPLICATE, thrice): 2, (GM.GEN_TAG_ZERO, 0): 1, (GM.GEN_DEAD, dead): 1})
        gen_held, dpt_held = d.kangaroo_tames_gen_read(), d.kangaroo_dptable_read()
        assert {t for t, _ in gen_held} == {e[0] for e in dpt_held} == set(once) | {thrice}
        assert {t: v for t, v in gen_held if t in once} == {e[0]: e[1] for e in dpt_held if e[0] in once} == once
        assert gen_entries == dpt_entries == len(gen_held) == len(dpt_held) == len(once) + 1
    finally:
        d.close()
