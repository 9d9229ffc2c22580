"""CPU: the model of fe_sqr_add2's fold (tests/fe_fold_model.py) is right on every case of the generator the GPU test runs, stays below 2^256, and the
generator's cases take every branch of the ADD2 carry accounting -- so that the GPU test (tests/test_gpu_field_contract.py) meets them too."""
import random

import fe_fold_model as M

P = M.P


def test_model_is_exact_and_every_event_is_covered():
    """the model equals (a*a + c1 + c2) % P on every generated case (after the one conditional subtraction fe_canon makes), every result is below 2^256, and
    every event of fe_fold_model.EVENTS is taken by at least one case: top = 0, 1, 2, 3; the 33-bit word 8; h = 0 and 1; fold 3; the ripple into word 2
    inside fold 3.  None was dropped: all of them are reachable (the ripple only through addends aimed at it, fe_fold_model.aimed_addends)."""
    cases, counts = M.cases()
    assert len(cases) > 3000
    for a, c1, c2 in cases:
        r, _ = M.sqr_add2(a, c1, c2)
        assert r < 1 << 256, (hex(a), hex(c1), hex(c2))
        assert (r - P if r >= P else r) == (a * a + c1 + c2) % P, (hex(a), hex(c1), hex(c2))
    print("fe_sqr_add2 fold events over %d cases: %s" % (len(cases), counts))
    assert sorted(counts) == sorted(M.EVENTS)
    missing = [e for e in M.EVENTS if not counts[e]]
    assert not missing, missing


def test_h_is_one_through_both_of_its_terms():
    """h = co + FE_W15_HI: cases where only the join's carry sets it, and cases where only the 33rd bit of word 8 does"""
    cases, _ = M.cases()
    by_carry = by_w15 = 0
    for a, c1, c2 in cases:
        ev = M.sqr_add2(a, c1, c2)[1]
        if "h1" in ev:
            if "w15_33bit" in ev:
                by_w15 += 1
            else:
                by_carry += 1
    assert by_carry and by_w15, (by_carry, by_w15)


def test_aimed_addends_reach_the_ripple():
    a = (1 << 256) - 1
    c = M.aimed_addends(a, (1 << 64) - 5)
    assert c is not None
    r, ev = M.sqr_add2(a, *c)
    assert {"fold3", "fold3_ripple"} <= ev and r == (1 << 64) - 5 + M.KP and r == (a * a + sum(c)) % P


def test_fold_alone_on_random_512_bit_words():
    """reduce512_add2 on any 16 words, not only squares: congruent and below 2^256"""
    rnd = random.Random(5)
    for _ in range(2000):
        w, c1, c2 = rnd.randrange(1 << 512), rnd.randrange(1 << 256), rnd.randrange(1 << 256)
        r, _ = M.reduce512_add2(M.limbs(w, 16), M.limbs(c1), M.limbs(c2))
        r = M.value(r)
        assert r < 1 << 256 and r % P == (w + c1 + c2) % P
