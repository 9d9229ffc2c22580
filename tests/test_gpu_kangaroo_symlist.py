"""GPU: the symmetric herd that carries a key per kangaroo (bsgs_kangaroo_setup_sym_keys; csrc/kangaroo.hip kangaroo_sym_keys_kernel) against
tests/kangaroo_symlist_model.py, bit for bit: seeded states and their keys, one launch with a live cycle check, every record with its key word, re-seeding
onto another key, a start at infinity, verification against the key list, and the herds that must stay as they were."""
import pytest

import kangaroo_model as K
import kangaroo_sym_model as S
import kangaroo_symlist_model as SL
from pybsgs.ecpy import add, mul, neg

pytestmark = pytest.mark.gpu

A, W = 0x5A5A5A << 40, 1 << 40
KEYS = [A + 0x1234567890, A + 0xFEDCBA9876, A + 7]                  # three keys of [A, A + W)
R, DP, STEPS = 64, 2, 40
SHAPES = [(512, 2), (128, 2)]                                       # 256 threads x 2: blocks of four waves, one inversion per block; 64 x 2: one-wave blocks


@pytest.fixture(scope="module")
def dev():
    import pybsgs
    d = pybsgs.Device(0)
    yield d
    d.close()


def rec_key(r):
    return (r["x"], r["d"], r["kangaroo"], r["flags"], r["step"], r["key"])


def case(n):
    """Q_k, the jump table, offsets / types / keys of a herd: the first half tame, the wild half dealt out cyclically"""
    nmid = neg(mul(A + W // 2))
    Qs = [add(mul(k), nmid) for k in KEYS]
    scalars, jumps = S.jump_table(K.Stream(900 + n), n * (W ** 0.5) / 4, R)
    rng = K.Stream(4000 + n)
    wild = [i >= n // 2 for i in range(n)]
    keys = [(i - n // 2) % len(KEYS) if w else 0 for i, w in enumerate(wild)]
    offs = [S.herd_offset(rng, W, w) for w in wild]
    return Qs, scalars, jumps, wild, keys, offs


def model_state(Qs, d, wild, key):
    p = K.start(Qs[key], d, wild)
    return (0, 0, d & K.M128, (K.WILD if wild else 0) | K.DEAD, key) if p is None else (p[0], p[1], d & K.M128, K.WILD if wild else 0, key)


def seeded(dev, n, per_thread, cap=1 << 14):
    Qs, scalars, jumps, wild, keys, offs = case(n)
    dev.kangaroo_setup_sym_keys(jumps, scalars, DP, n, per_thread, cap)
    dev.kangaroo_set_keys(Qs)
    assert dev.kangaroo_seed_keys(offs, [K.WILD if w else 0 for w in wild], keys) == (0, 0)
    return Qs, scalars, jumps, wild, keys, [model_state(Qs, d, w, k) for d, w, k in zip(offs, wild, keys)]


@pytest.mark.parametrize("n, per_thread", SHAPES)
def test_walk_and_records_against_the_model(dev, n, per_thread):
    Qs, scalars, jumps, wild, keys, states = seeded(dev, n, per_thread)
    assert dev.kangaroo_geometry() == (n // per_thread, per_thread, 256 if n == 512 else 64)
    assert sum(s[1] & 1 for s in states) > n // 4 and sum(1 - (s[1] & 1) for s in states) > n // 4          # starts of both y parities
    assert dev.kangaroo_download(0, n) == states                     # flags WILD without key bits, the key beside them
    want, recs = SL.walk(states, jumps, scalars, STEPS, DP)          # 40 steps > the window: the cycle check is live
    got, dropped, _ = dev.kangaroo_run(STEPS)
    assert dropped == 0 and len(got) > n * STEPS // 8
    assert sorted(rec_key(r) for r in got) == sorted(recs)
    down = dev.kangaroo_download(0, n)
    assert down == want
    assert [s[4] for s in down] == keys and all(s[3] & S.LAST_VALID for s in down) and any(s[3] & S.NEG for s in down[n // 2:])
    assert {r["key"] for r in got if r["flags"] & K.WILD} == {0, 1, 2} and all(r["key"] == 0 for r in got if not r["flags"] & K.WILD)
    # through upload into the same herd and on: the key goes back as it came
    dev.kangaroo_upload(0, down)
    assert dev.kangaroo_download(0, n) == down
    want2, recs2 = SL.walk(down, jumps, scalars, 5, DP)
    got2, _, _ = dev.kangaroo_run(5)
    assert sorted(rec_key(r) for r in got2) == sorted(recs2) and dev.kangaroo_download(0, n) == want2


@pytest.mark.parametrize("n, per_thread", SHAPES)
def test_reseeding_onto_another_key_and_a_start_at_infinity(dev, n, per_thread):
    Qs, scalars, jumps, wild, keys, states = seeded(dev, n, per_thread)
    dev.kangaroo_run(3)
    walked, _ = SL.walk(states, jumps, scalars, 3, DP)
    # by index list: two wild kangaroos onto the next key, one tame, and a wild start at infinity (d = -k''_1 on key 1)
    h = n // 2
    idx = [h + 5, 3, n - 1, h + 1]
    kpp1 = KEYS[1] - (A + W // 2)
    nk = [(keys[h + 5] + 1) % 3, 0, (keys[n - 1] + 1) % 3, 1]
    offs = [-77, 123456, 99, -kpp1]
    assert dev.kangaroo_seed_keys(offs, [K.WILD, 0, K.WILD, K.WILD], nk, idx=idx) == (1, 3)
    for i, d, k in zip(idx, offs, nk):
        walked[i] = model_state(Qs, d, i >= h, k)
    assert walked[h + 1] == (0, 0, (-kpp1) & K.M128, K.WILD | K.DEAD, 1)          # key solved (k'' = -d), kangaroo dead
    assert dev.kangaroo_download(0, n) == walked
    want, recs = SL.walk(walked, jumps, scalars, 24, DP)
    got, dropped, _ = dev.kangaroo_run(24)
    assert dropped == 0 and sorted(rec_key(r) for r in got) == sorted(recs)
    assert dev.kangaroo_download(0, n) == want
    for i, k in ((h + 5, nk[0]), (n - 1, nk[2])):                    # the records of the next launch name the new key
        mine = [r for r in got if r["kangaroo"] == i]
        assert mine and all(r["key"] == k != keys[i] for r in mine)
    assert not [r for r in got if r["kangaroo"] == h + 1]


@pytest.mark.parametrize("n, per_thread", SHAPES)
def test_verification_against_the_key_list(dev, n, per_thread):
    Qs, scalars, jumps, wild, keys, states = seeded(dev, n, per_thread)
    dev.kangaroo_run(STEPS)
    assert dev.kangaroo_verify() == (0, [])
    down = dev.kangaroo_download(0, n)
    h = n // 2
    bad = {7: "d", h + 2: "d", h + 9: "key", n - 1: "key3"}
    broken = list(down)
    for i, what in bad.items():
        x, y, d, fl, k = down[i]
        broken[i] = (x, y, d ^ (1 << 37), fl, k) if what == "d" else (x, y, d, fl, len(KEYS) if what == "key" else len(KEYS) + 70000)
    dev.kangaroo_upload(0, broken)
    assert dev.kangaroo_verify() == (len(bad), sorted(bad))
    dev.kangaroo_upload_list(sorted(bad), [down[i] for i in sorted(bad)])
    assert dev.kangaroo_verify() == (0, [])
    # one Q named by the caller: the key array is not looked at (the wild kangaroos of the other keys fail)
    nbad, _ = dev.kangaroo_verify(q=Qs[0])
    assert nbad == sum(1 for i in range(h, n) if keys[i] != 0)


def test_other_herds_are_unchanged(dev):
    import pybsgs
    n, per_thread = 128, 2
    Qs, scalars, jumps, wild, keys, offs = case(n)
    # a herd of the single-key symmetric walk still takes no list, and its states come back as 4-tuples with all three reserved words zero
    dev.kangaroo_setup_sym(jumps, scalars, DP, n, per_thread, 1 << 12)
    with pytest.raises(pybsgs.BsgsError, match="bsgs error -3"):
        dev.kangaroo_set_keys(Qs)
    with pytest.raises(pybsgs.BsgsError, match="bsgs error -3"):
        dev.kangaroo_seed_keys([5], [0], [0])
    assert dev.kangaroo_seed(Qs[0], offs, [K.WILD if w else 0 for w in wild]) == (0, 0)
    st = dev.kangaroo_download(0, n)
    assert all(len(s) == 4 for s in st)
    dev.kangaroo_upload(0, [s + (5,) for s in st])                   # a key word given to such a herd is ignored
    assert dev.kangaroo_download(0, n) == st
    assert dev.kangaroo_download(0, n, reserved=True) == [s + ((0, 0, 0),) for s in st]
    got, _, _ = dev.kangaroo_run(20)
    assert got and all(r["key"] == 0 for r in got)
    # the plain walk with a key list: the key stays in the flags, the record's fourth word stays 0
    s64, j64 = K.jump_table(K.Stream(3), 1 << 30)
    dev.kangaroo_setup(j64, s64, DP, n, per_thread, 1 << 12)
    dev.kangaroo_set_keys(Qs)
    assert dev.kangaroo_seed_keys(offs, [K.WILD if w else 0 for w in wild], keys) == (0, 0)
    st = dev.kangaroo_download(0, n)
    assert [s[3] for s in st] == [K.WILD | k << 8 if w else 0 for w, k in zip(wild, keys)]
    assert all(s[-1] == (0, 0, 0) for s in dev.kangaroo_download(0, n, reserved=True))
    got, _, _ = dev.kangaroo_run(8)
    assert got and all(r["key"] == 0 for r in got)


def test_setup_sym_keys_checks_its_arguments(dev):
    import pybsgs
    scalars, jumps = S.jump_table(K.Stream(1), 1 << 20, 128)
    for bad_r in (32, 96):
        with pytest.raises(pybsgs.BsgsError):
            dev.kangaroo_setup_sym_keys(jumps[:bad_r], scalars[:bad_r], 0, 128, 1, 100)
    with pytest.raises(pybsgs.BsgsError):
        dev.kangaroo_setup_sym_keys(jumps, scalars, 0, 100, 1, 100)
