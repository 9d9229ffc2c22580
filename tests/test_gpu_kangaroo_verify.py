"""GPU: bsgs_kangaroo_verify / bsgs_kangaroo_verify_points (csrc/kangaroo_verify.hip; include/bsgs_hip.h "Kangaroo, verification").  A kangaroo (x, y, d, flags)
stands at sigma*Q + d*G: herds of the three walks verify clean after seeding and after walking and are left as they were, offsets at the edges of 128 bits
and the starts that double or cancel are model states (tests/kangaroo_model.py, kangaroo_sym_model.py) uploaded as they are, and every single-field change
of a state is found at exactly its index; table entries against the model's low 64 bits of x."""
import pytest

import kangaroo_model as K
import kangaroo_multi_model as M
import kangaroo_sym_model as S
from pybsgs.ecpy import N, P, add, mul, neg

pytestmark = pytest.mark.gpu

KQ = 0x1234567890ABCDEF1234                                         # Q = KQ * G
KPS = [KQ, 0xFEDCBA9876543210, (1 << 99) + 12345, 0x77777777777]    # a list of four keys
W = 1 << 60
ERR_ARG, ERR_STATE = -1, -3
SHAPES = [(1024, 16), (2048, 8)]                                    # one wave; one block of four waves


@pytest.fixture(scope="module")
def dev():
    import pybsgs
    d = pybsgs.Device(0)
    yield d
    d.close()


def rc_of(call):
    """the C-ABI's return code (pybsgs raises "bsgs error <code>: <text>")"""
    import pybsgs
    try:
        call()
    except pybsgs.BsgsError as e:
        return int(str(e).split()[2].rstrip(":"))
    return 0


def offsets(n, seed, wild, sym=False):
    rng = K.Stream(seed)
    return [(S.herd_offset if sym else K.herd_offset)(rng, W, w) for w in wild]


def point(Q, d, fl):
    """sigma*Q + d*G of the model; None: the point at infinity"""
    sg = S.sigma(fl)
    return add(mul(d % N), None if sg == 0 else Q if sg > 0 else neg(Q))


def model_state(Q, d, fl):
    p = point(Q, d, fl)
    return (0, 0, d & K.M128, fl | K.DEAD) if p is None else (p[0], p[1], d & K.M128, fl)


def plain_herd(dev, n, per_thread, interleaved=False):
    """half tame, half wild (interleaved: the odd ones wild), seeded on the GPU -> Q"""
    Q = mul(KQ)
    scalars, jumps = K.jump_table(K.Stream(5 + n), n * (W ** 0.5) / 4)
    dev.kangaroo_setup(jumps, scalars, 3, n, per_thread, 1 << 16)
    wild = [i % 2 == 1 if interleaved else i >= n // 2 for i in range(n)]
    assert dev.kangaroo_seed(Q, offsets(n, 4242 + n, wild), [K.WILD if w else 0 for w in wild]) == (0, 0)
    return Q


def sym_herd(dev, n, per_thread, interleaved=False):
    Q = mul(KQ)
    scalars, jumps = S.jump_table(K.Stream(7 + n), n * (W ** 0.5) / 4, 64)
    dev.kangaroo_setup_sym(jumps, scalars, 3, n, per_thread, 1 << 16)
    wild = [i % 2 == 1 if interleaved else i >= n // 2 for i in range(n)]
    assert dev.kangaroo_seed(Q, offsets(n, 777 + n, wild, sym=True), [K.WILD if w else 0 for w in wild]) == (0, 0)
    return Q


def keys_herd(dev, n, per_thread, interleaved=False):
    Qs = [mul(k) for k in KPS]
    scalars, jumps = K.jump_table(K.Stream(9 + n), n * (W ** 0.5) / 4)
    dev.kangaroo_setup(jumps, scalars, 3, n, per_thread, 1 << 16)
    dev.kangaroo_set_keys(Qs)
    wild = [i % 2 == 1 if interleaved else i >= n // 2 for i in range(n)]
    keys = [(i // 2) % len(KPS) if w else 0 for i, w in enumerate(wild)]
    assert dev.kangaroo_seed_keys(offsets(n, 99 + n, wild), [K.WILD if w else 0 for w in wild], keys) == (0, 0)
    return Qs


def walk_and_verify(dev, n, q):
    """clean as seeded; 40 steps at dp 3; clean again, and the verification leaves the herd as it was"""
    assert dev.kangaroo_verify(q) == (0, [])
    _, dropped, _ = dev.kangaroo_run(40)
    assert dropped == 0
    before = dev.kangaroo_download(0, n)
    assert dev.kangaroo_verify(q) == (0, [])
    assert dev.kangaroo_verify(q, first=n // 2 - 3, n=70) == (0, [])
    assert dev.kangaroo_download(0, n) == before
    return before


@pytest.mark.parametrize("n, per_thread", SHAPES)
def test_clean_plain_herd(dev, n, per_thread):
    Q = plain_herd(dev, n, per_thread)
    after = walk_and_verify(dev, n, Q)
    assert sum(1 for s in after if s[3] & K.WILD) == n // 2
    # a sample against the integers: what verifies clean is what the model says
    for x, y, d, fl in after[5::n // 8]:
        assert (x, y) == point(Q, K.signed128(d), fl)
    # the wrong Q: every wild kangaroo fails, no tame one does; the count is exact and the list holds the lowest chunk's failures in order
    nb, idx = dev.kangaroo_verify(mul(KQ + 1), max_bad=n)
    assert nb == n // 2 and idx == list(range(n // 2, n))


@pytest.mark.parametrize("n, per_thread", SHAPES)
def test_clean_symmetric_herd(dev, n, per_thread):
    Q = sym_herd(dev, n, per_thread)
    after = walk_and_verify(dev, n, Q)
    wild = after[n // 2:]
    assert n // 8 < sum(1 for s in wild if s[3] & S.NEG) < 3 * n // 8          # about half of the wild half
    assert all(s[3] & S.LAST_VALID for s in after if not s[3] & K.DEAD) and sum(1 for s in after if s[3] & S.LAST_MASK & ~S.LAST_VALID) > n // 2
    for x, y, d, fl in after[3::n // 8]:
        assert (x, y) == point(Q, K.signed128(d), fl)


@pytest.mark.parametrize("n, per_thread", SHAPES)
def test_clean_herd_with_a_key_list(dev, n, per_thread):
    Qs = keys_herd(dev, n, per_thread)
    after = walk_and_verify(dev, n, None)
    assert {M.key_of(s[3]) for s in after[n // 2:]} == {0, 1, 2, 3}
    for x, y, d, fl in after[n // 2 + 1::n // 16]:
        assert (x, y) == point(Qs[M.key_of(fl)], K.signed128(d), fl)
    # with one Q named the key bits are not looked at: only the kangaroos of that key stand
    nb, idx = dev.kangaroo_verify(Qs[1], max_bad=n)
    assert idx == [i for i in range(n // 2, n) if (i // 2) % 4 != 1] and nb == len(idx)


def test_offsets_at_the_edges(dev):
    n, per_thread = 1024, 16
    Q = plain_herd(dev, n, per_thread)
    edges = [1, -1, (1 << 64) - 1, 1 << 64, -(1 << 64), (1 << 127) - 1, -(1 << 127) + 1, 1 << 96, -(1 << 96), (1 << 120) + (1 << 32), -((1 << 120) + (1 << 64)), 127 << 120]
    cases = [(d, 0) for d in edges] + [(d, K.WILD) for d in edges] + [(d, K.WILD | S.NEG) for d in edges]
    cases += [(KQ, K.WILD), (-KQ, K.WILD | S.NEG)]                   # d*G == sigma*Q: the sum is a doubling
    cases += [(-KQ, K.WILD), (KQ, K.WILD | S.NEG), (0, 0)]           # d*G == -sigma*Q, and tame 0: infinity -- dead, x = y = 0
    states = [model_state(Q, d, fl) for d, fl in cases]
    assert states[-5][:2] == mul(2 * KQ) and states[-4][:2] == neg(mul(2 * KQ))
    assert all(s[:2] == (0, 0) and s[3] & K.DEAD for s in states[-3:]) and not any(s[3] & K.DEAD for s in states[:-3])
    idx = [(64 * k + 7 * (k // 16)) % n for k in range(len(states))]       # spread over the waves, tame and wild halves alike
    assert len(set(idx)) == len(idx)
    dev.kangaroo_upload_list(idx, states)
    assert dev.kangaroo_verify(Q) == (0, [])
    # the same offsets through the seeding kernel (it takes no NEG): the states the model gives, and clean
    plain = [(i, d, fl) for i, (d, fl) in zip(idx, cases) if not fl & S.NEG]
    ninf, _ = dev.kangaroo_seed(Q, [d for _, d, _ in plain], [fl for _, _, fl in plain], idx=[i for i, _, _ in plain])
    assert ninf == 2
    for i, d, fl in plain:
        assert dev.kangaroo_download(i, 1) == [model_state(Q, d, fl)]
    assert dev.kangaroo_verify(Q) == (0, [])
    # a live kangaroo at infinity is wrong, and so is a dead one with x = y = 0 whose offset is somewhere else
    i = idx[len(cases) - 3]
    dev.kangaroo_upload_list([i], [(0, 0, (-KQ) & K.M128, K.WILD)])
    assert dev.kangaroo_verify(Q) == (1, [i])
    dev.kangaroo_upload_list([i], [(0, 0, (-KQ + 1) & K.M128, K.WILD | K.DEAD)])
    assert dev.kangaroo_verify(Q) == (1, [i])


def flip(field, bit):
    def f(s):
        s = list(s)
        s[field] ^= 1 << bit
        return tuple(s)
    return f


def changed(dev, q, indices, change):
    """the states `indices` changed and put back by upload_list: what verify says meanwhile"""
    old = [dev.kangaroo_download(i, 1)[0] for i in indices]
    new = [change(s) for s in old]
    assert all(a != b for a, b in zip(old, new))
    dev.kangaroo_upload_list(indices, new)
    got = dev.kangaroo_verify(q)
    dev.kangaroo_upload_list(indices, old)
    return got


def corruption_indices(n, per_thread):
    T = n // per_thread
    return [0, 63, 64, T - 1, T, n - 1]                               # T: the second slot of thread 0


def dead_at_zero(s):
    return (0, 0, s[2], s[3] | K.DEAD)


def flip_y_high(s):
    """bit 254 of y, or bit 253 where that would leave the field"""
    return (s[0], s[1] ^ (1 << (254 if s[1] ^ (1 << 254) < P else 253)), s[2], s[3])


PLAIN_CHANGES = {"d bit 0": flip(2, 0), "d bit 127": flip(2, 127), "x bit 0": flip(0, 0), "y bit 254": flip_y_high, "y -> p - y": lambda s: (s[0], P - s[1], s[2], s[3]),
                 "WILD toggled": flip(3, 0), "dead at zero": dead_at_zero}


def every_change(dev, q, n, per_thread, changes):
    where = corruption_indices(n, per_thread)
    assert len(set(where)) == 6
    assert dev.kangaroo_verify(q) == (0, [])
    for name, change in changes.items():
        for i in where:
            assert changed(dev, q, [i], change) == (1, [i]), (name, i)
        assert changed(dev, q, where, change) == (6, sorted(where)), name
    assert dev.kangaroo_verify(q) == (0, [])


def test_every_changed_field_is_found_plain(dev):
    n, per_thread = 2048, 8
    Q = plain_herd(dev, n, per_thread, interleaved=True)
    dev.kangaroo_run(40)
    every_change(dev, Q, n, per_thread, PLAIN_CHANGES)
    # max_bad smaller than n_bad: the count is exact, the list is cut
    where = corruption_indices(n, per_thread)
    old = [dev.kangaroo_download(i, 1)[0] for i in where]
    dev.kangaroo_upload_list(where, [flip(2, 0)(s) for s in old])
    nb, idx = dev.kangaroo_verify(Q, max_bad=4)
    assert nb == 6 and len(idx) == 4 and idx == sorted(idx) and set(idx) < set(where)
    assert dev.kangaroo_verify(Q, max_bad=0) == (6, [])
    assert dev.kangaroo_verify(Q, first=64, n=n - 64 - 1) == (3, [where[2], where[3], where[4]])
    dev.kangaroo_upload_list(where, old)
    assert dev.kangaroo_verify(Q) == (0, [])


def test_every_changed_field_is_found_symmetric(dev):
    n, per_thread = 2048, 8
    Q = sym_herd(dev, n, per_thread, interleaved=True)
    dev.kangaroo_run(40)
    changes = dict(PLAIN_CHANGES)
    changes["NEG toggled"] = flip(3, 1)                               # (on a tame kangaroo: a state the walk never writes)
    every_change(dev, Q, n, per_thread, changes)
    # what the check does not look at: the last jump index and CYCLE
    where = corruption_indices(n, per_thread)
    assert changed(dev, Q, where, lambda s: (s[0], s[1], s[2], s[3] ^ (0x5A5 << S.LAST_SHIFT))) == (0, [])
    assert changed(dev, Q, where, lambda s: (s[0], s[1], s[2], s[3] & ~S.LAST_MASK)) == (0, [])
    assert changed(dev, Q, where, flip(3, 2)) == (0, [])              # CYCLE
    assert changed(dev, Q, where, lambda s: (s[0], s[1], s[2], s[3] | K.DEAD | S.CYCLE)) == (0, [])      # retired by the cycle check: it keeps its point


def test_every_changed_field_is_found_key_list(dev):
    n, per_thread = 2048, 8
    keys_herd(dev, n, per_thread, interleaved=True)
    dev.kangaroo_run(40)
    changes = dict(PLAIN_CHANGES)
    changes["key k -> k + 1"] = lambda s: (s[0], s[1], s[2], s[3] + (1 << M.KEY_SHIFT))       # (the last key: beyond the list; a tame one: a key where none belongs)
    where = corruption_indices(n, per_thread)
    keys = [M.key_of(dev.kangaroo_download(i, 1)[0][3]) for i in where]
    assert len(KPS) - 1 in keys
    every_change(dev, None, n, per_thread, changes)
    assert changed(dev, None, [where[-1]], lambda s: (s[0], s[1], s[2], s[3] | 0xFFFF << M.KEY_SHIFT)) == (1, [where[-1]])


def test_a_coordinate_that_is_not_below_p_fails(dev):
    """x + p is congruent to x and fits 256 bits only for x < 2^32 + 977: Q is a point with such an x, and a wild kangaroo at offset 0 stands on it"""
    xs = next(x for x in range(1, 100) if pow(x ** 3 + 7, (P - 1) // 2, P) == 1)
    ys = pow(xs ** 3 + 7, (P + 1) // 4, P)
    assert (ys * ys - xs ** 3 - 7) % P == 0
    n, per_thread = 1024, 16
    plain_herd(dev, n, per_thread)
    dev.kangaroo_upload_list([n - 2], [(xs, ys, 0, K.WILD)])
    assert dev.kangaroo_verify((xs, ys), first=n - 2, n=1) == (0, [])
    dev.kangaroo_upload_list([n - 2], [(xs + P, ys, 0, K.WILD)])
    assert dev.kangaroo_verify((xs, ys), first=n - 2, n=1) == (1, [n - 2])


def test_across_the_chunk_boundary(dev):
    """a herd of more than one chunk of 2^20: kangaroo 2^20 + 5 belongs to the second launch"""
    n, per_thread = (1 << 20) + (1 << 16), 16
    Q = mul(KQ)
    scalars, jumps = K.jump_table(K.Stream(3), 1 << 40)
    dev.kangaroo_setup(jumps, scalars, 20, n, per_thread, 1 << 12)
    offs = [((i * 0x9E3779B97F4A7C15 + 12345) & ((1 << 100) - 1)) - (i & 1) * (1 << 99) for i in range(n)]
    assert dev.kangaroo_seed(Q, offs, [i & 1 for i in range(n)])[0] == 0
    assert dev.kangaroo_verify(Q) == (0, [])
    i = (1 << 20) + 5
    assert changed(dev, Q, [i], flip(2, 0)) == (1, [i])
    assert changed(dev, Q, [(1 << 20) - 1, i, n - 1], flip(0, 3)) == (3, [(1 << 20) - 1, i, n - 1])
    assert dev.kangaroo_verify(Q) == (0, [])
    dev.kangaroo_setup(jumps, scalars, 20, 1024, per_thread, 1 << 12)       # (the large herd is released)


def test_verify_points(dev):
    n, per_thread = 1024, 16
    Qs = keys_herd(dev, n, per_thread)
    Q = Qs[0]
    rng = K.Stream(2025)
    # one Q: tame, wild, wild with NEG
    fl1 = [(0, K.WILD, K.WILD | S.NEG)[k % 3] for k in range(300)]
    d1 = [K.herd_offset(rng, 1 << 124, True) for _ in range(300)]
    base = [mul(d % N) for d in d1]                                   # d*G once per entry
    lo64 = lambda b, q, fl: add(b, None if not fl & K.WILD else neg(q) if fl & S.NEG else q)[0] & 0xFFFFFFFFFFFFFFFF      # noqa: E731
    x1 = [lo64(b, Q, fl) for b, fl in zip(base, fl1)]
    assert x1[:3] == [point(Q, d, fl)[0] & 0xFFFFFFFFFFFFFFFF for d, fl in zip(d1[:3], fl1[:3])]
    assert dev.kangaroo_verify_points(Q, d1, fl1, x1) == (0, [])
    # the key list: tame, and wild of three keys
    fl2 = [0 if k % 4 == 0 else M.wild_flags(k % 4 - 1) for k in range(300)]
    x2 = [lo64(b, Qs[M.key_of(fl)], fl) for b, fl in zip(base, fl2)]
    assert dev.kangaroo_verify_points(None, d1, fl2, x2) == (0, [])
    for k in (0, 1, 63, 64, 255, 256, 299):
        for q, fl, x in ((Q, fl1, x1), (None, fl2, x2)):
            bad_x = x[:k] + [x[k] ^ (1 << 63)] + x[k + 1:]
            assert dev.kangaroo_verify_points(q, d1, fl, bad_x) == (1, [k]), k
            bad_d = d1[:k] + [d1[k] ^ 1] + d1[k + 1:]
            assert dev.kangaroo_verify_points(q, bad_d, fl, x) == (1, [k]), k
        assert dev.kangaroo_verify_points(Q, d1, fl1[:k] + [fl1[k] ^ K.WILD] + fl1[k + 1:], x1) == (1, [k]), k      # another owner: tame <-> wild
        other = M.wild_flags((M.key_of(fl2[k]) + 1) % 3) if fl2[k] else M.wild_flags(0)
        assert dev.kangaroo_verify_points(None, d1, fl2[:k] + [other] + fl2[k + 1:], x2) == (1, [k]), k
    # n = 1, and nothing at all
    assert dev.kangaroo_verify_points(Q, d1[:1], fl1[:1], x1[:1]) == (0, [])
    assert dev.kangaroo_verify_points(Q, d1[1:2], fl1[1:2], [x1[1] ^ 1]) == (1, [0])
    assert dev.kangaroo_verify_points(Q, [], [], []) == (0, [])
    # an entry at infinity is no table entry; the count is exact when the list is short
    assert dev.kangaroo_verify_points(Q, [-KQ, 5], [K.WILD, 0], [0, mul(5)[0] & 0xFFFFFFFFFFFFFFFF]) == (1, [0])
    nb, idx = dev.kangaroo_verify_points(Q, d1, fl1, [v ^ 2 for v in x1], max_bad=7)
    assert nb == 300 and len(idx) == 7 and idx == sorted(idx)


def test_error_codes(dev):
    import pybsgs
    fresh = pybsgs.Device(0)
    try:                                                              # no herd
        assert rc_of(lambda: fresh.kangaroo_verify(mul(KQ), first=0, n=0)) == ERR_STATE
        assert rc_of(lambda: fresh.kangaroo_verify_points(mul(KQ), [1], [0], [0])) == ERR_STATE
    finally:
        fresh.close()
    n, per_thread = 1024, 16
    Q = plain_herd(dev, n, per_thread)
    assert rc_of(lambda: dev.kangaroo_verify(None)) == ERR_STATE      # no Q named and no key list
    assert rc_of(lambda: dev.kangaroo_verify_points(None, [1], [0], [0])) == ERR_STATE
    assert rc_of(lambda: dev.kangaroo_verify(Q, first=1, n=n)) == ERR_ARG
    assert dev.kangaroo_verify(Q) == (0, [])
    Qs = keys_herd(dev, n, per_thread)
    # a key beyond the list: the caller's input for points, the state's fault for a herd
    assert rc_of(lambda: dev.kangaroo_verify_points(None, [1, 2], [M.wild_flags(0), M.wild_flags(len(Qs))], [0, 0])) == ERR_ARG
    s = dev.kangaroo_download(n - 1, 1)[0]
    dev.kangaroo_upload_list([n - 1], [(s[0], s[1], s[2], M.wild_flags(len(Qs)))])
    assert dev.kangaroo_verify(None) == (1, [n - 1])
    # a symmetric herd takes no key list: no Q named is a state error there too
    sym_herd(dev, n, per_thread)
    assert rc_of(lambda: dev.kangaroo_verify(None)) == ERR_STATE
