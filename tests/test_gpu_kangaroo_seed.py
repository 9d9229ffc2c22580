"""GPU: bsgs_kangaroo_seed (csrc/kangaroo_seed.hip) against the model's `start` (tests/kangaroo_model.py) -- every seeded state bit for bit, the walk that
follows, crafted offsets (both signs, single windows, zero bytes, the start that doubles Q, the start at infinity), a chunk large enough for four starts per thread, and seeding by
index list, also between two calls that seed from a key list."""
import pytest

import kangaroo_model as K
from pybsgs.ecpy import add, mul, neg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import pybsgs
    d = pybsgs.Device(0)
    yield d
    d.close()


def model_state(Q, d, wild):
    """what bsgs_kangaroo_seed must leave: the model's start, or a dead kangaroo at (0, 0) for the point at infinity"""
    p = K.start(Q, d, wild)
    fl = K.WILD if wild else 0
    return (0, 0, d & K.M128, fl | K.DEAD) if p is None else (p[0], p[1], d & K.M128, fl)


@pytest.mark.parametrize("wbits", [40, 125])
@pytest.mark.parametrize("n, per_thread", [(2048, 8), (1024, 16)])          # blocks of 256 threads / of 64
def test_seed_parity_then_walk(dev, n, per_thread, wbits):
    W = 1 << wbits
    a = 0x123456789 << 130
    Q = add(mul(a + (W // 5) * 3 + 0x9876543210), neg(mul(a)))
    scalars, jumps = K.jump_table(K.Stream(77 + wbits), min(2.0 ** 62, n * (W ** 0.5) / 4))
    dev.kangaroo_setup(jumps, scalars, 4, n, per_thread, 1 << 16)
    rng = K.Stream(5000 + n + wbits)
    wild = [i >= n // 2 for i in range(n)]
    offs = [K.herd_offset(rng, W, w) for w in wild]
    assert dev.kangaroo_seed(Q, offs, [K.WILD if w else 0 for w in wild]) == (0, 0)
    states = [model_state(Q, d, w) for d, w in zip(offs, wild)]
    assert dev.kangaroo_download(0, n) == states
    # the seeded herd walks as an uploaded one does
    want, recs = K.walk(states, jumps, scalars, 8, 4)
    got, dropped, _ = dev.kangaroo_run(8)
    assert dropped == 0
    assert dev.kangaroo_download(0, n) == want
    assert sorted((r["x"], r["d"], r["kangaroo"], r["flags"], r["step"]) for r in got) == sorted(recs)


def test_crafted_offsets_in_one_batch(dev):
    n, per_thread = 1024, 4
    kp = 0x1234567890ABCDEF1234                                     # k' = k - a: Q = k' G
    Q = mul(kp)
    scalars, jumps = K.jump_table(K.Stream(3), 1 << 40)
    dev.kangaroo_setup(jumps, scalars, 0, n, per_thread, 1 << 12)
    rng = K.Stream(99)
    W = 1 << 100
    wild = [i % 2 == 1 for i in range(n)]
    offs = [K.herd_offset(rng, W, w) for w in wild]
    sparse = (0x6B << 120) | (0xCD << 64) | (0x01 << 40) | 0xEF     # zero bytes in most windows (below 2^127: offsets are signed)
    crafted = {2: (1, False), 4: (-1, False), 6: (1 << 64, False), 8: (1 << 124, False), 10: (-(1 << 124), False), 12: (sparse, False), 14: (-sparse, False),
               3: (0, True), 5: (kp, True), 7: (-kp, True), 9: (sparse, True), 11: (-1, True), 13: ((1 << 127) - 1, False),
               15: (-(1 << 127), True), 600: (0, False), 601: (255, True), 603: (256, True)}
    for i, (d, w) in crafted.items():
        offs[i], wild[i] = d, w
    ninf, first = dev.kangaroo_seed(Q, offs, [K.WILD if w else 0 for w in wild])
    assert (ninf, first) == (2, 7)                                  # wild -k' (Q - k' G) and tame 0, the lower position reported
    want = [model_state(Q, d, w) for d, w in zip(offs, wild)]
    got = dev.kangaroo_download(0, n)
    assert got[3][:2] == Q and got[5][:2] == mul(2 * kp)            # wild 0 starts on Q, wild k' on 2 Q
    assert got[7] == (0, 0, (-kp) & K.M128, K.WILD | K.DEAD) and got[600] == (0, 0, 0, K.DEAD)
    assert got == want


def test_four_starts_share_a_threads_inversion(dev):
    """a chunk of 2^18 positions or more: B = 4 positions per thread (k = b * TT + thread, TT = 65536 here) behind one running product and one block
    inversion -- the only path of a full herd.  Two starts at infinity in different b slots, each of which puts 1 into its thread's product."""
    n, per_thread, TT = 1 << 18, 16, 65536
    kp = 0x1234567890ABCDEF1234
    Q = mul(kp)
    scalars, jumps = K.jump_table(K.Stream(4), 1 << 40)
    dev.kangaroo_setup(jumps, scalars, 0, n, per_thread, 1 << 12)
    wild = [i % 2 == 1 for i in range(n)]
    # cheap to make for 2^18 positions: the low 100 bits of a multiple of i, tame in [1, 2^100), wild in [-2^99, 2^99)
    offs = [(((i + 1) * 0x9E3779B97F4A7C15F39CC0605CEDC835) & ((1 << 100) - 1)) - (w << 99) or 1 for i, w in enumerate(wild)]
    crafted = {7: (0, False), 2 * TT + 5: (-kp, True)}
    for i, (d, w) in crafted.items():
        offs[i], wild[i] = d, w
    assert dev.kangaroo_seed(Q, offs, [K.WILD if w else 0 for w in wild]) == (2, 7)
    assert dev.kangaroo_verify(Q) == (0, [])                        # the whole herd, the two dead kangaroos at (0, 0) among it
    sample = sorted({b * TT + t for b in range(4) for t in (0, 5, 6, 7, 8, 63, 64, 255, 256, 257, 4099, 32768, TT - 257, TT - 256, TT - 2, TT - 1)})
    assert len(sample) == 64 and all(i in sample for i in crafted)
    for i in sample:
        assert dev.kangaroo_download(i, 1) == [model_state(Q, offs[i], wild[i])], i
    assert dev.kangaroo_download(7, 1) == [(0, 0, 0, K.DEAD)]
    assert dev.kangaroo_download(2 * TT + 5, 1) == [(0, 0, (-kp) & K.M128, K.WILD | K.DEAD)]


def test_seed_by_index_list_leaves_the_others_untouched(dev):
    n, per_thread = 1024, 4
    Q = mul(0xFEDCBA9876543210)
    scalars, jumps = K.jump_table(K.Stream(8), 1 << 40)
    dev.kangaroo_setup(jumps, scalars, 0, n, per_thread, 1 << 12)
    rng = K.Stream(123)
    W = 1 << 90
    wild = [i >= n // 2 for i in range(n)]
    offs = [K.herd_offset(rng, W, w) for w in wild]
    assert dev.kangaroo_seed(Q, offs, [K.WILD if w else 0 for w in wild]) == (0, 0)
    before = dev.kangaroo_download(0, n)
    idx = [1000, 3, 517, 64, 255, 256, 1023, 0, 700]                # scattered, unordered
    fresh = [K.herd_offset(rng, W, wild[i]) for i in idx]
    assert dev.kangaroo_seed(Q, fresh, [K.WILD if wild[i] else 0 for i in idx], idx=idx) == (0, 0)
    want = list(before)
    for i, d in zip(idx, fresh):
        want[i] = model_state(Q, d, wild[i])
        assert want[i] != before[i]
    assert dev.kangaroo_download(0, n) == want
    # a range in the middle, by first / n
    mid = [K.herd_offset(rng, W, False) for _ in range(100)]
    assert dev.kangaroo_seed(None, mid, [0] * 100, first=200) == (0, 0)
    for k, d in enumerate(mid):
        want[200 + k] = model_state(Q, d, False)
    assert dev.kangaroo_download(0, n) == want
    with pytest.raises(Exception):
        dev.kangaroo_seed(Q, [1, 2], [0, 0], idx=[5, 5])            # a kangaroo listed twice
    with pytest.raises(Exception):
        dev.kangaroo_seed(Q, [1], [0], idx=[n])                     # outside the herd
    # the one-Q call leaves the herd's key list alone: seeded with key 1 of a list, then with a Q of the call's own, then with key 1 again
    Q0, Q1, Q2 = mul(0xABCDEF0123456789), mul(0x1357924680ACE), mul(0x2468ACE013579BDF)
    dev.kangaroo_set_keys([Q0, Q1])
    keyed = K.WILD | 1 << 8                                          # flags of a wild kangaroo of key 1

    def seeded_with_key_1(idx):
        ds = [K.herd_offset(rng, W, True) for _ in idx]
        assert dev.kangaroo_seed_keys(ds, [K.WILD] * len(idx), [1] * len(idx), idx=idx) == (0, 0)
        for i, d in zip(idx, ds):
            p = K.start(Q1, d, True)
            want[i] = (p[0], p[1], d & K.M128, keyed)

    seeded_with_key_1([10, 900, 333])
    assert dev.kangaroo_download(0, n) == want
    idx2 = [11, 901, 334, 10]
    ds2 = [K.herd_offset(rng, W, True) for _ in idx2]
    assert dev.kangaroo_seed(Q2, ds2, [K.WILD] * len(idx2), idx=idx2) == (0, 0)
    for i, d in zip(idx2, ds2):
        want[i] = model_state(Q2, d, True)
    seeded_with_key_1([12, 902, 335, 11])
    assert dev.kangaroo_download(0, n) == want
