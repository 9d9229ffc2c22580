"""GPU: bsgs_kangaroo_set_keys / bsgs_kangaroo_seed_keys (csrc/kangaroo_seed.hip) against the model's `start` (tests/kangaroo_model.py) with one Q per
key -- every seeded state bit for bit with flags WILD | key << 8, by range and by index list, the start that doubles Q_k and the one at infinity, one key
against bsgs_kangaroo_seed, the error codes; then the key through the unchanged walk: every record and every downloaded state still names it."""
import pytest

import kangaroo_model as K
import kangaroo_multi_model as M
from pybsgs.ecpy import mul

pytestmark = pytest.mark.gpu

KPS = [0x1234567890ABCDEF1234, 0xFEDCBA9876543210, 3, (1 << 99) + 12345, 0xC0FFEE << 70, 0x77777777777]       # k'_k = k_k - a: Q_k = k'_k G


@pytest.fixture(scope="module")
def dev():
    import pybsgs
    d = pybsgs.Device(0)
    yield d
    d.close()


def model_state(Qs, d, wild, key):
    p = K.start(Qs[key], d, wild)
    fl = M.wild_flags(key) if wild else 0
    return (0, 0, d & K.M128, fl | K.DEAD) if p is None else (p[0], p[1], d & K.M128, fl)


def mixed_herd(n, W, seed):
    """tame and wild of every key, both signs, the doubling start of key 1 and the start at infinity of key 4"""
    rng = K.Stream(seed)
    wild = [i % 2 == 1 for i in range(n)]
    keys = [(i // 2) % len(KPS) if w else 0 for i, w in enumerate(wild)]
    offs = [K.herd_offset(rng, W, w) for w in wild]
    for i, (d, w, k) in {3: (KPS[1], True, 1), 9: (-KPS[4], True, 4), 11: (0, True, 2), 13: (-1, True, 5), 700: (-KPS[0], True, 0), 20: (-(1 << 124), False, 0)}.items():
        offs[i], wild[i], keys[i] = d, w, k
    return offs, wild, keys


@pytest.mark.parametrize("n, per_thread", [(1024, 4), (2048, 8)])
def test_seed_keys_parity_range_and_list(dev, n, per_thread):
    import pybsgs
    assert pybsgs.KANGAROO_KEY_SHIFT == M.KEY_SHIFT == 8
    Qs = [mul(k) for k in KPS]
    scalars, jumps = K.jump_table(K.Stream(5), 1 << 40)
    dev.kangaroo_setup(jumps, scalars, 0, n, per_thread, 1 << 12)
    dev.kangaroo_set_keys(Qs)
    W = 1 << 100
    offs, wild, keys = mixed_herd(n, W, 4242 + n)
    ninf, first = dev.kangaroo_seed_keys(offs, [K.WILD if w else 0 for w in wild], keys)
    assert (ninf, first) == (2, 9)                                   # -k'_4 of key 4 and -k'_0 of key 0; the lower position
    want = [model_state(Qs, d, w, k) for d, w, k in zip(offs, wild, keys)]
    got = dev.kangaroo_download(0, n)
    assert got[3][:2] == mul(2 * KPS[1]) and got[3][3] == K.WILD | 1 << 8
    assert got[11][:2] == Qs[2] and got[9] == (0, 0, (-KPS[4]) & K.M128, K.WILD | 4 << 8 | K.DEAD)
    assert got == want
    # by index list, scattered and unordered, every key once more, the others untouched
    rng = K.Stream(777)
    idx = [1001, 3, 517, 65, 255, 257, 1023, 1, 701, 0, 512]
    fresh = [K.herd_offset(rng, W, wild[i]) for i in idx]
    nk = [(keys[i] + 1) % len(KPS) if wild[i] else 0 for i in idx]  # a re-seeded kangaroo may change its key
    assert dev.kangaroo_seed_keys(fresh, [K.WILD if wild[i] else 0 for i in idx], nk, idx=idx) == (0, 0)
    for i, d, k in zip(idx, fresh, nk):
        want[i] = model_state(Qs, d, wild[i], k)
    # a range in the middle, by first / n: tame only
    mid = [K.herd_offset(rng, W, False) for _ in range(100)]
    assert dev.kangaroo_seed_keys(mid, [0] * 100, [0] * 100, first=200) == (0, 0)
    for k, d in enumerate(mid):
        want[200 + k] = model_state(Qs, d, False, 0)
    assert dev.kangaroo_download(0, n) == want


def test_one_key_equals_the_single_q_kernel(dev):
    n, per_thread = 1024, 4
    Q = mul(KPS[0])
    scalars, jumps = K.jump_table(K.Stream(6), 1 << 40)
    dev.kangaroo_setup(jumps, scalars, 0, n, per_thread, 1 << 12)
    rng = K.Stream(31337)
    wild = [i >= n // 2 for i in range(n)]
    offs = [K.herd_offset(rng, 1 << 90, w) for w in wild]
    offs[600], offs[601] = KPS[0], -KPS[0]
    fl = [K.WILD if w else 0 for w in wild]
    r1 = dev.kangaroo_seed(Q, offs, fl)
    one = dev.kangaroo_download(0, n)
    dev.kangaroo_set_keys([Q])
    r2 = dev.kangaroo_seed_keys([0] * n, [0] * n, [0] * n)          # the herd overwritten (all dead at infinity) so that the next call is seen to write
    assert r2 == (n, 0)
    assert dev.kangaroo_seed_keys(offs, fl, [0] * n) == r1 == (1, 601)
    assert dev.kangaroo_download(0, n) == one


def test_error_cases_leave_the_herd_as_it_was(dev):
    import pybsgs
    n, per_thread = 1024, 4
    Qs = [mul(k) for k in KPS]
    scalars, jumps = K.jump_table(K.Stream(7), 1 << 40)
    dev.kangaroo_setup(jumps, scalars, 0, n, per_thread, 1 << 12)

    def rc(offs, fl, keys, idx=None):
        """the C-ABI's return code (pybsgs raises "bsgs error <code>: <text>")"""
        try:
            dev.kangaroo_seed_keys(offs, fl, keys, idx=idx)
        except pybsgs.BsgsError as e:
            return int(str(e).split()[2].rstrip(":"))
        return 0

    before = dev.kangaroo_download(0, n)
    ERR_ARG, ERR_STATE = -1, -3
    assert rc([1], [K.WILD], [0]) == ERR_STATE                       # a wild position before set_keys
    assert dev.kangaroo_download(0, n) == before
    dev.kangaroo_set_keys(Qs)
    offs, wild, keys = mixed_herd(n, 1 << 80, 99)
    assert dev.kangaroo_seed_keys(offs, [K.WILD if w else 0 for w in wild], keys)[0] == 2
    before = dev.kangaroo_download(0, n)
    assert rc([5, 6], [K.WILD, K.WILD], [0, len(Qs)]) == ERR_ARG     # key out of the list
    assert rc([5], [0], [1]) == ERR_ARG                              # a tame position with a key
    assert rc([5], [2], [0]) == ERR_ARG                              # flags other than WILD
    assert rc([5, 6], [0, 0], [0, 0], idx=[4, 4]) == ERR_ARG         # a kangaroo listed twice
    assert dev.kangaroo_download(0, n) == before
    with pytest.raises(Exception):
        dev.kangaroo_set_keys([])
    # a herd of the symmetric walk takes one key
    s2, j2 = K.jump_table(K.Stream(8), 1 << 40)
    dev.kangaroo_setup_sym(j2, s2, 0, n, per_thread, 1 << 12)
    with pytest.raises(pybsgs.BsgsError, match="bsgs error -3"):
        dev.kangaroo_set_keys(Qs)


@pytest.mark.parametrize("n, per_thread", [(1024, 16), (2048, 8)])
def test_the_key_travels_through_the_walk(dev, n, per_thread):
    Qs = [mul(k) for k in KPS]
    W = 1 << 60
    scalars, jumps = K.jump_table(K.Stream(11 + n), n * (W ** 0.5) / 4)
    dp = 3
    dev.kangaroo_setup(jumps, scalars, dp, n, per_thread, 1 << 16)
    dev.kangaroo_set_keys(Qs)
    rng = K.Stream(2024 + n)
    wild = [i >= n // 2 for i in range(n)]
    keys = [i % len(KPS) if w else 0 for i, w in enumerate(wild)]
    offs = [K.herd_offset(rng, W, w) for w in wild]
    assert dev.kangaroo_seed_keys(offs, [K.WILD if w else 0 for w in wild], keys) == (0, 0)
    states = [model_state(Qs, d, w, k) for d, w, k in zip(offs, wild, keys)]
    want, recs = K.walk(states, jumps, scalars, 12, dp)              # the model carries the flags word along and looks at DEAD only, as the kernel must
    got, dropped, _ = dev.kangaroo_run(12)
    assert dropped == 0 and len(got) > n                             # dp 3, 12 steps: about 1.5 records per kangaroo
    assert sorted((r["x"], r["d"], r["kangaroo"], r["flags"], r["step"]) for r in got) == sorted(recs)
    for r in got:
        i = r["kangaroo"]
        assert r["flags"] == (M.wild_flags(keys[i]) if wild[i] else 0), r
    down = dev.kangaroo_download(0, n)
    assert down == want
    assert [s[3] for s in down] == [M.wild_flags(k) if w else 0 for w, k in zip(wild, keys)]
    # and through upload: the word goes back as it came
    dev.kangaroo_upload(0, down)
    assert dev.kangaroo_download(0, n) == down
