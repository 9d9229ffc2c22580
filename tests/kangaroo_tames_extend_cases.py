"""The case lists of the load and of the sorted read of a growing tame table, shared by the CPU check of the model (tests/test_kangaroo_tames_extend_cli.py) and
the GPU tests (tests/test_gpu_kangaroo_tames_extend.py).  The smallest herd and table: 64 kangaroos, record capacity 64, capacity 64 -> 256 slots."""
import kangaroo_model as K
import kangaroo_tames_extend_model as XM
import kangaroo_tames_gen_model as GM

HERD = CAP = CAPACITY = 64
SLOTS = GM.n_slots(CAPACITY, CAP)
B = XM.SORT_TILE
C_D = 0x9E3779B97F4A7C15F39CC0605CEDC835                              # d = f(tag): a d that arrives with another tag shows


def f(tag):
    return (tag * C_D + 1) & K.M128


def fresh_tags(rng, n, avoid=()):
    out, seen = [], set(avoid) | {0}
    while len(out) < n:
        t = rng.u64()
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


def load_cases():
    """name -> a list of steps, ("insert", [(tag, d, flags)]) or ("load", [(tag, d)]), run in order on a fresh table of CAPACITY"""
    assert SLOTS == 256
    rng = K.Stream(41)
    cases = {}
    cases["chain"] = [("load", [(t, 100 + k) for k, t in enumerate(GM.chain_tags(5, SLOTS, 40))])]
    cases["chain_wraps"] = [("load", [(t, 200 + k) for k, t in enumerate(GM.chain_tags(SLOTS - 1, SLOTS, 40))])]
    # three blocks of four waves: one tag in all 64 lanes of wave 0, another in one lane of each of the waves 1..8; the other lanes hold a few new tags and
    # tag 0, so that the 256 slots never fill
    x, y, *fill = fresh_tags(rng, 2 + 96)
    tags = [0] * 768
    for i in range(768):
        if i % 8 == 1:
            tags[i] = fill[i // 8]
    tags[:64] = [x] * 64
    for w in range(1, 9):
        tags[64 * w + 5] = y
    cases["equal_tags"] = [("load", [(t, 1000 + i) for i, t in enumerate(tags)])]
    first = fresh_tags(rng, 50)
    cases["after_insert"] = [("insert", [(t, 7, 0) for t in first]), ("load", [(t, 8) for t in first[10:40]] + [(t, 9) for t in fresh_tags(rng, 20, avoid=first)])]
    cases["tag_zero"] = [("load", [(0, 1), (7, 3), (0, 2)])]
    cases["ragged"] = [("load", [(t, f(t)) for t in fresh_tags(rng, 64 + 37)])]      # no multiple of the wave
    cases["empty"] = [("load", [])]
    return cases


def sort_cases():
    """name -> (tags, max_entries or None); d = f(tag)"""
    rng = K.Stream(43)
    cases = {"empty": ([], None), "one": ([0x1234567890ABCDEF], None)}
    for n in (B - 1, B, B + 1, 3 * B + 5):
        cases["n%d" % n] = (fresh_tags(rng, n), None)
    order = list(range(1, 256))
    order = [order[(k * 101) % 255] for k in range(255)]
    cases["lowest_byte"] = ([0x0123456789ABCD00 | v for v in order], None)
    cases["highest_byte"] = ([(((k * 37) % 256) << 56) | 0x00A5A5A5A5A5A5A5 for k in range(256)], None)
    cases["top_56_shared"] = ([0xFFFFFFFFFFFFFF00 | ((k * 59) % 256) for k in range(256)], None)
    cases["low_16_zero"] = ([t << 16 & XM.M64 for t in fresh_tags(K.Stream(47), B + 7) if t << 16 & XM.M64], None)
    cases["cut"] = (fresh_tags(rng, 3 * B + 5), B + 3)
    for name, (tags, _) in cases.items():
        assert len(set(tags)) == len(tags) and 0 not in tags, name
    return cases
