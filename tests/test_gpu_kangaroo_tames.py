"""GPU: the tame table in device memory (csrc/kangaroo_tames.hip) against the model (tests/kangaroo_tames_model.py): kangaroo_run_tames hands back exactly
the records of a launch whose x is in the table plus the DEAD ones, each with its entry number; chained and wrapped images probed entry by entry; the record
capacity; the state errors."""
import pytest

import kangaroo_model as K
import kangaroo_tames_model as TM
from pybsgs.ecpy import P, add, mul, neg

pytestmark = pytest.mark.gpu

DP, STEPS = 2, 40


@pytest.fixture(scope="module")
def dev():
    import pybsgs
    d = pybsgs.Device(0)
    yield d
    d.close()


def herd(seed, W, Q, n):
    rng = K.Stream(seed)
    out = []
    for i in range(n):
        wild = i >= n // 2
        d = K.herd_offset(rng, W, wild)
        p = K.start(Q, d, wild)
        out.append((p[0], p[1], d & K.M128, K.WILD if wild else 0))
    return out


def got_key(r):
    return (r["x"], r["d"], r["kangaroo"], r["flags"], r["step"], r["entry"])


_JUMPS = {}


def jumps_with_a_fixed_point():
    """a jump table with a point J_j whose x selects j itself: a kangaroo standing on -J_j dies at its next step"""
    if not _JUMPS:
        seed = next(s for s in range(1, 2000) if any(p[0] & 63 == j for j, p in enumerate(K.jump_table(K.Stream(s), 1 << 30)[1])))
        scalars, jumps = K.jump_table(K.Stream(seed), 1 << 30)
        _JUMPS["v"] = (scalars, jumps, next(j for j, p in enumerate(jumps) if p[0] & 63 == j))
    return _JUMPS["v"]


_LAUNCH = {}


def launch(n, per_thread):
    """the herd of one case and the model's records of its one launch, computed once"""
    if (n, per_thread) not in _LAUNCH:
        scalars, jumps, j = jumps_with_a_fixed_point()
        states = herd(50 + n, 1 << 36, mul(0xABCDEF123), n)
        states[n // 2 + 3] = (jumps[j][0], neg(jumps[j])[1], 7, K.WILD | (5 << 8))      # x + J_j is infinity: one DEAD record at step 0
        final, recs = K.walk(states, jumps, scalars, STEPS, DP)
        _LAUNCH[(n, per_thread)] = (states, recs, final)
    return _LAUNCH[(n, per_thread)]


# the issue's two shapes (both run blocks of 256 threads: 256 and 1024 threads) and one whose 192 threads run in blocks of 64
@pytest.mark.parametrize("n, per_thread, block", [(512, 2, 256), (1024, 1, 256), (384, 2, 64)])
@pytest.mark.parametrize("table", ["every third", "all", "unrelated"])
def test_match_against_the_model(dev, n, per_thread, block, table):
    scalars, jumps, _ = jumps_with_a_fixed_point()
    states, recs, final = launch(n, per_thread)
    dead = [r for r in recs if r[3] & K.DEAD]
    assert len(dead) == 1 and len(recs) > n * STEPS // 8            # dp = 2: about one step in four is a DP
    xs = [r[0] & TM.M64 for r in recs if not r[3] & K.DEAD]
    if table == "every third":
        tags = list(dict.fromkeys(xs[::3]))
    elif table == "all":
        tags = list(dict.fromkeys(xs))
    else:
        tags = [t for t in ((v * 0x9E3779B97F4A7C15 + 12345) & TM.M64 for v in range(3000)) if t not in set(xs)]
    want = TM.match(recs, tags)
    dev.kangaroo_setup(jumps, scalars, DP, n, per_thread, 1 << 15)
    assert dev.kangaroo_geometry() == (n // per_thread, per_thread, block)
    dev.kangaroo_upload(0, states)
    dev.kangaroo_tames_install(tags)
    got, seen, dropped, ms = dev.kangaroo_run_tames(STEPS)
    print(table, n, "records", len(recs), "returned", len(got), "ms", ms)
    assert seen == len(recs) and dropped == 0
    assert sorted(got_key(r) for r in got) == want
    if table == "unrelated":
        assert [(r[2], r[5]) for r in want] == [(n // 2 + 3, None)]
    elif table == "all":
        assert len(want) == len(recs) and [r[5] for r in want if r[3] & K.DEAD] == [None]
    else:
        assert len(recs) // 3 <= len(want) - 1 < len(recs)
    # the walk itself is the plain one: the herd ends where kangaroo_run would have left it
    assert dev.kangaroo_download(0, n) == final
    # a second table replaces the first
    dev.kangaroo_upload(0, states)
    dev.kangaroo_tames_install(tags[:1])
    got2, seen2, _, _ = dev.kangaroo_run_tames(STEPS)
    assert seen2 == len(recs) and sorted(got_key(r) for r in got2) == TM.match(recs, tags[:1])


def probe(dev, table_tags, probe_tags):
    """64 kangaroos, kangaroo j standing on -J_j of a jump table whose J_j has x = probe_tags[j] (bits 0..5 of it are j): each dies at step 0 and writes
    one DEAD record of that x -> {tag: entry or None} as matched against table_tags"""
    assert [t & 63 for t in probe_tags] == list(range(64))
    jumps = [(t, 1000 + j) for j, t in enumerate(probe_tags)]
    dev.kangaroo_setup(jumps, [1 + j for j in range(64)], 0, 64, 1, 256)
    dev.kangaroo_upload(0, [(t, P - (1000 + j), j, K.WILD) for j, t in enumerate(probe_tags)])
    dev.kangaroo_tames_install(table_tags)
    got, seen, dropped, _ = dev.kangaroo_run_tames(1)
    assert seen == 64 and dropped == 0 and len(got) == 64
    assert all(r["flags"] == K.WILD | K.DEAD and r["step"] == 0 and r["d"] == r["kangaroo"] and r["x"] == probe_tags[r["kangaroo"]] for r in got)
    return {r["x"]: r["entry"] for r in got}


@pytest.mark.parametrize("first_line", [5, 60])                      # 60: the chain wraps past the last line
def test_chains(dev, first_line):
    tags = TM.chain_tags(first_line)
    L = TM.build(tags)
    assert [L[(first_line + k) & 63][2] for k in range(16)] == [1] * 15 + [0]
    assert probe(dev, tags, tags) == {t: e for e, t in enumerate(tags)}
    others = TM.chain_tags(first_line, salt=2)                       # the same home line, never inserted
    assert not set(others) & set(tags) and {TM.home(t, 64) for t in others} == {first_line}
    assert probe(dev, tags, others) == {t: None for t in others}
    mixed = tags[:32] + others[32:]
    assert probe(dev, tags, mixed) == {t: (j if j < 32 else None) for j, t in enumerate(mixed)}
    # entries in another order get other numbers, and a table of one entry finds that one
    assert probe(dev, tags[::-1], tags) == {t: 63 - e for e, t in enumerate(tags)}
    assert probe(dev, tags[9:10], tags) == {t: (0 if j == 9 else None) for j, t in enumerate(tags)}


def test_capacity(dev):
    """more records than the record buffer holds: the 64 that fit are matched, the rest counted"""
    scalars, jumps = K.jump_table(K.Stream(4), 1 << 30)
    n = 256
    states = herd(4, 1 << 30, mul(99), n)
    want_states, recs = K.walk(states, jumps, scalars, 2, 0)
    tags = list(dict.fromkeys(r[0] & TM.M64 for r in recs))
    want = {r[:5]: r[5] for r in TM.match(recs, tags)}
    assert len(recs) == 2 * n and len(want) == 2 * n
    dev.kangaroo_setup(jumps, scalars, 0, n, 1, 64)
    dev.kangaroo_upload(0, states)
    dev.kangaroo_tames_install(tags)
    got, seen, dropped, _ = dev.kangaroo_run_tames(2)
    assert seen == 2 * n and len(got) == 64 and dropped == 2 * n - 64
    keys = [got_key(r) for r in got]
    assert len(set(keys)) == 64 and all(want[k[:5]] == k[5] for k in keys)
    assert dev.kangaroo_download(0, n) == want_states
    # the plain call on the same herd is as it was
    dev.kangaroo_upload(0, states)
    plain, dropped, _ = dev.kangaroo_run(2)
    assert len(plain) == 64 and dropped == 2 * n - 64 and all(r["key"] == 0 for r in plain)


def test_state_errors():
    import pybsgs
    d = pybsgs.Device(0)
    try:
        with pytest.raises(pybsgs.BsgsError, match="bsgs_kangaroo_setup first"):
            d.kangaroo_tames_install([1, 2, 3])
        with pytest.raises(pybsgs.BsgsError, match="bsgs_kangaroo_setup first"):
            d.kangaroo_run_tames(1)
        scalars, jumps = K.jump_table(K.Stream(4), 1 << 30)
        d.kangaroo_setup(jumps, scalars, 0, 64, 1, 64)
        with pytest.raises(pybsgs.BsgsError, match="bsgs_kangaroo_tames_install first"):
            d.kangaroo_run_tames(1)
        with pytest.raises(pybsgs.BsgsError, match="share the tag"):
            d.kangaroo_tames_install([7, 8, 7])
        d.kangaroo_tames_install([1, 2, 3])
        d.kangaroo_upload(0, herd(4, 1 << 30, mul(99), 64))
        assert d.kangaroo_run_tames(1)[1] == 64
        d.kangaroo_setup(jumps, scalars, 0, 64, 1, 64)               # a new herd: the table is gone with the old one
        with pytest.raises(pybsgs.BsgsError, match="bsgs_kangaroo_tames_install first"):
            d.kangaroo_run_tames(1)
        d.kangaroo_setup_sym(jumps, scalars, 0, 64, 1, 64)           # the symmetric herd takes a table too
        d.kangaroo_tames_install([1, 2, 3])
        d.kangaroo_setup_sym_keys(jumps, scalars, 0, 64, 1, 64)      # the keyed herd's records carry their key in the word the match writes
        with pytest.raises(pybsgs.BsgsError, match="tame table serves"):
            d.kangaroo_tames_install([1, 2, 3])
    finally:
        d.close()
