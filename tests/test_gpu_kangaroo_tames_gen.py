"""GPU: the tame table grown in device memory (csrc/kangaroo_tames_gen.hip) against the model (tests/kangaroo_tames_gen_model.py), through pybsgs: crafted
records through bsgs_kangaroo_tames_gen_insert -- distinct tags, equal tags in one wave, across waves and across launches, chains that wrap and interleave,
DEAD / CYCLE / tag-0 records, a table filled to the last slot -- then the insert behind the plain and the symmetric walk, and the state errors.  A herd of
512 kangaroos with a record capacity of 1024."""
from collections import Counter

import pytest

import kangaroo_model as K
import kangaroo_sym_model as S
import kangaroo_tames_gen_model as GM

pytestmark = pytest.mark.gpu

HERD, CAP = 512, 1024
DP, STEPS, LAUNCHES = 4, 24, 3                                       # about 512 * 24 / 16 = 768 records per launch, below the capacity


@pytest.fixture(scope="module")
def jump_table():
    return K.jump_table(K.Stream(11), 1 << 30)


@pytest.fixture(scope="module")
def dev(jump_table):
    import pybsgs
    d = pybsgs.Device(0)
    scalars, jumps = jump_table
    d.kangaroo_setup(jumps, scalars, DP, HERD, 2, CAP)
    yield d
    d.close()


def fresh_tags(rng, n, avoid=()):
    out, seen = [], set(avoid) | {0}
    while len(out) < n:
        t = rng.u64()
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


def launch(dev, table, records):
    """one insert of records (tag, d, flags) on the device and in the model: the hand-backs agree as multisets of (tag, reason), the handed-back records are
    the records sent, and the entry count is the model's -> (the model's new table, the handed-back records)"""
    table, want = GM.insert(table, records)
    got, n_entries = dev.kangaroo_tames_gen_insert(records)
    assert Counter((r["x"] & GM.M64, r["reason"]) for r in got) == want
    assert n_entries == GM.entries(table)
    sent = Counter((t, d & K.M128, fl, k) for k, (t, d, fl) in enumerate(records))
    assert not Counter((r["x"], r["d"], r["flags"], r["kangaroo"]) for r in got) - sent      # as the caller wrote them, apart from the reason
    return table, got


def check_read(dev, table):
    """what the device holds is the model's tag set, each with one of its candidate offsets"""
    got = dev.kangaroo_tames_gen_read()
    assert len(got) == GM.entries(table) and sorted(t for t, _ in got) == sorted(table["cand"])
    assert all(d in table["cand"][t] for t, d in got)
    return dict(got)


def test_distinct_tags(dev):
    rng = K.Stream(1)
    dev.kangaroo_tames_gen_begin(2048)
    table = GM.new_table(2048, CAP)
    assert table["slots"] == 8192
    recs = [(t, rng.u128(), 0) for t in fresh_tags(rng, 1000)]
    table, back = launch(dev, table, recs)
    assert back == [] and GM.entries(table) == 1000
    assert sorted(check_read(dev, table).items()) == sorted((t, d) for t, d, _ in recs)      # exactly the model's (tag, d) set


def test_duplicates(dev):
    rng = K.Stream(2)
    dev.kangaroo_tames_gen_begin(2048)
    table = GM.new_table(2048, CAP)
    x, y, *tags = fresh_tags(rng, 1002)
    for i in range(64):
        tags[i] = x                                                   # one tag 64 times in one wave
    for w in range(1, 9):
        tags[64 * w + 5] = y                                          # one tag in 8 different waves (of three blocks)
    recs = [(t, rng.u128(), 0) for t in tags]
    table, back = launch(dev, table, recs)
    assert Counter((r["x"], r["reason"]) for r in back) == Counter({(x, GM.GEN_DUPLICATE): 63, (y, GM.GEN_DUPLICATE): 7})
    stored = check_read(dev, table)
    assert len(stored) == 1000 - 63 - 7
    for t in (x, y):                                                  # exactly one of the copies is stored, and the others are the ones that came back
        assert Counter([stored[t]] + [r["d"] for r in back if r["x"] == t]) == Counter(d for tt, d, _ in recs if tt == t)
    # a tag repeated in a second batch: what was stored stays
    again = [(x, 1, 0), (y, 2, 0), (tags[700], 3, 0)] + [(t, rng.u128(), 0) for t in fresh_tags(rng, 200, avoid=tags)] + [(tags[701], 4, 0)]
    table, back = launch(dev, table, again)
    assert Counter((r["x"], r["d"], r["reason"]) for r in back) == Counter({(x, 1, 1): 1, (y, 2, 1): 1, (tags[700], 3, 1): 1, (tags[701], 4, 1): 1})
    assert check_read(dev, table) == {**stored, **{t: d for t, d, _ in again[3:-1]}}


@pytest.mark.parametrize("case", ["wraps", "interleaved"])
def test_probing(dev, case):
    dev.kangaroo_tames_gen_begin(2048)
    table = GM.new_table(2048, CAP)
    slots = table["slots"]
    if case == "wraps":
        tags = GM.chain_tags(slots - 1, slots, 200)                   # 200 tags of the last slot: the chain runs on from slot 0
    else:
        chain = GM.chain_tags(100, slots, 200)
        inside = [GM.chain_tags(100 + k, slots, 1, salt=7)[0] for k in range(1, 200)]      # tags whose home lies inside that chain
        tags = [t for pair in zip(chain, inside + [None]) for t in pair if t is not None]
    assert len(set(tags)) == len(tags) <= CAP
    table, back = launch(dev, table, [(t, 1000 + k, 0) for k, t in enumerate(tags)])
    assert back == [] and check_read(dev, table) == {t: 1000 + k for k, t in enumerate(tags)}
    occupied = [s for s, t in enumerate(table["tags"]) if t]
    assert occupied == (list(range(199)) + [slots - 1] if case == "wraps" else list(range(100, 100 + len(tags))))
    table, back = launch(dev, table, [(t, 5, 0) for t in reversed(tags)])      # every one is found again
    assert sorted(r["x"] for r in back) == sorted(tags) and {r["reason"] for r in back} == {GM.GEN_DUPLICATE}
    assert check_read(dev, table) == {t: 1000 + k for k, t in enumerate(tags)}


def test_dead_cycle_and_tag_zero(dev):
    rng = K.Stream(4)
    dev.kangaroo_tames_gen_begin(2048)
    table = GM.new_table(2048, CAP)
    a, b, c = fresh_tags(rng, 3)
    table, back = launch(dev, table, [(c, 9, 0), (a, 1, K.DEAD), (b, 2, K.DEAD | S.CYCLE), (0, 3, 0), (0, 4, K.DEAD)])
    assert sorted((r["x"], r["d"], r["flags"], r["reason"]) for r in back) == sorted(
        [(a, 1, K.DEAD, GM.GEN_DEAD), (b, 2, K.DEAD | S.CYCLE, GM.GEN_DEAD), (0, 3, 0, GM.GEN_TAG_ZERO), (0, 4, K.DEAD, GM.GEN_DEAD)])
    assert check_read(dev, table) == {c: 9}
    table, back = launch(dev, table, [(a, 5, 0), (b, 6, 0)])          # none of them was stored: their tags are still free
    assert back == [] and check_read(dev, table) == {c: 9, a: 5, b: 6}


def test_full(dev):
    rng = K.Stream(5)
    dev.kangaroo_tames_gen_begin(64)
    table = GM.new_table(64, CAP)
    assert table["slots"] == 4096
    tags = fresh_tags(rng, 6 * 1024)
    sent = stored = full = 0
    for b in range(5):
        table, back = launch(dev, table, [(t, b, 0) for t in tags[1024 * b:1024 * (b + 1)]])
        sent += 1024
        full += len(back)
        assert {r["reason"] for r in back} <= {GM.GEN_FULL}
        stored = GM.entries(table)
        assert stored <= 4096 and stored + full == sent
    assert stored == 4096 and full == 1024                            # every record beyond the last slot came back, the call returned
    # one more batch on the full table: a tag that is there is still found, a new one is FULL
    table, back = launch(dev, table, [(t, 7, 0) for t in tags[:512] + tags[5 * 1024:5 * 1024 + 512]])
    assert Counter(r["reason"] for r in back) == Counter({GM.GEN_DUPLICATE: 512, GM.GEN_FULL: 512})
    got = check_read(dev, table)
    assert len(got) == 4096 and got == {t: k // 1024 for k, t in enumerate(tags[:4096])}


def walk_case(dev, model, setup, states, jumps, scalars, twins):
    """LAUNCHES launches of run_tames_gen against the model's walk: n_seen, the table and the hand-backs"""
    setup()
    dev.kangaroo_upload(0, states)
    dev.kangaroo_tames_gen_begin(4096)
    table = GM.new_table(4096, CAP)
    dead = 0
    for _ in range(LAUNCHES):
        states, recs = model.walk(states, jumps, scalars, STEPS, DP)
        assert 0 < len(recs) <= CAP
        table, want = GM.insert(table, [(x & GM.M64, d, fl) for x, d, _, fl, _ in recs])
        got, seen, n_entries, dropped, ms = dev.kangaroo_run_tames_gen(STEPS)
        assert seen == len(recs) and dropped == 0 and n_entries == GM.entries(table)
        assert Counter((r["x"] & GM.M64, r["reason"]) for r in got) == want
        by_rec = {(x, d, k, fl, s) for x, d, k, fl, s in recs}
        assert all((r["x"], r["d"], r["kangaroo"], r["flags"], r["step"]) in by_rec for r in got)      # the records as the walk wrote them
        assert all(r["kangaroo"] in twins for r in got if r["reason"] == GM.GEN_DUPLICATE)             # the model's duplicates and nothing else
        assert all(r["flags"] & K.DEAD for r in got if r["reason"] == GM.GEN_DEAD)
        dead += sum(1 for r in got if r["reason"] == GM.GEN_DEAD)
        assert {r["reason"] for r in got} <= {GM.GEN_DEAD, GM.GEN_DUPLICATE}
    assert GM.entries(table) > HERD
    stored = check_read(dev, table)
    assert all(len(c) == 1 for c in table["cand"].values())          # (equal tags here are the twins' equal records: the model's tag -> d map is exact)
    assert stored == {t: next(iter(c)) for t, c in table["cand"].items()}
    assert dev.kangaroo_download(0, HERD) == states                   # the walk is the walk: the herd ends where the model's does
    return table, dead


def test_with_the_plain_walk(dev, jump_table):
    scalars, jumps = jump_table
    rng = K.Stream(6)
    states = []
    for _ in range(HERD):
        t = 1 + rng.u128() % ((1 << 40) - 1)
        p = K.start(None, t, False)
        states.append((p[0], p[1], t, 0))
    states[300] = states[17]                                          # two kangaroos planted on the same start: every record of theirs comes twice
    table, dead = walk_case(dev, K, lambda: dev.kangaroo_setup(jumps, scalars, DP, HERD, 2, CAP), states, jumps, scalars, {17, 300})
    assert dead == 0


def test_with_the_symmetric_walk(dev):
    scalars, jumps, cyc, _, _ = S.short_cycle_case(3, 64)             # a jump table with a 2-cycle the last-jump rule does not prevent, and a start on it
    rng = K.Stream(7)
    states = []
    for _ in range(HERD):
        t = 1 + rng.u128() % ((1 << 60) - 1)
        p = K.start(None, t, False)
        states.append((p[0], p[1], t, 0))
    states[7] = cyc
    table, dead = walk_case(dev, S, lambda: dev.kangaroo_setup_sym(jumps, scalars, DP, HERD, 2, CAP), states, jumps, scalars, set())
    assert dead >= 1                                                  # the cycle check's DEAD | CYCLE record came back and was never stored (check_read)


def test_states(jump_table):
    import pybsgs
    scalars, jumps = jump_table
    d = pybsgs.Device(0)
    try:
        for call in (lambda: d.kangaroo_run_tames_gen(1), d.kangaroo_tames_gen_read, lambda: d.kangaroo_tames_gen_begin(64)):
            with pytest.raises(pybsgs.BsgsError, match="error -3: bsgs_kangaroo_setup first"):
                call()
        d.kangaroo_tames_gen_end()                                    # no herd, no table: not an error
        d.kangaroo_setup(jumps, scalars, 0, 64, 1, 64)
        for call in (lambda: d.kangaroo_run_tames_gen(1), d.kangaroo_tames_gen_read, lambda: d.kangaroo_tames_gen_insert([(1, 1, 0)])):
            with pytest.raises(pybsgs.BsgsError, match="error -3: bsgs_kangaroo_tames_gen_begin first"):
                call()
        for capacity in (0, (1 << 31) + 1):
            with pytest.raises(pybsgs.BsgsError, match="error -1: .*1..2\\^31"):
                d.kangaroo_tames_gen_begin(capacity)
            with pytest.raises(pybsgs.BsgsError, match="error -3: bsgs_kangaroo_tames_gen_begin first"):      # a begin that is refused leaves no table
                d.kangaroo_run_tames_gen(1)
        d.kangaroo_tames_gen_begin(64)                                # and a good one after it works
        with pytest.raises(pybsgs.BsgsError, match="error -1: .*record capacity"):
            d.kangaroo_tames_gen_insert([(k + 1, 1, 0) for k in range(65)])
        back, n = d.kangaroo_tames_gen_insert([(5, 1, 0), (6, 2, 0), (5, 3, 0)])
        assert n == 2 and [(r["x"], r["reason"]) for r in back] == [(5, GM.GEN_DUPLICATE)]
        with pytest.raises(pybsgs.BsgsError, match="error -1: room for 1 entries, the table holds 2"):
            d.kangaroo_tames_gen_read(max_entries=1)
        assert len(d.kangaroo_tames_gen_read()) == 2
        # the other launches behave as before on a herd that has a growing table
        states = [(p[0], p[1], t, 0) for t in range(1, 65) for p in [K.start(None, t, False)]]
        want_states, recs = K.walk(states, jumps, scalars, 2, 0)
        d.kangaroo_upload(0, states)
        plain, dropped, _ = d.kangaroo_run(2)
        assert len(plain) == 64 and dropped == 64 and all(r["key"] == 0 for r in plain) and d.kangaroo_download(0, 64) == want_states
        tags = list(dict.fromkeys(r[0] & GM.M64 for r in recs))
        d.kangaroo_tames_install(tags[:10])
        d.kangaroo_upload(0, states)
        got, seen, dropped, _ = d.kangaroo_run_tames(2)
        assert seen == 128 and dropped == 64 and all(r["x"] & GM.M64 in tags[:10] and r["entry"] == tags.index(r["x"] & GM.M64) for r in got)
        assert len(d.kangaroo_tames_gen_read()) == 2                 # and the growing table is as it was
        d.kangaroo_tames_gen_begin(128)                               # a second begin replaces the table
        assert d.kangaroo_tames_gen_read() == []
        d.kangaroo_tames_gen_end()
        d.kangaroo_tames_gen_end()                                    # twice is fine
        with pytest.raises(pybsgs.BsgsError, match="bsgs_kangaroo_tames_gen_begin first"):
            d.kangaroo_tames_gen_read()
        d.kangaroo_tames_gen_begin(64)
        d.kangaroo_setup(jumps, scalars, 0, 64, 1, 64)               # a new herd drops the table
        with pytest.raises(pybsgs.BsgsError, match="bsgs_kangaroo_tames_gen_begin first"):
            d.kangaroo_run_tames_gen(1)
        d.kangaroo_setup_sym(jumps, scalars, 0, 64, 1, 64)           # the symmetric herd grows one too
        d.kangaroo_tames_gen_begin(64)
        d.kangaroo_setup_sym_keys(jumps, scalars, 0, 64, 1, 64)      # the keyed herd is refused
        with pytest.raises(pybsgs.BsgsError, match="error -3: a tame table grows under the herds"):
            d.kangaroo_tames_gen_begin(64)
    finally:
        d.close()
