"""GPU: the distinguished-point table in device memory (csrc/kangaroo_dptable.hip) against the model (tests/kangaroo_dptable_model.py), through pybsgs:
crafted records through bsgs_kangaroo_dptable_insert / load / read -- one tag in all lanes of a wave and in 8 waves of three blocks, tag 0 and DEAD, homes at
the last slot, a loaded entry met by a record, a table filled to the last slot, a host buffer that ends in the middle of a pair -- then the insert behind the
plain and the symmetric walk of 4096 kangaroos against bsgs_kangaroo_run on the same herd, and the state errors."""
import struct
from collections import Counter

import pytest

import kangaroo_model as K
import kangaroo_sym_model as S
import kangaroo_dptable_model as DM

pytestmark = pytest.mark.gpu

HERD, CAP = 512, 1024
WALK_HERD, WALK_CAP, WALK_DP, WALK_STEPS, WALK_LAUNCHES = 4096, 8192, 4, 20, 3      # about 4096 * 20 / 16 = 5120 records per launch, below the capacity


@pytest.fixture(scope="module")
def jump_table():
    return K.jump_table(K.Stream(11), 1 << 30)


@pytest.fixture(scope="module")
def dev(jump_table):
    import pybsgs
    d = pybsgs.Device(0)
    scalars, jumps = jump_table
    d.kangaroo_setup(jumps, scalars, 4, HERD, 2, CAP)
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
    """one insert of records (tag, d, flags, kangaroo) on the device, judged by the model -> (the model's new table, the hand-backs as the model writes them)"""
    got, n_entries, dropped = dev.kangaroo_dptable_insert(records)
    assert dropped == 0
    return DM.check_device(table, records, got, n_entries)


def check_read(dev, table):
    got = dev.kangaroo_dptable_read()
    assert len(got) == len(set(got)) == DM.entries(table)
    assert set(got) == DM.read(table)
    return set(got)


def test_distinct_tags(dev):
    rng = K.Stream(1)
    dev.kangaroo_dptable_begin(2048)
    table = DM.new_table(2048, CAP)
    assert table["slots"] == 8192
    recs = [(t, rng.u128(), (0, 1, 3, 1 | 1 << 8 | 37 << 9)[k % 4], 5000 + k) for k, t in enumerate(fresh_tags(rng, 1000))]
    table, back = launch(dev, table, recs)
    assert back == []
    assert check_read(dev, table) == {(t, d, kid, DM.type_of(fl)) for t, d, fl, kid in recs}


def test_one_tag_in_a_wave_and_across_waves_and_blocks(dev):
    rng = K.Stream(2)
    dev.kangaroo_dptable_begin(2048)
    table = DM.new_table(2048, CAP)
    x, y, *tags = fresh_tags(rng, 1002)
    for i in range(64):
        tags[i] = x                                                   # one tag in all 64 lanes of a wave
    for w in range(1, 9):
        tags[64 * w + 5] = y                                          # one tag in 8 different waves (of three blocks)
    recs = [(t, rng.u128(), k & 1, k) for k, t in enumerate(tags)]
    table, back = launch(dev, table, recs)
    assert Counter((r, rec[0]) for r, rec, _ in back) == Counter({(DM.DPT_DUPLICATE, x): 63, (DM.DPT_DUPLICATE, y): 7})
    stored = check_read(dev, table)                                   # check_device has named the one stored entry of x and of y: exactly one entry each
    assert len(stored) == 1000 - 63 - 7
    for t in (x, y):                                                  # the stored words equal one of the inputs'
        (e,) = [e for e in stored if e[0] == t]
        assert e in {(tt, d, kid, DM.type_of(fl)) for tt, d, fl, kid in recs if tt == t}
    # a second launch: what was stored stays, and the new records come back paired with it
    again = [(x, 1, 1, 2000), (y, 2, 0, 2001), (tags[700], 3, 3, 2002)] + [(t, rng.u128(), 1, 3000 + k) for k, t in enumerate(fresh_tags(rng, 200, avoid=tags))]
    table, back = launch(dev, table, again)
    assert sorted(rec[3] for r, rec, _ in back) == [2000, 2001, 2002] and all(st in stored for _, _, st in back)
    assert check_read(dev, table) == stored | {(t, d, kid, DM.type_of(fl)) for t, d, fl, kid in again[3:]}


def test_tag_zero_and_dead_come_back_and_are_never_stored(dev):
    rng = K.Stream(4)
    dev.kangaroo_dptable_begin(2048)
    table = DM.new_table(2048, CAP)
    a, b, c = fresh_tags(rng, 3)
    recs = [(c, 9, 1, 0), (a, 1, K.DEAD, 1), (b, 2, K.DEAD | S.CYCLE | 1, 2), (0, 3, 0, 3), (0, 4, K.DEAD, 4)]
    table, back = launch(dev, table, recs)
    assert sorted((r, rec[3]) for r, rec, _ in back) == [(DM.DPT_DEAD, 1), (DM.DPT_DEAD, 2), (DM.DPT_DEAD, 4), (DM.DPT_TAG_ZERO, 3)]
    assert check_read(dev, table) == {(c, 9, 0, 1)}
    table, back = launch(dev, table, [(a, 5, 0, 1), (b, 6, 3, 2)])   # none of them was stored: their tags are still free
    assert back == [] and check_read(dev, table) == {(c, 9, 0, 1), (a, 5, 1, 0), (b, 6, 2, 3)}


@pytest.mark.parametrize("case", ["wraps", "interleaved"])
def test_probing(dev, case):
    dev.kangaroo_dptable_begin(2048)
    table = DM.new_table(2048, CAP)
    slots = table["slots"]
    if case == "wraps":
        tags = DM.chain_tags(slots - 1, slots, 200)                   # 200 tags of the last slot: the chain runs on from slot 0
    else:
        chain = DM.chain_tags(100, slots, 200)
        inside = [DM.chain_tags(100 + k, slots, 1, salt=7)[0] for k in range(1, 200)]      # tags whose home lies inside that chain
        tags = [t for pair in zip(chain, inside + [None]) for t in pair if t is not None]
    assert len(set(tags)) == len(tags) <= CAP
    table, back = launch(dev, table, [(t, 1000 + k, 1, k) for k, t in enumerate(tags)])
    want = {(t, 1000 + k, k, 1) for k, t in enumerate(tags)}
    assert back == [] and check_read(dev, table) == want
    occupied = [s for s, t in enumerate(table["tags"]) if t]
    assert occupied == (list(range(199)) + [slots - 1] if case == "wraps" else list(range(100, 100 + len(tags))))
    table, back = launch(dev, table, [(t, 5, 0, 7000 + k) for k, t in enumerate(reversed(tags))])      # every one is found again, with its own entry
    assert len(back) == len(tags) and {st for _, _, st in back} == want
    assert check_read(dev, table) == want


def test_load_then_records_meet_the_loaded_entries(dev):
    rng = K.Stream(6)
    dev.kangaroo_dptable_begin(4096)
    table = DM.new_table(4096, CAP)
    tags = fresh_tags(rng, 3000) + DM.chain_tags(table["slots"] - 1, table["slots"], 40)
    ent = [(t, rng.u128(), rng.u64() & 0xFFFFFFFF, (0, 1, 3)[k % 3]) for k, t in enumerate(tags)]
    raw = b"".join(struct.pack("<QQQII", t, d & DM.M64, d >> 64, kid, ty) for t, d, kid, ty in ent)
    extra = [(0, 1, 2, 0), (0, 3, 4, 1)]
    table, want = DM.load(table, ent + extra)
    got = dev.kangaroo_dptable_load(raw + b"".join(struct.pack("<QQQII", t, d, 0, kid, ty) for t, d, kid, ty in extra))
    assert got == want + (3040,) and want == (3040, 0, 2, 0)
    held = dev.kangaroo_dptable_read(raw=True)
    assert len(held) == len(raw) and sorted(held[o:o + 32] for o in range(0, len(held), 32)) == sorted(raw[o:o + 32] for o in range(0, len(raw), 32))      # the exact 32 bytes
    probe = [ent[k] for k in (0, 17, 2999, 3000, 3039)]
    table, back = launch(dev, table, [(t, 99, 1, 50 + k) for k, (t, _, _, _) in enumerate(probe)])
    assert sorted(st for _, _, st in back) == sorted(probe) and all(r == DM.DPT_DUPLICATE for r, _, _ in back)
    # the same entries again are duplicates to the load too, and the table is as it was
    assert dev.kangaroo_dptable_load(raw)[:4] == (0, 3040, 0, 0)
    check_read(dev, table)


def test_full(dev):
    rng = K.Stream(5)
    dev.kangaroo_dptable_begin(64)
    slots = DM.n_slots(64, CAP)
    assert slots == 4096
    tags = fresh_tags(rng, 6 * 1024)
    held, full = {}, 0
    for b in range(5):
        got, n_entries, dropped = dev.kangaroo_dptable_insert([(t, b, 1, 1024 * b + k) for k, t in enumerate(tags[1024 * b:1024 * (b + 1)])])
        assert dropped == 0 and {r["reason"] for r in got} <= {DM.DPT_FULL}
        full += len(got)
        assert n_entries <= slots and n_entries + full == 1024 * (b + 1)       # stored + handed back = records in
    assert n_entries == slots and full == 1024                        # every record beyond the last slot came back, and the call returned
    # on the full table a tag that is there is still found with its entry, a new one is FULL
    got, n_entries, _ = dev.kangaroo_dptable_insert([(t, 7, 0, 9) for t in tags[:512] + tags[5 * 1024:5 * 1024 + 512]])
    assert n_entries == slots and Counter(r["reason"] for r in got) == Counter({DM.DPT_STORED: 512, DM.DPT_DUPLICATE: 512, DM.DPT_FULL: 512})
    held = {e[0]: e for e in dev.kangaroo_dptable_read()}
    assert len(held) == slots
    for k, r in enumerate(got):
        if r["reason"] == DM.DPT_STORED:
            assert got[k + 1]["reason"] == DM.DPT_DUPLICATE and got[k + 1]["x"] == r["x"]
            assert held[r["x"]] == (r["x"], r["d"], r["kangaroo"], r["flags"]) and r["d"] == tags.index(r["x"]) // 1024
    assert dev.kangaroo_dptable_load([(tags[5 * 1024 + 600], 1, 2, 1), (tags[0], 1, 2, 1)])[:4] == (0, 1, 0, 1)


def test_a_buffer_that_ends_inside_a_pair_drops_the_pair_whole(dev):
    rng = K.Stream(7)
    dev.kangaroo_dptable_begin(2048)
    tags = fresh_tags(rng, 8)
    got, n, dropped = dev.kangaroo_dptable_insert([(t, k, 0, k) for k, t in enumerate(tags)])
    assert (got, n, dropped) == ([], 8, 0)
    recs = [(t, 100 + k, 1, 10 + k) for k, t in enumerate(tags)]     # eight duplicates: sixteen records
    for room in (16, 15, 14, 5, 1, 0):
        got, n, dropped = dev.kangaroo_dptable_insert(recs, max_recs=room)
        assert n == 8 and len(got) == room // 2 * 2 and dropped == 8 - room // 2, (room, len(got), dropped)
        for k in range(0, len(got), 2):
            assert got[k]["reason"] == DM.DPT_STORED and got[k + 1]["reason"] == DM.DPT_DUPLICATE and got[k]["x"] == got[k + 1]["x"]
            assert got[k]["d"] == tags.index(got[k]["x"]) and got[k + 1]["d"] == 100 + got[k]["d"]
    # singles and pairs mixed: whatever the order, a cut never leaves half a pair, and the count is of the walk's records
    mixed = recs[:3] + [(0, 1, 0, 30), (tags[0], 2, K.DEAD, 31)]
    for room in range(9):
        got, n, dropped = dev.kangaroo_dptable_insert(mixed, max_recs=room)
        walk = [r for r in got if r["reason"] != DM.DPT_STORED]
        assert len(walk) + dropped == 5 and len(got) in (room, room - 1)
        assert sum(r["reason"] == DM.DPT_STORED for r in got) == sum(r["reason"] == DM.DPT_DUPLICATE for r in got)
        assert all(got[k + 1]["reason"] == DM.DPT_DUPLICATE for k, r in enumerate(got) if r["reason"] == DM.DPT_STORED)


def walk_parity(dev, setup, seed_herd):
    """the same herd twice: WALK_LAUNCHES launches of bsgs_kangaroo_run, then of bsgs_kangaroo_run_dptable.  The non-dead records of the first, as a multiset of
    (tag, d, kangaroo, type), are the table's entries plus the hand-backs of the second; the dead records are equal as sets; every pair names an entry of the
    table with the record's tag."""
    setup()
    seed_herd()
    plain = []
    for _ in range(WALK_LAUNCHES):
        recs, dropped, _ = dev.kangaroo_run(WALK_STEPS)
        assert dropped == 0 and 0 < len(recs) < WALK_CAP
        plain += recs
    end_plain = dev.kangaroo_download(0, WALK_HERD)
    setup()
    seed_herd()
    dev.kangaroo_dptable_begin(1 << 15)
    back, seen_all = [], 0
    for _ in range(WALK_LAUNCHES):
        got, seen, n_entries, dropped, ms = dev.kangaroo_run_dptable(WALK_STEPS)
        assert dropped == 0 and ms > 0
        seen_all += seen
        back += got
    assert seen_all == len(plain) and dev.kangaroo_download(0, WALK_HERD) == end_plain      # the walk is the walk
    table = dev.kangaroo_dptable_read()
    assert n_entries == len(table) == len({e[0] for e in table})
    key = lambda r: (r["x"] & DM.M64, r["d"], r["kangaroo"], DM.type_of(r["flags"]))
    walk_back = [r for r in back if r["reason"] != DM.DPT_STORED]
    live_back = [r for r in walk_back if r["reason"] != DM.DPT_DEAD]
    assert all(r["flags"] & K.DEAD for r in walk_back if r["reason"] == DM.DPT_DEAD) and not any(r["flags"] & K.DEAD for r in live_back)
    assert Counter(key(r) for r in plain if not r["flags"] & K.DEAD) == Counter(table) + Counter(key(r) for r in live_back)
    full = lambda r: (r["x"], r["d"], r["kangaroo"], r["flags"], r["step"])
    assert {full(r) for r in plain if r["flags"] & K.DEAD} == {full(r) for r in walk_back if r["reason"] == DM.DPT_DEAD}
    by_full = {full(r) for r in plain}
    assert all(full(r) in by_full for r in walk_back)                 # the records as the walk wrote them
    held = {e[0]: e for e in table}
    n_pairs = 0
    for k, r in enumerate(back):
        if r["reason"] == DM.DPT_STORED:
            w = back[k + 1]
            assert w["reason"] == DM.DPT_DUPLICATE and w["x"] & DM.M64 == r["x"] and held[r["x"]] == (r["x"], r["d"], r["kangaroo"], r["flags"])
            n_pairs += 1
    assert n_pairs == sum(r["reason"] == DM.DPT_DUPLICATE for r in back)
    assert {r["reason"] for r in back} <= {DM.DPT_STORED, DM.DPT_DUPLICATE, DM.DPT_DEAD}
    return back, table


def test_walk_parity_plain(dev, jump_table):
    scalars, jumps = jump_table
    rng = K.Stream(21)
    q = 0x1234567 + (1 << 39)
    Q = K.start(None, q, False)
    offsets = [1 + rng.u128() % ((1 << 40) - 1) for _ in range(WALK_HERD // 2)] + [K.signed128(rng.u128()) % (1 << 40) - (1 << 39) for _ in range(WALK_HERD // 2)]
    flags = [0] * (WALK_HERD // 2) + [K.WILD] * (WALK_HERD // 2)
    offsets[300] = offsets[17]                                        # two tame kangaroos on one start: every record of theirs comes twice, same type
    offsets[WALK_HERD // 2 + 5] = offsets[40] - q                     # a wild one on a tame one's start: equal points of different type
    back, table = walk_parity(dev, lambda: dev.kangaroo_setup(jumps, scalars, WALK_DP, WALK_HERD, 4, WALK_CAP),
                              lambda: dev.kangaroo_seed(Q, offsets, flags))
    pairs = [(back[k], back[k + 1]) for k, r in enumerate(back) if r["reason"] == DM.DPT_STORED]
    assert {frozenset((st["kangaroo"], w["kangaroo"])) for st, w in pairs} >= {frozenset((17, 300)), frozenset((40, WALK_HERD // 2 + 5))}
    mixed = [(st, w) for st, w in pairs if {st["kangaroo"], w["kangaroo"]} == {40, WALK_HERD // 2 + 5}]
    assert all({st["flags"], DM.type_of(w["flags"])} == {0, 1} for st, w in mixed)
    for st, w in mixed:                                               # and the pair solves for q by the host's rule: d_T - d_W
        dt, dw = (st["d"], w["d"]) if st["flags"] == 0 else (w["d"], st["d"])
        assert K.signed128(dt - dw) == q


def test_walk_parity_symmetric(dev):
    scalars, jumps, cyc, _, _ = S.short_cycle_case(3, 64)             # a jump table with a 2-cycle the last-jump rule does not prevent, and a start on it
    rng = K.Stream(22)
    q = 0x7654321 + (1 << 38)
    Q = K.start(None, q, False)
    offsets = [1 + rng.u128() % ((1 << 39) - 1) for _ in range(WALK_HERD // 2)] + [K.signed128(rng.u128()) % (1 << 39) - (1 << 38) for _ in range(WALK_HERD // 2)]
    flags = [0] * (WALK_HERD // 2) + [K.WILD] * (WALK_HERD // 2)
    offsets[WALK_HERD // 2 + 9] = -offsets[60] - q                    # a wild kangaroo on the NEGATIVE of a tame one's start: one class, so equal records

    def seed_herd():
        dev.kangaroo_seed(Q, offsets, flags)
        dev.kangaroo_upload_list([7], [cyc])

    back, table = walk_parity(dev, lambda: dev.kangaroo_setup_sym(jumps, scalars, WALK_DP, WALK_HERD, 4, WALK_CAP), seed_herd)
    assert any(r["reason"] == DM.DPT_DEAD and r["flags"] & S.CYCLE and r["kangaroo"] == 7 for r in back)      # the cycle check's record came back, never stored
    pairs = [(back[k], back[k + 1]) for k, r in enumerate(back) if r["reason"] == DM.DPT_STORED]
    mixed = [(st, w) for st, w in pairs if {st["kangaroo"], w["kangaroo"]} == {60, WALK_HERD // 2 + 9}]
    assert mixed and all({st["flags"], DM.type_of(w["flags"])} <= {0, 1, 3} and st["flags"] != DM.type_of(w["flags"]) for st, w in mixed)
    assert {e[3] for e in table} == {0, 1, 3}                         # tame, wild and wild with NEG all live in the table


def test_states(jump_table):
    import pybsgs
    scalars, jumps = jump_table
    d = pybsgs.Device(0)
    try:
        for call in (lambda: d.kangaroo_run_dptable(1), d.kangaroo_dptable_read, lambda: d.kangaroo_dptable_begin(64), lambda: d.kangaroo_dptable_load([])):
            with pytest.raises(pybsgs.BsgsError, match="error -3: bsgs_kangaroo_setup first"):
                call()
        d.kangaroo_dptable_end()                                      # no herd, no table: not an error
        d.kangaroo_setup(jumps, scalars, 0, 64, 1, 64)
        for call in (lambda: d.kangaroo_run_dptable(1), d.kangaroo_dptable_read, lambda: d.kangaroo_dptable_insert([(1, 1, 0)]), lambda: d.kangaroo_dptable_load([])):
            with pytest.raises(pybsgs.BsgsError, match="error -3: bsgs_kangaroo_dptable_begin first"):
                call()
        for capacity in (0, (1 << 31) + 1):
            with pytest.raises(pybsgs.BsgsError, match="error -1: .*1..2\\^31"):
                d.kangaroo_dptable_begin(capacity)
        d.kangaroo_dptable_begin(64)
        with pytest.raises(pybsgs.BsgsError, match="error -1: .*record capacity"):
            d.kangaroo_dptable_insert([(k + 1, 1, 0) for k in range(65)])
        back, n, dropped = d.kangaroo_dptable_insert([(5, 1, 0), (6, 2, 1), (5, 3, 1)])
        assert n == 2 and dropped == 0 and [r["reason"] for r in back] == [DM.DPT_STORED, DM.DPT_DUPLICATE]
        assert {(back[0]["d"], back[0]["kangaroo"], back[0]["flags"]), (back[1]["d"], back[1]["kangaroo"], back[1]["flags"])} == {(1, 0, 0), (3, 2, 1)}
        with pytest.raises(pybsgs.BsgsError, match="error -1: room for 1 entries, the table holds 2"):
            d.kangaroo_dptable_read(max_entries=1)
        assert len(d.kangaroo_dptable_read()) == 2
        # the growing tame table is another table: both live under one herd, and the plain launch behaves as before
        d.kangaroo_tames_gen_begin(64)
        assert d.kangaroo_tames_gen_insert([(5, 1, 0)]) == ([], 1)
        assert len(d.kangaroo_dptable_read()) == 2
        states = [(p[0], p[1], t, 0) for t in range(1, 65) for p in [K.start(None, t, False)]]
        want_states, recs = K.walk(states, jumps, scalars, 2, 0)
        d.kangaroo_upload(0, states)
        plain, dropped, _ = d.kangaroo_run(2)
        assert len(plain) == 64 and dropped == 64 and d.kangaroo_download(0, 64) == want_states
        assert len(d.kangaroo_dptable_read()) == 2
        # more records than the record buffer holds: the rest is counted as dropped, nothing of it is inserted
        d.kangaroo_upload(0, states)
        got, seen, n_entries, dropped, _ = d.kangaroo_run_dptable(2)
        assert seen == 128 and dropped == 64 and n_entries + sum(r["reason"] != DM.DPT_STORED for r in got) == 2 + 64
        d.kangaroo_dptable_begin(128)                                 # a second begin replaces the table
        assert d.kangaroo_dptable_read() == []
        d.kangaroo_dptable_end()
        d.kangaroo_dptable_end()                                      # twice is fine
        with pytest.raises(pybsgs.BsgsError, match="bsgs_kangaroo_dptable_begin first"):
            d.kangaroo_dptable_read()
        d.kangaroo_dptable_begin(64)
        d.kangaroo_setup(jumps, scalars, 0, 64, 1, 64)               # a new herd drops the table
        with pytest.raises(pybsgs.BsgsError, match="bsgs_kangaroo_dptable_begin first"):
            d.kangaroo_run_dptable(1)
        d.kangaroo_setup_sym(jumps, scalars, 0, 64, 1, 64)           # the symmetric herd takes one too
        d.kangaroo_dptable_begin(64)
        d.kangaroo_setup_sym_keys(jumps, scalars, 0, 64, 1, 64)      # the keyed herd is refused
        with pytest.raises(pybsgs.BsgsError, match="error -3: a distinguished-point table serves the herds"):
            d.kangaroo_dptable_begin(64)
    finally:
        d.close()
