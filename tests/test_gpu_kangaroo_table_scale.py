"""GPU: the kangaroo tables in device memory at launch sizes where every wave strides (tests/kangaroo_table_scale_cases.py has the shapes, the set reference
and the checks; tests/test_kangaroo_table_scale_model.py pins them on the CPU).  524325 crafted records a launch -- two full iterations of the 1024 x 256
grid and a ragged third -- through bsgs_kangaroo_tames_gen_insert and bsgs_kangaroo_dptable_insert into tables of 2^21 slots: tags that occur 2 .. 4096
times at random positions of the whole launch, one tag in a whole wave and in lane 5 of 512 waves, chains of 4096 and 2048 tags with one home slot, tag 0
and DEAD; the same launch again (the hand-back buffer of the distinguished-point table at its bound), a fresh and a mixed one; loads of two staged chunks;
and behind a walk of 8192 kangaroos that writes 270336 records a launch: both inserts, the tame-table match and the keyed match against what
bsgs_kangaroo_run returns for the same herd.  No launch here comes near a full table: FULL stays tested at the small sizes of the tables' own files."""
import time

import numpy as np
import pytest

import kangaroo_model as K
import kangaroo_sym_model as S
import kangaroo_table_scale_cases as SC
from pybsgs.ecpy import P, add, mul, neg

pytestmark = pytest.mark.gpu

U64 = np.dtype("<u8")


@pytest.fixture(scope="module")
def case():
    return SC.scale_case()                                            # asserts load <= 70 % and chains <= 4096 on the CPU, before any device call


@pytest.fixture(scope="module")
def jump_table():
    """64 jump points, one of them at the index its own x selects: a kangaroo that stands on its negative dies at the next step"""
    scalars, jumps = K.jump_table(K.Stream(11), 1 << 30)
    j = jumps[0][0] & 63
    scalars[0], scalars[j], jumps[0], jumps[j] = scalars[j], scalars[0], jumps[j], jumps[0]
    assert jumps[j][0] & 63 == j
    return scalars, jumps, j


@pytest.fixture
def dev(jump_table):
    import pybsgs
    d = pybsgs.Device(0)
    scalars, jumps, _ = jump_table
    d.kangaroo_setup(jumps, scalars, 0, SC.HERD, 1, SC.CAP)          # the herd never walks here: it lends its record buffers
    yield d
    d.close()


def read_gen(dev):
    tags, d = dev.kangaroo_tames_gen_read(raw=True)
    return SC.pair_rows(np.frombuffer(tags, U64), np.frombuffer(d, U64))


def read_dpt(dev):
    return SC.entry_rows(SC.from_bytes(dev.kangaroo_dptable_read(raw=True), SC.DP_ENTRY))


def by_tag(table):
    return table[np.argsort(table[:, 0], kind="stable")]


def gen_launch(dev, ref, recs, before, insert):
    """one launch on the growing tame table, by `insert` -> (handed-back bytes, n_entries); judged, with both reads -> the table's rows"""
    back, n_entries = insert()
    back = SC.from_bytes(back)
    table = read_gen(dev)
    SC.check_launch(ref, recs, back, n_entries, table, before)
    (tags, d), n = dev.kangaroo_tames_gen_read_sorted(raw=True)
    assert n == ref["entries"]
    SC.check_sorted(np.frombuffer(tags, U64), np.frombuffer(d, U64), table)
    return table


def dpt_launch(dev, ref, recs, before, insert):
    """one launch on the distinguished-point table, by `insert` -> (hand-back bytes, n_entries, dropped); judged -> the table's rows"""
    got, n_entries, dropped = insert()
    got = SC.from_bytes(got)
    assert dropped == 0
    n_dup = int((ref["back"][:, 1] == SC.R_DUPLICATE).sum())
    assert len(got) == len(ref["back"]) + n_dup, "places = records handed back + duplicates"
    walk, stored, dup = SC.split_pairs(got)
    table = read_dpt(dev)
    SC.check_launch(ref, recs, walk, n_entries, table, before)
    SC.check_pairs(stored, dup, table)
    return table


def test_tames_gen_insert_at_scale(dev, case):
    dev.kangaroo_tames_gen_begin(SC.CAPACITY)
    before = None
    for (name, recs), ref in zip(case["launches"], case["refs"]):
        t0 = time.perf_counter()
        table = gen_launch(dev, ref, recs, before, lambda: dev.kangaroo_tames_gen_insert(recs.tobytes(), raw=True))
        if name == "again":
            assert np.array_equal(by_tag(table), by_tag(before))     # every record handed back, the table what it was
        print("tames_gen", name, "entries", ref["entries"], "handed back", len(ref["back"]), "load %.3f" % ref["load"], "%.2f s" % (time.perf_counter() - t0))
        before = table


def test_dptable_insert_at_scale(dev, case):
    dev.kangaroo_dptable_begin(SC.CAPACITY)
    before = None
    for (name, recs), ref in zip(case["launches"], case["refs"]):
        t0 = time.perf_counter()
        table = dpt_launch(dev, ref, recs, before, lambda: dev.kangaroo_dptable_insert(recs.tobytes(), raw=True))
        if name == "again":                                           # the hand-back buffer at its bound: two places for every record but the single-place ones
            assert len(ref["back"]) == SC.N1 and 2 * SC.N1 - (SC.N_DEAD + SC.N_ZERO) > SC.CAP
            assert np.array_equal(by_tag(table), by_tag(before))
        print("dptable", name, "entries", ref["entries"], "handed back", len(ref["back"]), "load %.3f" % ref["load"], "%.2f s" % (time.perf_counter() - t0))
        before = table


def test_dptable_hand_back_buffer_exactly_full(dev):
    """every record of a full launch a duplicate: 2 x cap places, the last pair ends at the last place of the buffer"""
    rng = np.random.default_rng(7)
    recs = SC.fresh_launch(rng, SC.CAP, 5)
    ref = SC.reference(np.zeros(0, np.uint64), recs)
    SC.assert_far_from_full(ref["tags"], SC.SLOTS)
    dev.kangaroo_dptable_begin(SC.CAPACITY)
    before = dpt_launch(dev, ref, recs, None, lambda: dev.kangaroo_dptable_insert(recs.tobytes(), raw=True))
    again = SC.reference(ref["tags"], recs)
    assert len(again["back"]) == SC.CAP and (again["back"][:, 1] == SC.R_DUPLICATE).all()
    got, n_entries, dropped = dev.kangaroo_dptable_insert(recs.tobytes(), raw=True)
    assert len(got) == 64 * 2 * SC.CAP and dropped == 0
    walk, stored, dup = SC.split_pairs(SC.from_bytes(got))
    table = read_dpt(dev)
    SC.check_launch(again, recs, walk, n_entries, table, before)
    SC.check_pairs(stored, dup, table)
    assert np.array_equal(by_tag(table), by_tag(before))


@pytest.mark.parametrize("which", ["tames_gen", "dptable"])
def test_load_in_two_chunks(dev, case, which):
    e = case["entries"]
    if which == "tames_gen":
        dev.kangaroo_tames_gen_begin(SC.CAPACITY)
        out = dev.kangaroo_tames_gen_load(e["tag"].tobytes(), np.ascontiguousarray(e["d"]).tobytes())
        table = read_gen(dev)
    else:
        dev.kangaroo_dptable_begin(SC.CAPACITY)
        out = dev.kangaroo_dptable_load(e.tobytes())
        table = read_dpt(dev)
    SC.check_loaded(out[:4], out[4], table, case["load_counts"], case["load_tags"], e)


def as_dicts(raw, last="reason"):
    """the bytes of records as the default forms of the wrappers give them; an "entry" word is the entry number + 1, 0 for none"""
    r = SC.from_bytes(raw)
    word = (lambda v: v - 1 if v else None) if last == "entry" else (lambda v: v)
    return [{"x": sum(int(w) << (64 * k) for k, w in enumerate(r["x"][i])), "d": int(r["d"][i, 0]) | int(r["d"][i, 1]) << 64, "kangaroo": int(r["kangaroo"][i]),
             "flags": int(r["flags"][i]), "step": int(r["step"][i]), last: word(int(r["reserved"][i]))} for i in range(len(r))]


def canon(dicts):
    return sorted(sorted((k, -1 if v is None else v) for k, v in d.items()) for d in dicts)


def test_the_raw_forms_say_what_the_default_forms_say(jump_table):
    """a small herd, each call in both forms from the same state: the same records (in any order) and the same counts"""
    import pybsgs
    scalars, jumps, _ = jump_table
    n, cap, steps = 64, 1024, 6
    rng = K.Stream(5)
    states = [(p[0], p[1], t, K.WILD if k & 1 else 0) for k in range(n) for t in [1 + rng.u64()] for p in [K.start(None, t, False)]]
    states[9] = states[3]                                             # every record of these two twice
    d = pybsgs.Device(0)
    try:
        d.kangaroo_setup(jumps, scalars, 0, n, 1, cap)

        def both(call, last, drop=()):
            """-> the records of the default form, which the raw form's equal as a multiset, as the counts behind them do (the last is the kernel's time)"""
            d.kangaroo_upload(0, states)
            a = call(False)
            d.kangaroo_upload(0, states)
            b = call(True)
            less = lambda recs: canon([{k: v for k, v in r.items() if k not in drop} for r in recs])
            assert less(a[0]) == less(as_dicts(b[0], last)) and a[1:-1] == b[1:-1] and len(a[0]) > 0
            return a[0]

        plain = both(lambda raw: d.kangaroo_run(steps, raw=raw), "key")
        assert len(plain) == n * steps
        d.kangaroo_tames_install(sorted({r["x"] & ((1 << 64) - 1) for r in plain})[::2])
        assert len(both(lambda raw: d.kangaroo_run_tames(steps, raw=raw), "entry")) >= n * steps // 2
        for begin, run in ((d.kangaroo_tames_gen_begin, d.kangaroo_run_tames_gen), (d.kangaroo_dptable_begin, d.kangaroo_run_dptable)):
            def call(raw):
                begin(4096)
                return run(steps, raw=raw)
            assert len(both(call, "reason", drop=("kangaroo",))) >= steps      # which of kangaroos 3 and 9 is stored may differ between two runs
        # the inserts alone: the default form builds the records from (x, d, flags, kangaroo), the raw form takes them as they are.  Which copy of a tag is
        # stored may differ between two runs, so the hand-backs are compared by tag and reason
        recs = SC.make_records(np.random.default_rng(3), np.array([5, 6, 5, 0, 7, 6, 5], np.uint64), np.array([0, 1, 3, 0, SC.DEAD, 1, 1], np.uint32), 9)
        tup = [(int(r["x"][0]) | int(r["x"][1]) << 64 | int(r["x"][2]) << 128 | int(r["x"][3]) << 192, int(r["d"][0]) | int(r["d"][1]) << 64, int(r["flags"]),
                int(r["kangaroo"])) for r in recs]
        for begin, insert, read in ((d.kangaroo_tames_gen_begin, d.kangaroo_tames_gen_insert, d.kangaroo_tames_gen_read),
                                    (d.kangaroo_dptable_begin, d.kangaroo_dptable_insert, d.kangaroo_dptable_read)):
            begin(64)
            a = insert(tup)
            begin(64)
            b = insert(recs.tobytes(), raw=True)
            mine = as_dicts(b[0])
            assert a[1:] == b[1:] and len(a[0]) == len(mine) >= 5
            assert sorted((r["x"] & ((1 << 64) - 1), r["reason"]) for r in a[0]) == sorted((r["x"] & ((1 << 64) - 1), r["reason"]) for r in mine)
            assert sorted(e[0] for e in read()) == [5, 6]
        tags, dd = d.kangaroo_tames_gen_read(raw=True)
        pairs = zip(np.frombuffer(tags, U64).tolist(), [int(v[0]) | int(v[1]) << 64 for v in np.frombuffer(dd, U64).reshape(-1, 2)])
        assert sorted(pairs) == sorted(d.kangaroo_tames_gen_read())
        with pytest.raises(pybsgs.BsgsError, match="no multiple of 64"):
            d.kangaroo_tames_gen_insert(b"\0" * 65, raw=True)
    finally:
        d.close()


# ---- behind the walk -------------------------------------------------------------------------------------------------------------------------------------------
WALK_DEAD = (5, 4100, 8191)                                           # kangaroos on -J_j


@pytest.fixture(scope="module")
def walked(jump_table):
    """the plain herd of 8192 and the records of its first two launches as bsgs_kangaroo_run returns them (that path is checked against the Python model at
    small sizes): the reference of everything behind the walk.  Kangaroo 300 starts where 17 does (every record twice in a launch), 5000 where 40 stands after
    the first launch (its records of the first launch are 40's of the second: across launches), and three stand on -J_j (DEAD at step 0)."""
    import pybsgs
    scalars, jumps, j = jump_table
    n = SC.WALK_HERD
    rng = K.Stream(31)
    Q = K.start(None, 0x1234567 + (1 << 39), False)
    offsets = [1 + rng.u128() % ((1 << 40) - 1) for _ in range(n // 2)] + [K.signed128(rng.u128()) % (1 << 40) - (1 << 39) for _ in range(n // 2)]
    d = pybsgs.Device(0)
    try:
        d.kangaroo_setup(jumps, scalars, 0, n, SC.WALK_PER_THREAD, SC.WALK_CAP)
        assert d.kangaroo_geometry() == (n // 2, 2, 256)
        assert d.kangaroo_seed(Q, offsets, [0] * (n // 2) + [K.WILD] * (n // 2)) == (0, 0)
        states = d.kangaroo_download(0, n)
        states[300] = states[17]
        states[5000] = K.walk([states[40]], jumps, scalars, SC.WALK_STEPS, 0)[0][0]
        for i, k in enumerate(WALK_DEAD):
            states[k] = (jumps[j][0], P - jumps[j][1], 1000 + i, K.WILD if i else 0)
        d.kangaroo_upload(0, states)
        launches = []
        for _ in range(2):
            recs, dropped, _ = d.kangaroo_run(SC.WALK_STEPS, raw=True)
            assert dropped == 0
            launches.append(SC.from_bytes(recs))
    finally:
        d.close()
    first, second = launches
    n_first = n * SC.WALK_STEPS - len(WALK_DEAD) * (SC.WALK_STEPS - 1)
    assert len(first) == n_first > SC.INSERT_GRID_MAX * SC.BLOCK and n_first % 64     # a second iteration for the first waves, and a ragged wave
    assert len(second) == (n - len(WALK_DEAD)) * SC.WALK_STEPS > SC.INSERT_GRID_MAX * SC.BLOCK
    assert ((first["flags"] & SC.DEAD) != 0).sum() == len(WALK_DEAD) and not first["reserved"].any()
    return {"states": states, "launches": launches}


@pytest.fixture
def walk_dev(jump_table, walked):
    import pybsgs
    d = pybsgs.Device(0)
    scalars, jumps, _ = jump_table
    d.kangaroo_setup(jumps, scalars, 0, SC.WALK_HERD, SC.WALK_PER_THREAD, SC.WALK_CAP)
    d.kangaroo_upload(0, walked["states"])
    yield d
    d.close()


@pytest.mark.parametrize("which", ["tames_gen", "dptable"])
def test_insert_behind_the_walk(walk_dev, walked, which):
    dev = walk_dev
    slots = SC.n_slots(SC.CAPACITY, SC.WALK_CAP)
    (dev.kangaroo_tames_gen_begin if which == "tames_gen" else dev.kangaroo_dptable_begin)(SC.CAPACITY)
    held, before = np.zeros(0, np.uint64), None
    for k, recs in enumerate(walked["launches"]):
        ref = SC.reference(held, recs)
        SC.assert_far_from_full(ref["tags"], slots)
        n_dup = int((ref["back"][:, 1] == SC.R_DUPLICATE).sum())
        assert n_dup >= SC.WALK_STEPS and (k == 0 or len(ref["new_tags"]) < len(np.unique(recs["x"][:, 0])))      # the second launch meets the first's entries
        seen = []

        def insert():
            if which == "tames_gen":
                got, n_seen, n_entries, dropped, ms = dev.kangaroo_run_tames_gen(SC.WALK_STEPS, raw=True)
                assert dropped == 0 and ms > 0
                seen.append(n_seen)
                return got, n_entries
            got, n_seen, n_entries, dropped, ms = dev.kangaroo_run_dptable(SC.WALK_STEPS, raw=True)
            assert ms > 0
            seen.append(n_seen)
            return got, n_entries, dropped

        before = (gen_launch if which == "tames_gen" else dpt_launch)(dev, ref, recs, before, insert)
        assert seen == [len(recs)]
        held = ref["tags"]


def test_match_behind_the_walk(walk_dev, walked):
    dev = walk_dev
    recs = walked["launches"][0]
    table = np.unique(recs["x"][:, 0])[::3]                           # every third tag, entries in ascending order
    keep, word = SC.reference_match(recs, table)
    want = recs[keep].copy()
    want["reserved"] = word
    assert len(recs) // 4 < len(want) < len(recs) // 2 and (word == 0).sum() <= len(WALK_DEAD)
    dev.kangaroo_tames_install(table.tolist())
    got, seen, dropped, ms = dev.kangaroo_run_tames(SC.WALK_STEPS, raw=True)
    assert seen == len(recs) and dropped == 0 and ms > 0
    assert np.array_equal(SC.sorted_words(SC.from_bytes(got)), SC.sorted_words(want))


def test_keyed_match_behind_the_walk():
    """the herd of bsgs_kangaroo_setup_sym_keys: the kept records are the walk's own in all 64 bytes -- the key word untouched -- and the parallel entry words
    name the right entries"""
    import pybsgs
    n, A, W = SC.WALK_HERD, 0x5A5A5A << 40, 1 << 40
    keys = [A + 0x1234567890, A + 0xFEDCBA9876, A + 7]
    nmid = neg(mul(A + W // 2))
    Qs = [add(mul(k), nmid) for k in keys]
    scalars, jumps = S.jump_table(K.Stream(901), n * (W ** 0.5) / 4, 64)
    rng = K.Stream(4001)
    wild = [i >= n // 2 for i in range(n)]
    key_of = [(i - n // 2) % len(keys) if w else 0 for i, w in enumerate(wild)]
    offs = [S.herd_offset(rng, W, w) for w in wild]
    d = pybsgs.Device(0)
    try:
        d.kangaroo_setup_sym_keys(jumps, scalars, 0, n, SC.WALK_PER_THREAD, SC.WALK_CAP)
        d.kangaroo_set_keys(Qs)
        assert d.kangaroo_seed_keys(offs, [K.WILD if w else 0 for w in wild], key_of) == (0, 0)
        states = d.kangaroo_download(0, n)
        recs, dropped, _ = d.kangaroo_run(SC.WALK_STEPS, raw=True)
        recs = SC.from_bytes(recs)
        assert dropped == 0 and SC.INSERT_GRID_MAX * SC.BLOCK < len(recs) <= SC.WALK_CAP
        assert set(np.unique(recs["reserved"]).tolist()) == {0, 1, 2}                # the key word of the records
        table = np.unique(recs["x"][:, 0])[::3]
        keep, word = SC.reference_match(recs, table)
        d.kangaroo_upload(0, states)
        d.kangaroo_tames_install_keys(table.tolist())
        (got, ent), seen, dropped, ms = d.kangaroo_run_tames_keys(SC.WALK_STEPS, raw=True)
        got, ent = SC.from_bytes(got), np.frombuffer(ent, "<u4")
        assert seen == len(recs) and dropped == 0 and ms > 0 and len(got) == len(ent) == keep.sum() > len(recs) // 4
        assert np.array_equal(SC.sorted_words(got, ent), SC.sorted_words(recs[keep], word))
    finally:
        d.close()
