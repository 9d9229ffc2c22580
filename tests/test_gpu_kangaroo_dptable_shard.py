"""GPU: the distinguished-point table divided over engines (csrc/kangaroo_dptable_shard.hip) against its model (tests/kangaroo_dptable_shard_model.py) and the
model of the one table (tests/kangaroo_dptable_model.py), through pybsgs, at the smallest shapes at which the routing can go wrong: every destination in one
wave; one foreign record per wave and one own record per wave; one destination only and none; a launch of 524325 records in which every wave strides, with
duplicates, DEAD records and tag-0 records; an outbox that does not fit the caller's buffer; the state errors; and two engines on one GPU whose launches a
relay in the test carries to each other."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import kangaroo_model as K
import kangaroo_dptable_model as DM
import kangaroo_dptable_shard_model as SM
import kangaroo_table_scale_cases as SC

pytestmark = pytest.mark.gpu

CAP, CAPACITY = 4096, 8192                                           # the small cases: 64 waves of records at most, a table of 2^15 slots


@pytest.fixture(scope="module")
def jump_table():
    return K.jump_table(K.Stream(11), 1 << 30)


@pytest.fixture(scope="module")
def dev(jump_table):
    import pybsgs
    d = pybsgs.Device(0)
    scalars, jumps = jump_table
    d.kangaroo_setup(jumps, scalars, 0, 64, 1, CAP)
    yield d
    d.close()


def tags_of_shard(rng, s, shards, n):
    """n different tags of shard s, their 16 shard bits spread over the shard's whole range"""
    lo, hi = -(-s * 65536 // shards), -(-(s + 1) * 65536 // shards)
    t = (rng.integers(lo, hi, size=2 * n + 8, dtype=np.uint64) << np.uint64(48)) | rng.integers(1, 1 << 48, size=2 * n + 8, dtype=np.uint64)
    t = rng.permutation(np.unique(t))[:n]
    assert len(t) == n and all(SM.shard(int(v), shards) == s for v in t[:64])
    return t


def shard_of(tags, shards):
    return ((np.asarray(tags, np.uint64) >> np.uint64(48)) * np.uint64(shards)) >> np.uint64(16)


def model_records(r):
    """REC array -> the model's (tag, d, flags, kangaroo)"""
    return list(zip(r["x"][:, 0].tolist(), [lo | hi << 64 for lo, hi in r["d"].tolist()], r["flags"].tolist(), r["kangaroo"].tolist()))


def as_dicts(got):
    """hand-backs (REC) as pybsgs lists them; x cut to the tag, which is all the model knows of it (the upper words are compared in check_verbatim)"""
    return [{"x": x, "d": lo | hi << 64, "kangaroo": k, "flags": f, "step": s, "reason": w}
            for x, (lo, hi), k, f, s, w in zip(got["x"][:, 0].tolist(), got["d"].tolist(), got["kangaroo"].tolist(), got["flags"].tolist(), got["step"].tolist(),
                                               got["reserved"].tolist())]


def check_verbatim(back, sent):
    """the walk's records among the hand-backs are sent records in all 64 bytes but the reason word, none twice"""
    walk = back[back["reserved"] != SC.R_STORED].copy()
    walk["reserved"] = 0
    clean = sent.copy()
    clean["reserved"] = 0
    have = Counter(map(bytes, SC.sorted_words(clean).astype("<u4")))
    came = Counter(map(bytes, SC.sorted_words(walk).astype("<u4")))
    assert not came - have, "a handed-back record is a sent one, and none comes twice"


def check_call(table, recs, out, own, shards, base=0):
    """one call's answer (hand-backs, groups, n_entries, dropped; raw) for the records `recs` (REC, local ids) on shard `own`, against the rule:
      every record is exactly one of stored, handed back or routed; each group holds exactly the records of its shard, verbatim but for kangaroo = base +
      local; the hand-backs pass check_device of the one table's model, fed the shard's own records with global ids; n_entries is right.
    -> the model's new table"""
    back, groups, n_entries, dropped = out
    back, groups = SC.from_bytes(back), [SC.from_bytes(g) for g in groups]
    assert dropped == 0 and len(groups) == shards and len(groups[own]) == 0
    sent = recs.copy()
    sent["kangaroo"] += np.uint32(base)
    live = ((sent["flags"] & SC.DEAD) == 0) & (sent["x"][:, 0] != 0)
    to = np.where(live, shard_of(sent["x"][:, 0], shards), own)
    for s in range(shards):
        assert np.array_equal(SC.sorted_words(groups[s]), SC.sorted_words(sent[to == s])) or s == own, "group %d: exactly its records, as they came" % s
    mine = sent[to == own]
    new, pairs = DM.check_device(table, model_records(mine), as_dicts(back), n_entries)
    check_verbatim(back, mine)
    n_back = int((back["reserved"] != SC.R_STORED).sum())
    assert (DM.entries(new) - DM.entries(table)) + n_back + sum(map(len, groups)) == len(recs)      # stored, handed back or routed: each exactly once
    return new


def begin(dev, own, shards, base=0, capacity=CAPACITY, cap=CAP):
    dev.kangaroo_dptable_begin_shard(capacity, own, shards, base)
    return DM.new_table(capacity, cap)


def check_read(dev, table):
    got = dev.kangaroo_dptable_read()
    assert len(got) == len({e[0] for e in got}) == DM.entries(table) and {e[0] for e in got} == set(table["cand"])
    assert all(e in table["cand"][e[0]] for e in got)
    return got


# ---- 1. every destination in one wave ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("own", [0, 5, 15])
def test_every_destination_in_one_wave(dev, own):
    rng = np.random.default_rng(1)
    per = [tags_of_shard(rng, s, 16, 4) for s in range(16)]
    tags = np.array([per[l % 16][l // 16] for l in range(64)], np.uint64)      # lane l is bound for shard l mod 16
    recs = SC.make_records(rng, tags, rng.choice(SC.FLAG_CHOICES, size=64), 1)
    table = begin(dev, own, 16)
    out = dev.kangaroo_dptable_insert_shard(recs.tobytes(), raw=True)
    table = check_call(table, recs, out, own, 16)
    assert [len(g) // 64 for g in out[1]] == [0 if s == own else 4 for s in range(16)] and out[2] == 4
    assert {e[2] for e in check_read(dev, table)} == {recs["kangaroo"][l] for l in range(64) if l % 16 == own}


# ---- 2. one foreign record per wave, and one own record per wave ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lone", ["foreign", "own"])
def test_one_record_per_wave_differs(dev, lone):
    """64 waves of 64 records in one launch; in wave w the record at lane w is of another kind than the other 63"""
    rng = np.random.default_rng(2)
    own, shards = 1, 3
    mine, other = tags_of_shard(rng, own, shards, 4096), [tags_of_shard(rng, 0, shards, 4096), tags_of_shard(rng, 2, shards, 4096)]
    at = np.arange(64) * 64 + np.arange(64)                           # lane w of wave w
    diag = np.zeros(4096, bool)
    diag[at] = True
    foreign = diag if lone == "foreign" else ~diag
    dest = np.where((np.arange(4096) // 64) % 2 == 0, 0, 1)           # even waves route to shard 0, odd waves to shard 2 ...
    if lone == "own":
        dest = (np.arange(4096) + np.arange(4096) // 64) % 2          # ... and where all but one are foreign both destinations stand in every wave
    tags = np.where(foreign, np.where(dest == 0, other[0], other[1]), mine)
    recs = SC.make_records(rng, tags, rng.choice(SC.FLAG_CHOICES, size=4096), 2)
    table = begin(dev, own, shards)
    out = dev.kangaroo_dptable_insert_shard(recs.tobytes(), raw=True)
    table = check_call(table, recs, out, own, shards)
    n_foreign = 64 if lone == "foreign" else 4096 - 64
    assert sum(len(g) for g in out[1]) // 64 == n_foreign and out[2] == 4096 - n_foreign and len(out[0]) == 0
    if lone == "foreign":
        assert [len(g) // 64 for g in out[1]] == [32, 0, 32]
    check_read(dev, table)


# ---- 3. one destination only, and none ---------------------------------------------------------------------------------------------------------------------
def test_all_to_one_destination_and_all_own(dev):
    rng = np.random.default_rng(3)
    own, shards = 2, 5
    table = begin(dev, own, shards)
    n = 1000                                                          # 15 waves and 40 lanes
    for to in (4, own, 0):
        recs = SC.make_records(rng, tags_of_shard(rng, to, shards, n), rng.choice(SC.FLAG_CHOICES, size=n), 3 + to)
        out = dev.kangaroo_dptable_insert_shard(recs.tobytes(), raw=True)
        table = check_call(table, recs, out, own, shards)
        assert [len(g) // 64 for g in out[1]] == [n if s == to and to != own else 0 for s in range(shards)]
        assert out[2] == DM.entries(table) == (n if to in (own, 0) else 0)
    check_read(dev, table)


# ---- 4. every wave strides -------------------------------------------------------------------------------------------------------------------------------------
def striding_launch(rng, own, shards):
    """N1 records of random tags, so a third for every shard of three, with copies planted at random positions for every shard alike: 48 tags twice, 8
    tags three times, one tag in all lanes of a wave, one tag in lane 5 of 512 waves; 1000 tag-0 records (tag 0 names shard 0) and 1000 DEAD records, some
    with CYCLE, on tags of any shard, a third of them tags of live records; the ragged last wave holds both kinds.  (The model's check_device walks the
    whole launch once per tag that comes several times, hence not more of those.)"""
    n = SC.N1
    tags = SC.random_tags(rng, n)
    free = rng.permutation(n - 37 - 64)                               # positions before the wave planted whole and the tail
    at = 0
    for s in range(shards):
        pool = tags_of_shard(rng, s, shards, 48 + 8 + 2)
        for copies, t in [(2, pool[:48]), (3, pool[48:56])]:
            tags[free[at:at + copies * len(t)]] = np.repeat(t, copies)
            at += copies * len(t)
        waves = rng.permutation((n - 37 - 64) // 64)[:512 if s == own else 64]
        tags[64 * waves + 5] = pool[56]
    whole = (n - 37 - 64) // 64 * 64
    tags[whole:whole + 64] = tags_of_shard(rng, own, shards, 1)[0]
    flags = rng.choice(SC.FLAG_CHOICES, size=n)
    special = rng.permutation(np.flatnonzero((np.arange(n) % 64 != 5) & (np.arange(n) < whole)))[:1994]
    zero, dead = np.concatenate([special[:997], n - 37 + np.array(SC.TAIL_ZERO)]), np.concatenate([special[997:], n - 37 + np.array(SC.TAIL_DEAD)])
    tags[zero] = 0
    tags[dead[:333]] = tags[(dead[:333] + 64) % (whole - 64)]        # DEAD copies of tags that live records of this launch hold
    flags[dead] = SC.DEAD | rng.choice(np.array([0, SC.WILD, SC.WILD | SC.CYCLE, SC.WILD | SC.NEG | SC.CYCLE], np.uint32), size=len(dead))
    return SC.make_records(rng, tags, flags, 1)


def test_every_wave_strides():
    """E = 3, shard 1, 2 * 1024 * 256 + 37 records: every wave strides twice and the last one is ragged; then the same launch again, when every own record
    meets the table"""
    import pybsgs
    own, shards = 1, 3
    recs = striding_launch(np.random.default_rng(4), own, shards)
    assert len(recs) == SC.N1 == 2 * 1024 * 256 + 37
    dead_or_zero = ((recs["flags"] & SC.DEAD) != 0) | (recs["x"][:, 0] == 0)
    assert dead_or_zero.sum() >= 1990 and set(shard_of(recs["x"][dead_or_zero, 0], shards).tolist()) == {0, 1, 2}
    live_tags = np.unique(recs["x"][~dead_or_zero, 0])
    SC.assert_far_from_full(live_tags[shard_of(live_tags, shards) == own], SC.SLOTS)      # (on the CPU, before the first device call)
    scalars, jumps = K.jump_table(K.Stream(11), 1 << 30)
    d = pybsgs.Device(0)
    try:
        d.kangaroo_setup(jumps, scalars, 0, SC.HERD, 1, SC.CAP)
        table = begin(d, own, shards, capacity=SC.CAPACITY, cap=SC.CAP)
        assert table["slots"] == SC.SLOTS
        out = d.kangaroo_dptable_insert_shard(recs.tobytes(), raw=True)
        table = check_call(table, recs, out, own, shards)
        sizes = [len(g) // 64 for g in out[1]]
        assert sizes[own] == 0 and min(sizes[0], sizes[2]) > SC.N1 // 4 and out[2] > SC.N1 // 4
        held = sorted(d.kangaroo_dptable_read())
        n_back = len(out[0]) // 64
        back, groups, n_entries, dropped = d.kangaroo_dptable_insert_shard(recs.tobytes(), raw=True)      # again: every live own record meets the table
        reasons = Counter(SC.from_bytes(back)["reserved"].tolist())
        assert dropped == 0 and [len(g) // 64 for g in groups] == sizes and n_entries == len(held) and sorted(d.kangaroo_dptable_read()) == held
        n_live = SC.N1 - sum(sizes) - int(dead_or_zero.sum())
        assert reasons[SC.R_STORED] == reasons[SC.R_DUPLICATE] == n_live and sum(reasons.values()) == 2 * n_live + int(dead_or_zero.sum()) > n_back
    finally:
        d.close()


# ---- 5. an outbox that does not fit the caller's buffer ----------------------------------------------------------------------------------------------------------
def test_a_routed_buffer_too_small_is_cut_and_counted(dev):
    import pybsgs
    rng = np.random.default_rng(5)
    own, shards, n = 1, 4, 640
    tags = np.concatenate([tags_of_shard(rng, s, shards, n // 4) for s in range(shards)])
    recs = SC.make_records(rng, rng.permutation(tags), rng.choice(SC.FLAG_CHOICES, size=n), 5)
    want = [0 if s == own else n // 4 for s in range(shards)]
    for room in (0, 1, 159, 160, 161, 479, 480):
        begin(dev, own, shards)
        arr, m, keep = dev._raw_records_in(recs.tobytes())
        buf = C.create_string_buffer(b"\xA5" * (64 * (room + 1)), 64 * (room + 1))      # a guard record behind the room offered
        out, obuf = dev._raw_records_out(2 * CAP)
        nrecs, entries, dropped = C.c_uint32(), C.c_uint64(), C.c_uint64()
        counts = (C.c_uint32 * 16)(*([0xDEAD] * 16))
        pybsgs._chk(dev.L.bsgs_kangaroo_dptable_insert_shard(dev.h, arr, m, out, 2 * CAP, C.byref(nrecs), C.cast(buf, C.POINTER(pybsgs.KangarooRecord)), room, counts,
                                                             C.byref(entries), C.byref(dropped)))
        got = list(counts)[:shards]
        cut, left = [], room
        for w in want:                                                # the groups in the order of their shards; the cut falls where the room ends
            cut.append(min(w, left))
            left -= cut[-1]
        assert got == cut and dropped.value == sum(want) - sum(cut) and nrecs.value == 0 and entries.value == n // 4, (room, got, dropped.value)
        assert buf.raw[64 * room:] == b"\xA5" * 64, "the guard behind the buffer"
        groups, at = SC.from_bytes(buf.raw[:64 * room]), 0
        for s, c in enumerate(got):                                   # what was handed over is of the right shard, and sent
            assert (shard_of(groups[at:at + c]["x"][:, 0], shards) == s).all()
            at += c
        sent = Counter(map(bytes, SC.sorted_words(recs).astype("<u4")))
        assert not Counter(map(bytes, SC.sorted_words(groups[:at]).astype("<u4"))) - sent


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------------------------
def test_states(jump_table):
    import pybsgs
    import kangaroo_sym_model as S
    from pybsgs.ecpy import mul
    scalars, jumps = jump_table
    sym_scalars, sym_jumps = S.jump_table(K.Stream(901), 2.0 ** 30, 64)
    t0, t1 = (0x1000 << 48) | 5, (0xF000 << 48) | 5                   # a tag of shard 0 and one of shard 1 of two
    d = pybsgs.Device(0)
    try:
        with pytest.raises(pybsgs.BsgsError, match="error -3: bsgs_kangaroo_setup first"):
            d.kangaroo_dptable_begin_shard(64, 0, 2)
        d.kangaroo_setup(jumps, scalars, 0, 64, 1, 64)
        for shard, shards in ((0, 0), (0, 17), (2, 2), (16, 16)):
            with pytest.raises(pybsgs.BsgsError, match="error -1: shard %d of %d" % (shard, shards)):
                d.kangaroo_dptable_begin_shard(64, shard, shards)
        for call in (lambda: d.kangaroo_run_dptable_shard(1), lambda: d.kangaroo_dptable_insert_shard([(t0, 1, 0, 0)])):
            with pytest.raises(pybsgs.BsgsError, match="error -3: bsgs_kangaroo_dptable_begin_shard first"):
                call()
        # a sharded table refuses the run and the insert of the other kinds, and stays as it was
        d.kangaroo_dptable_begin_shard(64, 1, 2, 1000)
        back, groups, n, dropped = d.kangaroo_dptable_insert_shard([(t1, 7, K.WILD, 3), (t0, 8, 0, 4)])
        assert (back, n, dropped) == ([], 1, 0) and [[(r["x"], r["d"], r["kangaroo"]) for r in g] for g in groups] == [[(t0, 8, 4)], []]
        for call in (lambda: d.kangaroo_run_dptable(1), lambda: d.kangaroo_dptable_insert([(6, 1, 0)]), lambda: d.kangaroo_run_dptable_keys(1),
                     lambda: d.kangaroo_dptable_insert_keys([(6, 1, 0, 0, 0)])):
            with pytest.raises(pybsgs.BsgsError, match="error -3: .*bsgs_kangaroo_dptable_begin_shard"):
                call()
        assert d.kangaroo_dptable_read() == [(t1, 7, 3, 1)]
        assert d.kangaroo_dptable_load([(t1 + 1, 2, 99, 3)]) == (1, 0, 0, 0, 2)                  # load, read and end serve it
        assert sorted(d.kangaroo_dptable_read()) == [(t1, 7, 3, 1), (t1 + 1, 2, 99, 3)]
        # a table of one engine refuses the sharded run and insert
        d.kangaroo_dptable_begin(64)
        assert d.kangaroo_dptable_insert([(t1, 1, K.WILD)]) == ([], 1, 0)
        for call in (lambda: d.kangaroo_run_dptable_shard(1), lambda: d.kangaroo_dptable_insert_shard([(t0, 1, 0, 0)])):
            with pytest.raises(pybsgs.BsgsError, match="error -3: the table was begun by bsgs_kangaroo_dptable_begin:"):
                call()
        assert d.kangaroo_dptable_read() == [(t1, 1, 0, 1)]
        d.kangaroo_dptable_begin_shard(64, 0, 1)                      # a begin of the other kind replaces the table; one shard routes nothing
        back, groups, n, dropped = d.kangaroo_dptable_insert_shard([(t1, 7, K.WILD, 3), (t0, 8, 0, 4)])
        assert (back, groups, n, dropped) == ([], [[]], 2, 0)
        d.kangaroo_dptable_end()
        d.kangaroo_dptable_end()
        d.kangaroo_dptable_begin(64)                                  # and the outbox went with it: the table of one engine works as ever
        assert d.kangaroo_dptable_insert([(t1, 1, K.WILD)]) == ([], 1, 0)
        # herds with a key list
        d.kangaroo_set_keys([mul(3), mul(5)])
        with pytest.raises(pybsgs.BsgsError, match="error -3: a distinguished-point table divided over engines serves one key"):
            d.kangaroo_dptable_begin_shard(64, 0, 2)
        d.kangaroo_dptable_begin_keys(64)
        with pytest.raises(pybsgs.BsgsError, match="error -3: a distinguished-point table divided over engines serves one key"):
            d.kangaroo_run_dptable_shard(1)
        d.kangaroo_setup_sym_keys(sym_jumps, sym_scalars, 0, 64, 1, 64)
        with pytest.raises(pybsgs.BsgsError, match="error -3: a distinguished-point table divided over engines serves the herds"):
            d.kangaroo_dptable_begin_shard(64, 0, 2)
        d.kangaroo_setup_sym(sym_jumps, sym_scalars, 0, 64, 1, 64)    # the symmetric herd for one key takes one
        d.kangaroo_dptable_begin_shard(64, 0, 2)
        d.kangaroo_setup_sym(sym_jumps, sym_scalars, 0, 64, 1, 64)    # a new herd drops it
        with pytest.raises(pybsgs.BsgsError, match="bsgs_kangaroo_dptable_begin_shard first"):
            d.kangaroo_run_dptable_shard(1)
    finally:
        d.close()


# ---- 7. two engines on one GPU -------------------------------------------------------------------------------------------------------------------------------------
KN, STEPS = 64, 33


def test_two_engines_relay(jump_table):
    """two devices opened on GPU 0, two shards, dp 0, 64 kangaroos each (half tame, half wild), 33 steps; the test is the relay.  Tame kangaroo 5 of
    engine 0 and wild kangaroo 40 of engine 1 start on one point: every point of theirs comes back once as a pair, on the engine its tag names, under the
    global ids 5 and 64 + 40, and the pair solves for the key."""
    import pybsgs
    scalars, jumps = jump_table
    q = 0x1234567 + (1 << 39)
    Q = K.start(None, q, False)
    rng = K.Stream(77)
    flags = [0] * (KN // 2) + [K.WILD] * (KN // 2)
    offsets = [[1 + rng.u128() % ((1 << 40) - 1) for _ in range(KN // 2)] + [K.signed128(rng.u128()) % (1 << 40) - (1 << 39) for _ in range(KN // 2)] for _ in range(2)]
    offsets[1][40] = offsets[0][5] - q
    devs = [pybsgs.Device(0), pybsgs.Device(0)]
    try:
        plain = []
        for e, d in enumerate(devs):
            d.kangaroo_setup(jumps, scalars, 0, KN, 1, KN * STEPS)
            assert d.kangaroo_seed(Q, offsets[e], flags) == (0, 0)
            states = d.kangaroo_download(0, KN)
            recs, dropped, _ = d.kangaroo_run(STEPS)                  # the herd's records, by the plain run
            assert dropped == 0 and len(recs) == KN * STEPS
            plain += [(r["x"] & DM.M64, r["d"], r["flags"], r["kangaroo"] + e * KN) for r in recs]
            d.kangaroo_upload(0, states)
            d.kangaroo_dptable_begin_shard(1 << 13, e, 2, e * KN)
        assert not any(fl & K.DEAD for _, _, fl, _ in plain) and all(t for t, _, _, _ in plain)
        one, want_back = DM.insert(DM.new_table(1 << 14, 2 * KN * STEPS), plain)
        back, inbox, entries = [], [[], []], [0, 0]
        for e, d in enumerate(devs):
            got, groups, seen, entries[e], dropped, ms = d.kangaroo_run_dptable_shard(STEPS)
            assert seen == KN * STEPS and dropped == 0 and ms > 0 and groups[e] == []
            assert all(SM.shard(r["x"] & DM.M64, 2) == 1 - e and e * KN <= r["kangaroo"] < (e + 1) * KN for r in groups[1 - e])
            back += got
            inbox[1 - e] += groups[1 - e]
        assert sum(map(len, inbox)) + sum(entries) + sum(r["reason"] != DM.DPT_STORED for r in back) == 2 * KN * STEPS
        for e, d in enumerate(devs):                                  # the relay: every group to its shard
            got, groups, entries[e], dropped = d.kangaroo_dptable_insert_shard([(r["x"], r["d"], r["flags"], r["kangaroo"]) for r in inbox[e]])
            assert dropped == 0 and groups == [[], []]
            back += got
        reads = [d.kangaroo_dptable_read() for d in devs]
        assert [len(r) for r in reads] == entries and all(SM.shard(t, 2) == e for e, r in enumerate(reads) for t, _, _, _ in r)
    finally:
        for d in devs:
            d.close()
    union = reads[0] + reads[1]
    assert len(union) == len({e[0] for e in union}) == DM.entries(one) and {e[0] for e in union} == set(one["cand"])
    assert all(e in one["cand"][e[0]] for e in union)
    # the hand-backs: the one pair of kangaroos, once per step, under both global ids
    assert Counter(r["reason"] for r in back) == Counter({DM.DPT_STORED: STEPS, DM.DPT_DUPLICATE: STEPS}) == Counter(
        {DM.DPT_STORED: len(want_back), DM.DPT_DUPLICATE: len(want_back)})
    for k in range(0, len(back), 2):
        st, w = back[k], back[k + 1]
        assert st["reason"] == DM.DPT_STORED and w["reason"] == DM.DPT_DUPLICATE and st["x"] == w["x"] & DM.M64
        assert {st["kangaroo"], w["kangaroo"]} == {5, KN + 40} and {st["flags"], DM.type_of(w["flags"])} == {0, 1}
        assert (st["x"], st["d"], st["kangaroo"], st["flags"]) in union
        dt, dw = (st["d"], w["d"]) if st["flags"] == 0 else (w["d"], st["d"])
        assert K.signed128(dt - dw) == q
    assert {SM.shard(back[k]["x"], 2) for k in range(0, len(back), 2)} == {0, 1}      # (33 points: both engines paired some)
