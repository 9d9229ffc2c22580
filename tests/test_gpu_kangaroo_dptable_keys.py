"""GPU: the distinguished-point table for a key list (csrc/kangaroo_dptable_keys.hip) against its model (tests/kangaroo_dptable_keys_model.py), through
pybsgs, under both herds that serve a list -- bsgs_kangaroo_setup with a key list (the key in the flags) and bsgs_kangaroo_setup_sym_keys (the key in
`reserved`, NEG in the owner): 1024 crafted records; a launch of 524325 records in which every wave strides (the generators and the set reference of
tests/kangaroo_table_scale_cases.py, with key words added); the insert behind the walk of 8192 kangaroos over three keys against bsgs_kangaroo_run on the
same herd; a load of version-3 and version-4 style entries in two staged chunks; and the state errors."""
import time
from collections import Counter

import numpy as np
import pytest

import kangaroo_model as K
import kangaroo_sym_model as S
import kangaroo_dptable_model as DM
import kangaroo_dptable_keys_model as KM
import kangaroo_table_scale_cases as SC
from pybsgs.ecpy import add, mul, neg

pytestmark = pytest.mark.gpu

KINDS = ["plain", "sym"]
CAP = 1024
KEYS3 = [0x1234567890, 0xFEDCBA9876, 7]


def open_dev(kind, herd, per_thread, cap, qs=None):
    """a herd that serves a key list: of bsgs_kangaroo_setup ("plain") or of bsgs_kangaroo_setup_sym_keys ("sym"), dp 0, with a list of three keys"""
    import pybsgs
    d = pybsgs.Device(0)
    try:
        if kind == "plain":
            scalars, jumps = K.jump_table(K.Stream(11), 1 << 30)
            d.kangaroo_setup(jumps, scalars, 0, herd, per_thread, cap)
        else:
            scalars, jumps = S.jump_table(K.Stream(901), 2.0 ** 30, 64)
            d.kangaroo_setup_sym_keys(jumps, scalars, 0, herd, per_thread, cap)
        d.kangaroo_set_keys(qs or [mul(k) for k in KEYS3])
    except Exception:
        d.close()
        raise
    return d


def rec_of(kind, tag, d, key, kang, fl):
    """a record of key `key` as the herd writes it: (tag, d, flags, kangaroo, reserved)"""
    return (tag, d, fl, kang, key) if kind == "sym" else (tag, d, fl | key << KM.KEY_SHIFT, kang, 0)


def fresh_tags(rng, n, avoid=()):
    out, seen = [], set(avoid) | {0}
    while len(out) < n:
        t = rng.u64()
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


# ---- 1. crafted records ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_crafted_records(kind):
    sym = kind == "sym"
    rng = K.Stream(2)
    table = DM.new_table(2048, CAP)
    slots = table["slots"]
    assert slots == 8192
    x, y, *tags = fresh_tags(rng, 2 + 1024)
    kinds = [(0, 0), (KM.WILD, 0), (KM.WILD, 1), (KM.WILD, 65534), (KM.WILD | KM.NEG, 2), (KM.WILD | KM.NEG, 65534)]      # tame; wild of keys 0, 1, 65534; NEG
    recs = []
    for k in range(1024):
        fl, key = kinds[k % len(kinds)]
        recs.append([tags[k], rng.u128(), key, 7000 + k, fl])
    for lane in range(64):                                            # one tag in all 64 lanes of wave 0, with 64 different keys
        recs[lane][0], recs[lane][2], recs[lane][4] = x, 100 + lane, KM.WILD
    for w in range(1, 9):                                             # one tag in lane 5 of eight waves: blocks 0, 1 and 2
        recs[64 * w + 5][0] = y
    chain = DM.chain_tags(slots - 1, slots, 40)                       # forty tags whose home is the last slot: the chain wraps to slot 0
    for j, t in enumerate(chain):
        recs[600 + 7 * j][0] = t
    dead = {300: K.DEAD | KM.WILD, 301: K.DEAD | S.CYCLE | KM.WILD, 302: K.DEAD, 900: K.DEAD | S.CYCLE | KM.WILD | KM.NEG}
    for k, fl in dead.items():
        recs[k][4] = fl
    recs[303][0] = x                                                  # a DEAD copy of a live tag: it comes back alone
    dead[303] = recs[303][4] = K.DEAD | KM.WILD
    zero = (310, 311, 1023)
    for k in zero:
        recs[k][0] = 0
    recs[311][4], recs[311][2] = KM.WILD, 65534                       # tag 0 keeps its key too
    recs = [rec_of(kind, t, d, key, kang, fl) for t, d, key, kang, fl in recs]
    assert len(recs) == 1024 and len({r[3] for r in recs}) == 1024

    dev = open_dev(kind, 512, 2, CAP)
    try:
        dev.kangaroo_dptable_begin_keys(2048)
        got, n_entries, dropped = dev.kangaroo_dptable_insert_keys(recs)
        assert dropped == 0
        table, pairs = KM.check_device(table, recs, got, n_entries, sym)
        # exactly one copy of each tag is stored, every owner word exact
        held = dev.kangaroo_dptable_read()
        assert len(held) == len({e[0] for e in held}) == n_entries == 1024 - 63 - 7 - len(dead) - len(zero)
        assert set(held) == DM.read(table)
        live = [r for r in recs if not r[2] & K.DEAD and r[0]]
        assert set(held) <= {KM.entry_of(r, sym) for r in live}
        owners = {e[3] for e in held}
        want_owners = {0, 1, 2, 65535} | ({3 | 1 << 31, 65535 | 1 << 31} if sym else {3}) | {e[3] for e in held if e[0] == x}
        assert owners == want_owners and next(e[3] for e in held if e[0] == x) in range(101, 165)
        # every other copy came back as a pair with the stored copy's owner and its own key and reason; DEAD and tag 0 alone with theirs
        assert Counter((r, rec[0] & DM.M64) for r, rec, _ in pairs if r == KM.DPT_DUPLICATE) == Counter({(KM.DPT_DUPLICATE, x): 63, (KM.DPT_DUPLICATE, y): 7})
        by_kang = {r[3]: r for r in recs}
        for reason, rec, st in pairs:
            sent = by_kang[rec[3]]
            assert rec[4] == KM.key_of(sent[2], sent[4], sym) and rec[2] == sent[2]
            assert reason == (KM.DPT_DEAD if sent[2] & K.DEAD else KM.DPT_TAG_ZERO if sent[0] == 0 else KM.DPT_DUPLICATE)
            if st is not None:
                assert st in held and st[3] == KM.owner_of(by_kang[st[2]][2], by_kang[st[2]][4], sym)
        assert sorted(rec[3] - 7000 for r, rec, _ in pairs if r == KM.DPT_DEAD) == sorted(dead)
        assert sorted(rec[3] - 7000 for r, rec, _ in pairs if r == KM.DPT_TAG_ZERO) == sorted(zero)
        assert {rec[4] for r, rec, _ in pairs if rec[3] == 7311} == {65534}
        # a second launch: what was stored stays; every record meets it and names its own key beside the stored owner
        again = [rec_of(kind, x, 1, 40000, 9000, KM.WILD), rec_of(kind, y, 2, 0, 9001, 0), rec_of(kind, chain[39], 3, 65534, 9002, KM.WILD | KM.NEG),
                 rec_of(kind, chain[0], 4, 5, 9003, KM.WILD)]
        got, n_entries2, dropped = dev.kangaroo_dptable_insert_keys(again)
        table, pairs = KM.check_device(table, again, got, n_entries2, sym)
        assert n_entries2 == n_entries and [r for r, _, _ in pairs] == [KM.DPT_DUPLICATE] * 4 and all(st in held for _, _, st in pairs)
        assert sorted(rec[4] for _, rec, _ in pairs) == [0, 5, 40000, 65534]
        assert set(dev.kangaroo_dptable_read()) == set(held)
        # the raw form says the same: `reserved` = reason | key << 8, the stored half exactly DPT_STORED with the owner in its flags
        arr = np.zeros(1, SC.REC)
        arr["x"][0, 0], arr["flags"], arr["kangaroo"], arr["reserved"] = x, again[0][2], 9100, again[0][4]
        raw, _, _ = dev.kangaroo_dptable_insert_keys(arr.tobytes(), raw=True)
        raw = SC.from_bytes(raw)
        assert raw["reserved"].tolist() == [KM.DPT_STORED, KM.encode_reserved(KM.DPT_DUPLICATE, 40000)]
        assert int(raw["flags"][0]) == next(e[3] for e in held if e[0] == x) and int(raw["flags"][1]) == again[0][2]
    finally:
        dev.close()


# ---- 2. a launch in which every wave strides ---------------------------------------------------------------------------------------------------------------
def keyed_launch(recs, sym, seed):
    """key words for a launch of the scale generators: a key of 0 .. 65534 for every record -- in flag bits 8..23 for the plain herd (the symmetric walk's
    jump-index bits of the generated flags give way), in `reserved` for the symmetric list's herd, whose flags stay as generated -> (records, key, owner)"""
    rng = np.random.default_rng(seed)
    r = recs.copy()
    key = rng.choice(np.array([0, 1, 2, 255, 256, 65534], np.uint32), size=len(r))
    wild = (r["flags"] & SC.WILD) != 0
    if sym:
        r["reserved"] = key
        owner = np.where(wild, (key + 1) | np.where(r["flags"] & SC.NEG, 1 << 31, 0), 0)
    else:
        key = np.where(wild, key, 0).astype(np.uint32)                # (a tame record's flags carry no key there)
        r["flags"] = (r["flags"] & np.uint32(0xFF0000FF)) | (key << np.uint32(8))
        owner = np.where(wild, key + 1, 0)
    return r, key.astype(np.uint64), owner.astype(np.uint64)


@pytest.fixture(scope="module")
def scale():
    """the main launch of the scale cases and its reference: built, and its conditions asserted, on the CPU before any device call"""
    case = SC.scale_case()
    (name, recs), ref = case["launches"][0], case["refs"][0]
    assert name == "main" and len(recs) == SC.N1 == 2 * 1024 * 256 + 37 == 524325 and SC.SLOTS == 1 << 21
    load, chain = SC.assert_far_from_full(ref["tags"], SC.SLOTS)
    assert load <= SC.MAX_LOAD and chain <= SC.MAX_CHAIN
    return case


@pytest.mark.parametrize("kind", KINDS)
def test_every_wave_strides(scale, kind):
    sym = kind == "sym"
    ref = scale["refs"][0]
    recs, key, owner = keyed_launch(scale["launches"][0][1], sym, 5)
    again_ref = SC.reference(ref["tags"], recs)
    SC.assert_far_from_full(again_ref["tags"], SC.SLOTS)              # (on the CPU, before the first device call)
    ids = SC.record_ids(recs)
    order = np.argsort(ids)
    dev = open_dev(kind, SC.HERD, 1, SC.CAP)
    try:
        dev.kangaroo_dptable_begin_keys(SC.CAPACITY)
        before = None
        for name, want in (("main", ref), ("again", again_ref)):
            t0 = time.perf_counter()
            got, n_entries, dropped = dev.kangaroo_dptable_insert_keys(recs.tobytes(), raw=True)
            got = SC.from_bytes(got)
            assert dropped == 0
            st_at = np.flatnonzero(got["reserved"] == SC.R_STORED)
            walk_at = np.flatnonzero(got["reserved"] != SC.R_STORED)
            walk = got[walk_at].copy()
            back_key = walk["reserved"] >> np.uint32(KM.DPT_KEY_SHIFT)
            walk["reserved"] &= np.uint32(0xFF)                       # the reason, as the set reference reads it
            du_at = walk_at[walk["reserved"] == SC.R_DUPLICATE]
            assert np.array_equal(st_at + 1, du_at), "every DUPLICATE directly behind a STORED record, and no other STORED record"
            stored = got[st_at]
            assert np.array_equal(stored["x"][:, 0], got[du_at]["x"][:, 0]) and not stored["x"][:, 1:].any() and not stored["step"].any()
            table5 = SC.entry_rows(SC.from_bytes(dev.kangaroo_dptable_read(raw=True), SC.DP_ENTRY))
            SC.check_launch(want, recs, walk, n_entries, table5[:, :4], None if before is None else before[:, :4])      # the set reference, owners aside
            SC.check_pairs(stored, got[du_at], table5)                # the stored half is the table's entry, its owner word included
            # every handed-back record names the key of the record that was sent
            at = order[np.searchsorted(ids[order], SC.record_ids(walk))]
            assert np.array_equal(back_key.astype(np.uint64), key[at])
            # every stored owner is the owner of the copy that was stored: (tag, d, kangaroo) names a sent record
            kang_at = order[np.searchsorted(ids[order] >> np.uint64(32), table5[:, 3])]
            assert np.array_equal(recs["kangaroo"][kang_at].astype(np.uint64), table5[:, 3]) and np.array_equal(recs["x"][kang_at, 0], table5[:, 0])
            assert np.array_equal(owner[kang_at], table5[:, 4])
            if before is not None:
                assert np.array_equal(table5[np.argsort(table5[:, 0])], before[np.argsort(before[:, 0])])
            print("dptable_keys", kind, name, "entries", n_entries, "handed back", len(walk), "%.2f s" % (time.perf_counter() - t0))
            before = table5
        assert (before[:, 4] >> np.uint64(31)).any() == sym
    finally:
        dev.close()


# ---- 3. behind the walk --------------------------------------------------------------------------------------------------------------------------------------
WALK_HERD, WALK_STEPS = 8192, 20                                      # dp 0: a record per kangaroo and step; 20 steps: the symmetric walk's cycle check runs


@pytest.mark.parametrize("kind", KINDS)
def test_behind_the_walk(kind):
    sym = kind == "sym"
    n, A, W = WALK_HERD, 0x5A5A5A << 40, 1 << 40
    keys = [A + k for k in KEYS3]
    base = neg(mul(A + W // 2)) if sym else neg(mul(A))
    qs = [add(mul(k), base) for k in keys]
    rng = K.Stream(4001)
    wild = [i >= n // 2 for i in range(n)]
    key_of = [(i - n // 2) % len(keys) if w else 0 for i, w in enumerate(wild)]
    offs = [(S.herd_offset if sym else K.herd_offset)(rng, W, w) for w in wild]
    offs[300] = offs[17]                                              # two tame kangaroos on one start
    offs[n // 2 + 3], key_of[n // 2 + 3] = offs[n // 2 + 9], key_of[n // 2 + 9]      # two wild kangaroos of one key on one start
    cap = n * WALK_STEPS
    dev = open_dev(kind, n, 2, cap, qs)
    try:
        assert dev.kangaroo_seed_keys(offs, [K.WILD if w else 0 for w in wild], key_of) == (0, 0)
        states = dev.kangaroo_download(0, n)
        plain, dropped, _ = dev.kangaroo_run(WALK_STEPS, raw=True)
        plain = SC.from_bytes(plain)
        assert dropped == 0 and cap // 2 < len(plain) <= cap
        dev.kangaroo_upload(0, states)
        dev.kangaroo_dptable_begin_keys(1 << 18)
        got, seen, n_entries, dropped, ms = dev.kangaroo_run_dptable_keys(WALK_STEPS, raw=True)
        got = SC.from_bytes(got)
        assert seen == len(plain) and dropped == 0 and ms > 0
        table = SC.entry_rows(SC.from_bytes(dev.kangaroo_dptable_read(raw=True), SC.DP_ENTRY))
    finally:
        dev.close()

    def owners(r):
        k = (r["reserved"] if sym else r["flags"] >> np.uint32(8)) & np.uint32(0xFFFF)
        neg_bit = np.where((r["flags"] & SC.NEG) != 0, np.uint64(1 << 31), np.uint64(0)) if sym else np.uint64(0)
        return np.where((r["flags"] & SC.WILD) != 0, (k.astype(np.uint64) + np.uint64(1)) | neg_bit, np.uint64(0)), k

    walk = got[got["reserved"] != SC.R_STORED].copy()
    reason, back_key = walk["reserved"] & np.uint32(0xFF), walk["reserved"] >> np.uint32(8)
    walk["reserved"] = back_key if sym else 0                         # the record as the walk wrote it
    own_back, k_back = owners(walk)
    assert np.array_equal(back_key, k_back)                           # the key a hand-back names is the key its record named
    own_plain, k_plain = owners(plain)
    assert set(np.unique(k_plain[(plain["flags"] & SC.WILD) != 0]).tolist()) == {0, 1, 2}
    # entries read back plus handed-back walk records = the plain run's records, as a multiset of (tag, d, kangaroo, owner)
    rows_of = lambda r, own: SC.rows(r["x"][:, 0], r["d"][:, 0], r["d"][:, 1], r["kangaroo"], own)
    assert n_entries == len(table) == len(np.unique(table[:, 0]))
    assert SC.same_rows(np.concatenate([table, rows_of(walk, own_back)]), rows_of(plain, own_plain))
    # and the handed-back records are the walk's own in all 64 bytes; DEAD ones came back as DEAD, the others as duplicates in pairs
    sent = {bytes(r) for r in SC.sorted_words(plain).astype("<u4")}
    assert all(bytes(r) in sent for r in SC.sorted_words(walk).astype("<u4"))
    dead = (walk["flags"] & SC.DEAD) != 0
    assert np.array_equal(reason[dead], np.full(dead.sum(), SC.R_DEAD)) and np.array_equal(reason[~dead], np.full((~dead).sum(), SC.R_DUPLICATE))
    assert (~dead).sum() >= WALK_STEPS and (got["reserved"] == SC.R_STORED).sum() == (~dead).sum()
    st_at = np.flatnonzero(got["reserved"] == SC.R_STORED)
    SC.check_pairs(got[st_at], got[st_at + 1], table)
    assert ((table[:, 4] >> np.uint64(31)) != 0).any() == sym and set(np.unique(table[:, 4] & np.uint64(0x7FFFFFFF)).tolist()) == {0, 1, 2, 3}


# ---- 4. load ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_load_in_two_chunks(scale, kind):
    """version-3 style entries (owner 0 .. 65535) under the plain herd, version-4 style (bit 31 too) under the symmetric list's"""
    e = scale["entries"].copy()
    assert len(e) == (1 << 20) + (1 << 18)
    rng = np.random.default_rng(44)
    owner = rng.choice(np.array([0, 1, 2, 256, 65535], np.uint32), size=len(e))
    if kind == "sym":
        owner = np.where((owner != 0) & (rng.integers(0, 2, size=len(e)) == 1), owner | np.uint32(1 << 31), owner).astype(np.uint32)
    e["type"] = owner
    dev = open_dev(kind, SC.HERD, 1, SC.CAP)
    try:
        dev.kangaroo_dptable_begin_keys(SC.CAPACITY)
        out = dev.kangaroo_dptable_load(e.tobytes())
        assert sum(out[:4]) == len(e)
        raw = dev.kangaroo_dptable_read(raw=True)
    finally:
        dev.close()
    table = SC.entry_rows(SC.from_bytes(raw, SC.DP_ENTRY))
    SC.check_loaded(out[:4], out[4], table, scale["load_counts"], scale["load_tags"], e)
    # byte for byte: every 32-byte entry read is one of those sent, and the tags sent once came back as they were
    got = SC.from_bytes(raw, SC.DP_ENTRY)
    assert np.array_equal(got, e[got["d"][:, 0].astype(np.int64)])
    once = np.isin(e["tag"], scale["load_plan"]["fresh_2"])
    assert np.isin(e[once]["d"][:, 0], got["d"][:, 0]).all()
    assert set(np.unique(got["type"]).tolist()) == set(np.unique(owner).tolist())


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------------------------
def test_states():
    import pybsgs
    scalars, jumps = K.jump_table(K.Stream(11), 1 << 30)
    sym_scalars, sym_jumps = S.jump_table(K.Stream(901), 2.0 ** 30, 64)
    qs = [mul(k) for k in KEYS3]
    needs_list = "error -3: a distinguished-point table for a key list serves the herds of bsgs_kangaroo_setup and bsgs_kangaroo_setup_sym_keys after bsgs_kangaroo_set_keys"
    d = pybsgs.Device(0)
    try:
        with pytest.raises(pybsgs.BsgsError, match="error -3: bsgs_kangaroo_setup first"):
            d.kangaroo_dptable_begin_keys(64)
        d.kangaroo_setup(jumps, scalars, 0, 64, 1, 64)
        with pytest.raises(pybsgs.BsgsError, match=needs_list):      # a herd without a list
            d.kangaroo_dptable_begin_keys(64)
        for call in (lambda: d.kangaroo_run_dptable_keys(1), lambda: d.kangaroo_dptable_insert_keys([(1, 1, 0, 0, 0)])):
            with pytest.raises(pybsgs.BsgsError, match=needs_list):
                call()
        d.kangaroo_setup_sym(sym_jumps, sym_scalars, 0, 64, 1, 64)    # the symmetric walk for one key takes no list, so no keyed table either
        with pytest.raises(pybsgs.BsgsError, match=needs_list):
            d.kangaroo_dptable_begin_keys(64)
        d.kangaroo_setup(jumps, scalars, 0, 64, 1, 64)
        d.kangaroo_set_keys(qs)
        for call in (lambda: d.kangaroo_run_dptable_keys(1), lambda: d.kangaroo_dptable_insert_keys([(1, 1, 0, 0, 0)])):
            with pytest.raises(pybsgs.BsgsError, match="error -3: bsgs_kangaroo_dptable_begin_keys first"):
                call()
        for capacity in (0, (1 << 31) + 1):
            with pytest.raises(pybsgs.BsgsError, match="error -1: .*1..2\\^31"):
                d.kangaroo_dptable_begin_keys(capacity)
        # a keyed table refuses the unkeyed run and insert, and stays as it was
        d.kangaroo_dptable_begin_keys(64)
        assert d.kangaroo_dptable_insert_keys([(5, 1, K.WILD | 2 << 8, 0, 0)]) == ([], 1, 0)
        for call in (lambda: d.kangaroo_run_dptable(1), lambda: d.kangaroo_dptable_insert([(6, 1, 0)])):
            with pytest.raises(pybsgs.BsgsError, match="error -3: the table was begun by bsgs_kangaroo_dptable_begin_keys"):
                call()
        assert d.kangaroo_dptable_read() == [(5, 1, 0, 3)]
        assert d.kangaroo_dptable_load([(9, 2, 3, 65535 | 1 << 31)]) == (1, 0, 0, 0, 2)      # load and read serve it, the owner word as it is
        assert sorted(d.kangaroo_dptable_read()) == [(5, 1, 0, 3), (9, 2, 3, 65535 | 1 << 31)]
        # an unkeyed table refuses the keyed run and insert
        d.kangaroo_dptable_begin(64)
        assert d.kangaroo_dptable_read() == []
        for call in (lambda: d.kangaroo_run_dptable_keys(1), lambda: d.kangaroo_dptable_insert_keys([(6, 1, 0, 0, 0)])):
            with pytest.raises(pybsgs.BsgsError, match="error -3: the table was begun by bsgs_kangaroo_dptable_begin:"):
                call()
        assert d.kangaroo_dptable_insert([(5, 1, K.WILD | 2 << 8)]) == ([], 1, 0) and d.kangaroo_dptable_read() == [(5, 1, 0, 1)]
        d.kangaroo_dptable_begin_keys(64)                             # a begin of the other kind replaces the table
        assert d.kangaroo_dptable_read() == []
        d.kangaroo_dptable_end()
        d.kangaroo_dptable_end()
        with pytest.raises(pybsgs.BsgsError, match="bsgs_kangaroo_dptable_begin first"):
            d.kangaroo_dptable_read()
        # the symmetric list's herd: the pinned refusal of the unkeyed begin is still given, with and without a keyed table under the herd
        d.kangaroo_setup_sym_keys(sym_jumps, sym_scalars, 0, 64, 1, 64)
        with pytest.raises(pybsgs.BsgsError, match="error -3: a distinguished-point table serves the herds"):
            d.kangaroo_dptable_begin(64)
        with pytest.raises(pybsgs.BsgsError, match=needs_list):
            d.kangaroo_dptable_begin_keys(64)
        d.kangaroo_set_keys(qs)
        d.kangaroo_dptable_begin_keys(64)
        with pytest.raises(pybsgs.BsgsError, match="error -3: a distinguished-point table serves the herds"):
            d.kangaroo_dptable_begin(64)
        with pytest.raises(pybsgs.BsgsError, match="error -3: the table was begun by bsgs_kangaroo_dptable_begin_keys"):
            d.kangaroo_run_dptable(1)
        got, n, dropped = d.kangaroo_dptable_insert_keys([(5, 1, K.WILD | KM.NEG, 0, 2), (5, 2, K.WILD, 1, 65534)])
        assert n == 1 and dropped == 0 and [(r["reason"], r["key"]) for r in got] == [(KM.DPT_STORED, None), (KM.DPT_DUPLICATE, got[1]["key"])]
        assert {(got[0]["flags"], got[1]["key"])} <= {(3 | 1 << 31, 65534), (65535, 2)}
        d.kangaroo_setup_sym_keys(sym_jumps, sym_scalars, 0, 64, 1, 64)      # a new herd drops the table
        d.kangaroo_set_keys(qs)
        with pytest.raises(pybsgs.BsgsError, match="bsgs_kangaroo_dptable_begin_keys first"):
            d.kangaroo_run_dptable_keys(1)
    finally:
        d.close()
