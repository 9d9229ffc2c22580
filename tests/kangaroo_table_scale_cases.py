"""The kangaroo tables in device memory at launch sizes where a wave strides over the records (csrc/kangaroo_table.hip.h and the units that include it;
csrc/kangaroo_tames.hip): a reference that needs no slots, the checks a device's answer must pass, and seeded generators of launches.  numpy only: no
product code runs here, and tests/test_kangaroo_table_scale_model.py pins all of it on the CPU against the slot-level models.

The reference.  While no record is FULL, what a launch does to a table does not depend on the order the records are taken in, nor on where a tag comes
to stand: DEAD records and live records of tag 0 come back; of the live copies of a tag all come back as DUPLICATE but one when the tag is new, all of them
when the table held it; the new tag set is the union.  Which copy of a new tag is stored is unspecified: the reference names the candidates.

Records are numpy arrays with the 64-byte layout of bsgs_kangaroo_record (REC), table entries rows of u64: (tag, d.lo, d.hi) or, with owners,
(tag, d.lo, d.hi, kangaroo, type)."""
import functools

import numpy as np

REC = np.dtype([("x", "<u8", (4,)), ("d", "<u8", (2,)), ("kangaroo", "<u4"), ("flags", "<u4"), ("step", "<u4"), ("reserved", "<u4")])
DP_ENTRY = np.dtype([("tag", "<u8"), ("d", "<u8", (2,)), ("kangaroo", "<u4"), ("type", "<u4")])      # bsgs_kangaroo_dp_entry
assert REC.itemsize == 64 and DP_ENTRY.itemsize == 32

WILD, NEG, CYCLE, DEAD = 1, 2, 4, 0x80000000
LAST_VALID, LAST_SHIFT = 0x100, 9                                     # the symmetric walk's last jump index, kept in the flags
R_DEAD, R_DUPLICATE, R_TAG_ZERO, R_FULL, R_STORED = range(5)          # BSGS_KANGAROO_GEN_* and BSGS_KANGAROO_DPT_*: the first four are the same numbers

# ---- the shapes: the smallest that reach the second and the ragged iteration of every stride -------------------------------------------------------------
INSERT_GRID_MAX, SCAN_GRID_MAX, BLOCK = 1024, 4096, 256               # KT_INSERT_GRID_MAX = TAMES_GRID_MAX, KT_SCAN_GRID_MAX, threads per block
MIN_SLOTS = 128
HERD = 64                                                             # one per thread: the herd only lends its record buffers
N1 = CAP = 2 * INSERT_GRID_MAX * BLOCK + 37                           # every wave strides twice; wave 0 of block 0 a third time, with 37 live lanes
CAPACITY = 1 << 18
MAX_LOAD, MAX_CHAIN = 0.70, 4096                                      # a FULL record probes every slot: no scale launch comes near one
LOAD_CHUNK = 1 << 20                                                  # BSGS_KANGAROO_TAMES_LOAD_CHUNK = BSGS_KANGAROO_DPT_LOAD_CHUNK
LOAD_PAIRS = (1 << 20) + (1 << 18)                                    # two staged chunks
WALK_HERD, WALK_PER_THREAD, WALK_STEPS = 8192, 2, 33                  # dp 0: a record per kangaroo and step
WALK_CAP = WALK_HERD * WALK_STEPS                                     # 270336, just above 1024 x 256: the first 128 waves stride twice


def n_slots(capacity, record_cap):
    """bsgs_kang_table_slots: the power of two at or above 2 * (capacity + record_cap), at least 128"""
    slots = MIN_SLOTS
    while slots < 2 * (capacity + record_cap):
        slots *= 2
    return slots


SLOTS = n_slots(CAPACITY, CAP)
assert N1 > 2 * INSERT_GRID_MAX * BLOCK and N1 % 64 == 37
assert SLOTS == 1 << 21 and SLOTS > 1 << 20 and SLOTS == 2 * SCAN_GRID_MAX * BLOCK      # each harvest: two iterations of the full scan grid
assert INSERT_GRID_MAX * BLOCK < WALK_CAP < 2 * INSERT_GRID_MAX * BLOCK and LOAD_CHUNK < LOAD_PAIRS <= 2 * LOAD_CHUNK
# device memory of the herd with both tables: two record buffers, the hand-backs of the distinguished-point table, tags + offsets (+ owners)
assert 2 * 64 * CAP + 2 * 64 * CAP + SLOTS * 24 + SLOTS * 32 < 300 << 20


# ---- rows and multisets ------------------------------------------------------------------------------------------------------------------------------------
def rows(*cols):
    """columns -> an (n, k) array of u64"""
    return np.stack([np.asarray(c).astype(np.uint64) for c in cols], axis=1) if len(cols[0]) else np.zeros((0, len(cols)), np.uint64)


def sort_rows(a):
    """the rows in lexicographic order: two multisets of rows are equal when their sorted arrays are"""
    return a[np.lexsort(a.T[::-1])] if len(a) else a


def same_rows(a, b):
    return a.shape == b.shape and np.array_equal(sort_rows(a), sort_rows(b))


def home(tags, slots):
    return (np.asarray(tags, np.uint64) >> np.uint64(6)) & np.uint64(slots - 1)


def entry_type(flags):
    """dpt_type: 0 tame, WILD, WILD | NEG"""
    flags = np.asarray(flags, np.uint32)
    return np.where(flags & WILD, flags & (WILD | NEG), 0).astype(np.uint32)


def from_bytes(b, dtype=REC):
    return np.frombuffer(b, dtype=dtype)


def record_ids(recs):
    """kangaroo << 32 | step"""
    return recs["kangaroo"].astype(np.uint64) << np.uint64(32) | recs["step"].astype(np.uint64)


def sorted_words(recs, *more):
    """the records as rows of their sixteen u32 words (and further u32 columns beside them), in lexicographic order: equal for equal multisets"""
    a = np.ascontiguousarray(recs).view(np.uint32).reshape(-1, 16)
    a = np.concatenate([a] + [np.asarray(m, np.uint32).reshape(-1, 1) for m in more], axis=1)
    return a[np.lexsort(a.T[::-1])] if len(a) else a


def entry_rows(e):
    """DP_ENTRY array -> rows (tag, d.lo, d.hi, kangaroo, type)"""
    return rows(e["tag"], e["d"][:, 0], e["d"][:, 1], e["kangaroo"], e["type"])


def pair_rows(tags, d):
    """the growing tame table's (tags as u64, offsets as 16 bytes each) -> rows (tag, d.lo, d.hi)"""
    d = np.asarray(d).reshape(-1, 2)
    return rows(tags, d[:, 0], d[:, 1])


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------------
def is_in(values, sorted_unique):
    """membership of u64 values in a sorted array without duplicates"""
    if not len(sorted_unique):
        return np.zeros(len(values), bool)
    at = np.minimum(np.searchsorted(sorted_unique, values), len(sorted_unique) - 1)
    return sorted_unique[at] == values


def reference(held, recs):
    """held: the tags in the table (sorted, no duplicates); recs: a launch (REC) -> a dict:
      tags      the new tag set, sorted
      back      the hand-backs as sorted rows (tag, reason): every DEAD record, every live record of tag 0, the copies of a tag minus one if it is new
      new_tags  the tags new in this launch, sorted
      cand      sorted rows (tag, d.lo, d.hi, kangaroo, type) of the live copies of the new tags: per tag exactly one of them is the stored one
      entries   the entry count"""
    held = np.asarray(held, np.uint64)
    tag, fl = recs["x"][:, 0], recs["flags"]
    dead = (fl & DEAD) != 0
    zero = ~dead & (tag == 0)
    live = ~dead & ~zero
    uniq, counts = np.unique(tag[live], return_counts=True)
    new = ~is_in(uniq, held)
    back = np.concatenate([rows(tag[dead], np.full(dead.sum(), R_DEAD)), rows(tag[zero], np.full(zero.sum(), R_TAG_ZERO)),
                           rows(np.repeat(uniq, counts - new), np.full(int((counts - new).sum()), R_DUPLICATE))])
    new_tags = uniq[new]
    fresh = live & is_in(tag, new_tags)
    r = recs[fresh]
    cand = rows(r["x"][:, 0], r["d"][:, 0], r["d"][:, 1], r["kangaroo"], entry_type(r["flags"]))
    tags = np.union1d(held, uniq)
    return {"tags": tags, "back": sort_rows(back), "new_tags": new_tags, "cand": sort_rows(cand), "entries": len(tags)}


def reference_load(held, tags):
    """a load of pairs or entries with these tags on a table that holds `held` -> ((stored, duplicate, zero, full), the new tag set)"""
    held, tags = np.asarray(held, np.uint64), np.asarray(tags, np.uint64)
    zero = int((tags == 0).sum())
    uniq = np.unique(tags[tags != 0])
    stored = int((~is_in(uniq, held)).sum())
    return (stored, len(tags) - zero - stored, zero, 0), np.union1d(held, uniq)


def reference_match(recs, table_tags):
    """the match of a launch against a tame table whose entries are these tags in this order (sorted, no duplicates) -> (which records are kept: those whose
    tag is in the table and the DEAD ones; the entry word of each kept record: entry number + 1, 0 for a DEAD record that matched nothing)"""
    tag = recs["x"][:, 0]
    found = is_in(tag, table_tags)
    word = np.where(found, np.searchsorted(table_tags, tag) + 1, 0).astype(np.uint32)
    keep = found | ((recs["flags"] & DEAD) != 0)
    return keep, word[keep]


# ---- what a device's answer must pass (AssertionError names the first thing wrong) -----------------------------------------------------------------------------
def split_pairs(got):
    """the hand-backs of the distinguished-point table -> (the walk's records among them, the stored entries, their duplicates, in step).  Every DUPLICATE is
    directly preceded by a STORED record of its tag, and a STORED record stands nowhere else; a STORED record is (tag, 0.., d, kangaroo, type, step 0)."""
    reason = got["reserved"]
    assert reason.max(initial=0) <= R_STORED
    st, du = np.flatnonzero(reason == R_STORED), np.flatnonzero(reason == R_DUPLICATE)
    assert len(st) == len(du) and np.array_equal(st + 1, du), "every DUPLICATE directly behind a STORED record, and no other STORED record"
    stored, dup = got[st], got[du]
    assert np.array_equal(stored["x"][:, 0], dup["x"][:, 0]), "a pair is of one tag"
    assert not stored["x"][:, 1:].any() and not stored["step"].any(), "a stored entry is its tag, d, kangaroo and type alone"
    return got[reason != R_STORED], stored, dup


def check_launch(ref, sent, back, n_entries, table, before=None):
    """one launch `sent` against its reference: back = the walk's records handed back (REC, the reason in `reserved`; without the STORED records of the
    distinguished-point table), table = the table's rows read after the launch (3 or 5 columns), before = its rows before the launch.
      the entry count; the hand-backs as a multiset of (tag, reason); every handed-back record a sent one in all 64 bytes but the reason word, none twice;
      the table's tags; what stood in the table stands there unchanged; per new tag the stored entry and the handed-back copies are the copies sent."""
    assert n_entries == ref["entries"], ("entries", n_entries, ref["entries"])
    assert same_rows(rows(back["x"][:, 0], back["reserved"]), ref["back"]), "the hand-backs as a multiset of (tag, reason)"
    # the records as they were sent: (kangaroo, step) names a record of a launch, a crafted one or a walk's
    sent_id, back_id = record_ids(sent), record_ids(back)
    order = np.argsort(sent_id, kind="stable")
    ids = sent_id[order]
    assert len(np.unique(ids)) == len(ids)
    at = np.minimum(np.searchsorted(ids, back_id), len(ids) - 1)
    assert np.array_equal(ids[at], back_id), "a handed-back record names a record that was sent"
    a, b = np.ascontiguousarray(back).view(np.uint32).reshape(-1, 16), np.ascontiguousarray(sent[order[at]]).view(np.uint32).reshape(-1, 16)
    assert np.array_equal(a[:, :15], b[:, :15]), "a handed-back record equals the sent one in all but the reason word"
    assert len(np.unique(back_id)) == len(back), "no sent record comes back twice"
    # the table
    table = table[np.argsort(table[:, 0], kind="stable")]
    assert np.array_equal(table[:, 0], ref["tags"]), "the table's tags"
    if before is not None and len(before):
        before = before[np.argsort(before[:, 0], kind="stable")]
        assert np.array_equal(table[is_in(table[:, 0], before[:, 0])], before), "what stood in the table stands there unchanged"
    # per new tag: stored + handed back = sent
    k = table.shape[1]
    stored = table[is_in(table[:, 0], ref["new_tags"])]
    dup = back[(back["reserved"] == R_DUPLICATE) & is_in(back["x"][:, 0], ref["new_tags"])]
    came = rows(dup["x"][:, 0], dup["d"][:, 0], dup["d"][:, 1], dup["kangaroo"], entry_type(dup["flags"]))[:, :k]
    assert same_rows(np.concatenate([stored, came]), ref["cand"][:, :k]), "per new tag the stored entry and the handed-back copies are exactly the copies sent"


def check_pairs(stored, dup, table):
    """the pairs of a launch on the distinguished-point table against the table read after it (5 columns): the STORED record of every pair is the entry the
    table holds for the tag, so all copies of a tag name one entry"""
    table = table[np.argsort(table[:, 0], kind="stable")]
    if not len(stored):
        return
    at = np.minimum(np.searchsorted(table[:, 0], stored["x"][:, 0]), len(table) - 1)
    named = rows(stored["x"][:, 0], stored["d"][:, 0], stored["d"][:, 1], stored["kangaroo"], stored["flags"])
    assert np.array_equal(named, table[at]), "the STORED record of a pair is the table's entry of the tag"


def check_loaded(counts, n_entries, table, want_counts, want_tags, entries):
    """a load of `entries` (DP_ENTRY) into an empty table: the four counts, the entry count, the tags, and every entry of the table one of those sent (d.lo
    numbers them) -- with its owner when the table has owners"""
    assert tuple(counts) == tuple(want_counts) and n_entries == len(want_tags), (counts, n_entries, want_counts, len(want_tags))
    table = table[np.argsort(table[:, 0], kind="stable")]
    assert np.array_equal(table[:, 0], want_tags), "the table's tags"
    assert (table[:, 1] < len(entries)).all()
    assert np.array_equal(table, entry_rows(entries[table[:, 1].astype(np.int64)])[:, :table.shape[1]]), "every entry of the table is one that was sent"


def check_sorted(tags, d, unsorted):
    """read_sorted's (tags, offsets) against the rows of gen_read: strictly ascending, the same tags, each with its own d"""
    got = pair_rows(tags, d)
    assert len(got) < 2 or (got[1:, 0] > got[:-1, 0]).all(), "ascending, no tag twice"
    assert np.array_equal(got, unsorted[np.argsort(unsorted[:, 0], kind="stable")]), "the tags of the table, each with its own d"


# ---- occupancy without probing order -------------------------------------------------------------------------------------------------------------------------
def occupied(tags, slots):
    """which slots a table of these (different, non-zero) tags occupies: with linear probing that does not depend on the order of insertion.  c[s] tags have
    their home at s; the tags pushed on from slot s are w[s] = max(0, w[s-1] + c[s] - 1), and s is occupied when w[s-1] + c[s] >= 1.  Two laps: the second
    starts from the true carry, since a table that is not full has a slot nothing is pushed into."""
    assert len(tags) < slots
    c = np.bincount(home(tags, slots).astype(np.int64), minlength=slots).astype(np.int64)
    a = np.concatenate([c, c]) - 1
    p = np.cumsum(a)
    w = p - np.minimum(0, np.minimum.accumulate(p))
    prev = np.concatenate([[0], w[:-1]])
    return (prev + a >= 0)[slots:]


def longest_run(occ):
    """the longest run of occupied slots, the table taken as a ring: no record of the table's tags probes more slots than that, plus one"""
    empty = np.flatnonzero(~occ)
    if not len(empty):
        return len(occ)
    gaps = np.diff(empty) - 1
    return int(max(gaps.max(initial=0), empty[0] + len(occ) - empty[-1] - 1))


def assert_far_from_full(tags, slots):
    """the condition of every scale launch, on the tag set it leaves behind: at most 70 % of the slots taken, no probe chain above 4096"""
    assert len(tags) <= MAX_LOAD * slots, ("load", len(tags), slots)
    run = longest_run(occupied(tags, slots))
    assert run <= MAX_CHAIN, ("chain", run)
    return len(tags) / slots, run


# ---- generators: seeded, vectorised ----------------------------------------------------------------------------------------------------------------------------
CHAIN_A_HOME, CHAIN_A_LEN = 0x123456, 4096                            # a chain with one home slot in the middle of the table ...
CHAIN_B_HOME, CHAIN_B_LEN = SLOTS - 1, 2048                           # ... and one whose home is the last slot: it runs on from slot 0
GUARD = 4096                                                          # no random tag has its home this close in front of a chain, inside it or at its end:
                                                                      # the chains are the longest runs of the table, exactly as long as they are made
FLAG_CHOICES = np.array([0, WILD, WILD | NEG, WILD | LAST_VALID | 37 << LAST_SHIFT, WILD | NEG | LAST_VALID | 4095 << LAST_SHIFT], np.uint32)


def guarded(homes, slots=SLOTS):
    """homes a random tag must not have"""
    h = np.asarray(homes, np.int64)
    a = (h >= CHAIN_A_HOME - GUARD) & (h <= CHAIN_A_HOME + CHAIN_A_LEN)
    b = (h >= slots - 1 - GUARD) | (h <= CHAIN_B_LEN - 1)              # the chain takes the last slot and 0 .. CHAIN_B_LEN - 2; CHAIN_B_LEN - 1 stays empty
    return a | b


def random_tags(rng, n, slots=SLOTS):
    """n different non-zero tags in random order, none with a guarded home"""
    t = rng.integers(1, 1 << 64, size=n + n // 50 + 4096, dtype=np.uint64, endpoint=False)
    t = np.unique(t[~guarded(home(t, slots), slots)])
    assert len(t) >= n
    return rng.permutation(t)[:n]


def chain_tags(rng, home_slot, n, slots=SLOTS):
    """n different non-zero tags with the one home slot"""
    bits = slots.bit_length() - 1
    hi = np.unique(rng.integers(1, 1 << (58 - bits), size=2 * n, dtype=np.uint64))
    assert len(hi) >= n
    hi = rng.permutation(hi)[:n]
    t = rng.integers(0, 64, size=n, dtype=np.uint64) | np.uint64(home_slot << 6) | (hi << np.uint64(6 + bits))
    assert (home(t, slots) == home_slot).all() and len(np.unique(t)) == n
    return t


def make_records(rng, tags, flags, launch):
    """a launch of these tags and flags: every record with its own d, kangaroo and step (`kangaroo` numbers the records: launch << 20 | position), the upper
    words of x random, and a reason word the device has to overwrite"""
    n = len(tags)
    assert n < 1 << 20 and launch < 1 << 12
    r = np.zeros(n, REC)
    i = np.arange(n, dtype=np.uint64)
    r["x"][:, 0] = tags
    r["x"][:, 1:] = rng.integers(0, 1 << 64, size=(n, 3), dtype=np.uint64, endpoint=False)
    r["d"][:, 0] = (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(launch)      # odd multiplier: different for every position
    r["d"][:, 1] = rng.integers(0, 1 << 64, size=n, dtype=np.uint64, endpoint=False)
    r["kangaroo"] = (launch << 20) | i.astype(np.uint32)
    r["flags"] = flags
    r["step"] = (i.astype(np.uint32) * np.uint32(2654435761)) ^ np.uint32(launch)                # odd multiplier again
    r["reserved"] = 0xC0DE0000 | (i.astype(np.uint32) & 0xFFFF)
    return r


MAIN_GROUPS = ((2, 30000), (3, 3000), (64, 64), (4096, 8))           # (copies, tags): the copies at uniformly random positions of the whole launch
LANE5_WAVES, N_ZERO, N_DEAD = 512, 1000, 1000
TAIL_ZERO, TAIL_DEAD = (0, 7, 36), (1, 20, 35)                        # lanes of the ragged last wave that hold a tag-0 and a DEAD record


def main_launch(rng):
    """the launch of N1 records the issue describes -> (records, plan); plan says where everything stands, for the test of this generator"""
    n, waves = N1, N1 // 64
    tags = np.zeros(n, np.uint64)
    flags = rng.choice(FLAG_CHOICES, size=n)
    free = np.ones(n, bool)
    plan = {}
    # fixed positions: one tag in all lanes of a wave, one tag in lane 5 of 512 other waves (the ragged one may be among them), the tail's tag 0 and DEAD
    w = rng.permutation(waves + 1)
    whole = int(w[w < waves][0])
    lane5 = np.sort(w[w != whole][:LANE5_WAVES])
    pool = random_tags(rng, 2 + sum(t for _, t in MAIN_GROUPS) + N_DEAD + n)
    cursor = [0]

    def fresh(k):
        cursor[0] += k
        return pool[cursor[0] - k:cursor[0]]

    plan["whole"] = (int(fresh(1)[0]), whole)
    tags[64 * whole:64 * whole + 64] = plan["whole"][0]
    free[64 * whole:64 * whole + 64] = False
    plan["lane5"] = (int(fresh(1)[0]), lane5)
    tags[64 * lane5 + 5] = plan["lane5"][0]
    free[64 * lane5 + 5] = False
    tail0 = n - 37
    zero_tail, dead_tail = tail0 + np.array(TAIL_ZERO), tail0 + np.array(TAIL_DEAD)
    assert free[zero_tail].all() and free[dead_tail].all()
    free[zero_tail] = free[dead_tail] = False
    rest = rng.permutation(np.flatnonzero(free))
    at = [0]

    def places(k):
        at[0] += k
        return rest[at[0] - k:at[0]]

    plan["groups"] = {}
    for copies, n_tags in MAIN_GROUPS:
        t = fresh(n_tags)
        tags[places(copies * n_tags)] = np.repeat(t, copies)
        plan["groups"][copies] = t
    plan["chain_a"], plan["chain_b"] = chain_tags(rng, CHAIN_A_HOME, CHAIN_A_LEN), chain_tags(rng, CHAIN_B_HOME, CHAIN_B_LEN)
    tags[places(CHAIN_A_LEN)] = plan["chain_a"]
    tags[places(CHAIN_B_LEN)] = plan["chain_b"]
    plan["zero"] = np.concatenate([zero_tail, places(N_ZERO - len(zero_tail))])
    plan["dead"] = np.concatenate([dead_tail, places(N_DEAD - len(dead_tail))])
    singles = places(len(rest) - at[0])
    plan["singles"] = fresh(len(singles))
    tags[singles] = plan["singles"]
    tags[plan["zero"]] = 0
    # the DEAD records: tags that stand nowhere else, tags of live records of this launch (which are stored all the same), tag 0; some with CYCLE
    d = plan["dead"]
    third = len(d) // 3
    tags[d[:third]] = fresh(third)
    tags[d[third:2 * third]] = plan["singles"][:third]
    tags[d[2 * third:]] = 0
    flags[d] = DEAD | rng.choice(np.array([0, WILD, WILD | CYCLE, WILD | NEG | CYCLE], np.uint32), size=len(d))
    return make_records(rng, tags, flags, 1), plan


def fresh_launch(rng, n, launch):
    return make_records(rng, random_tags(rng, n), rng.choice(FLAG_CHOICES, size=n), launch)


def mixed_launch(rng, held, n, launch):
    """half fresh tags, half tags the table holds (drawn with repetition: some of them twice), at random positions"""
    t = np.concatenate([random_tags(rng, n - n // 2), rng.choice(held, size=n // 2)])
    return make_records(rng, rng.permutation(t), rng.choice(FLAG_CHOICES, size=n), launch)


LOAD_PLAN = {"once": 900000, "twice_in_1": 40000, "both_chunks": 68000, "zero_1": 576, "again_in_2": 20000, "twice_in_2": 10000, "zero_2": 144}


def load_pairs(rng):
    """LOAD_PAIRS entries for a load in two chunks -> (DP_ENTRY array, plan): duplicates inside each chunk and across the two, tag 0 in both.  d.lo numbers
    the entries, so every entry is different.  The growing tame table takes the tags and the offsets of the same array."""
    L = LOAD_PLAN
    n2 = LOAD_PAIRS - LOAD_CHUNK
    fresh_2 = n2 - L["both_chunks"] - L["again_in_2"] - 2 * L["twice_in_2"] - L["zero_2"]
    assert L["once"] + 2 * L["twice_in_1"] + L["both_chunks"] + L["zero_1"] == LOAD_CHUNK and fresh_2 > 0
    pool = random_tags(rng, L["once"] + L["twice_in_1"] + L["both_chunks"] + L["twice_in_2"] + fresh_2)
    once, tw1, both, tw2, fr2 = np.split(pool, np.cumsum([L["once"], L["twice_in_1"], L["both_chunks"], L["twice_in_2"]]))
    again = rng.choice(once, size=L["again_in_2"], replace=False)
    c1 = rng.permutation(np.concatenate([once, tw1, tw1, both, np.zeros(L["zero_1"], np.uint64)]))
    c2 = rng.permutation(np.concatenate([both, again, tw2, tw2, fr2, np.zeros(L["zero_2"], np.uint64)]))
    e = np.zeros(LOAD_PAIRS, DP_ENTRY)
    e["tag"] = np.concatenate([c1, c2])
    e["d"][:, 0] = np.arange(LOAD_PAIRS, dtype=np.uint64)
    e["d"][:, 1] = rng.integers(0, 1 << 64, size=LOAD_PAIRS, dtype=np.uint64, endpoint=False)
    e["kangaroo"] = rng.integers(0, 1 << 32, size=LOAD_PAIRS, dtype=np.uint32, endpoint=False)
    e["type"] = rng.choice(np.array([0, WILD, WILD | NEG], np.uint32), size=LOAD_PAIRS)
    return e, {"once": once, "twice_in_1": tw1, "both_chunks": both, "again_in_2": again, "twice_in_2": tw2, "fresh_2": fr2}


@functools.lru_cache(maxsize=None)
def scale_case():
    """everything the scale tests send, built once: the four launches on one table with their references in a row, and the entries of the load.  The
    conditions on load and chains are asserted here, on the CPU, before anything reaches a device."""
    rng = np.random.default_rng(20261021)
    main, plan = main_launch(rng)
    launches, refs, held = [], [], np.zeros(0, np.uint64)
    fresh = fresh_launch(rng, N1, 3)
    for name, recs in (("main", main), ("again", main), ("fresh", fresh), ("mixed", None)):
        if recs is None:
            recs = mixed_launch(rng, held, N1, 4)
        ref = reference(held, recs)
        ref["load"], ref["chain"] = assert_far_from_full(ref["tags"], SLOTS)
        launches.append((name, recs))
        refs.append(ref)
        held = ref["tags"]
    assert 0.40 <= refs[2]["load"] <= 0.50 and refs[3]["load"] <= 0.60
    entries, load_plan = load_pairs(rng)
    counts, tags = reference_load(np.zeros(0, np.uint64), entries["tag"])
    assert_far_from_full(tags, SLOTS)
    return {"launches": launches, "refs": refs, "plan": plan, "entries": entries, "load_plan": load_plan, "load_counts": counts, "load_tags": tags}
