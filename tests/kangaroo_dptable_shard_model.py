"""Pure-Python restatement of the distinguished-point table divided over engines (include/bsgs_hip.h, "Kangaroo, distinguished-point table divided over
engines"), built on tests/kangaroo_dptable_model.py: the shard function, the routing of a launch, and a relay that delivers every routed group to its shard.
A test model: no product code runs here.

A record is (tag, d, flags, kangaroo) as in the unsharded model; `kangaroo` is the index in the engine's herd where a launch produced it and the global id
base + index wherever it went from there."""
import kangaroo_model as K
import kangaroo_dptable_model as DM

MAX_SHARDS = 16
M64 = DM.M64


def shard(tag, shards):
    """bits 48..63 of the tag, scaled: below `shards` for every tag"""
    assert 1 <= shards <= MAX_SHARDS and 0 <= tag <= M64
    return ((tag >> 48) * shards) >> 16


def routable(rec):
    """a live record with a tag: the only kind that belongs to a shard"""
    tag, _, fl, _ = rec
    return not fl & K.DEAD and tag != 0


def with_base(rec, base):
    tag, d, fl, kang = rec
    return (tag, d, fl, kang + base)


def split(records, own, shards, base=0):
    """a launch of engine `own` -> (its own records, [routed group per shard]), every id made global.  DEAD and tag-0 records stay whatever their tag bits."""
    mine, groups = [], [[] for _ in range(shards)]
    for rec in records:
        g = with_base(rec, base)
        to = shard(rec[0], shards) if routable(rec) else own
        (mine if to == own else groups[to]).append(g)
    return mine, groups


def insert(table, records, own, shards, base=0):
    """one launch on shard `own` -> (the new table, the hand-backs, the routed groups): the unsharded insert of the shard's own records"""
    mine, groups = split(records, own, shards, base)
    new, back = DM.insert(table, mine)
    return new, back, groups


def relay(tables, launches, bases):
    """launches[e]: the records of engine e's launch.  Every engine inserts its launch, then every routed group is inserted on its shard (ids global, base
    0; nothing is routed a second time) -> (the new tables, hand-backs per engine)"""
    shards = len(tables)
    tables, backs, inbox = list(tables), [[] for _ in range(shards)], [[] for _ in range(shards)]
    for e in range(shards):
        tables[e], back, groups = insert(tables[e], launches[e], e, shards, bases[e])
        backs[e] += back
        for to, g in enumerate(groups):
            inbox[to] += g
    for e in range(shards):
        tables[e], back, groups = insert(tables[e], inbox[e], e, shards)
        assert not any(groups)
        backs[e] += back
    return tables, backs


def duplicate_pairs(backs):
    """the DUPLICATE hand-backs as (tag, the record's kangaroo) -- which stored entry a record met depends on the order only where tags are fresh"""
    return sorted((rec[0], rec[3]) for reason, rec, _ in backs if reason == DM.DPT_DUPLICATE)
