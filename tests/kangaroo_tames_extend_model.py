"""Pure-Python restatement of what stands around the tame table grown on the device (include/bsgs_hip.h, "Kangaroo, tame table grown on the device", the
paragraphs "load" and "sorted read"; csrc/kangaroo_tames_extend.hip): the load of (tag, d) pairs with its four counts, the sorted and cut read, which passes
of the radix sort run, and the host's rules for extending a table and merging tables (host/host_kangaroo_tames.cpp).  The table is the one of
tests/kangaroo_tames_gen_model.py (new_table, n_slots, home).  A test model: no product code runs here."""
import kangaroo_model as K
import kangaroo_tames_gen_model as GM

M64 = GM.M64
LOAD_CHUNK = 1 << 20                                                  # BSGS_KANGAROO_TAMES_LOAD_CHUNK: pairs staged per kernel
SORT_TILE = 2048                                                      # BSGS_KANGAROO_TAMES_SORT_TILE: entries per block and pass of the sort


def load(table, pairs):
    """pairs = [(tag, d)] -> (the new table, {"stored", "duplicate", "zero", "full"}).  The insert's rule without hand-backs: a pair with tag 0 is counted and
    skipped; every other pair looks from its home slot on, wrapping, at most `slots` slots: an empty slot takes it, a slot with its tag makes it a duplicate.
    Of several pairs with one tag that is new to the table exactly one is stored, which one is unspecified: cand[tag] holds every d that may stand there."""
    slots = table["slots"]
    tags, cand = list(table["tags"]), {t: set(c) for t, c in table["cand"].items()}
    n = {"stored": 0, "duplicate": 0, "zero": 0, "full": 0}
    fresh = set()
    for tag, d in pairs:
        assert 0 <= tag <= M64
        if tag == 0:
            n["zero"] += 1
            continue
        s = GM.home(tag, slots)
        for _ in range(slots):
            if tags[s] == 0:
                tags[s] = tag
                cand[tag] = {d & K.M128}
                fresh.add(tag)
                n["stored"] += 1
                break
            if tags[s] == tag:
                n["duplicate"] += 1
                if tag in fresh:
                    cand[tag].add(d & K.M128)
                break
            s = (s + 1) & (slots - 1)
        else:
            n["full"] += 1
    assert sum(n.values()) == len(pairs)
    return {"slots": slots, "tags": tags, "cand": cand}, n


def read_sorted(table, max_entries=None):
    """-> (the entries ascending by tag, cut to the max_entries lowest, as [(tag, the set of offsets one of which stands there)], the full count)"""
    full = sorted(table["cand"].items())
    return (full if max_entries is None else full[:max_entries]), len(full)


def sort_passes(tags):
    """the digit shifts whose pass the radix sort runs: those on which not every tag has the same 8 bits (a zero byte of OR ^ AND costs no pass)"""
    if not tags:
        return []
    any_, all_ = 0, M64
    for t in tags:
        any_ |= t
        all_ &= t
    return [s for s in range(0, 64, 8) if ((any_ ^ all_) >> s) & 255]


def radix_sort(pairs, tile=SORT_TILE):
    """the sort as the device runs it: stable passes of 8-bit digits, low digit first, skipping the constant ones; each pass places tile b's entries of digit v
    at (entries of the digits below v) + (entries of digit v in the tiles before b) + (their rank inside the tile) -> the pairs ascending by tag"""
    cur = list(pairs)
    for shift in sort_passes([t for t, _ in cur]):
        nb = (len(cur) + tile - 1) // tile
        counts = [[0] * nb for _ in range(256)]
        for i, (t, _) in enumerate(cur):
            counts[(t >> shift) & 255][i // tile] += 1
        start, run = [[0] * nb for _ in range(256)], 0
        for v in range(256):
            for b in range(nb):
                start[v][b] = run
                run += counts[v][b]
        out = [None] * len(cur)
        for i, (t, d) in enumerate(cur):
            v, b = (t >> shift) & 255, i // tile
            out[start[v][b]] = (t, d)
            start[v][b] += 1
        cur = out
    return cur


# ---- the host's rules -----------------------------------------------------------------------------------------------------------------------------------------
def merge(tables, T=None):
    """tables = [[(tag, d)] strictly ascending]: one entry per tag, the first table that has the tag wins -> (the union ascending, cut to the T lowest tags;
    the tags dropped because an earlier table had them).  T above the union: ValueError"""
    seen, dropped = {}, 0
    for tab in tables:
        for t, d in tab:
            if t in seen:
                dropped += 1
            else:
                seen[t] = d
    out = sorted(seen.items())
    if T is not None:
        if T > len(out):
            raise ValueError("-ktn above the union")
        out = out[:T]
    return out, dropped


def extend_refusal(file_T, file_seed, file_dp, T, seed, dp=None, ktamesdev=True, ktnplan=None):
    """why -ktamesgen OUT -ktamesfrom IN -ktn T is refused before any device is looked for, or None"""
    if not ktamesdev:
        return "-ktamesfrom belongs to -ktamesgen -ktamesdev"
    if ktnplan is not None:
        return "-ktnplan cannot be combined with -ktamesfrom"
    if T <= file_T:
        return "-ktn must be above the entries of the table that is extended"
    if seed == file_seed:
        return "-kseed is the seed the table was made with"
    if dp is not None and dp != file_dp:
        return "-dp differs from the table's"
    return None
