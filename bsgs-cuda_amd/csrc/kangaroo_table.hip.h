// kangaroo_table.hip.h -- the device side of the one table that kangaroo_tames_gen.hip, kangaroo_tames_extend.hip and kangaroo_dptable.hip keep in device
// memory (struct KangTable and its host functions: bsgs_internal.h; DESIGN.md 10, "The table in device memory").  Included by those three units only.
//   table     open addressing with linear probing, nothing is ever deleted: tag[slots] (u64, the low 64 bits of x; 0 = empty, eight tags to a 64-byte line),
//             d[slots] (16-byte vectors, the offset as the record holds it) and, for the distinguished-point table, who[slots].  slots is a power of two, at
//             least KT_MIN_SLOTS.  Home slot (tag >> 6) & (slots - 1), as in the search's image.
//   counters  ctr[8] (u64), indexed by CTR_*: entries in the table, occupied slots met by the last harvest, the four outcomes of a load, OR and AND of the tags.
//   equal tags in one launch: which of them is stored is unspecified; exactly one is, the others are duplicates.
// Vector stores only, every store bounded by its caller; no LDS, no scratch.
#pragma once
#include "bsgs_internal.h"

#define KT_MIN_SLOTS 128ull
#define KT_MAX_CAPACITY (1ull << 31)
#define KT_INSERT_GRID_MAX 1024u                            // blocks of an insert (and the resolve): four per CU; a wave strides over the records
#define KT_SCAN_GRID_MAX 4096u                              // blocks of a load, a harvest, the sort's gather

#define CTR_ENTRIES 0
#define CTR_MET 1
#define CTR_STORED 2                                        // (the outcomes of kt_claim are named by the counter a load gives them)
#define CTR_DUPLICATE 3
#define CTR_ZERO 4
#define CTR_FULL 5
#define CTR_OR 6
#define CTR_AND 7

// The claim: `tag` (not 0) takes a slot from its home slot on, wrapping, after at most slot_mask + 1 probes.  CTR_STORED: slot s was empty and is this tag's
// now, fill(s) has written what belongs to it (one vector store per array); CTR_DUPLICATE: slot s holds the tag already; CTR_FULL: no slot.
// Coherence: L2 is not coherent across XCDs within a kernel, and the records of one launch are inserted from all of them.  A SLOT'S TAG IS DECIDED ONLY BY THE
// RETURN VALUE OF THE COMPARE-AND-SWAP, which is carried out where every XCD sees it.  A plain load might be used as a shortcut only when it shows a non-zero
// tag (slots never change once set, so a non-zero tag seen anywhere is final); a plain load must never be used to conclude that a slot is empty -- no kernel
// that inserts makes a plain load of a tag at all.  What fill() wrote is read only by a kernel launched after this one (a resolve, a harvest).
template <class Fill> __device__ __forceinline__ u32 kt_claim(u64 *tags, u64 slot_mask, u64 tag, u64 &s, Fill fill)
{
    s = (tag >> 6) & slot_mask;
    for (u64 it = 0; it <= slot_mask; it++) {
        const u64 old = atomicCAS((unsigned long long *)&tags[s], 0ull, (unsigned long long)tag);      // the only way a tag is read
        if (old == 0ull) { fill(s); return CTR_STORED; }
        if (old == tag) return CTR_DUPLICATE;
        s = (s + 1ull) & slot_mask;
    }
    return CTR_FULL;
}

// one atomic per wave: the first lane of m adds the number of m's lanes to *counter.  Every lane of the wave passes the same m.
__device__ __forceinline__ void kt_count(u64 *counter, u64 m, u32 lane)
{
    if (m && (int)lane == __builtin_ctzll(m)) atomicAdd((unsigned long long *)counter, (unsigned long long)__builtin_popcountll(m));
}

// The wave's reservation in a dense array, reached by every lane of the wave: the lanes with `pred` take consecutive places in lane order, plus `add`
// (wave-uniform) behind them, with one atomic on *counter.  -> this lane's place (meaningless without pred); the caller bounds its store.
__device__ __forceinline__ u64 kt_reserve(bool pred, u32 lane, u64 *counter, u32 add)
{
    const u64 m = __ballot(pred);
    if (!m) return 0;
    u64 pos0 = 0;
    const int leader = __builtin_ctzll(m);
    if ((int)lane == leader) pos0 = atomicAdd((unsigned long long *)counter, (unsigned long long)(__builtin_popcountll(m) + add));
    pos0 = __shfl(pos0, leader);
    return pos0 + (u64)__builtin_popcountll(m & ((1ull << lane) - 1));
}

// the outcomes of a load, reached by every lane of the wave: `what` is 0 (no entry in this lane) or CTR_STORED..CTR_FULL; one atomic per wave and outcome,
// and what was stored is an entry more
__device__ __forceinline__ void kt_count_outcomes(u64 *ctr, u32 what, u32 lane)
{
    for (u32 k = CTR_STORED; k <= CTR_FULL; k++) {
        const u64 m = __ballot(what == k);
        kt_count(&ctr[k], m, lane);
        if (k == CTR_STORED) kt_count(&ctr[CTR_ENTRIES], m, lane);
    }
}
