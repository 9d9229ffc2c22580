// kangaroo_dptable_shard.hip -- the distinguished-point table of a search divided over several engines (include/bsgs_hip.h, "Kangaroo, distinguished-point
// table divided over engines"; tests/kangaroo_dptable_shard_model.py restates it).  Every engine holds the table of kangaroo_dptable.hip for its
// share of the tags, shard(tag) = ((tag >> 48) * E) >> 16, and every record that leaves the device names its kangaroo by the global id base + local.  The
// table, its claim and the coherence rule: kangaroo_table.hip.h.
//   insert    the insert of kangaroo_dptable.hip -- one record per lane, a wave strides, DEAD and tag-0 records handed back, a duplicate handed back as a
//             PAIR behind a placeholder, no slot handed back as FULL, one reservation and one count per wave, every store bounded -- for the records of this
//             shard; a live record of another shard is FOREIGN: it takes no slot and no place among the hand-backs and is counted for its destination.
//             A wave keeps its sixteen counts in registers over all its strides and adds them to hist[] at its end: one atomic per wave and destination.
//   scatter   a second kernel behind the insert, when every count is final: the foreign records go into the outbox, ONE buffer of `cap` records in which
//             the group of destination s starts at hist[0] + .. + hist[s - 1].  A wave counts its own foreign records again (the same strides, so the same
//             counts), takes all its places of a group with one atomic on cursor[s], and deals them out in a second pass over its strides.  Every store
//             bounded by the buffer's capacity.
//   resolve, load, harvest: those of kangaroo_dptable.hip; the host side is that unit's too (bsgs_kang_dpt_*).
// The loop over the destinations of a wave (dpt_each_dest) is wave-uniform: ballot the pending lanes, take the first one's destination, ballot the lanes
// that share it, serve them, at most `shards` times.  What a wave keeps per destination (DptPerDest) is wave-uniform too and reached by compare-and-select
// over all sixteen, never by an index: registers, no scratch.  (With an atomic per stride and destination in both kernels a launch of 2.1e6 records cost
// 4.9 ms more at E = 8 than the one table's insert: 2 x 229 000 atomics on seven addresses, seven round trips in a row per wave and stride.)
#include "kangaroo_table.hip.h"

#define DPT_KEEP 0xFFFFFFFFu                                // (not a reason: the record went into the table)
#define DPT_MAX_SHARDS BSGS_KANGAROO_DPT_MAX_SHARDS

__device__ __forceinline__ u32 dpt_type(u32 flags) { return (flags & BSGS_KANGAROO_WILD) ? (flags & (BSGS_KANGAROO_WILD | BSGS_KANGAROO_NEG)) : 0u; }
__device__ __forceinline__ u32 dpt_shard_of(u32 tag_hi, u32 shards) { return ((tag_hi >> 16) * shards) >> 16; }      // bits 48..63 of the tag: below `shards`

struct DptShardArgs {
    const u32 *rec;        // the walk's record buffer: u64 count | records
    u64 *tag;              // [slots]
    u32x4 *d;              // [slots]
    u32x2 *who;            // [slots]
    u32 *out;              // the hand-backs: u64 places taken, u64 records handed back | records; `reserved` = BSGS_KANGAROO_DPT_*
    u64 *ctr;              // the table's counters
    u64 *route;            // the outbox: hist[16], cursor[16] | records from byte KANG_ROUTE_HEADER
    u64 slot_mask;
    u32 cap;               // records read at most, and the records the outbox holds
    u32 out_cap;           // places of `out`
    u32 shard, shards;     // this table's share
    u32 base;              // added to every kangaroo id that is stored or leaves
};

// sixteen wave-uniform words, one per destination
struct DptPerDest {
    u32 v[DPT_MAX_SHARDS];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (u32 t = 0; t < DPT_MAX_SHARDS; t++) v[t] = 0;
    }
    __device__ __forceinline__ u32 get(u32 to) const {
        u32 r = 0;
#pragma unroll
        for (u32 t = 0; t < DPT_MAX_SHARDS; t++) r = t == to ? v[t] : r;
        return r;
    }
    __device__ __forceinline__ void add(u32 to, u32 c) {
#pragma unroll
        for (u32 t = 0; t < DPT_MAX_SHARDS; t++) v[t] += t == to ? c : 0u;
    }
};

// serve(dest, m) for every destination present among the wave's lanes with `foreign`: m = the lanes bound for it.  Reached by every lane of the wave.
template <class Serve> __device__ __forceinline__ void dpt_each_dest(bool foreign, u32 dest, u32 shards, Serve serve)
{
    u64 pending = __ballot(foreign);
    for (u32 it = 0; it < shards && pending; it++) {                 // every turn serves one destination: at most shards - 1 of them exist
        const u32 to = (u32)__builtin_amdgcn_readlane((int)dest, __builtin_ctzll(pending));      // (a scalar: what hangs on it stays wave-uniform)
        const u64 m = __ballot(foreign && dest == to);
        serve(to, m);
        pending &= ~m;
    }
}

__global__ void __launch_bounds__(256) kangaroo_dptable_shard_insert_kernel(const DptShardArgs A)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 count = *(const u64 *)A.rec;
    const u32 n = count < (u64)A.cap ? (u32)count : A.cap;           // what the walk wrote; the rest was counted only
    const u32 stride = gridDim.x * blockDim.x;
    const u32x4 *const recs = (const u32x4 *)((const char *)A.rec + KANG_REC_HEADER);
    DptPerDest cnt;
    cnt.clear();
    for (u32 base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n; base += stride) {      // wave-uniform: every lane reaches the ballots
        const u32 i = base + lane;
        u32 reason = DPT_KEEP, dest = 0;
        bool stored = false, foreign = false;
        u64 s = 0;
        u32x4 r0 = {0, 0, 0, 0}, r3 = {0, 0, 0, 0};
        if (i < n) {
            r0 = recs[(u64)i * 4];
            r3 = recs[(u64)i * 4 + 3];
            r3.x += A.base;                                          // the global id, wherever the record goes
            const u64 tag = ((u64)r0.y << 32) | r0.x;
            dest = dpt_shard_of(r0.y, A.shards);
            if (r3.y & BSGS_KANGAROO_DEAD) reason = BSGS_KANGAROO_DPT_DEAD;
            else if (tag == 0ull) reason = BSGS_KANGAROO_DPT_TAG_ZERO;
            else if (dest != A.shard) foreign = true;
            else {
                const u32 got = kt_claim(A.tag, A.slot_mask, tag, s, [&](u64 at) {
                    A.d[at] = recs[(u64)i * 4 + 2];
                    A.who[at] = (u32x2){r3.x, dpt_type(r3.y)};
                });
                stored = got == CTR_STORED;                          // (the claim names its outcome by the counter a load gives it)
                if (!stored) reason = got == CTR_DUPLICATE ? BSGS_KANGAROO_DPT_DUPLICATE : BSGS_KANGAROO_DPT_FULL;
            }
        }
        kt_count(&A.ctr[CTR_ENTRIES], __ballot(stored), lane);
        dpt_each_dest(foreign, dest, A.shards, [&](u32 to, u64 m) { cnt.add(to, (u32)__builtin_popcountll(m)); });
        const bool back = reason != DPT_KEEP && !foreign, dup = reason == BSGS_KANGAROO_DPT_DUPLICATE;
        const u64 md = __ballot(dup);
        const u64 pos = kt_reserve(back, lane, (u64 *)A.out, (u32)__builtin_popcountll(md)) + (u64)__builtin_popcountll(md & ((1ull << lane) - 1));      // a duplicate takes two places
        kt_count((u64 *)A.out + 1, __ballot(back), lane);
        if (back && pos + (dup ? 1u : 0u) < A.out_cap) {             // the bound of every store: a pair goes in whole or not at all
            u32x4 *o = (u32x4 *)((char *)A.out + KANG_REC_HEADER) + pos * 4;
            if (dup) {                                               // the placeholder: the slot, for the resolve
                o[0] = (u32x4){(u32)s, (u32)(s >> 32), 0, 0};
                o[1] = (u32x4){0, 0, 0, 0};
                o[2] = (u32x4){0, 0, 0, 0};
                o[3] = (u32x4){0, 0, 0, BSGS_KANGAROO_DPT_STORED};
                o += 4;
            }
            o[0] = r0;
            o[1] = recs[(u64)i * 4 + 1];
            o[2] = recs[(u64)i * 4 + 2];
            o[3] = (u32x4){r3.x, r3.y, r3.z, reason};
        }
    }
#pragma unroll
    for (u32 t = 0; t < DPT_MAX_SHARDS; t++)                         // the header holds sixteen counts whatever `shards` is
        if (cnt.v[t] && lane == 0) atomicAdd((unsigned long long *)&A.route[t], (unsigned long long)cnt.v[t]);
}

// whether record i of the launch is foreign, and where it belongs: the insert's own classes, from the two vectors that decide them
__device__ __forceinline__ bool dpt_foreign(const u32x4 r0, const u32x4 r3, u32 shard, u32 shards, u32 &dest)
{
    dest = dpt_shard_of(r0.y, shards);
    return !(r3.y & BSGS_KANGAROO_DEAD) && (r0.x | r0.y) != 0u && dest != shard;
}

// NOTHING MAY WRITE A.rec BETWEEN THE START OF THE INSERT AND THE END OF THE SCATTER: the insert, pass 1 and pass 2 below each read the records again and
// must put every one of them into the same class, or counts, places and groups no longer agree.
// a kernel of its own behind the insert: every hist[] is final here, so a group's start is a sum of them.  The same records, the same classes; only the
// foreign ones are touched, and they are written as they came but for the id.
__global__ void __launch_bounds__(256) kangaroo_dptable_shard_scatter_kernel(const DptShardArgs A)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 count = *(const u64 *)A.rec;
    const u32 n = count < (u64)A.cap ? (u32)count : A.cap;
    const u32 stride = gridDim.x * blockDim.x;
    const u32x4 *const recs = (const u32x4 *)((const char *)A.rec + KANG_REC_HEADER);
    u32x4 *const box = (u32x4 *)((char *)A.route + KANG_ROUTE_HEADER);
    const u32 first = blockIdx.x * blockDim.x + (threadIdx.x & ~63u);
    // pass 1: what this wave will write, per destination
    DptPerDest cur;
    cur.clear();
    for (u32 base = first; base < n; base += stride) {               // wave-uniform: every lane reaches the ballots
        const u32 i = base + lane;
        u32 dest = 0;
        const bool foreign = i < n && dpt_foreign(recs[(u64)i * 4], recs[(u64)i * 4 + 3], A.shard, A.shards, dest);
        dpt_each_dest(foreign, dest, A.shards, [&](u32 to, u64 m) { cur.add(to, (u32)__builtin_popcountll(m)); });
    }
    // the wave's places: the start of each group (every count is below 2^32: the records of a launch) plus what the cursor hands out, one atomic per group
    u32 start = 0;
#pragma unroll
    for (u32 t = 0; t < DPT_MAX_SHARDS; t++) {
        const u32 mine = cur.v[t];
        u32 at = 0;
        if (mine && lane == 0) at = (u32)atomicAdd((unsigned long long *)&A.route[DPT_MAX_SHARDS + t], (unsigned long long)mine);
        cur.v[t] = start + (u32)__builtin_amdgcn_readfirstlane((int)at);
        start += (u32)A.route[t];                                    // (hist of the own shard is 0)
    }
    // pass 2: the same strides, the same classes; the records as they came but for the id
    for (u32 base = first; base < n; base += stride) {
        const u32 i = base + lane;
        u32 dest = 0;
        u32x4 r0 = {0, 0, 0, 0}, r3 = {0, 0, 0, 0};
        bool foreign = false;
        if (i < n) {
            r0 = recs[(u64)i * 4];
            r3 = recs[(u64)i * 4 + 3];
            foreign = dpt_foreign(r0, r3, A.shard, A.shards, dest);
        }
        dpt_each_dest(foreign, dest, A.shards, [&](u32 to, u64 m) {
            const u32 pos = cur.get(to) + (u32)__builtin_popcountll(m & ((1ull << lane) - 1));
            cur.add(to, (u32)__builtin_popcountll(m));
            if (((m >> lane) & 1ull) && pos < A.cap) {               // the bound of every store
                u32x4 *o = box + (u64)pos * 4;
                o[0] = r0;
                o[1] = recs[(u64)i * 4 + 1];
                o[2] = recs[(u64)i * 4 + 2];
                o[3] = (u32x4){r3.x + A.base, r3.y, r3.z, r3.w};
            }
        });
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------------
static_assert(KANG_ROUTE_HEADER == 2 * DPT_MAX_SHARDS * 8, "the outbox's header: a count and a cursor per shard");

int bsgs_kang_dpt_insert_shard_launch(bsgs_dev *d, bsgs_kangaroo *k, uint32_t blocks, uint32_t base)
{
    DptShardArgs A;
    A.rec = k->rec; A.tag = k->dpt.tag; A.d = k->dpt.d; A.who = k->dpt.who; A.out = k->dpt_out; A.ctr = k->dpt.ctr; A.route = (u64 *)k->dpt_route;
    A.slot_mask = k->dpt.slots - 1; A.cap = k->cap; A.out_cap = bsgs_kang_dpt_out_cap(k); A.shard = k->dpt_shard; A.shards = k->dpt_shards; A.base = base;
    HIPCHK(hipMemsetAsync(k->dpt_route, 0, KANG_ROUTE_HEADER, d->stream));
    hipLaunchKernelGGL(kangaroo_dptable_shard_insert_kernel, dim3(blocks), dim3(256), 0, d->stream, A);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(kangaroo_dptable_shard_scatter_kernel, dim3(blocks), dim3(256), 0, d->stream, A);
    HIPCHK(hipGetLastError());
    return BSGS_OK;
}

// the groups stand in the order of their shards and without gaps, so what is handed over is the head of the outbox and a cut falls into the last groups
int bsgs_kang_dpt_routed_out(bsgs_dev *d, bsgs_kangaroo *k, uint64_t held, const DptRouted *rt, uint64_t *cut)
{
    uint64_t hist[DPT_MAX_SHARDS];
    HIPCHK(hipMemcpyAsync(hist, k->dpt_route, sizeof hist, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    const uint64_t room = rt->recs ? rt->max : 0;
    uint64_t at = 0, lost = 0;
    for (uint32_t s = 0; s < k->dpt_shards; s++) {
        const uint64_t n = s == k->dpt_shard ? 0 : std::min<uint64_t>(hist[s], held - std::min(held, at));      // (never more than the records there were)
        const uint64_t give = std::min<uint64_t>(n, room - std::min(room, at));
        rt->n[s] = (uint32_t)give;
        lost += n - give;
        at += n;
    }
    const uint64_t give = std::min<uint64_t>(at, room);              // at <= held <= cap: one piece of the herd's pinned buffer, which holds cap records
    if (give) {
        HIPCHK(hipMemcpyAsync(k->rec_host, (const char *)k->dpt_route + KANG_ROUTE_HEADER, give * 64, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
        memcpy(rt->recs, k->rec_host, give * 64);
    }
    *cut = lost;
    return BSGS_OK;
}

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int bsgs_kangaroo_dptable_begin_shard(bsgs_dev *d, uint64_t capacity, uint32_t shard, uint32_t shards, uint32_t kangaroo_base)
{
    if (shards < 1 || shards > DPT_MAX_SHARDS || shard >= shards)
        return fail(BSGS_ERR_ARG, "shard %u of %u: 1..%u shards, the shard below their number", shard, shards, DPT_MAX_SHARDS);
    if (int rc = bsgs_kang_dpt_begin(d, capacity, BSGS_DPT_SHARDED)) return rc;
    bsgs_kangaroo *k = d->kangaroo;
    const size_t bytes = KANG_ROUTE_HEADER + (size_t)k->cap * 64;
    const hipError_t e = hipMalloc(&k->dpt_route, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        k->dpt_route = nullptr;
        (void)bsgs_kangaroo_dptable_end(d);                          // after any failure no table is left
        return fail(BSGS_ERR_NOMEM, "distinguished-point table divided over engines: %llu bytes for the outbox (%s)", (unsigned long long)bytes, hipGetErrorString(e));
    }
    k->dpt_shard = shard; k->dpt_shards = shards; k->dpt_base = kangaroo_base;
    return BSGS_OK;
}

extern "C" int bsgs_kangaroo_run_dptable_shard(bsgs_dev *d, uint32_t steps, bsgs_kangaroo_record *recs, uint32_t max_recs, uint32_t *nrecs, bsgs_kangaroo_record *routed,
                                               uint32_t max_routed, uint32_t *n_routed, uint64_t *n_seen, uint64_t *n_entries, uint64_t *dropped, float *kernel_ms)
{
    if (!d || !n_routed) return fail(BSGS_ERR_ARG, "null");
    const DptRouted rt = {routed, max_routed, n_routed, d->kangaroo ? d->kangaroo->dpt_base : 0u};
    return bsgs_kang_dpt_run(d, BSGS_DPT_SHARDED, steps, recs, max_recs, nrecs, n_seen, n_entries, dropped, kernel_ms, &rt);
}

extern "C" int bsgs_kangaroo_dptable_insert_shard(bsgs_dev *d, const bsgs_kangaroo_record *recs_in, uint32_t n, bsgs_kangaroo_record *recs_out, uint32_t max_recs,
                                                  uint32_t *nrecs, bsgs_kangaroo_record *routed, uint32_t max_routed, uint32_t *n_routed, uint64_t *n_entries,
                                                  uint64_t *dropped)
{
    if (!d || !n_routed) return fail(BSGS_ERR_ARG, "null");
    const DptRouted rt = {routed, max_routed, n_routed, 0u};         // the caller's records name their kangaroos by global ids already
    return bsgs_kang_dpt_insert(d, BSGS_DPT_SHARDED, recs_in, n, recs_out, max_recs, nrecs, n_entries, dropped, &rt);
}
