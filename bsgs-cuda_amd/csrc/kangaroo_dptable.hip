// kangaroo_dptable.hip -- the distinguished-point table of a search, kept in device memory (include/bsgs_hip.h, "Kangaroo, distinguished-point table in device
// memory"; tests/kangaroo_dptable_model.py restates it).  The growing tame table of kangaroo_tames_gen.hip with the owner of every entry: a record
// that meets a stored point comes back WITH that point, so the host can pair tame and wild without holding the table.  The table, its claim and the coherence
// rule: kangaroo_table.hip.h; here who[slots] stands beside d[slots] (u32 kangaroo, u32 type: 0 tame, 1 wild, 3 wild with NEG).
//   insert    one record per lane, a wave strides over the records.  DEAD and tag-0 records are handed back; every other record claims a slot: stored -- d[s]
//             and who[s] are written with one vector store each; a duplicate -- handed back as a PAIR of consecutive records: a placeholder that names the
//             slot, then the record; no slot -- handed back as FULL.  One reservation per wave for the places (a duplicate takes two) and one atomic for the
//             count; the entry counter is bumped once per wave too.  Every store bounded.
//   resolve   a second kernel on the same stream: every placeholder becomes the slot's (tag, d, kangaroo, type) as a record.  d[s] and who[s] are read only
//             by a kernel launched after the one that wrote them, which is why the pairing is not done inside the insert.
//   equal tags in one launch: every one but the stored one comes back paired with it.
//   load      32-byte entries of the caller's by the same rule, staged in chunks; the four outcomes are counted, nothing else comes back.
//   harvest   strides over the slots and compacts the occupied ones into 32-byte entries, in any order.
// The table for a key list (kangaroo_dptable_keys.hip) is this table with the work file's owner word where the type stands: its insert is that unit's kernel,
// and resolve, load and harvest -- which copy who[s].y as it is -- and the host side below serve both.  The table divided over engines
// (kangaroo_dptable_shard.hip) is this table for one share of the tags with global kangaroo ids: its insert and scatter are that unit's kernels, the rest is here.
#include "kangaroo_table.hip.h"

#define DPT_LOAD_CHUNK BSGS_KANGAROO_DPT_LOAD_CHUNK
#define DPT_KEEP 0xFFFFFFFFu                                // (not a reason: the record went into the table)

__device__ __forceinline__ u32 dpt_type(u32 flags) { return (flags & BSGS_KANGAROO_WILD) ? (flags & (BSGS_KANGAROO_WILD | BSGS_KANGAROO_NEG)) : 0u; }

struct DptArgs {
    const u32 *rec;        // the walk's record buffer: u64 count | records
    u64 *tag;              // [slots]
    u32x4 *d;              // [slots]
    u32x2 *who;            // [slots]
    u32 *out;              // the hand-backs: u64 places taken, u64 records handed back | records; `reserved` = BSGS_KANGAROO_DPT_*
    u64 *ctr;              // the table's counters
    u64 slot_mask;
    u32 cap;               // records read at most
    u32 out_cap;           // places of `out`
};

__global__ void __launch_bounds__(256) kangaroo_dptable_insert_kernel(const DptArgs A)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 count = *(const u64 *)A.rec;
    const u32 n = count < (u64)A.cap ? (u32)count : A.cap;           // what the walk wrote; the rest was counted only
    const u32 stride = gridDim.x * blockDim.x;
    const u32x4 *const recs = (const u32x4 *)((const char *)A.rec + KANG_REC_HEADER);
    for (u32 base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n; base += stride) {      // wave-uniform: every lane reaches the ballots
        const u32 i = base + lane;
        u32 reason = DPT_KEEP;
        bool stored = false;
        u64 s = 0;
        u32x4 r0 = {0, 0, 0, 0}, r3 = {0, 0, 0, 0};
        if (i < n) {
            r0 = recs[(u64)i * 4];
            r3 = recs[(u64)i * 4 + 3];
            const u64 tag = ((u64)r0.y << 32) | r0.x;
            if (r3.y & BSGS_KANGAROO_DEAD) reason = BSGS_KANGAROO_DPT_DEAD;
            else if (tag == 0ull) reason = BSGS_KANGAROO_DPT_TAG_ZERO;
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
        const bool back = reason != DPT_KEEP, dup = reason == BSGS_KANGAROO_DPT_DUPLICATE;
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
}

// a kernel of its own behind the insert: what the insert stored is in order here.  Every placeholder is rewritten in place by the lane that read it.
__global__ void __launch_bounds__(256) kangaroo_dptable_resolve_kernel(const DptArgs A)
{
    const u64 used = *(const u64 *)A.out;
    const u32 n = used < (u64)A.out_cap ? (u32)used : A.out_cap;
    const u32 stride = gridDim.x * blockDim.x;
    u32x4 *const out = (u32x4 *)((char *)A.out + KANG_REC_HEADER);
    for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
        u32x4 *o = out + (u64)j * 4;
        if (o[3].w != BSGS_KANGAROO_DPT_STORED) continue;
        const u32x4 p = o[0];
        const u64 s = (((u64)p.y << 32) | p.x) & A.slot_mask;        // (a slot of the table whatever the placeholder says)
        const u64 t = A.tag[s];
        const u32x2 w = A.who[s];
        o[0] = (u32x4){(u32)t, (u32)(t >> 32), 0, 0};
        o[2] = A.d[s];
        o[3] = (u32x4){w.x, w.y, 0, BSGS_KANGAROO_DPT_STORED};       // flags = the type: WILD, WILD | NEG or none
    }
}

struct DptLoadArgs {
    const u32x4 *in;       // [n][2] the staged chunk: tag, d.lo | d.hi, kangaroo, type
    u64 *tag;              // [slots]
    u32x4 *d;              // [slots]
    u32x2 *who;            // [slots]
    u64 *ctr;              // the table's counters
    u64 slot_mask;
    u32 n;
};

__global__ void __launch_bounds__(256) kangaroo_dptable_load_kernel(const DptLoadArgs A)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 stride = gridDim.x * blockDim.x;
    for (u32 base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < A.n; base += stride) {      // wave-uniform: every lane reaches the ballots
        const u32 i = base + lane;
        u32 what = 0;                                                // 0: no entry in this lane; else CTR_*
        if (i < A.n) {
            const u32x4 e0 = A.in[(u64)i * 2], e1 = A.in[(u64)i * 2 + 1];
            const u64 tag = ((u64)e0.y << 32) | e0.x;
            u64 s;
            what = tag == 0ull ? CTR_ZERO : kt_claim(A.tag, A.slot_mask, tag, s, [&](u64 at) {
                A.d[at] = (u32x4){e0.z, e0.w, e1.x, e1.y};
                A.who[at] = (u32x2){e1.z, e1.w};
            });
        }
        kt_count_outcomes(A.ctr, what, lane);
    }
}

struct DptHarvestArgs {
    const u64 *tag;        // [slots]
    const u32x4 *d;        // [slots]
    const u32x2 *who;      // [slots]
    u32x4 *out;            // [max][2] entries as the load takes them
    u64 *ctr;              // the table's counters: [CTR_MET] occupied slots met (zeroed by the caller)
    u64 slots, max;
};

// a kernel of its own, after every insert and load: plain loads are in order here
__global__ void __launch_bounds__(256) kangaroo_dptable_harvest_kernel(const DptHarvestArgs A)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 base = (u64)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < A.slots; base += stride) {      // wave-uniform (slots is a multiple of 64)
        const u64 s = base + lane;
        const u64 t = s < A.slots ? A.tag[s] : 0ull;
        const bool occ = t != 0ull;
        const u64 pos = kt_reserve(occ, lane, &A.ctr[CTR_MET], 0);
        if (occ && pos < A.max) {                                    // the bound of every store
            const u32x4 dd = A.d[s];
            const u32x2 w = A.who[s];
            A.out[pos * 2] = (u32x4){(u32)t, (u32)(t >> 32), dd.x, dd.y};
            A.out[pos * 2 + 1] = (u32x4){dd.z, dd.w, w.x, w.y};
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(bsgs_kangaroo_dp_entry) == 32, "table entry: 32 bytes");

static void dpt_free(bsgs_kangaroo *k)
{
    bsgs_kang_table_free(&k->dpt);
    if (k->dpt_out) (void)hipFree(k->dpt_out);
    if (k->dpt_route) (void)hipFree(k->dpt_route);
    k->dpt_out = k->dpt_route = nullptr;
    k->dpt_keyed = false;
    k->dpt_shards = k->dpt_shard = k->dpt_base = 0;
}

static inline uint32_t dpt_out_cap(const bsgs_kangaroo *k) { return bsgs_kang_dpt_out_cap(k); }

static DptArgs dpt_args(const bsgs_kangaroo *k)
{
    DptArgs A;
    A.rec = k->rec; A.tag = k->dpt.tag; A.d = k->dpt.d; A.who = k->dpt.who; A.out = k->dpt_out; A.ctr = k->dpt.ctr; A.slot_mask = k->dpt.slots - 1;
    A.cap = k->cap; A.out_cap = dpt_out_cap(k);
    return A;
}

int bsgs_kang_dpt_resolve(bsgs_dev *d, bsgs_kangaroo *k, uint32_t blocks)
{
    hipLaunchKernelGGL(kangaroo_dptable_resolve_kernel, dim3(blocks), dim3(256), 0, d->stream, dpt_args(k));
    HIPCHK(hipGetLastError());
    return BSGS_OK;
}

// insert and resolve of the records in k->rec (their count at its head) on the stream; a keyed table takes the insert of kangaroo_dptable_keys.hip, a
// sharded one that of kangaroo_dptable_shard.hip (base: what it adds to the records' kangaroo ids)
static int dpt_insert(bsgs_dev *d, bsgs_kangaroo *k, u32 base)
{
    const u32 blocks = std::min((k->cap + 255u) / 256u, KT_INSERT_GRID_MAX);
    if (k->dpt_keyed) {
        if (int rc = bsgs_kang_dpt_insert_keys_launch(d, k, blocks)) return rc;
    } else if (k->dpt_shards) {
        if (int rc = bsgs_kang_dpt_insert_shard_launch(d, k, blocks, base)) return rc;
    } else {
        hipLaunchKernelGGL(kangaroo_dptable_insert_kernel, dim3(blocks), dim3(256), 0, d->stream, dpt_args(k));
        HIPCHK(hipGetLastError());
    }
    return bsgs_kang_dpt_resolve(d, k, blocks);
}

// the hand-backs of the launch that has finished -> recs, through the herd's pinned buffer in pieces of its size.  A pair is never split: when the cut at
// max_recs falls behind a stored entry, that entry stays behind too.  *kept = records of the walk among those handed over (a pair holds one).
static int dpt_copy_out(bsgs_dev *d, bsgs_kangaroo *k, uint64_t places, bsgs_kangaroo_record *recs, uint32_t max_recs, uint32_t *given, uint64_t *kept)
{
    uint64_t give = recs ? std::min<uint64_t>(places, max_recs) : 0;
    for (uint64_t at = 0; at < give; at += k->cap) {
        const uint64_t n = std::min<uint64_t>(give - at, k->cap);
        HIPCHK(hipMemcpyAsync(k->rec_host, (const char *)k->dpt_out + KANG_REC_HEADER + at * 64, n * 64, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
        memcpy(recs + at, k->rec_host, n * 64);
    }
    if (give && give < places && recs[give - 1].reserved == BSGS_KANGAROO_DPT_STORED) give--;
    uint64_t walk = 0;
    for (uint64_t q = 0; q < give; q++) walk += recs[q].reserved != BSGS_KANGAROO_DPT_STORED;
    *given = (uint32_t)give;
    *kept = walk;
    return BSGS_OK;
}

// `table`: the call needs one; `want`: DPT_EITHER, or the kind of table the call is for.  A keyed table stands under a herd with a key list, that of
// bsgs_kangaroo_setup_sym_keys included, which every other table call refuses.  A sharded table stands under the unkeyed table's herds and holds global ids.
enum { DPT_EITHER = BSGS_DPT_EITHER, DPT_UNKEYED = BSGS_DPT_UNKEYED, DPT_KEYED = BSGS_DPT_KEYED, DPT_SHARDED = BSGS_DPT_SHARDED };
static int dpt_herd(bsgs_dev *d, bsgs_kangaroo **k, bool table, int want = DPT_UNKEYED)
{
    if (d && d->kangaroo && d->kangaroo->dpt.tag && d->kangaroo->dpt_shards && table && want != DPT_EITHER && want != DPT_SHARDED)
        return fail(BSGS_ERR_STATE, "the table was begun by bsgs_kangaroo_dptable_begin_shard: bsgs_kangaroo_run_dptable_shard and bsgs_kangaroo_dptable_insert_shard fill it");
    if (want == DPT_SHARDED) {
        if (int rc = bsgs_kang_table_herd(d, k, &bsgs_kangaroo::dpt, "a distinguished-point table divided over engines serves the herds of bsgs_kangaroo_setup and bsgs_kangaroo_setup_sym",
                                          table ? "bsgs_kangaroo_dptable_begin_shard first" : nullptr)) return rc;
        if ((*k)->keys && (*k)->n_keys)
            return fail(BSGS_ERR_STATE, "a distinguished-point table divided over engines serves one key: this herd has a key list (bsgs_kangaroo_set_keys)");
        if (table && !(*k)->dpt_shards)
            return fail(BSGS_ERR_STATE, "the table was begun by bsgs_kangaroo_dptable_begin%s: it holds the ids of one engine", (*k)->dpt_keyed ? "_keys" : "");
        return BSGS_OK;
    }
    if (d && d->kangaroo && d->kangaroo->dpt.tag && d->kangaroo->dpt_keyed && table) {
        *k = d->kangaroo;
        if (want == DPT_UNKEYED)
            return fail(BSGS_ERR_STATE, "the table was begun by bsgs_kangaroo_dptable_begin_keys: bsgs_kangaroo_run_dptable_keys and bsgs_kangaroo_dptable_insert_keys fill it");
        return BSGS_OK;
    }
    if (want == DPT_KEYED) {
        if (!d) return fail(BSGS_ERR_ARG, "null");
        *k = d->kangaroo;
        if (!*k) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_setup first");
        if (!(*k)->keys || !(*k)->n_keys)
            return fail(BSGS_ERR_STATE, "a distinguished-point table for a key list serves the herds of bsgs_kangaroo_setup and bsgs_kangaroo_setup_sym_keys after bsgs_kangaroo_set_keys");
        if (table) return fail(BSGS_ERR_STATE, (*k)->dpt.tag ? "the table was begun by bsgs_kangaroo_dptable_begin: bsgs_kangaroo_run_dptable and bsgs_kangaroo_dptable_insert fill it"
                                                              : "bsgs_kangaroo_dptable_begin_keys first");
        return BSGS_OK;
    }
    return bsgs_kang_table_herd(d, k, &bsgs_kangaroo::dpt, "a distinguished-point table serves the herds of bsgs_kangaroo_setup and bsgs_kangaroo_setup_sym",
                                table ? "bsgs_kangaroo_dptable_begin first" : nullptr);
}

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------------------------------
int bsgs_kang_dpt_begin(bsgs_dev *d, uint64_t capacity, int kind)
{
    const bool keyed = kind == DPT_KEYED;
    bsgs_kangaroo *k = nullptr;
    if (int rc = dpt_herd(d, &k, false, kind)) return rc;
    if (!capacity || capacity > KT_MAX_CAPACITY) return fail(BSGS_ERR_ARG, "distinguished-point table of %llu entries: 1..2^31", (unsigned long long)capacity);
    HIPCHK(hipSetDevice(d->id));
    HIPCHK(hipStreamSynchronize(d->stream));
    dpt_free(k);
    const uint64_t slots = bsgs_kang_table_slots(capacity, k->cap);
    const size_t out_bytes = KANG_REC_HEADER + (size_t)dpt_out_cap(k) * 64;
    bool nomem = false;
    const hipError_t e = bsgs_kang_table_begin(d, &k->dpt, slots, true, &k->dpt_out, out_bytes, &nomem);
    if (e != hipSuccess) dpt_free(k);                                // (the hand-backs' buffer too)
    if (nomem)
        return fail(BSGS_ERR_NOMEM, "distinguished-point table of %llu entries: %llu slots need %llu bytes of tags, %llu of offsets, %llu of owners and %llu of records (%s)",
                    (unsigned long long)capacity, (unsigned long long)slots, (unsigned long long)(slots * 8), (unsigned long long)(slots * 16), (unsigned long long)(slots * 8),
                    (unsigned long long)out_bytes, hipGetErrorString(e));
    HIPCHK(e);
    k->dpt_keyed = keyed;
    return BSGS_OK;
}

extern "C" int bsgs_kangaroo_dptable_begin(bsgs_dev *d, uint64_t capacity) { return bsgs_kang_dpt_begin(d, capacity, DPT_UNKEYED); }

int bsgs_kang_dpt_run(bsgs_dev *d, int kind, uint32_t steps, bsgs_kangaroo_record *recs, uint32_t max_recs, uint32_t *nrecs, uint64_t *n_seen, uint64_t *n_entries,
                      uint64_t *dropped, float *kernel_ms, const DptRouted *rt)
{
    if (!d || !nrecs) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = nullptr;
    if (int rc = dpt_herd(d, &k, true, kind)) return rc;
    HIPCHK(hipSetDevice(d->id));
    HIPCHK(hipMemsetAsync(k->dpt_out, 0, KANG_REC_HEADER, d->stream));
    if (int rc = bsgs_kangaroo_launch(d, steps)) return rc;          // the walk, timed from ev0
    if (int rc = dpt_insert(d, k, rt ? rt->base : 0u)) return rc;
    uint64_t count = 0, places = 0, back = 0, cut = 0;
    if (int rc = bsgs_kangaroo_finish(d, &count, k->dpt_out, &places, kernel_ms)) return rc;      // ev1 behind the resolve, both counts, the synchronisation
    HIPCHK(hipMemcpyAsync(&back, (const char *)k->dpt_out + 8, 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    const uint64_t held = std::min<uint64_t>(count, k->cap);
    back = std::min<uint64_t>(back, held);
    places = std::min<uint64_t>(places, std::min<uint64_t>(2 * back, dpt_out_cap(k)));
    uint32_t give = 0;
    uint64_t kept = 0;
    if (int rc = dpt_copy_out(d, k, places, recs, max_recs, &give, &kept)) return rc;
    if (rt) if (int rc = bsgs_kang_dpt_routed_out(d, k, held, rt, &cut)) return rc;
    if (int rc = bsgs_kang_table_entries(d, &k->dpt, n_entries)) return rc;
    *nrecs = give;
    if (n_seen) *n_seen = count;
    if (dropped) *dropped = (count - held) + (back - kept) + cut;    // never inserted, handed back but not handed over (a pair counts once), routed but cut
    return BSGS_OK;
}

extern "C" int bsgs_kangaroo_run_dptable(bsgs_dev *d, uint32_t steps, bsgs_kangaroo_record *recs, uint32_t max_recs, uint32_t *nrecs, uint64_t *n_seen,
                                         uint64_t *n_entries, uint64_t *dropped, float *kernel_ms)
{
    return bsgs_kang_dpt_run(d, DPT_UNKEYED, steps, recs, max_recs, nrecs, n_seen, n_entries, dropped, kernel_ms);
}

int bsgs_kang_dpt_insert(bsgs_dev *d, int kind, const bsgs_kangaroo_record *recs_in, uint32_t n, bsgs_kangaroo_record *recs_out, uint32_t max_recs, uint32_t *nrecs,
                         uint64_t *n_entries, uint64_t *dropped, const DptRouted *rt)
{
    if (!d || !nrecs || (n && !recs_in)) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = nullptr;
    if (int rc = dpt_herd(d, &k, true, kind)) return rc;
    const uint64_t count = n;
    if (int rc = bsgs_kang_table_stage(d, k, k->dpt_out, recs_in, &count)) return rc;
    if (int rc = dpt_insert(d, k, rt ? rt->base : 0u)) return rc;
    uint64_t head[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(head, k->dpt_out, 16, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    const uint64_t back = std::min<uint64_t>(head[1], n);
    const uint64_t places = std::min<uint64_t>(head[0], std::min<uint64_t>(2 * back, dpt_out_cap(k)));
    uint32_t give = 0;
    uint64_t kept = 0, cut = 0;
    if (int rc = dpt_copy_out(d, k, places, recs_out, max_recs, &give, &kept)) return rc;
    if (rt) if (int rc = bsgs_kang_dpt_routed_out(d, k, n, rt, &cut)) return rc;
    *nrecs = give;
    if (dropped) *dropped = back - kept + cut;
    return bsgs_kang_table_entries(d, &k->dpt, n_entries);
}

extern "C" int bsgs_kangaroo_dptable_insert(bsgs_dev *d, const bsgs_kangaroo_record *recs_in, uint32_t n, bsgs_kangaroo_record *recs_out, uint32_t max_recs,
                                            uint32_t *nrecs, uint64_t *n_entries, uint64_t *dropped)
{
    return bsgs_kang_dpt_insert(d, DPT_UNKEYED, recs_in, n, recs_out, max_recs, nrecs, n_entries, dropped);
}

extern "C" int bsgs_kangaroo_dptable_load(bsgs_dev *d, const bsgs_kangaroo_dp_entry *entries, uint64_t n, uint64_t *n_stored, uint64_t *n_duplicate, uint64_t *n_zero,
                                          uint64_t *n_full, uint64_t *n_entries)
{
    if (!d || (n && !entries)) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = nullptr;
    if (int rc = dpt_herd(d, &k, true, DPT_EITHER)) return rc;
    if (n > KT_MAX_CAPACITY) return fail(BSGS_ERR_ARG, "%llu entries to load: at most 2^31", (unsigned long long)n);
    HIPCHK(hipSetDevice(d->id));
    HIPCHK(hipMemsetAsync(k->dpt.ctr + CTR_STORED, 0, 32, d->stream));
    u32x4 *stage = nullptr;
    const uint64_t chunk = std::min<uint64_t>(n, DPT_LOAD_CHUNK);
    if (chunk) {
        hipError_t e = hipMalloc(&stage, (size_t)chunk * 32);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(BSGS_ERR_NOMEM, "loading %llu entries into the distinguished-point table: %llu bytes of staging (%s)", (unsigned long long)n,
                        (unsigned long long)(chunk * 32), hipGetErrorString(e));
        }
    }
    hipError_t e = hipSuccess;
    for (uint64_t at = 0; at < n && e == hipSuccess; at += chunk) {
        const uint64_t m = std::min<uint64_t>(chunk, n - at);
        e = hipMemcpyAsync(stage, entries + at, (size_t)m * 32, hipMemcpyHostToDevice, d->stream);
        if (e != hipSuccess) break;
        DptLoadArgs A;
        A.in = stage; A.tag = k->dpt.tag; A.d = k->dpt.d; A.who = k->dpt.who; A.ctr = k->dpt.ctr; A.slot_mask = k->dpt.slots - 1; A.n = (u32)m;
        const u32 blocks = (u32)std::min<uint64_t>((m + 255u) / 256u, KT_SCAN_GRID_MAX);
        hipLaunchKernelGGL(kangaroo_dptable_load_kernel, dim3(blocks), dim3(256), 0, d->stream, A);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(d->stream);    // the caller's buffer is pageable: the stage is free again
    }
    const int rc = bsgs_kang_table_loaded(d, &k->dpt, e, n, n_stored, n_duplicate, n_zero, n_full, n_entries,
                                          "distinguished-point table: %llu entries to load, %llu accounted for");
    if (stage) (void)hipFree(stage);
    return rc;
}

extern "C" int bsgs_kangaroo_dptable_read(bsgs_dev *d, bsgs_kangaroo_dp_entry *entries, uint64_t max, uint64_t *n)
{
    if (!d || !n) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = nullptr;
    if (int rc = dpt_herd(d, &k, true, DPT_EITHER)) return rc;
    HIPCHK(hipSetDevice(d->id));
    uint64_t held = 0;
    if (int rc = bsgs_kang_table_entries(d, &k->dpt, &held)) return rc;
    *n = held;
    if (!max && !entries) return BSGS_OK;                            // the count alone
    if (max < held) return fail(BSGS_ERR_ARG, "room for %llu entries, the table holds %llu", (unsigned long long)max, (unsigned long long)held);
    if (!held) return BSGS_OK;
    if (!entries) return fail(BSGS_ERR_ARG, "null");
    DptHarvestArgs H;
    H.tag = k->dpt.tag; H.d = k->dpt.d; H.who = k->dpt.who; H.out = nullptr; H.ctr = k->dpt.ctr; H.slots = k->dpt.slots; H.max = held;
    hipError_t e = hipMalloc(&H.out, (size_t)held * 32);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(BSGS_ERR_NOMEM, "reading a distinguished-point table of %llu entries: %llu bytes of device memory (%s)", (unsigned long long)held,
                    (unsigned long long)(held * 32), hipGetErrorString(e));
    }
    uint64_t met = 0;
    e = hipMemsetAsync(k->dpt.ctr + CTR_MET, 0, 8, d->stream);
    if (e == hipSuccess) {
        const u32 blocks = (u32)std::min<uint64_t>((k->dpt.slots + 255u) / 256u, KT_SCAN_GRID_MAX);
        hipLaunchKernelGGL(kangaroo_dptable_harvest_kernel, dim3(blocks), dim3(256), 0, d->stream, H);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&met, k->dpt.ctr + CTR_MET, 8, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(entries, H.out, (size_t)held * 32, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    (void)hipFree(H.out);
    HIPCHK(e);
    return bsgs_kang_table_met_check(met, held, "distinguished-point table");
}

extern "C" int bsgs_kangaroo_dptable_end(bsgs_dev *d)
{
    if (!d) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = d->kangaroo;
    if (!k || !k->dpt.tag) return BSGS_OK;
    HIPCHK(hipSetDevice(d->id));
    HIPCHK(hipStreamSynchronize(d->stream));
    dpt_free(k);
    return BSGS_OK;
}
