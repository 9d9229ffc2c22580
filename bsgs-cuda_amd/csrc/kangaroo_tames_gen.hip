// kangaroo_tames_gen.hip -- the tame table while it grows, kept in device memory (include/bsgs_hip.h, "Kangaroo, tame table grown on the device"; DESIGN.md 10;
// tests/kangaroo_tames_gen_model.py restates it).  Generation is all tame and never saved, so "insert, or report that the tag is already there" is the whole
// contract: a kernel behind the walk inserts the launch's records, and only the records the host must act on -- merges, dead kangaroos, cycles -- cross the bus.
//   table     open addressing with linear probing, nothing is ever deleted: tag[slots] (u64, the low 64 bits of x; 0 = empty, eight tags to a 64-byte line) and
//             d[slots] (16-byte vectors, the offset as the record holds it).  Home slot (tag >> 6) & (slots - 1), as in the search's image.
//   insert    one record per lane, a wave strides over the records as tames_match does.  DEAD and tag-0 records are handed back; every other record runs
//             old = atomicCAS(&tag[s], 0, t) from its home slot on: 0 -- the slot is ours, d[s] is written with one 16-byte store; t -- a duplicate, handed back;
//             else the next slot, wrapping, at most `slots` times (then handed back as FULL).  Handed-back records are compacted as tames_match's: __ballot, one
//             atomic per wave, vector stores only, every store bounded; the entry counter is bumped once per wave too.  No LDS, no scratch.
//   coherence L2 is not coherent across XCDs within a kernel.  A slot's tag is DECIDED ONLY BY THE RETURN VALUE OF THE COMPARE-AND-SWAP, which is carried out where
//             every XCD sees it.  A plain load might be used as a shortcut only when it shows a non-zero tag (slots never change once set, so a non-zero tag seen
//             anywhere is final); a plain load must never be used to conclude that a slot is empty -- this kernel makes no plain load of a tag at all.  d[s] is
//             read by nobody before the next kernel (the harvest, or nothing).
//   equal tags in one launch: which of them is stored is unspecified; exactly one is, the others come back as duplicates.
//   harvest   strides over the slots and compacts the occupied ones (tag, d) into two dense arrays by ballot, in any order; the host sorts.
#include "bsgs_internal.h"

#define TAMES_GEN_MIN_SLOTS 128ull
#define TAMES_GEN_MAX_CAPACITY (1ull << 31)
#define TAMES_GEN_GRID_MAX 1024u                            // blocks of the insert: four per CU; a wave strides over the records
#define TAMES_GEN_HARVEST_GRID_MAX 4096u
#define TAMES_GEN_KEEP 0xFFFFFFFFu                          // (not a reason: the record went into the table)

struct TamesGenArgs {
    const u32 *rec;        // the walk's record buffer: u64 count | records
    u64 *tag;              // [slots]
    u32x4 *d;              // [slots]
    u32 *out;              // the handed-back records, same layout as rec; `reserved` = BSGS_KANGAROO_GEN_*
    u64 *entries;          // entries in the table
    u64 slot_mask;
    u32 cap;
};

__global__ void __launch_bounds__(256) kangaroo_tames_gen_insert_kernel(const TamesGenArgs A)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 count = *(const u64 *)A.rec;
    const u32 n = count < (u64)A.cap ? (u32)count : A.cap;           // what the walk wrote; the rest was counted only
    const u32 stride = gridDim.x * blockDim.x;
    const u32x4 *const recs = (const u32x4 *)((const char *)A.rec + KANG_REC_HEADER);
    for (u32 base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n; base += stride) {      // wave-uniform: every lane reaches the ballots
        const u32 i = base + lane;
        u32 reason = TAMES_GEN_KEEP;
        bool stored = false;
        u32x4 r0 = {0, 0, 0, 0}, r3 = {0, 0, 0, 0};
        if (i < n) {
            r0 = recs[(u64)i * 4];
            r3 = recs[(u64)i * 4 + 3];
            const u64 tag = ((u64)r0.y << 32) | r0.x;
            if (r3.y & BSGS_KANGAROO_DEAD) reason = BSGS_KANGAROO_GEN_DEAD;
            else if (tag == 0ull) reason = BSGS_KANGAROO_GEN_TAG_ZERO;
            else {
                reason = BSGS_KANGAROO_GEN_FULL;
                u64 s = (tag >> 6) & A.slot_mask;
                for (u64 it = 0; it <= A.slot_mask; it++) {
                    const u64 old = atomicCAS((unsigned long long *)&A.tag[s], 0ull, (unsigned long long)tag);      // the only way a tag is read
                    if (old == 0ull) {
                        A.d[s] = recs[(u64)i * 4 + 2];
                        stored = true;
                        reason = TAMES_GEN_KEEP;
                        break;
                    }
                    if (old == tag) { reason = BSGS_KANGAROO_GEN_DUPLICATE; break; }
                    s = (s + 1ull) & A.slot_mask;
                }
            }
        }
        const u64 ms = __ballot(stored);
        if (ms && (int)lane == __builtin_ctzll(ms)) atomicAdd((unsigned long long *)A.entries, (unsigned long long)__builtin_popcountll(ms));
        const bool back = reason != TAMES_GEN_KEEP;
        const u64 m = __ballot(back);
        if (m) {
            u64 slot0 = 0;
            const int leader = __builtin_ctzll(m);
            if ((int)lane == leader) slot0 = atomicAdd((unsigned long long *)A.out, (unsigned long long)__builtin_popcountll(m));
            slot0 = __shfl(slot0, leader);
            const u64 slot = slot0 + (u64)__builtin_popcountll(m & ((1ull << lane) - 1));
            if (back && slot < A.cap) {                              // (never more handed back than read; the bound of every store)
                u32x4 *o = (u32x4 *)((char *)A.out + KANG_REC_HEADER) + slot * 4;
                o[0] = r0;
                o[1] = recs[(u64)i * 4 + 1];
                o[2] = recs[(u64)i * 4 + 2];
                o[3] = (u32x4){r3.x, r3.y, r3.z, reason};
            }
        }
    }
}

struct TamesGenHarvestArgs {
    const u64 *tag;        // [slots]
    const u32x4 *d;        // [slots]
    u64 *out_tag;          // [max]
    u32x4 *out_d;          // [max]
    u64 *count;            // occupied slots met (zeroed by the caller)
    u64 slots, max;
};

// a kernel of its own, after every insert: plain loads are in order here
__global__ void __launch_bounds__(256) kangaroo_tames_gen_harvest_kernel(const TamesGenHarvestArgs A)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 base = (u64)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < A.slots; base += stride) {      // wave-uniform (slots is a multiple of 64)
        const u64 s = base + lane;
        const u64 t = s < A.slots ? A.tag[s] : 0ull;
        const bool occ = t != 0ull;
        const u64 m = __ballot(occ);
        if (m) {
            u64 pos0 = 0;
            const int leader = __builtin_ctzll(m);
            if ((int)lane == leader) pos0 = atomicAdd((unsigned long long *)A.count, (unsigned long long)__builtin_popcountll(m));
            pos0 = __shfl(pos0, leader);
            const u64 pos = pos0 + (u64)__builtin_popcountll(m & ((1ull << lane) - 1));
            if (occ && pos < A.max) {                                // the bound of every store
                A.out_tag[pos] = t;
                A.out_d[pos] = A.d[s];
            }
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------------
static uint64_t tames_gen_slots(uint64_t capacity, uint32_t record_cap)
{
    uint64_t slots = TAMES_GEN_MIN_SLOTS;
    while (slots < 2 * (capacity + record_cap)) slots *= 2;          // at most half full even after the last launch overshoots `capacity`
    return slots;
}

static void tames_gen_free(bsgs_kangaroo *k)
{
    for (void *p : {(void *)k->gen_tag, (void *)k->gen_d, (void *)k->gen_ctr}) if (p) (void)hipFree(p);
    k->gen_tag = nullptr; k->gen_d = nullptr; k->gen_ctr = nullptr; k->gen_slots = 0;
}

// the insert of the n records in k->rec (their count at its head) on the stream, the hand-backs to recs, the entry count
static int tames_gen_insert(bsgs_dev *d, bsgs_kangaroo *k)
{
    TamesGenArgs A;
    A.rec = k->rec; A.tag = k->gen_tag; A.d = k->gen_d; A.out = k->tames_rec; A.entries = k->gen_ctr; A.slot_mask = k->gen_slots - 1; A.cap = k->cap;
    const u32 blocks = std::min((k->cap + 255u) / 256u, TAMES_GEN_GRID_MAX);
    hipLaunchKernelGGL(kangaroo_tames_gen_insert_kernel, dim3(blocks), dim3(256), 0, d->stream, A);
    HIPCHK(hipGetLastError());
    return BSGS_OK;
}
static int tames_gen_entries(bsgs_dev *d, bsgs_kangaroo *k, uint64_t *n_entries)
{
    uint64_t n = 0;
    HIPCHK(hipMemcpyAsync(&n, k->gen_ctr, 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    if (n_entries) *n_entries = n;
    return BSGS_OK;
}

static int tames_gen_herd(bsgs_dev *d, bsgs_kangaroo **k, bool table)
{
    if (!d) return fail(BSGS_ERR_ARG, "null");
    *k = d->kangaroo;
    if (!*k) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_setup first");
    if ((*k)->key) return fail(BSGS_ERR_STATE, "a tame table grows under the herds of bsgs_kangaroo_setup and bsgs_kangaroo_setup_sym");
    if (table && !(*k)->gen_tag) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_tames_gen_begin first");
    return BSGS_OK;
}

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int bsgs_kangaroo_tames_gen_begin(bsgs_dev *d, uint64_t capacity)
{
    bsgs_kangaroo *k = nullptr;
    if (int rc = tames_gen_herd(d, &k, false)) return rc;
    if (!capacity || capacity > TAMES_GEN_MAX_CAPACITY) return fail(BSGS_ERR_ARG, "growing tame table of %llu entries: 1..2^31", (unsigned long long)capacity);
    HIPCHK(hipSetDevice(d->id));
    HIPCHK(hipStreamSynchronize(d->stream));
    tames_gen_free(k);
    const uint64_t slots = tames_gen_slots(capacity, k->cap);
    const size_t rec_bytes = KANG_REC_HEADER + (size_t)k->cap * 64;
    hipError_t e = hipMalloc(&k->gen_tag, (size_t)slots * 8);
    if (e == hipSuccess) e = hipMalloc(&k->gen_d, (size_t)slots * 16);
    if (e == hipSuccess) e = hipMalloc(&k->gen_ctr, 64);
    if (e == hipSuccess && !k->tames_rec) e = hipMalloc(&k->tames_rec, rec_bytes);      // the hand-back buffer: the match's buffer of this herd, never used by both at once
    if (e != hipSuccess) {
        (void)hipGetLastError();
        tames_gen_free(k);
        return fail(BSGS_ERR_NOMEM, "growing tame table of %llu entries: %llu slots need %llu bytes of tags, %llu of offsets and %llu of records (%s)", (unsigned long long)capacity,
                    (unsigned long long)slots, (unsigned long long)(slots * 8), (unsigned long long)(slots * 16), (unsigned long long)rec_bytes, hipGetErrorString(e));
    }
    HIPCHK(hipMemsetAsync(k->gen_tag, 0, (size_t)slots * 8, d->stream));          // empty = tag 0; an offset is read only where a tag stands
    HIPCHK(hipMemsetAsync(k->gen_ctr, 0, 64, d->stream));
    HIPCHK(hipMemsetAsync(k->tames_rec, 0, KANG_REC_HEADER, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    k->gen_slots = slots;
    return BSGS_OK;
}

extern "C" int bsgs_kangaroo_run_tames_gen(bsgs_dev *d, uint32_t steps, bsgs_kangaroo_record *recs, uint32_t max_recs, uint32_t *nrecs, uint64_t *n_seen,
                                           uint64_t *n_entries, uint64_t *dropped, float *kernel_ms)
{
    if (!d || !nrecs) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = nullptr;
    if (int rc = tames_gen_herd(d, &k, true)) return rc;
    HIPCHK(hipSetDevice(d->id));
    HIPCHK(hipMemsetAsync(k->tames_rec, 0, KANG_REC_HEADER, d->stream));
    if (int rc = bsgs_kangaroo_launch(d, steps)) return rc;          // the walk, timed from ev0
    if (int rc = tames_gen_insert(d, k)) return rc;
    uint64_t count = 0, back = 0;
    if (int rc = bsgs_kangaroo_finish(d, &count, k->tames_rec, &back, kernel_ms)) return rc;      // ev1 behind the insert, both counts, the synchronisation
    const uint64_t held = std::min<uint64_t>(count, k->cap);
    back = std::min<uint64_t>(back, held);
    uint32_t give = 0;
    if (int rc = bsgs_kangaroo_copy_out(d, k->tames_rec, back, recs, max_recs, &give)) return rc;
    if (int rc = tames_gen_entries(d, k, n_entries)) return rc;
    *nrecs = give;
    if (n_seen) *n_seen = count;
    if (dropped) *dropped = (count - held) + (back - give);          // never inserted, and handed back but not handed over
    return BSGS_OK;
}

extern "C" int bsgs_kangaroo_tames_gen_insert(bsgs_dev *d, const bsgs_kangaroo_record *recs_in, uint32_t n, bsgs_kangaroo_record *recs_out, uint32_t max_recs,
                                              uint32_t *nrecs, uint64_t *n_entries)
{
    if (!d || !nrecs || (n && !recs_in)) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = nullptr;
    if (int rc = tames_gen_herd(d, &k, true)) return rc;
    if (n > k->cap) return fail(BSGS_ERR_ARG, "%u records: at most the record capacity %u", n, k->cap);
    HIPCHK(hipSetDevice(d->id));
    const uint64_t count = n;
    HIPCHK(hipMemsetAsync(k->tames_rec, 0, KANG_REC_HEADER, d->stream));
    HIPCHK(hipMemsetAsync(k->rec, 0, KANG_REC_HEADER, d->stream));
    HIPCHK(hipMemcpyAsync(k->rec, &count, 8, hipMemcpyHostToDevice, d->stream));
    if (n) HIPCHK(hipMemcpyAsync((char *)k->rec + KANG_REC_HEADER, recs_in, (size_t)n * 64, hipMemcpyHostToDevice, d->stream));      // into the walk's record buffer
    if (int rc = tames_gen_insert(d, k)) return rc;
    uint64_t back = 0;
    HIPCHK(hipMemcpyAsync(&back, k->tames_rec, 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    back = std::min<uint64_t>(back, n);
    uint32_t give = 0;
    if (int rc = bsgs_kangaroo_copy_out(d, k->tames_rec, back, recs_out, max_recs, &give)) return rc;
    *nrecs = give;
    return tames_gen_entries(d, k, n_entries);
}

extern "C" int bsgs_kangaroo_tames_gen_read(bsgs_dev *d, uint64_t *x_lo64, uint8_t *d_le, uint64_t max, uint64_t *n)
{
    if (!d || !n) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = nullptr;
    if (int rc = tames_gen_herd(d, &k, true)) return rc;
    HIPCHK(hipSetDevice(d->id));
    uint64_t entries = 0;
    if (int rc = tames_gen_entries(d, k, &entries)) return rc;
    *n = entries;
    if (max < entries) return fail(BSGS_ERR_ARG, "room for %llu entries, the table holds %llu", (unsigned long long)max, (unsigned long long)entries);
    if (!entries) return BSGS_OK;
    if (!x_lo64 || !d_le) return fail(BSGS_ERR_ARG, "null");
    TamesGenHarvestArgs H;
    H.tag = k->gen_tag; H.d = k->gen_d; H.out_tag = nullptr; H.out_d = nullptr; H.count = k->gen_ctr + 1; H.slots = k->gen_slots; H.max = entries;
    hipError_t e = hipMalloc(&H.out_tag, (size_t)entries * 8);
    if (e == hipSuccess) e = hipMalloc(&H.out_d, (size_t)entries * 16);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (H.out_tag) (void)hipFree(H.out_tag);
        return fail(BSGS_ERR_NOMEM, "reading a growing tame table of %llu entries: %llu bytes of device memory (%s)", (unsigned long long)entries, (unsigned long long)(entries * 24),
                    hipGetErrorString(e));
    }
    uint64_t met = 0;
    e = hipMemsetAsync(k->gen_ctr + 1, 0, 8, d->stream);
    if (e == hipSuccess) {
        const u32 blocks = (u32)std::min<uint64_t>((k->gen_slots + 255u) / 256u, TAMES_GEN_HARVEST_GRID_MAX);
        hipLaunchKernelGGL(kangaroo_tames_gen_harvest_kernel, dim3(blocks), dim3(256), 0, d->stream, H);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&met, k->gen_ctr + 1, 8, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(x_lo64, H.out_tag, (size_t)entries * 8, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_le, H.out_d, (size_t)entries * 16, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    (void)hipFree(H.out_tag);
    (void)hipFree(H.out_d);
    HIPCHK(e);
    if (met != entries) return fail(BSGS_ERR_STATE, "growing tame table: %llu occupied slots, %llu entries counted", (unsigned long long)met, (unsigned long long)entries);
    return BSGS_OK;
}

extern "C" int bsgs_kangaroo_tames_gen_end(bsgs_dev *d)
{
    if (!d) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = d->kangaroo;
    if (!k || !k->gen_tag) return BSGS_OK;
    HIPCHK(hipSetDevice(d->id));
    HIPCHK(hipStreamSynchronize(d->stream));
    tames_gen_free(k);
    return BSGS_OK;
}
