// kangaroo_tames_gen.hip -- the tame table while it grows, kept in device memory (include/bsgs_hip.h, "Kangaroo, tame table grown on the device"; DESIGN.md 10;
// tests/kangaroo_tames_gen_model.py restates it), and the host side of every such table (struct KangTable, bsgs_internal.h).  Generation is all tame and never
// saved, so "insert, or report that the tag is already there" is the whole contract: a kernel behind the walk inserts the launch's records, and only the
// records the host must act on -- merges, dead kangaroos, cycles -- cross the bus.  The table, its claim and the coherence rule: kangaroo_table.hip.h.
//   insert    one record per lane, a wave strides over the records as tames_match does.  DEAD and tag-0 records are handed back; every other record claims a
//             slot: stored -- d[s] is written with one 16-byte store; a duplicate or no slot (FULL) -- handed back.  Handed-back records are compacted as
//             tames_match's, one atomic per wave, every store bounded; the entry counter is bumped once per wave too.
//   harvest   strides over the slots and compacts the occupied ones (tag, d) into two dense arrays, in any order; the host sorts.
#include "kangaroo_table.hip.h"

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
                u64 s;
                const u32 got = kt_claim(A.tag, A.slot_mask, tag, s, [&](u64 at) { A.d[at] = recs[(u64)i * 4 + 2]; });
                stored = got == CTR_STORED;                          // (the claim names its outcome by the counter a load gives it)
                if (!stored) reason = got == CTR_DUPLICATE ? BSGS_KANGAROO_GEN_DUPLICATE : BSGS_KANGAROO_GEN_FULL;
            }
        }
        kt_count(A.entries, __ballot(stored), lane);
        const bool back = reason != TAMES_GEN_KEEP;
        const u64 slot = kt_reserve(back, lane, (u64 *)A.out, 0);
        if (back && slot < A.cap) {                                  // (never more handed back than read; the bound of every store)
            u32x4 *o = (u32x4 *)((char *)A.out + KANG_REC_HEADER) + slot * 4;
            o[0] = r0;
            o[1] = recs[(u64)i * 4 + 1];
            o[2] = recs[(u64)i * 4 + 2];
            o[3] = (u32x4){r3.x, r3.y, r3.z, reason};
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
        const u64 pos = kt_reserve(occ, lane, A.count, 0);
        if (occ && pos < A.max) {                                    // the bound of every store
            A.out_tag[pos] = t;
            A.out_d[pos] = A.d[s];
        }
    }
}

// ---- host: a KangTable, for this unit, kangaroo_tames_extend.hip and kangaroo_dptable.hip ----------------------------------------------------------------
uint64_t bsgs_kang_table_slots(uint64_t capacity, uint32_t record_cap)
{
    uint64_t slots = KT_MIN_SLOTS;
    while (slots < 2 * (capacity + record_cap)) slots *= 2;          // at most half full even after the last launch overshoots `capacity`
    return slots;
}

void bsgs_kang_table_free(KangTable *t)
{
    for (void *p : {(void *)t->tag, (void *)t->d, (void *)t->who, (void *)t->ctr}) if (p) (void)hipFree(p);
    *t = KangTable();
}

hipError_t bsgs_kang_table_begin(bsgs_dev *d, KangTable *t, uint64_t slots, bool owners, u32 **out, size_t out_bytes, bool *nomem)
{
    hipError_t e = hipMalloc(&t->tag, (size_t)slots * 8);
    if (e == hipSuccess) e = hipMalloc(&t->d, (size_t)slots * 16);
    if (e == hipSuccess && owners) e = hipMalloc(&t->who, (size_t)slots * 8);
    if (e == hipSuccess) e = hipMalloc(&t->ctr, 64);
    if (e == hipSuccess && !*out) e = hipMalloc(out, out_bytes);
    *nomem = e != hipSuccess;
    if (*nomem) (void)hipGetLastError();
    if (e == hipSuccess) e = hipMemsetAsync(t->tag, 0, (size_t)slots * 8, d->stream);      // empty = tag 0; offset and owner are read only where a tag stands
    if (e == hipSuccess) e = hipMemsetAsync(t->ctr, 0, 64, d->stream);
    if (e == hipSuccess) e = hipMemsetAsync(*out, 0, KANG_REC_HEADER, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) bsgs_kang_table_free(t);                    // no table is left, whatever failed
    else t->slots = slots;
    return e;
}

int bsgs_kang_table_entries(bsgs_dev *d, const KangTable *t, uint64_t *n_entries)
{
    uint64_t n = 0;
    HIPCHK(hipMemcpyAsync(&n, t->ctr + CTR_ENTRIES, 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    if (n_entries) *n_entries = n;
    return BSGS_OK;
}

int bsgs_kang_table_herd(bsgs_dev *d, bsgs_kangaroo **k, KangTable bsgs_kangaroo::*table, const char *herds, const char *begin)
{
    if (!d) return fail(BSGS_ERR_ARG, "null");
    *k = d->kangaroo;
    if (!*k) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_setup first");
    if ((*k)->key) return fail(BSGS_ERR_STATE, "%s", herds);
    if (begin && !((*k)->*table).tag) return fail(BSGS_ERR_STATE, "%s", begin);
    return BSGS_OK;
}

int bsgs_kang_table_stage(bsgs_dev *d, bsgs_kangaroo *k, u32 *out, const bsgs_kangaroo_record *recs, const uint64_t *n)
{
    if (*n > k->cap) return fail(BSGS_ERR_ARG, "%u records: at most the record capacity %u", (uint32_t)*n, k->cap);
    HIPCHK(hipSetDevice(d->id));
    HIPCHK(hipMemsetAsync(out, 0, KANG_REC_HEADER, d->stream));
    HIPCHK(hipMemsetAsync(k->rec, 0, KANG_REC_HEADER, d->stream));
    HIPCHK(hipMemcpyAsync(k->rec, n, 8, hipMemcpyHostToDevice, d->stream));
    if (*n) HIPCHK(hipMemcpyAsync((char *)k->rec + KANG_REC_HEADER, recs, (size_t)*n * 64, hipMemcpyHostToDevice, d->stream));      // into the walk's record buffer
    return BSGS_OK;
}

int bsgs_kang_table_loaded(bsgs_dev *d, const KangTable *t, hipError_t e, uint64_t n, uint64_t *n_stored, uint64_t *n_duplicate, uint64_t *n_zero, uint64_t *n_full,
                           uint64_t *n_entries, const char *text)
{
    uint64_t c[8] = {0};
    if (e == hipSuccess) e = hipMemcpyAsync(c, t->ctr, sizeof c, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    HIPCHK(e);
    if (n_stored) *n_stored = c[CTR_STORED];
    if (n_duplicate) *n_duplicate = c[CTR_DUPLICATE];
    if (n_zero) *n_zero = c[CTR_ZERO];
    if (n_full) *n_full = c[CTR_FULL];
    if (n_entries) *n_entries = c[CTR_ENTRIES];
    const uint64_t sum = c[CTR_STORED] + c[CTR_DUPLICATE] + c[CTR_ZERO] + c[CTR_FULL];
    if (sum != n) return fail(BSGS_ERR_STATE, text, (unsigned long long)n, (unsigned long long)sum);
    return BSGS_OK;
}

int bsgs_kang_table_met_check(uint64_t met, uint64_t entries, const char *what)
{
    if (met != entries) return fail(BSGS_ERR_STATE, "%s: %llu occupied slots, %llu entries counted", what, (unsigned long long)met, (unsigned long long)entries);
    return BSGS_OK;
}

// ---- host: the growing tame table -----------------------------------------------------------------------------------------------------------------------
int bsgs_kangaroo_tames_gen_herd(bsgs_dev *d, bsgs_kangaroo **k, bool table)
{
    return bsgs_kang_table_herd(d, k, &bsgs_kangaroo::gen, "a tame table grows under the herds of bsgs_kangaroo_setup and bsgs_kangaroo_setup_sym",
                                table ? "bsgs_kangaroo_tames_gen_begin first" : nullptr);
}

// the insert of the n records in k->rec (their count at its head) on the stream, the hand-backs to recs, the entry count
static int tames_gen_insert(bsgs_dev *d, bsgs_kangaroo *k)
{
    TamesGenArgs A;
    A.rec = k->rec; A.tag = k->gen.tag; A.d = k->gen.d; A.out = k->tames_rec; A.entries = k->gen.ctr + CTR_ENTRIES; A.slot_mask = k->gen.slots - 1; A.cap = k->cap;
    const u32 blocks = std::min((k->cap + 255u) / 256u, KT_INSERT_GRID_MAX);
    hipLaunchKernelGGL(kangaroo_tames_gen_insert_kernel, dim3(blocks), dim3(256), 0, d->stream, A);
    HIPCHK(hipGetLastError());
    return BSGS_OK;
}

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int bsgs_kangaroo_tames_gen_begin(bsgs_dev *d, uint64_t capacity)
{
    bsgs_kangaroo *k = nullptr;
    if (int rc = bsgs_kangaroo_tames_gen_herd(d, &k, false)) return rc;
    if (!capacity || capacity > KT_MAX_CAPACITY) return fail(BSGS_ERR_ARG, "growing tame table of %llu entries: 1..2^31", (unsigned long long)capacity);
    HIPCHK(hipSetDevice(d->id));
    HIPCHK(hipStreamSynchronize(d->stream));
    bsgs_kang_table_free(&k->gen);
    const uint64_t slots = bsgs_kang_table_slots(capacity, k->cap);
    const size_t rec_bytes = KANG_REC_HEADER + (size_t)k->cap * 64;
    bool nomem = false;
    const hipError_t e = bsgs_kang_table_begin(d, &k->gen, slots, false, &k->tames_rec, rec_bytes, &nomem);      // the hand-back buffer: the match's buffer of this herd, never used by both at once
    if (nomem)
        return fail(BSGS_ERR_NOMEM, "growing tame table of %llu entries: %llu slots need %llu bytes of tags, %llu of offsets and %llu of records (%s)", (unsigned long long)capacity,
                    (unsigned long long)slots, (unsigned long long)(slots * 8), (unsigned long long)(slots * 16), (unsigned long long)rec_bytes, hipGetErrorString(e));
    HIPCHK(e);
    return BSGS_OK;
}

extern "C" int bsgs_kangaroo_run_tames_gen(bsgs_dev *d, uint32_t steps, bsgs_kangaroo_record *recs, uint32_t max_recs, uint32_t *nrecs, uint64_t *n_seen,
                                           uint64_t *n_entries, uint64_t *dropped, float *kernel_ms)
{
    if (!d || !nrecs) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = nullptr;
    if (int rc = bsgs_kangaroo_tames_gen_herd(d, &k, true)) return rc;
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
    if (int rc = bsgs_kang_table_entries(d, &k->gen, n_entries)) return rc;
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
    if (int rc = bsgs_kangaroo_tames_gen_herd(d, &k, true)) return rc;
    const uint64_t count = n;
    if (int rc = bsgs_kang_table_stage(d, k, k->tames_rec, recs_in, &count)) return rc;
    if (int rc = tames_gen_insert(d, k)) return rc;
    uint64_t back = 0;
    HIPCHK(hipMemcpyAsync(&back, k->tames_rec, 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    back = std::min<uint64_t>(back, n);
    uint32_t give = 0;
    if (int rc = bsgs_kangaroo_copy_out(d, k->tames_rec, back, recs_out, max_recs, &give)) return rc;
    *nrecs = give;
    return bsgs_kang_table_entries(d, &k->gen, n_entries);
}

extern "C" int bsgs_kangaroo_tames_gen_read(bsgs_dev *d, uint64_t *x_lo64, uint8_t *d_le, uint64_t max, uint64_t *n)
{
    if (!d || !n) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = nullptr;
    if (int rc = bsgs_kangaroo_tames_gen_herd(d, &k, true)) return rc;
    HIPCHK(hipSetDevice(d->id));
    uint64_t entries = 0;
    if (int rc = bsgs_kang_table_entries(d, &k->gen, &entries)) return rc;
    *n = entries;
    if (max < entries) return fail(BSGS_ERR_ARG, "room for %llu entries, the table holds %llu", (unsigned long long)max, (unsigned long long)entries);
    if (!entries) return BSGS_OK;
    if (!x_lo64 || !d_le) return fail(BSGS_ERR_ARG, "null");
    TamesGenHarvestArgs H;
    H.tag = k->gen.tag; H.d = k->gen.d; H.out_tag = nullptr; H.out_d = nullptr; H.count = k->gen.ctr + CTR_MET; H.slots = k->gen.slots; H.max = entries;
    hipError_t e = hipMalloc(&H.out_tag, (size_t)entries * 8);
    if (e == hipSuccess) e = hipMalloc(&H.out_d, (size_t)entries * 16);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (H.out_tag) (void)hipFree(H.out_tag);
        return fail(BSGS_ERR_NOMEM, "reading a growing tame table of %llu entries: %llu bytes of device memory (%s)", (unsigned long long)entries, (unsigned long long)(entries * 24),
                    hipGetErrorString(e));
    }
    uint64_t met = 0;
    e = hipMemsetAsync(H.count, 0, 8, d->stream);
    if (e == hipSuccess) {
        const u32 blocks = (u32)std::min<uint64_t>((k->gen.slots + 255u) / 256u, KT_SCAN_GRID_MAX);
        hipLaunchKernelGGL(kangaroo_tames_gen_harvest_kernel, dim3(blocks), dim3(256), 0, d->stream, H);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&met, H.count, 8, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(x_lo64, H.out_tag, (size_t)entries * 8, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_le, H.out_d, (size_t)entries * 16, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    (void)hipFree(H.out_tag);
    (void)hipFree(H.out_d);
    HIPCHK(e);
    return bsgs_kang_table_met_check(met, entries, "growing tame table");
}

extern "C" int bsgs_kangaroo_tames_gen_end(bsgs_dev *d)
{
    if (!d) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = d->kangaroo;
    if (!k || !k->gen.tag) return BSGS_OK;
    HIPCHK(hipSetDevice(d->id));
    HIPCHK(hipStreamSynchronize(d->stream));
    bsgs_kang_table_free(&k->gen);
    return BSGS_OK;
}
