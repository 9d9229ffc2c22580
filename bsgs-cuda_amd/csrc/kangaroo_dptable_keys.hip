// kangaroo_dptable_keys.hip -- the distinguished-point table of a search for a LIST of keys, kept in device memory (include/bsgs_hip.h, "Kangaroo,
// distinguished-point table for a key list"; tests/kangaroo_dptable_keys_model.py restates it).  The table of kangaroo_dptable.hip with the work
// file's owner word where the type stands: who[slots] = (u32 kangaroo, u32 owner), owner 0 tame, 1 + key wild, bit 31 for a wild record with NEG in the herd
// of bsgs_kangaroo_setup_sym_keys.  The table, its claim and the coherence rule: kangaroo_table.hip.h.
//   insert    the insert of kangaroo_dptable.hip -- one record per lane, a wave strides, DEAD and tag-0 records handed back, a duplicate handed back as a
//             PAIR behind a placeholder, no slot handed back as FULL, one reservation and one count per wave, every store bounded -- with two differences:
//             the owner word is stored, and a handed-back record keeps its key: `reserved` = reason | key << BSGS_KANGAROO_DPT_KEY_SHIFT.  The key is
//             (flags >> BSGS_KANGAROO_KEY_SHIFT) & 0xFFFF in the herd of bsgs_kangaroo_setup, the record's `reserved` in that of bsgs_kangaroo_setup_sym_keys
//             (`sym`, a kernel argument: wave-uniform, one select per record).  Nothing is ever indexed by a key.
//   resolve, load, harvest: those of kangaroo_dptable.hip, which copy who[s].y as it is; the host side is that unit's too (bsgs_kang_dpt_*).
#include "kangaroo_table.hip.h"

#define DPT_KEEP 0xFFFFFFFFu                                // (not a reason: the record went into the table)

struct DptKeysArgs {
    const u32 *rec;        // the walk's record buffer: u64 count | records
    u64 *tag;              // [slots]
    u32x4 *d;              // [slots]
    u32x2 *who;            // [slots]
    u32 *out;              // the hand-backs: u64 places taken, u64 records handed back | records; `reserved` = reason | key << 8, or BSGS_KANGAROO_DPT_STORED
    u64 *ctr;              // the table's counters
    u64 slot_mask;
    u32 cap;               // records read at most
    u32 out_cap;           // places of `out`
    u32 sym;               // the herd of bsgs_kangaroo_setup_sym_keys: the key in `reserved`, NEG in the owner
};

__global__ void __launch_bounds__(256) kangaroo_dptable_insert_keys_kernel(const DptKeysArgs A)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 count = *(const u64 *)A.rec;
    const u32 n = count < (u64)A.cap ? (u32)count : A.cap;           // what the walk wrote; the rest was counted only
    const u32 stride = gridDim.x * blockDim.x;
    const u32x4 *const recs = (const u32x4 *)((const char *)A.rec + KANG_REC_HEADER);
    for (u32 base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n; base += stride) {      // wave-uniform: every lane reaches the ballots
        const u32 i = base + lane;
        u32 reason = DPT_KEEP, key = 0;
        bool stored = false;
        u64 s = 0;
        u32x4 r0 = {0, 0, 0, 0}, r3 = {0, 0, 0, 0};
        if (i < n) {
            r0 = recs[(u64)i * 4];
            r3 = recs[(u64)i * 4 + 3];
            const u64 tag = ((u64)r0.y << 32) | r0.x;
            key = (A.sym ? r3.w : r3.y >> BSGS_KANGAROO_KEY_SHIFT) & 0xFFFFu;
            if (r3.y & BSGS_KANGAROO_DEAD) reason = BSGS_KANGAROO_DPT_DEAD;
            else if (tag == 0ull) reason = BSGS_KANGAROO_DPT_TAG_ZERO;
            else {
                const u32 neg = A.sym ? (r3.y & BSGS_KANGAROO_NEG) << 30 : 0u;      // NEG = 2 -> bit 31
                const u32 owner = (r3.y & BSGS_KANGAROO_WILD) ? ((1u + key) | neg) : 0u;
                const u32 got = kt_claim(A.tag, A.slot_mask, tag, s, [&](u64 at) {
                    A.d[at] = recs[(u64)i * 4 + 2];
                    A.who[at] = (u32x2){r3.x, owner};
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
            o[3] = (u32x4){r3.x, r3.y, r3.z, reason | key << BSGS_KANGAROO_DPT_KEY_SHIFT};      // never BSGS_KANGAROO_DPT_STORED: a reason is 0..3
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------------
static_assert(BSGS_KANGAROO_DPT_STORED < (1u << BSGS_KANGAROO_DPT_KEY_SHIFT), "a reason stays below the key");

int bsgs_kang_dpt_insert_keys_launch(bsgs_dev *d, bsgs_kangaroo *k, uint32_t blocks)
{
    DptKeysArgs A;
    A.rec = k->rec; A.tag = k->dpt.tag; A.d = k->dpt.d; A.who = k->dpt.who; A.out = k->dpt_out; A.ctr = k->dpt.ctr; A.slot_mask = k->dpt.slots - 1;
    A.cap = k->cap; A.out_cap = bsgs_kang_dpt_out_cap(k); A.sym = k->key ? 1u : 0u;
    hipLaunchKernelGGL(kangaroo_dptable_insert_keys_kernel, dim3(blocks), dim3(256), 0, d->stream, A);
    HIPCHK(hipGetLastError());
    return BSGS_OK;
}

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int bsgs_kangaroo_dptable_begin_keys(bsgs_dev *d, uint64_t capacity) { return bsgs_kang_dpt_begin(d, capacity, BSGS_DPT_KEYED); }

extern "C" int bsgs_kangaroo_run_dptable_keys(bsgs_dev *d, uint32_t steps, bsgs_kangaroo_record *recs, uint32_t max_recs, uint32_t *nrecs, uint64_t *n_seen,
                                              uint64_t *n_entries, uint64_t *dropped, float *kernel_ms)
{
    return bsgs_kang_dpt_run(d, BSGS_DPT_KEYED, steps, recs, max_recs, nrecs, n_seen, n_entries, dropped, kernel_ms);
}

extern "C" int bsgs_kangaroo_dptable_insert_keys(bsgs_dev *d, const bsgs_kangaroo_record *recs_in, uint32_t n, bsgs_kangaroo_record *recs_out, uint32_t max_recs,
                                                 uint32_t *nrecs, uint64_t *n_entries, uint64_t *dropped)
{
    return bsgs_kang_dpt_insert(d, BSGS_DPT_KEYED, recs_in, n, recs_out, max_recs, nrecs, n_entries, dropped);
}
