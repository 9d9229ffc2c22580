// kangaroo_tames_keys.hip -- the tame table for a herd whose records carry a key word (bsgs_kangaroo_setup_sym_keys; include/bsgs_hip.h "Kangaroo, tame
// table for the symmetric walk").  The match of kangaroo_tames.hip writes the entry number into the record's `reserved` word; in this herd that
// word is the kangaroo's key and the host needs both.  Here the same image and the same lookup, the kept record copied as the walk wrote it, and the entry
// number + 1 in a u32 array of its own, one word per kept record in the same slot order.  The array lies behind the compacted records in one allocation.
//   matching  one record per lane, one 64-byte line per lookup step (four 16-byte loads), the loop bounded by the number of lines; kept records compacted
//             with __ballot and one atomic per wave, vector stores only.  No LDS, no scratch.
// kangaroo_tames.hip is not touched: its kernel and its two calls serve the herds they served.
#include "bsgs_internal.h"

#define TAMES_REC_HEADER 64u                                // as the walk's record buffer: u64 count, then records from byte 64
#define TAMES_GRID_MAX 1024u                                // blocks of the match: four per CU; a wave strides over the records

struct TamesKeysArgs {
    const u32 *rec;        // the walk's record buffer: u64 count | records
    const u32x4 *image;    // [lines] lines of four vectors: tags 0 1 | tags 2 3 | entries | count, overflowed, 0, 0
    u32 *out;              // the compacted records, same layout as rec
    u32 *entry;            // [cap] entry number + 1 of the record in the same slot of out, 0: a DEAD record that matched nothing
    u32 line_mask, cap;
};

__global__ void __launch_bounds__(256) kangaroo_tames_match_keys_kernel(const TamesKeysArgs A)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 count = *(const u64 *)A.rec;
    const u32 n = count < (u64)A.cap ? (u32)count : A.cap;           // what the walk wrote; the rest was counted only
    const u32 stride = gridDim.x * blockDim.x;
    const u32x4 *const recs = (const u32x4 *)((const char *)A.rec + TAMES_REC_HEADER);
    for (u32 base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n; base += stride) {      // wave-uniform: every lane reaches the ballot
        const u32 i = base + lane;
        bool keep = false;
        u32 found = 0;                                               // entry number + 1
        u32x4 r0 = {0, 0, 0, 0}, r3 = {0, 0, 0, 0};
        if (i < n) {
            r0 = recs[(u64)i * 4];
            r3 = recs[(u64)i * 4 + 3];
            const u64 tag = ((u64)r0.y << 32) | r0.x;
            u32 line = (u32)(tag >> 6) & A.line_mask;
            for (u32 it = 0; it <= A.line_mask; it++) {
                const u32x4 *L = A.image + (u64)line * 4;
                const u32x4 t01 = L[0], t23 = L[1], e = L[2], c = L[3];
                const u32 live = c.x;                                // (a damaged count above four reads the four slots there are)
                if (live > 0u && t01.x == r0.x && t01.y == r0.y) found = e.x + 1u;
                if (live > 1u && t01.z == r0.x && t01.w == r0.y) found = e.y + 1u;
                if (live > 2u && t23.x == r0.x && t23.y == r0.y) found = e.z + 1u;
                if (live > 3u && t23.z == r0.x && t23.w == r0.y) found = e.w + 1u;
                if (found || !c.y) break;
                line = (line + 1u) & A.line_mask;
            }
            keep = found != 0u || (r3.y & BSGS_KANGAROO_DEAD) != 0u;
        }
        const u64 m = __ballot(keep);
        if (m) {
            u64 slot0 = 0;
            const int leader = __builtin_ctzll(m);
            if ((int)lane == leader) slot0 = atomicAdd((unsigned long long *)A.out, (unsigned long long)__builtin_popcountll(m));
            slot0 = __shfl(slot0, leader);
            const u64 slot = slot0 + (u64)__builtin_popcountll(m & ((1ull << lane) - 1));
            if (keep && slot < A.cap) {                              // (never more kept than read; the bound of both stores)
                u32x4 *o = (u32x4 *)((char *)A.out + TAMES_REC_HEADER) + slot * 4;
                o[0] = r0;
                o[1] = recs[(u64)i * 4 + 1];
                o[2] = recs[(u64)i * 4 + 2];
                o[3] = r3;                                           // kangaroo, flags, step and the key, as the walk wrote them
                A.entry[slot] = found;
            }
        }
    }
}

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int bsgs_kangaroo_tames_install_keys(bsgs_dev *d, const uint64_t *x_lo64, uint64_t n)
{
    if (!d || !x_lo64) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = d->kangaroo;
    if (!k) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_setup first");
    if (!k->key) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_tames_install_keys serves the herd of bsgs_kangaroo_setup_sym_keys");
    uint64_t lines = 0;
    if (int rc = bsgs_kangaroo_tames_image(x_lo64, n, nullptr, 0, &lines)) return rc;
    std::vector<uint8_t> image((size_t)lines * 64);
    if (int rc = bsgs_kangaroo_tames_image(x_lo64, n, image.data(), image.size(), &lines)) return rc;
    HIPCHK(hipSetDevice(d->id));
    HIPCHK(hipStreamSynchronize(d->stream));
    if (k->tames) (void)hipFree(k->tames);
    k->tames = nullptr; k->tames_lines = 0; k->tames_n = 0;
    HIPCHK(hipMalloc(&k->tames, image.size()));
    if (!k->tames_rec) HIPCHK(hipMalloc(&k->tames_rec, TAMES_REC_HEADER + (size_t)k->cap * 64 + (size_t)k->cap * 4));      // records, then the entry words
    HIPCHK(hipMemcpyAsync(k->tames, image.data(), image.size(), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    k->tames_lines = lines; k->tames_n = n;
    return BSGS_OK;
}

extern "C" int bsgs_kangaroo_run_tames_keys(bsgs_dev *d, uint32_t steps, bsgs_kangaroo_record *recs, uint32_t *entries, uint32_t max_recs, uint32_t *nrecs,
                                            uint64_t *n_seen, uint64_t *dropped, float *kernel_ms)
{
    if (!d || !nrecs || (recs && !entries)) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = d->kangaroo;
    if (!k) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_setup first");
    if (!k->key) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_run_tames_keys serves the herd of bsgs_kangaroo_setup_sym_keys");
    if (!k->tames) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_tames_install_keys first");
    HIPCHK(hipSetDevice(d->id));
    HIPCHK(hipMemsetAsync(k->tames_rec, 0, TAMES_REC_HEADER, d->stream));
    if (int rc = bsgs_kangaroo_launch(d, steps)) return rc;          // the walk, timed from ev0
    u32 *const entry_dev = (u32 *)((char *)k->tames_rec + TAMES_REC_HEADER + (size_t)k->cap * 64);
    TamesKeysArgs A;
    A.rec = k->rec; A.image = k->tames; A.out = k->tames_rec; A.entry = entry_dev; A.line_mask = (u32)(k->tames_lines - 1); A.cap = k->cap;
    const u32 blocks = std::min((k->cap + 255u) / 256u, TAMES_GRID_MAX);
    hipLaunchKernelGGL(kangaroo_tames_match_keys_kernel, dim3(blocks), dim3(256), 0, d->stream, A);
    HIPCHK(hipGetLastError());
    uint64_t count = 0, kept = 0;
    if (int rc = bsgs_kangaroo_finish(d, &count, k->tames_rec, &kept, kernel_ms)) return rc;      // ev1 behind the match, both counts, the synchronisation
    const uint64_t held = std::min<uint64_t>(count, k->cap);
    kept = std::min<uint64_t>(kept, held);
    uint32_t give = 0;
    if (int rc = bsgs_kangaroo_copy_out(d, k->tames_rec, kept, recs, max_recs, &give)) return rc;
    if (give) {
        HIPCHK(hipMemcpyAsync(entries, entry_dev, (size_t)give * 4, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
    }
    *nrecs = give;
    if (n_seen) *n_seen = count;
    if (dropped) *dropped = (count - held) + (kept - give);          // never matched, and matched but not handed over
    return BSGS_OK;
}
