// kangaroo_tames.hip -- a tame table in device memory and the matching of a launch's records against it (include/bsgs_hip.h, "Kangaroo, tame table" and
// "Kangaroo, tame table for the symmetric walk").  A wild-only search at a low dp writes millions of records per second of which a handful
// matter: the records of a launch are matched here, in HBM, and only those that hit a table entry (and the DEAD ones, which the host must re-seed) cross the bus.
//   image     open addressing in 64-byte lines: four u64 tags (the low 64 bits of x), four u32 entry numbers, a u32 count, a u32 "overflowed" mark, 8 bytes
//             of zero.  Built on the host by a pure function (bsgs_kangaroo_tames_image), entries in the order given: byte for byte what the model builds.
//   matching  one record per lane: the home line in four 16-byte loads, the `count` live tags compared, the next line only while the line is marked; the loop
//             is bounded by the number of lines, so it ends on any image.  Kept records are compacted as kang_record does: __ballot, one atomic per wave,
//             vector stores only.  No LDS, no scratch.
//   two herds the plain match writes the entry number into the record's `reserved` word.  In the herd of bsgs_kangaroo_setup_sym_keys that word is the
//             kangaroo's key and the host needs both: the keyed match (KEYED) copies the kept record as the walk wrote it and puts the entry number + 1
//             into a u32 array of its own, one word per kept record in the same slot order.  The array lies behind the compacted records in one allocation.
#include "bsgs_internal.h"

#define TAMES_SLOTS 4u
#define TAMES_MIN_LINES 64ull
#define TAMES_MAX_ENTRIES (1ull << 31)
#define TAMES_GRID_MAX 1024u                                // blocks of the match: four per CU; a wave strides over the records

struct TamesLine { uint64_t tag[TAMES_SLOTS]; uint32_t entry[TAMES_SLOTS]; uint32_t count, overflowed, zero[2]; };
static_assert(sizeof(TamesLine) == 64, "a line of the tame table: 64 bytes");

struct TamesArgs {
    const u32 *rec;        // the walk's record buffer: u64 count | records
    const u32x4 *image;    // [lines] lines of four vectors: tags 0 1 | tags 2 3 | entries | count, overflowed, 0, 0
    u32 *out;              // the compacted records, same layout as rec
    u32 *entry;            // KEYED: [cap] entry number + 1 of the record in the same slot of out, 0: a DEAD record that matched nothing; else nullptr
    u32 line_mask, cap;
};

template <bool KEYED>
__device__ __forceinline__ void tames_match(const TamesArgs &A)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 count = *(const u64 *)A.rec;
    const u32 n = count < (u64)A.cap ? (u32)count : A.cap;           // what the walk wrote; the rest was counted only
    const u32 stride = gridDim.x * blockDim.x;
    const u32x4 *const recs = (const u32x4 *)((const char *)A.rec + KANG_REC_HEADER);
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
            if (keep && slot < A.cap) {                              // (never more kept than read; the bound of every store)
                u32x4 *o = (u32x4 *)((char *)A.out + KANG_REC_HEADER) + slot * 4;
                o[0] = r0;
                o[1] = recs[(u64)i * 4 + 1];
                o[2] = recs[(u64)i * 4 + 2];
                if (KEYED) {
                    o[3] = r3;                                       // kangaroo, flags, step and the key, as the walk wrote them
                    A.entry[slot] = found;
                } else o[3] = (u32x4){r3.x, r3.y, r3.z, found};
            }
        }
    }
}
__global__ void __launch_bounds__(256) kangaroo_tames_match_kernel(const TamesArgs A) { tames_match<false>(A); }
__global__ void __launch_bounds__(256) kangaroo_tames_match_keys_kernel(const TamesArgs A) { tames_match<true>(A); }

// ---- the builder: no device -------------------------------------------------------------------------------------------------------------------------
static uint64_t tames_lines(uint64_t n)
{
    uint64_t lines = TAMES_MIN_LINES;
    while (lines * 2 < n) lines *= 2;                                // the power of two at or above n / 2: at most half of the 4 * lines slots are used
    return lines;
}

extern "C" int bsgs_kangaroo_tames_image(const uint64_t *x_lo64, uint64_t n, void *out, uint64_t out_bytes, uint64_t *lines_out)
{
    if (!n || n > TAMES_MAX_ENTRIES) return fail(BSGS_ERR_ARG, "tame table of %llu entries: 1..2^31", (unsigned long long)n);
    const uint64_t lines = tames_lines(n), mask = lines - 1;
    if (lines_out) *lines_out = lines;
    if (!out) return BSGS_OK;                                        // the size alone
    if (!x_lo64) return fail(BSGS_ERR_ARG, "null");
    if (out_bytes < lines * 64) return fail(BSGS_ERR_ARG, "image buffer of %llu bytes: %llu lines need %llu", (unsigned long long)out_bytes,
                                            (unsigned long long)lines, (unsigned long long)(lines * 64));
    TamesLine *L = (TamesLine *)out;
    memset(L, 0, lines * 64);
    for (uint64_t e = 0; e < n; e++) {
        const uint64_t tag = x_lo64[e];
        uint64_t line = (tag >> 6) & mask;
        for (;;) {                                                   // ends: fewer than half of the slots are taken
            TamesLine &l = L[line];
            for (uint32_t s = 0; s < l.count; s++)
                if (l.tag[s] == tag) return fail(BSGS_ERR_ARG, "tame table: entries %u and %llu share the tag %016llx", l.entry[s], (unsigned long long)e,
                                                 (unsigned long long)tag);
            if (l.count < TAMES_SLOTS) {
                l.tag[l.count] = tag;
                l.entry[l.count] = (uint32_t)e;
                l.count++;
                break;
            }
            l.overflowed = 1;
            line = (line + 1) & mask;
        }
    }
    return BSGS_OK;
}

// ---- install and run, both herds: keyed = the herd of bsgs_kangaroo_setup_sym_keys (the callers have checked that it is) --------------------------------
static int tames_install(bsgs_dev *d, bsgs_kangaroo *k, const uint64_t *x_lo64, uint64_t n, bool keyed)
{
    uint64_t lines = 0;
    if (int rc = bsgs_kangaroo_tames_image(x_lo64, n, nullptr, 0, &lines)) return rc;
    std::vector<uint8_t> image((size_t)lines * 64);
    if (int rc = bsgs_kangaroo_tames_image(x_lo64, n, image.data(), image.size(), &lines)) return rc;
    HIPCHK(hipSetDevice(d->id));
    HIPCHK(hipStreamSynchronize(d->stream));
    if (k->tames) (void)hipFree(k->tames);
    k->tames = nullptr; k->tames_lines = 0; k->tames_n = 0;
    HIPCHK(hipMalloc(&k->tames, image.size()));
    if (!k->tames_rec) HIPCHK(hipMalloc(&k->tames_rec, KANG_REC_HEADER + (size_t)k->cap * 64 + (keyed ? (size_t)k->cap * 4 : 0)));      // records, then the entry words
    HIPCHK(hipMemcpyAsync(k->tames, image.data(), image.size(), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    k->tames_lines = lines; k->tames_n = n;
    return BSGS_OK;
}

static int tames_run(bsgs_dev *d, bsgs_kangaroo *k, bool keyed, uint32_t steps, bsgs_kangaroo_record *recs, uint32_t *entries, uint32_t max_recs, uint32_t *nrecs,
                     uint64_t *n_seen, uint64_t *dropped, float *kernel_ms)
{
    HIPCHK(hipSetDevice(d->id));
    HIPCHK(hipMemsetAsync(k->tames_rec, 0, KANG_REC_HEADER, d->stream));
    if (int rc = bsgs_kangaroo_launch(d, steps)) return rc;          // the walk, timed from ev0
    TamesArgs A;
    A.rec = k->rec; A.image = k->tames; A.out = k->tames_rec; A.line_mask = (u32)(k->tames_lines - 1); A.cap = k->cap;
    A.entry = keyed ? (u32 *)((char *)k->tames_rec + KANG_REC_HEADER + (size_t)k->cap * 64) : nullptr;
    const u32 blocks = std::min((k->cap + 255u) / 256u, TAMES_GRID_MAX);
    if (keyed) hipLaunchKernelGGL(kangaroo_tames_match_keys_kernel, dim3(blocks), dim3(256), 0, d->stream, A);
    else hipLaunchKernelGGL(kangaroo_tames_match_kernel, dim3(blocks), dim3(256), 0, d->stream, A);
    HIPCHK(hipGetLastError());
    uint64_t count = 0, kept = 0;
    if (int rc = bsgs_kangaroo_finish(d, &count, k->tames_rec, &kept, kernel_ms)) return rc;      // ev1 behind the match, both counts, the synchronisation
    const uint64_t held = std::min<uint64_t>(count, k->cap);
    kept = std::min<uint64_t>(kept, held);
    uint32_t give = 0;
    if (int rc = bsgs_kangaroo_copy_out(d, k->tames_rec, kept, recs, max_recs, &give)) return rc;
    if (keyed && give) {
        HIPCHK(hipMemcpyAsync(entries, A.entry, (size_t)give * 4, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
    }
    *nrecs = give;
    if (n_seen) *n_seen = count;
    if (dropped) *dropped = (count - held) + (kept - give);          // never matched, and matched but not handed over
    return BSGS_OK;
}

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int bsgs_kangaroo_tames_install(bsgs_dev *d, const uint64_t *x_lo64, uint64_t n)
{
    if (!d || !x_lo64) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = d->kangaroo;
    if (!k) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_setup first");
    if (k->key) return fail(BSGS_ERR_STATE, "a tame table serves the herds of bsgs_kangaroo_setup and bsgs_kangaroo_setup_sym");
    return tames_install(d, k, x_lo64, n, false);
}
extern "C" int bsgs_kangaroo_tames_install_keys(bsgs_dev *d, const uint64_t *x_lo64, uint64_t n)
{
    if (!d || !x_lo64) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = d->kangaroo;
    if (!k) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_setup first");
    if (!k->key) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_tames_install_keys serves the herd of bsgs_kangaroo_setup_sym_keys");
    return tames_install(d, k, x_lo64, n, true);
}

extern "C" int bsgs_kangaroo_run_tames(bsgs_dev *d, uint32_t steps, bsgs_kangaroo_record *recs, uint32_t max_recs, uint32_t *nrecs, uint64_t *n_seen,
                                       uint64_t *dropped, float *kernel_ms)
{
    if (!d || !nrecs) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = d->kangaroo;
    if (!k) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_setup first");
    if (!k->tames) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_tames_install first");
    return tames_run(d, k, false, steps, recs, nullptr, max_recs, nrecs, n_seen, dropped, kernel_ms);
}
extern "C" int bsgs_kangaroo_run_tames_keys(bsgs_dev *d, uint32_t steps, bsgs_kangaroo_record *recs, uint32_t *entries, uint32_t max_recs, uint32_t *nrecs,
                                            uint64_t *n_seen, uint64_t *dropped, float *kernel_ms)
{
    if (!d || !nrecs || (recs && !entries)) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = d->kangaroo;
    if (!k) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_setup first");
    if (!k->key) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_run_tames_keys serves the herd of bsgs_kangaroo_setup_sym_keys");
    if (!k->tames) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_tames_install_keys first");
    return tames_run(d, k, true, steps, recs, entries, max_recs, nrecs, n_seen, dropped, kernel_ms);
}
