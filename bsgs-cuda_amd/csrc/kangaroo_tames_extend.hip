// kangaroo_tames_extend.hip -- what stands around the tame table grown on the device (kangaroo_tames_gen.hip; include/bsgs_hip.h, "Kangaroo, tame table grown on
// the device", the paragraphs "load" and "sorted read"; tests/kangaroo_tames_extend_model.py restates it): entries made earlier are loaded into the
// growing table, and the finished table leaves the device sorted by tag and cut.  A unit of its own: the insert and the harvest of kangaroo_tames_gen.hip are
// compiled as they were.
//   load      (tag, d) pairs of the caller's, 24 bytes each, staged in chunks of TAMES_LOAD_CHUNK.  One pair per lane, a wave strides over the chunk; each pair
//             claims a slot by the table's rule (kangaroo_table.hip.h, with the coherence rule).  Nothing is handed back: the four outcomes are counted.
//   sorted    harvest as kangaroo_tames_gen.hip's (the wave's reservation of kangaroo_table.hip.h), which also numbers the entries and folds the OR and the AND of all
//   read      tags (one atomic each per wave); then an LSD radix sort of (tag, u32 number) by 8-bit digits.  A digit on which all tags agree -- a zero byte of
//             OR ^ AND -- costs no pass.  A pass is three kernels, and no block waits for another inside one:
//               hist     block b counts the digits of its tile of TAMES_SORT_TILE entries in LDS -> counts[digit][b]
//               scan     block `digit` turns counts[digit][*] into exclusive prefixes and leaves the digit's total
//               scatter  block b: where digit v of tile b starts = (totals of the digits below v) + counts[v][b]; its four waves own consecutive sub-tiles, a
//                        wave takes 64 entries a round in order, lanes of equal digit find each other by eight ballots and rank by lane, so the pass is stable
//             and one gather of the 16-byte d by number for the entries that cross the bus.  Every store is bounded by n.
#include "kangaroo_table.hip.h"

#define TAMES_LOAD_CHUNK BSGS_KANGAROO_TAMES_LOAD_CHUNK   // pairs staged per kernel
#define TAMES_SORT_TILE BSGS_KANGAROO_TAMES_SORT_TILE     // entries per block and pass: 4 waves x TAMES_SORT_ROUNDS rounds x 64 lanes
#define TAMES_SORT_ROUNDS 8u
static_assert(TAMES_SORT_TILE == 4u * TAMES_SORT_ROUNDS * 64u, "a block's tile is four waves' sub-tiles");

struct TamesLoadArgs {
    const u64 *in_tag;     // [n] the staged chunk
    const u32x4 *in_d;     // [n]
    u64 *tag;              // [slots]
    u32x4 *d;              // [slots]
    u64 *ctr;              // the table's counters
    u64 slot_mask;
    u32 n;
};

__global__ void __launch_bounds__(256) kangaroo_tames_load_kernel(const TamesLoadArgs A)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 stride = gridDim.x * blockDim.x;
    for (u32 base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < A.n; base += stride) {      // wave-uniform: every lane reaches the ballots
        const u32 i = base + lane;
        u32 what = 0;                                                // 0: no pair in this lane; else CTR_*
        if (i < A.n) {
            const u64 tag = A.in_tag[i];
            u64 s;
            what = tag == 0ull ? CTR_ZERO : kt_claim(A.tag, A.slot_mask, tag, s, [&](u64 at) { A.d[at] = A.in_d[i]; });
        }
        kt_count_outcomes(A.ctr, what, lane);
    }
}

struct TamesSortHarvestArgs {
    const u64 *tag;        // [slots]
    const u32x4 *d;        // [slots]
    u64 *out_tag;          // [max]
    u32 *out_idx;          // [max] the entry's number: where its d lies in out_d
    u32x4 *out_d;          // [max]
    u64 *ctr;              // the table's counters: CTR_MET (zeroed by the caller), CTR_OR of the tags (0), CTR_AND of the tags (all ones)
    u64 slots, max;
};

// a kernel of its own, after every insert and load: plain loads are in order here
__global__ void __launch_bounds__(256) kangaroo_tames_sort_harvest_kernel(const TamesSortHarvestArgs A)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    u64 any = 0ull, all = ~0ull;
    for (u64 base = (u64)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < A.slots; base += stride) {      // wave-uniform (slots is a multiple of 64)
        const u64 s = base + lane;
        const u64 t = s < A.slots ? A.tag[s] : 0ull;
        const bool occ = t != 0ull;
        if (occ) { any |= t; all &= t; }
        const u64 pos = kt_reserve(occ, lane, &A.ctr[CTR_MET], 0);
        if (occ && pos < A.max) {                                    // the bound of every store
            A.out_tag[pos] = t;
            A.out_idx[pos] = (u32)pos;
            A.out_d[pos] = A.d[s];
        }
    }
    for (int o = 32; o; o >>= 1) {                                   // the wave's OR and AND, then one atomic each
        any |= (u64)__shfl_xor((unsigned long long)any, o);
        all &= (u64)__shfl_xor((unsigned long long)all, o);
    }
    if (lane == 0 && any) {
        atomicOr((unsigned long long *)&A.ctr[CTR_OR], (unsigned long long)any);
        atomicAnd((unsigned long long *)&A.ctr[CTR_AND], (unsigned long long)all);
    }
}

struct TamesSortArgs {
    const u64 *key;        // [n] the pass reads ...
    const u32 *val;
    u64 *out_key;          // [n] ... and writes
    u32 *out_val;
    u32 *counts;           // [256][nblocks]: digit counts per tile, then their exclusive prefixes along a digit's row
    u32 *tot;              // [256] entries per digit
    u32 n, nblocks, shift;
};

// the inclusive sum over the block's 256 values, and their total; wsum: four words of LDS (two barriers inside)
__device__ __forceinline__ u32 block_scan256(u32 v, u32 *wsum, u32 *total)
{
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    u32 x = v;
    for (u32 o = 1; o < 64u; o <<= 1) {
        const u32 y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63u) wsum[w] = x;
    __syncthreads();
    const u32 s0 = wsum[0], s1 = wsum[1], s2 = wsum[2], s3 = wsum[3];
    __syncthreads();
    *total = s0 + s1 + s2 + s3;
    return x + (w > 0 ? s0 : 0u) + (w > 1 ? s1 : 0u) + (w > 2 ? s2 : 0u);
}

__global__ void __launch_bounds__(256) kangaroo_tames_sort_hist_kernel(const TamesSortArgs A)
{
    __shared__ u32 hist[256];
    hist[threadIdx.x] = 0u;
    __syncthreads();
    const u32 tile0 = blockIdx.x * TAMES_SORT_TILE;                  // (nblocks * TAMES_SORT_TILE < 2^32 + TAMES_SORT_TILE: i is compared as u64)
    for (u32 k = 0; k < TAMES_SORT_TILE / 256u; k++) {
        const u64 i = (u64)tile0 + k * 256u + threadIdx.x;
        if (i < A.n) atomicAdd(&hist[(u32)(A.key[i] >> A.shift) & 255u], 1u);
    }
    __syncthreads();
    A.counts[(u64)threadIdx.x * A.nblocks + blockIdx.x] = hist[threadIdx.x];
}

__global__ void __launch_bounds__(256) kangaroo_tames_sort_scan_kernel(const TamesSortArgs A)
{
    __shared__ u32 wsum[4];
    u32 *const row = A.counts + (u64)blockIdx.x * A.nblocks;
    u32 carry = 0u;
    for (u32 base = 0; base < A.nblocks; base += 256u) {             // block-uniform: every thread reaches the barriers
        const u32 i = base + threadIdx.x;
        const u32 v = i < A.nblocks ? row[i] : 0u;
        u32 total;
        const u32 incl = block_scan256(v, wsum, &total);
        if (i < A.nblocks) row[i] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) A.tot[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(256) kangaroo_tames_sort_scatter_kernel(const TamesSortArgs A)
{
    __shared__ u32 wsum[4];
    __shared__ u32 off[256];
    __shared__ u32 whist[4][256];
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    {
        const u32 t = A.tot[threadIdx.x];
        u32 total;
        const u32 incl = block_scan256(t, wsum, &total);
        off[threadIdx.x] = incl - t + A.counts[(u64)threadIdx.x * A.nblocks + blockIdx.x];
        for (u32 v = 0; v < 4u; v++) whist[v][threadIdx.x] = 0u;
    }
    __syncthreads();
    const u64 sub0 = (u64)blockIdx.x * TAMES_SORT_TILE + w * (TAMES_SORT_ROUNDS * 64u);
    u64 key[TAMES_SORT_ROUNDS];
    u32 val[TAMES_SORT_ROUNDS], pre[TAMES_SORT_ROUNDS];
#pragma unroll
    for (u32 k = 0; k < TAMES_SORT_ROUNDS; k++) {
        const u64 i = sub0 + k * 64u + lane;
        const bool valid = i < A.n;
        key[k] = valid ? A.key[i] : 0ull;
        val[k] = valid ? A.val[i] : 0u;
    }
    // each round: the lanes of one digit take consecutive places behind what the wave's earlier rounds counted for that digit
#pragma unroll
    for (u32 k = 0; k < TAMES_SORT_ROUNDS; k++) {
        const bool valid = sub0 + k * 64u + lane < A.n;
        const u32 dg = (u32)(key[k] >> A.shift) & 255u;
        u64 peers = __ballot(valid);
#pragma unroll
        for (u32 b = 0; b < 8u; b++) {
            const bool bit = (dg >> b) & 1u;
            const u64 m = __ballot(valid && bit);
            peers &= bit ? m : ~m;
        }
        const u32 before = whist[w][dg];
        pre[k] = before + (u32)__builtin_popcountll(peers & ((1ull << lane) - 1));
        __syncthreads();                                             // (uniform: every wave runs every round) all have read before the leaders write
        if (valid && (int)lane == __builtin_ctzll(peers)) whist[w][dg] = before + (u32)__builtin_popcountll(peers);
        __syncthreads();
    }
    {                                                                // counts per wave -> where each wave's share of a digit starts
        u32 run = off[threadIdx.x];
        for (u32 v = 0; v < 4u; v++) { const u32 c = whist[v][threadIdx.x]; whist[v][threadIdx.x] = run; run += c; }
    }
    __syncthreads();
#pragma unroll
    for (u32 k = 0; k < TAMES_SORT_ROUNDS; k++) {
        const bool valid = sub0 + k * 64u + lane < A.n;
        const u32 dg = (u32)(key[k] >> A.shift) & 255u;
        const u32 pos = whist[w][dg] + pre[k];
        if (valid && pos < A.n) {                                    // the bound of every store
            A.out_key[pos] = key[k];
            A.out_val[pos] = val[k];
        }
    }
}

struct TamesSortGatherArgs {
    const u32 *idx;        // [m] the numbers of the m lowest tags, ascending by tag
    const u32x4 *d;        // [n] as harvested
    u32x4 *out_d;          // [m]
    u32 m, n;
};

__global__ void __launch_bounds__(256) kangaroo_tames_sort_gather_kernel(const TamesSortGatherArgs A)
{
    const u32 stride = gridDim.x * blockDim.x;
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < A.m; j += stride) {
        const u32 i = A.idx[j];
        if (i < A.n) A.out_d[j] = A.d[i];
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------------
static void free_all(std::initializer_list<void *> ps) { for (void *p : ps) if (p) (void)hipFree(p); }

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int bsgs_kangaroo_tames_gen_load(bsgs_dev *d, const uint64_t *x_lo64, const uint8_t *d_le, uint64_t n, uint64_t *n_stored, uint64_t *n_duplicate, uint64_t *n_zero,
                                            uint64_t *n_full, uint64_t *n_entries)
{
    bsgs_kangaroo *k = nullptr;
    if (int rc = bsgs_kangaroo_tames_gen_herd(d, &k, true)) return rc;
    if (n && (!x_lo64 || !d_le)) return fail(BSGS_ERR_ARG, "null");
    if (n > KT_MAX_CAPACITY) return fail(BSGS_ERR_ARG, "loading %llu entries: at most 2^31", (unsigned long long)n);
    HIPCHK(hipSetDevice(d->id));
    const uint64_t chunk = std::min<uint64_t>(std::max<uint64_t>(n, 1), TAMES_LOAD_CHUNK);
    TamesLoadArgs A;
    A.in_tag = nullptr; A.in_d = nullptr; A.tag = k->gen.tag; A.d = k->gen.d; A.ctr = k->gen.ctr; A.slot_mask = k->gen.slots - 1; A.n = 0;
    hipError_t e = hipMalloc((void **)&A.in_tag, (size_t)chunk * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&A.in_d, (size_t)chunk * 16);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        free_all({(void *)A.in_tag});
        return fail(BSGS_ERR_NOMEM, "loading into a growing tame table: a chunk of %llu entries needs %llu bytes of tags and %llu of offsets (%s)", (unsigned long long)chunk,
                    (unsigned long long)(chunk * 8), (unsigned long long)(chunk * 16), hipGetErrorString(e));
    }
    e = hipMemsetAsync(k->gen.ctr + CTR_STORED, 0, 4 * 8, d->stream);
    for (uint64_t pos = 0; pos < n && e == hipSuccess; pos += chunk) {
        const uint32_t m = (uint32_t)std::min(chunk, n - pos);
        e = hipMemcpyAsync((void *)A.in_tag, x_lo64 + pos, (size_t)m * 8, hipMemcpyHostToDevice, d->stream);
        if (e == hipSuccess) e = hipMemcpyAsync((void *)A.in_d, d_le + 16 * pos, (size_t)m * 16, hipMemcpyHostToDevice, d->stream);
        if (e != hipSuccess) break;
        A.n = m;
        const u32 blocks = std::min((m + 255u) / 256u, KT_SCAN_GRID_MAX);
        hipLaunchKernelGGL(kangaroo_tames_load_kernel, dim3(blocks), dim3(256), 0, d->stream, A);
        e = hipGetLastError();
    }
    const int rc = bsgs_kang_table_loaded(d, &k->gen, e, n, n_stored, n_duplicate, n_zero, n_full, n_entries,
                                          "loading into a growing tame table: %llu pairs, %llu accounted for");
    free_all({(void *)A.in_tag, (void *)A.in_d});
    return rc;
}

extern "C" int bsgs_kangaroo_tames_gen_read_sorted(bsgs_dev *d, uint64_t *x_lo64, uint8_t *d_le, uint64_t max, uint64_t *n)
{
    if (!n) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = nullptr;
    if (int rc = bsgs_kangaroo_tames_gen_herd(d, &k, true)) return rc;
    HIPCHK(hipSetDevice(d->id));
    uint64_t entries = 0;
    if (int rc = bsgs_kang_table_entries(d, &k->gen, &entries)) return rc;
    *n = entries;
    const uint64_t m = std::min(entries, max);
    if (!m) return BSGS_OK;
    if (!x_lo64 || !d_le) return fail(BSGS_ERR_ARG, "null");
    if (entries >= (1ull << 32)) return fail(BSGS_ERR_STATE, "growing tame table: %llu entries cannot be numbered in 32 bits", (unsigned long long)entries);
    const u32 nblocks = (u32)((entries + TAMES_SORT_TILE - 1) / TAMES_SORT_TILE);
    u64 *key[2] = {nullptr, nullptr};
    u32 *val[2] = {nullptr, nullptr}, *counts = nullptr, *tot = nullptr;
    u32x4 *dh = nullptr, *ds = nullptr;
    const size_t b_key = (size_t)entries * 8, b_val = (size_t)entries * 4, b_d = (size_t)entries * 16, b_ds = (size_t)m * 16, b_counts = (size_t)nblocks * 256 * 4;
    hipError_t e = hipMalloc(&key[0], b_key);
    if (e == hipSuccess) e = hipMalloc(&key[1], b_key);
    if (e == hipSuccess) e = hipMalloc(&val[0], b_val);
    if (e == hipSuccess) e = hipMalloc(&val[1], b_val);
    if (e == hipSuccess) e = hipMalloc(&dh, b_d);
    if (e == hipSuccess) e = hipMalloc(&ds, b_ds);
    if (e == hipSuccess) e = hipMalloc(&counts, b_counts);
    if (e == hipSuccess) e = hipMalloc(&tot, 256 * 4);
    auto release = [&]() { free_all({key[0], key[1], val[0], val[1], dh, ds, counts, tot}); };
    if (e != hipSuccess) {
        (void)hipGetLastError();
        release();
        return fail(BSGS_ERR_NOMEM, "sorting a growing tame table of %llu entries: 2 x %llu bytes of tags, 2 x %llu of numbers, %llu + %llu of offsets and %llu of counts (%s)",
                    (unsigned long long)entries, (unsigned long long)b_key, (unsigned long long)b_val, (unsigned long long)b_d, (unsigned long long)b_ds,
                    (unsigned long long)(b_counts + 1024), hipGetErrorString(e));
    }
    uint64_t got[3] = {0, 0, 0};                                     // occupied slots met, OR, AND
    e = hipMemsetAsync(k->gen.ctr + CTR_MET, 0, 8, d->stream);
    if (e == hipSuccess) e = hipMemsetAsync(k->gen.ctr + CTR_OR, 0, 8, d->stream);
    if (e == hipSuccess) e = hipMemsetAsync(k->gen.ctr + CTR_AND, 0xFF, 8, d->stream);
    if (e == hipSuccess) {
        TamesSortHarvestArgs H;
        H.tag = k->gen.tag; H.d = k->gen.d; H.out_tag = key[0]; H.out_idx = val[0]; H.out_d = dh; H.ctr = k->gen.ctr; H.slots = k->gen.slots; H.max = entries;
        const u32 blocks = (u32)std::min<uint64_t>((k->gen.slots + 255u) / 256u, KT_SCAN_GRID_MAX);
        hipLaunchKernelGGL(kangaroo_tames_sort_harvest_kernel, dim3(blocks), dim3(256), 0, d->stream, H);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&got[0], k->gen.ctr + CTR_MET, 8, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&got[1], k->gen.ctr + CTR_OR, 16, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    if (e == hipSuccess && got[0] != entries) {
        release();
        return bsgs_kang_table_met_check(got[0], entries, "growing tame table");
    }
    int cur = 0;
    const uint64_t differ = got[1] ^ got[2];                         // the bits on which not all tags agree
    for (u32 shift = 0; shift < 64u && e == hipSuccess; shift += 8u) {
        if (!((differ >> shift) & 255ull)) continue;                 // every tag has the same digit here: the pass would move nothing
        TamesSortArgs S;
        S.key = key[cur]; S.val = val[cur]; S.out_key = key[cur ^ 1]; S.out_val = val[cur ^ 1]; S.counts = counts; S.tot = tot;
        S.n = (u32)entries; S.nblocks = nblocks; S.shift = shift;
        hipLaunchKernelGGL(kangaroo_tames_sort_hist_kernel, dim3(nblocks), dim3(256), 0, d->stream, S);
        hipLaunchKernelGGL(kangaroo_tames_sort_scan_kernel, dim3(256), dim3(256), 0, d->stream, S);
        hipLaunchKernelGGL(kangaroo_tames_sort_scatter_kernel, dim3(nblocks), dim3(256), 0, d->stream, S);
        e = hipGetLastError();
        cur ^= 1;
    }
    if (e == hipSuccess) {
        TamesSortGatherArgs G;
        G.idx = val[cur]; G.d = dh; G.out_d = ds; G.m = (u32)m; G.n = (u32)entries;
        const u32 blocks = (u32)std::min<uint64_t>((m + 255u) / 256u, KT_SCAN_GRID_MAX);
        hipLaunchKernelGGL(kangaroo_tames_sort_gather_kernel, dim3(blocks), dim3(256), 0, d->stream, G);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(x_lo64, key[cur], (size_t)m * 8, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_le, ds, b_ds, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    release();
    HIPCHK(e);
    return BSGS_OK;
}
