// kangaroo.hip -- Pollard's kangaroo (lambda) walk on gfx950: the search mode for ranges too wide for a baby table (include/bsgs_hip.h, "Kangaroo").
//
// One launch runs `steps` steps of every kangaroo of the herd.  A step is one affine addition (x, y) += J_j with j = x & 63 and d += s_j; its inversion is
// shared through one Montgomery batch per thread over the thread's G kangaroos, and with four-wave blocks one Fermat inversion per block (fe_inv_block, as the
// tile kernel).  The herd lives in device memory between launches in the engine's usual SoA of 16-byte vectors, [field][kangaroo] with field = x.lo, x.hi,
// y.lo, y.hi, d and kangaroo i = g * T + thread (a wave's access is one contiguous 1 KiB per instruction); the running products of a batch go to a scratch
// [g][2][T] between the two passes.  The 64 jump points sit in LDS.  Byte and VALU budget: DESIGN.md 10.
#include "bsgs_internal.h"

#define KANG_NJ 64u
#define KANG_TABLE_OFF (4u * KANG_REGION)                   // the jump table behind the inversion regions: x[64] | y[64] | s[64] (4608 bytes)
#define KANG_TABLE_BYTES (KANG_NJ * 32u * 2u + KANG_NJ * 8u)
#define KANG_LDS (KANG_TABLE_OFF + KANG_TABLE_BYTES)

struct KangArgs {
    u32x4 *st;             // [5][N]: x.lo, x.hi, y.lo, y.hi, d (128-bit, two's complement)
    u32 *flags;            // [N]: BSGS_KANGAROO_WILD | BSGS_KANGAROO_DEAD
    u32x4 *chain;          // [G][2][T]: running products of the batch
    const u32x4 *table;    // device copy of the jump table, KANG_TABLE_BYTES
    u32 *rec;              // record buffer (KANG_REC_HEADER + 64 * cap bytes)
    u32 N, T, G, steps, dp_mask, cap;
};

__device__ __forceinline__ void lds_fe(fe &r, const char *q)
{
    const u32x4 lo = *(const u32x4 *)q, hi = *(const u32x4 *)(q + 16);
    r.v[0] = lo.x; r.v[1] = lo.y; r.v[2] = lo.z; r.v[3] = lo.w; r.v[4] = hi.x; r.v[5] = hi.y; r.v[6] = hi.z; r.v[7] = hi.w;
}

// one record per lane with `hit`: vector stores, one atomic per wave (as report() in giant_kernel.hip.h); slots past the capacity are counted, not written.
// key: the per-kangaroo key array of a bsgs_kangaroo_setup_sym_keys herd, read here and nowhere else in the walk -- only by a lane that writes a record --
// into the record's fourth word; nullptr (a constant at every other call site): the word is 0
template <class ARGS>
__device__ __forceinline__ void kang_record(const ARGS &A, bool hit, const fe &x, const u32x4 &d, u32 idx, u32 flags, u32 step, u32 lane, const u32 *key = nullptr)
{
    const u64 m = __ballot(hit);
    if (m) {
        u64 base = 0;
        const int leader = __builtin_ctzll(m);
        if ((int)lane == leader) base = atomicAdd((unsigned long long *)A.rec, (unsigned long long)__builtin_popcountll(m));
        base = __shfl(base, leader);
        const u64 slot = base + (u64)__builtin_popcountll(m & ((1ull << lane) - 1));
        if (hit && slot < A.cap) {
            u32x4 *r = (u32x4 *)((char *)A.rec + KANG_REC_HEADER) + slot * 4;
            r[0] = (u32x4){x.v[0], x.v[1], x.v[2], x.v[3]};
            r[1] = (u32x4){x.v[4], x.v[5], x.v[6], x.v[7]};
            r[2] = d;
            r[3] = (u32x4){idx, flags, step, key ? key[idx] : 0u};
        }
    }
}

// the batch element of one kangaroo: J_j.x - x; 2y for a doubling (x == J_j.x, y == J_j.y); 1 for a dead kangaroo and for x == J_j.x, y == -J_j.y (the sum is
// infinity): never zero, so one degenerate kangaroo cannot spoil its batch.  kind: 0 add, 1 double, 2 dies now, 3 dead already
__device__ __forceinline__ u32 kang_element(fe &e, const fe &x, const fe &jx, const fe &jy, const u32x4 *ylo, const u32x4 *yhi, u32 fl)
{
    if (__builtin_expect((fl & BSGS_KANGAROO_DEAD) != 0u, 0)) { fe_set_one(e); return 3u; }
    fe_sub(e, jx, x);
    if (__builtin_expect(!fe_is_zero(e), 1)) return 0u;
    fe y;
    fe_load2(y, ylo, yhi);
    if (fe_eq(y, jy)) { fe_add(e, y, y); return 1u; }
    fe_set_one(e);
    return 2u;
}

template <bool BLOCK_INV>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) kangaroo_kernel(const KangArgs A)
{
    char *tab = bsgs_smem + KANG_TABLE_OFF;
    for (u32 k = threadIdx.x; k < KANG_TABLE_BYTES / 16u; k += blockDim.x) ((u32x4 *)tab)[k] = A.table[k];
    __syncthreads();
    const u32 T = A.T, N = A.N, G = A.G;
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;             // the launch has exactly T threads
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    u32x4 *const sx0 = A.st, *const sx1 = A.st + N, *const sy0 = A.st + 2 * (u64)N, *const sy1 = A.st + 3 * (u64)N, *const sd = A.st + 4 * (u64)N;
    for (u32 step = 0; step < A.steps; step++) {
        // pass 1: running products of the elements
        fe acc;
        fe_set_one(acc);
        for (u32 g = 0; g < G; g++) {
            const u32 i = g * T + t;
            fe x, jx, jy, e;
            fe_load2(x, sx0 + i, sx1 + i);
            const u32 j = x.v[0] & (KANG_NJ - 1u);
            lds_fe(jx, tab + j * 32u); lds_fe(jy, tab + KANG_NJ * 32u + j * 32u);
            kang_element(e, x, jx, jy, sy0 + i, sy1 + i, A.flags[i]);
            fe_mul(acc, acc, e);
            CHAIN_STORE(A.chain + ((u64)g * 2 + 0) * T + t, A.chain + ((u64)g * 2 + 1) * T + t, acc);
        }
        fe inv;
        if (BLOCK_INV) fe_inv_block<KANG_REGION, 4>(inv, acc, lane, wave, blockIdx.x & 3u);
        else fe_inv(inv, acc);
        // pass 2, backwards: 1 / e_g from the running products, then the addition
        for (u32 gg = 0; gg < G; gg++) {
            const u32 g = G - 1 - gg;
            const u32 i = g * T + t;
            fe x, y, jx, jy, e, s;
            fe_load2(x, sx0 + i, sx1 + i);
            u32 fl = A.flags[i];
            const u32 j = x.v[0] & (KANG_NJ - 1u);
            lds_fe(jx, tab + j * 32u); lds_fe(jy, tab + KANG_NJ * 32u + j * 32u);
            const u32 kind = kang_element(e, x, jx, jy, sy0 + i, sy1 + i, fl);
            if (g > 0) {
                fe c;
                CHAIN_LOAD(c, A.chain + ((u64)(g - 1) * 2 + 0) * T + t, A.chain + ((u64)(g - 1) * 2 + 1) * T + t);
                fe_mul(s, inv, c);
                fe_mul(inv, inv, e);
            } else {
                s = inv;
            }
            u32x4 d = sd[i];
            bool rec = false;
            if (__builtin_expect(kind < 2u, 1)) {
                fe_load2(y, sy0 + i, sy1 + i);
                fe lam, t1, nx, x3, y3;
                fe_neg(nx, x);
                if (__builtin_expect(kind == 0u, 1)) {
                    fe_sub(t1, jy, y);                                   // (J.y - y) / (J.x - x)
                    fe_mul(lam, t1, s);
                    fe njx;
                    fe_neg(njx, jx);
                    fe_sqr_add2(x3, lam, nx, njx);
                } else {
                    fe_sqr(t1, x);                                       // 3 x^2 / 2y
                    fe_add(e, t1, t1);
                    fe_add(t1, e, t1);
                    fe_mul(lam, t1, s);
                    fe_sqr_add2(x3, lam, nx, nx);
                }
                fe_canon(x3);
                fe_sub(t1, x, x3);
                fe_mul(y3, lam, t1);
                fe_sub(y3, y3, y);
                fe_canon(y3);
                const u64 sj = *(const u64 *)(tab + KANG_NJ * 64u + j * 8u);
                u32 c = 0, co;
                d.x = __builtin_addc(d.x, (u32)sj, c, &co); c = co;
                d.y = __builtin_addc(d.y, (u32)(sj >> 32), c, &co); c = co;
                d.z = __builtin_addc(d.z, 0u, c, &co); c = co;
                d.w = __builtin_addc(d.w, 0u, c, &co);
                fe_store2(sx0 + i, sx1 + i, x3);
                fe_store2(sy0 + i, sy1 + i, y3);
                sd[i] = d;
                x = x3;
                rec = (x3.v[7] & A.dp_mask) == 0u;
            } else if (kind == 2u) {                                     // x + J_j is infinity: one record of the point it stood on, then it rests
                fl |= BSGS_KANGAROO_DEAD;
                A.flags[i] = fl;
                rec = true;
            }
            kang_record(A, rec, x, d, i, fl, step, lane);
        }
    }
}

// ---- the symmetric walk (include/bsgs_hip.h, "Kangaroo, symmetric walk"): classes {P, -P}, never the same jump twice running, cycles retired by a mark ----
// The R jump points do not fit LDS next to the inversion regions (72 KiB at R = 1024): the table stays in device memory as {x, y}[R] | s[R] and is read
// through the caches.  The step is the plain one plus: the index rule on the flags' last index, y and d negated when the new y is odd, the flags written back
// every step, and in the last KANG_CYCLE_WINDOW steps of a launch one 32-byte compare against the x the kangaroo had before them.
#define KANG_LAST_VALID 0x100u
#define KANG_LAST_SHIFT 9u
#define KANG_LAST_MASK (0x1FFFu << 8)                       // valid bit and the 12 index bits

struct KangSymArgs {
    u32x4 *st;             // as KangArgs
    u32 *flags;            // [N]: BSGS_KANGAROO_WILD | NEG | CYCLE | DEAD, last jump index (bit 8 valid, bits 9..20); kangaroo_sym_keys_kernel: then key[N]
    u32x4 *chain;
    const u32x4 *table;    // {x, y}[R] (64 bytes each), then s[R]
    u32 *rec;
    u32x4 *mark;           // [2][N]: x after step mark_step of this launch
    u32 N, T, G, steps, dp_mask, cap, rmask;
    u32 mark_step;         // steps - 1 - KANG_CYCLE_WINDOW, or ~0u when the launch is too short for a check
};

__device__ __forceinline__ u32 kang_sym_index(u32 x0, u32 fl, u32 rmask)
{
    const u32 j = x0 & rmask;
    return ((fl & KANG_LAST_VALID) && ((fl >> KANG_LAST_SHIFT) & 0xFFFu) == j) ? (j + 1u) & rmask : j;
}

// (y, d, flags) -> the class representative's when y is odd
__device__ __forceinline__ void kang_sym_normalise(fe &y, u32x4 &d, u32 &fl)
{
    if (y.v[0] & 1u) {
        fe_neg(y, y);
        u32 c = 0, co;
        d.x = __builtin_subc(0u, d.x, c, &co); c = co;
        d.y = __builtin_subc(0u, d.y, c, &co); c = co;
        d.z = __builtin_subc(0u, d.z, c, &co); c = co;
        d.w = __builtin_subc(0u, d.w, c, &co);
        if (fl & BSGS_KANGAROO_WILD) fl ^= BSGS_KANGAROO_NEG;
    }
}
// kang_element on the representative: the equal-x cases compare the even one of y and p - y with J_j.y
__device__ __forceinline__ u32 kang_sym_element(fe &e, const fe &x, const fe &jx, const fe &jy, const u32x4 *ylo, const u32x4 *yhi, u32 fl)
{
    if (__builtin_expect((fl & BSGS_KANGAROO_DEAD) != 0u, 0)) { fe_set_one(e); return 3u; }
    fe_sub(e, jx, x);
    if (__builtin_expect(!fe_is_zero(e), 1)) return 0u;
    fe y;
    fe_load2(y, ylo, yhi);
    if (y.v[0] & 1u) fe_neg(y, y);
    if (fe_eq(y, jy)) { fe_add(e, y, y); return 1u; }
    fe_set_one(e);
    return 2u;
}

// the symmetric step, shared by the two entry points below.  KEYS: the herd of bsgs_kangaroo_setup_sym_keys, whose key array lies behind the flags
// (flags[N + i]: no pointer of its own, the walk has no scalar register to spare for one); see kang_record
template <bool BLOCK_INV, bool KEYS>
__device__ __forceinline__ void kang_sym_walk(const KangSymArgs &A)
{
    const u32 T = A.T, N = A.N, G = A.G, rmask = A.rmask;
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;             // the launch has exactly T threads
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    u32x4 *const sx0 = A.st, *const sx1 = A.st + N, *const sy0 = A.st + 2 * (u64)N, *const sy1 = A.st + 3 * (u64)N, *const sd = A.st + 4 * (u64)N;
    const u64 *const ts = (const u64 *)(A.table + 4 * ((u64)rmask + 1));
    for (u32 step = 0; step < A.steps; step++) {
        fe acc;
        fe_set_one(acc);
        for (u32 g = 0; g < G; g++) {
            const u32 i = g * T + t;
            fe x, jx, jy, e;
            fe_load2(x, sx0 + i, sx1 + i);
            const u32 fl = A.flags[i];
            const u32x4 *jp = A.table + 4 * (u64)kang_sym_index(x.v[0], fl, rmask);
            fe_load2(jx, jp, jp + 1); fe_load2(jy, jp + 2, jp + 3);
            kang_sym_element(e, x, jx, jy, sy0 + i, sy1 + i, fl);
            fe_mul(acc, acc, e);
            CHAIN_STORE(A.chain + ((u64)g * 2 + 0) * T + t, A.chain + ((u64)g * 2 + 1) * T + t, acc);
        }
        fe inv;
        if (BLOCK_INV) fe_inv_block<KANG_REGION, 4>(inv, acc, lane, wave, blockIdx.x & 3u);
        else fe_inv(inv, acc);
        for (u32 gg = 0; gg < G; gg++) {
            const u32 g = G - 1 - gg;
            const u32 i = g * T + t;
            fe x, y, jx, jy, e, s;
            fe_load2(x, sx0 + i, sx1 + i);
            u32 fl = A.flags[i];
            const u32 j = kang_sym_index(x.v[0], fl, rmask);
            const u32x4 *jp = A.table + 4 * (u64)j;
            fe_load2(jx, jp, jp + 1); fe_load2(jy, jp + 2, jp + 3);
            const u32 kind = kang_sym_element(e, x, jx, jy, sy0 + i, sy1 + i, fl);
            if (g > 0) {
                fe c;
                CHAIN_LOAD(c, A.chain + ((u64)(g - 1) * 2 + 0) * T + t, A.chain + ((u64)(g - 1) * 2 + 1) * T + t);
                fe_mul(s, inv, c);
                fe_mul(inv, inv, e);
            } else {
                s = inv;
            }
            u32x4 d = sd[i];
            bool rec = false;
            if (__builtin_expect(kind < 2u, 1)) {
                fe_load2(y, sy0 + i, sy1 + i);
                kang_sym_normalise(y, d, fl);                            // (a start of odd y; after a step y is even)
                fe lam, t1, nx, x3, y3;
                fe_neg(nx, x);
                if (__builtin_expect(kind == 0u, 1)) {
                    fe_sub(t1, jy, y);
                    fe_mul(lam, t1, s);
                    fe njx;
                    fe_neg(njx, jx);
                    fe_sqr_add2(x3, lam, nx, njx);
                } else {
                    fe_sqr(t1, x);
                    fe_add(e, t1, t1);
                    fe_add(t1, e, t1);
                    fe_mul(lam, t1, s);
                    fe_sqr_add2(x3, lam, nx, nx);
                }
                fe_canon(x3);
                fe_sub(t1, x, x3);
                fe_mul(y3, lam, t1);
                fe_sub(y3, y3, y);
                fe_canon(y3);
                const u64 sj = ts[j];
                u32 c = 0, co;
                d.x = __builtin_addc(d.x, (u32)sj, c, &co); c = co;
                d.y = __builtin_addc(d.y, (u32)(sj >> 32), c, &co); c = co;
                d.z = __builtin_addc(d.z, 0u, c, &co); c = co;
                d.w = __builtin_addc(d.w, 0u, c, &co);
                kang_sym_normalise(y3, d, fl);
                fl = (fl & ~KANG_LAST_MASK) | KANG_LAST_VALID | (j << KANG_LAST_SHIFT);
                fe_store2(sx0 + i, sx1 + i, x3);
                fe_store2(sy0 + i, sy1 + i, y3);
                sd[i] = d;
                x = x3;
                rec = (x3.v[7] & A.dp_mask) == 0u;
                if (step == A.mark_step) {
                    fe_store2(A.mark + i, A.mark + N + i, x3);
                } else if (step > A.mark_step) {                         // (never with mark_step = ~0u) back on the marked x: a cycle of at most the window
                    fe m;
                    fe_load2(m, A.mark + i, A.mark + N + i);
                    if (__builtin_expect(fe_eq(m, x3), 0)) { fl |= BSGS_KANGAROO_DEAD | BSGS_KANGAROO_CYCLE; rec = true; }
                }
                A.flags[i] = fl;
            } else if (kind == 2u) {
                fl |= BSGS_KANGAROO_DEAD;
                A.flags[i] = fl;
                rec = true;
            }
            kang_record(A, rec, x, d, i, fl, step, lane, KEYS ? A.flags + N : nullptr);
        }
    }
}

template <bool BLOCK_INV>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) kangaroo_sym_kernel(const KangSymArgs A)
{
    kang_sym_walk<BLOCK_INV, false>(A);
}

// the herd of bsgs_kangaroo_setup_sym_keys (include/bsgs_hip.h, "Kangaroo, many keys, symmetric walk"): the same step; a record names its kangaroo's key
template <bool BLOCK_INV>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) kangaroo_sym_keys_kernel(const KangSymArgs A)      // flags: [2][N], flags | key
{
    kang_sym_walk<BLOCK_INV, true>(A);
}

// ---- gather / scatter of whole states (host format bsgs_kangaroo_state, 96 bytes) -------------------------------------------------------------------
// key: the key array of a bsgs_kangaroo_setup_sym_keys herd (state word reserved[0]), or nullptr: the word is ignored on upload and 0 on download
__global__ void kangaroo_scatter_kernel(u32x4 *st, u32 *flags, u32 *key, u32 N, const u32x4 *in, const u32 *idx, u32 first, u32 n)
{
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const u32 i = idx ? idx[k] : first + k;
    if (i >= N) return;
    const u32x4 *s = in + (u64)k * 6;
    for (u32 f = 0; f < 5; f++) st[(u64)f * N + i] = s[f];
    flags[i] = s[5].x;
    if (key) key[i] = s[5].y;
}
__global__ void kangaroo_gather_kernel(const u32x4 *st, const u32 *flags, const u32 *key, u32 N, u32x4 *out, u32 first, u32 n)
{
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const u32 i = first + k;
    u32x4 *o = out + (u64)k * 6;
    for (u32 f = 0; f < 5; f++) o[f] = st[(u64)f * N + i];
    o[5] = (u32x4){flags[i], key ? key[i] : 0u, 0u, 0u};
}
// after kangaroo_seed_keys_kernel on a bsgs_kangaroo_setup_sym_keys herd: the seeded kangaroos' key leaves the flags, where the walk keeps its last jump index
__global__ void kangaroo_split_keys_kernel(u32 *flags, u32 *key, u32 N, const u32 *idx, u32 first, u32 n)
{
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const u32 i = idx ? idx[k] : first + k;
    if (i >= N) return;
    const u32 fl = flags[i];
    key[i] = (fl >> BSGS_KANGAROO_KEY_SHIFT) & 0xFFFFu;
    flags[i] = fl & (BSGS_KANGAROO_WILD | BSGS_KANGAROO_DEAD);
}
int bsgs_kangaroo_split_keys(bsgs_dev *d, const u32 *idx_dev, uint32_t first, uint32_t n)
{
    bsgs_kangaroo *k = d->kangaroo;
    hipLaunchKernelGGL(kangaroo_split_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, d->stream, k->flags, k->key, k->N, idx_dev, first, n);
    HIPCHK(hipGetLastError());
    return BSGS_OK;
}

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------------------------------
void bsgs_kangaroo_release(bsgs_dev *d)
{
    bsgs_kangaroo *k = d->kangaroo;
    if (!k) return;
    for (void *p : {(void *)k->st, (void *)k->chain, (void *)k->table, (void *)k->staging, (void *)k->flags, (void *)k->rec, (void *)k->idx, (void *)k->comb,
                    (void *)k->seed_in, (void *)k->seed_z, (void *)k->seed_out, (void *)k->mark, (void *)k->keys, (void *)k->verify_q, (void *)k->verify_out, (void *)k->tames,
                    (void *)k->tames_rec, (void *)k->dpt_out, (void *)k->dpt_route})
        if (p) (void)hipFree(p);
    bsgs_kang_table_free(&k->gen);
    bsgs_kang_table_free(&k->dpt);
    if (k->rec_host) (void)hipHostFree(k->rec_host);
    delete k;
    d->kangaroo = nullptr;
}

static_assert(sizeof(bsgs_kangaroo_state) == 96, "state record: 96 bytes");
static_assert(sizeof(bsgs_kangaroo_record) == 64, "DP record: 64 bytes");

// the herd of both walks; plain (sym false, n_jumps = 0): the walk's 64 points in its LDS layout x[64] | y[64] | s[64]; sym: the symmetric walk's
// {x, y}[R] | s[R], keyed: with the key array of bsgs_kangaroo_setup_sym_keys
static int kangaroo_alloc(bsgs_dev *d, const uint8_t *jumps_xy_le, const uint64_t *jump_scalars, uint32_t n_jumps, uint32_t dp, uint32_t herd, uint32_t per_thread,
                          uint32_t record_cap, bool sym, bool keyed)
{
    if (sym && (n_jumps < 64u || n_jumps > BSGS_KANGAROO_SYM_MAX_JUMPS || (n_jumps & (n_jumps - 1u))))
        return fail(BSGS_ERR_ARG, "%u jump points: a power of two, 64..%u", n_jumps, BSGS_KANGAROO_SYM_MAX_JUMPS);
    const uint32_t R = n_jumps ? n_jumps : KANG_NJ;
    if (!d || !jumps_xy_le || !jump_scalars) return fail(BSGS_ERR_ARG, "null");
    if (dp > 32) return fail(BSGS_ERR_ARG, "dp %u: at most 32", dp);
    if (!per_thread || !herd || herd % (64u * per_thread)) return fail(BSGS_ERR_ARG, "herd %u: a multiple of 64 * per_thread (%u)", herd, per_thread);
    if (!record_cap || record_cap > (1u << 26)) return fail(BSGS_ERR_ARG, "record capacity %u: 1..2^26", record_cap);
    for (int j = 0; j < (int)R; j++) if (!jump_scalars[j]) return fail(BSGS_ERR_ARG, "jump scalar %d is zero", j);
    HIPCHK(hipSetDevice(d->id));
    HIPCHK(hipStreamSynchronize(d->stream));
    bsgs_kangaroo_release(d);
    bsgs_kangaroo *k = new bsgs_kangaroo();
    d->kangaroo = k;
    k->N = herd; k->G = per_thread; k->T = herd / per_thread; k->dp = dp; k->cap = record_cap; k->R = n_jumps;
    k->block = k->T % 256u == 0 ? 256u : 64u;
    HIPCHK(hipMalloc(&k->st, (size_t)herd * 5 * 16));
    HIPCHK(hipMalloc(&k->flags, (size_t)herd * (keyed ? 8 : 4)));
    if (keyed) k->key = k->flags + herd;                                         // (the walk finds the keys behind the flags)
    HIPCHK(hipMalloc(&k->chain, (size_t)herd * 32));
    HIPCHK(hipMalloc(&k->table, (size_t)R * 72));
    if (n_jumps) HIPCHK(hipMalloc(&k->mark, (size_t)herd * 32));
    HIPCHK(hipMalloc(&k->rec, KANG_REC_HEADER + (size_t)record_cap * 64));
    HIPCHK(hipHostMalloc(&k->rec_host, (size_t)record_cap * 64, hipHostMallocDefault));
    HIPCHK(hipMemsetAsync(k->st, 0, (size_t)herd * 5 * 16, d->stream));
    HIPCHK(hipMemsetAsync(k->flags, 0xFF, (size_t)herd * 4, d->stream));         // every kangaroo dead until its state is uploaded
    if (n_jumps) HIPCHK(hipMemsetAsync(k->mark, 0, (size_t)herd * 32, d->stream));
    if (keyed) HIPCHK(hipMemsetAsync(k->key, 0, (size_t)herd * 4, d->stream));
    std::vector<uint8_t> tab((size_t)R * 72);
    for (uint32_t j = 0; j < R; j++) {
        if (n_jumps) memcpy(&tab[j * 64], jumps_xy_le + j * 64, 64);
        else {
            memcpy(&tab[j * 32], jumps_xy_le + j * 64, 32);
            memcpy(&tab[R * 32 + j * 32], jumps_xy_le + j * 64 + 32, 32);
        }
        memcpy(&tab[R * 64 + j * 8], &jump_scalars[j], 8);
    }
    HIPCHK(hipMemcpyAsync(k->table, tab.data(), tab.size(), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return BSGS_OK;
}
extern "C" int bsgs_kangaroo_setup(bsgs_dev *d, const uint8_t *jumps_xy_le, const uint64_t *jump_scalars, uint32_t dp, uint32_t herd, uint32_t per_thread,
                                   uint32_t record_cap)
{
    return kangaroo_alloc(d, jumps_xy_le, jump_scalars, 0, dp, herd, per_thread, record_cap, false, false);
}
extern "C" int bsgs_kangaroo_setup_sym(bsgs_dev *d, const uint8_t *jumps_xy_le, const uint64_t *jump_scalars, uint32_t n_jumps, uint32_t dp, uint32_t herd,
                                       uint32_t per_thread, uint32_t record_cap)
{
    return kangaroo_alloc(d, jumps_xy_le, jump_scalars, n_jumps, dp, herd, per_thread, record_cap, true, false);
}
extern "C" int bsgs_kangaroo_setup_sym_keys(bsgs_dev *d, const uint8_t *jumps_xy_le, const uint64_t *jump_scalars, uint32_t n_jumps, uint32_t dp, uint32_t herd,
                                            uint32_t per_thread, uint32_t record_cap)
{
    return kangaroo_alloc(d, jumps_xy_le, jump_scalars, n_jumps, dp, herd, per_thread, record_cap, true, true);
}

static int kangaroo_put(bsgs_dev *d, const uint32_t *idx, uint32_t first, uint32_t n, const bsgs_kangaroo_state *states)
{
    if (!d || !states) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = d->kangaroo;
    if (!k) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_setup first");
    if (!n) return BSGS_OK;
    if (idx) { for (uint32_t q = 0; q < n; q++) if (idx[q] >= k->N) return fail(BSGS_ERR_ARG, "kangaroo %u of %u", idx[q], k->N); }
    else if ((uint64_t)first + n > k->N) return fail(BSGS_ERR_ARG, "kangaroos [%u, %u) of %u", first, first + n, k->N);
    HIPCHK(hipSetDevice(d->id));
    if (k->staging_n < n) {
        if (k->staging) (void)hipFree(k->staging);
        if (k->idx) (void)hipFree(k->idx);
        k->staging = nullptr; k->idx = nullptr; k->staging_n = 0;
        HIPCHK(hipMalloc(&k->staging, (size_t)n * 96));
        HIPCHK(hipMalloc(&k->idx, (size_t)n * 4));
        k->staging_n = n;
    }
    HIPCHK(hipMemcpyAsync(k->staging, states, (size_t)n * 96, hipMemcpyHostToDevice, d->stream));
    if (idx) HIPCHK(hipMemcpyAsync(k->idx, idx, (size_t)n * 4, hipMemcpyHostToDevice, d->stream));
    hipLaunchKernelGGL(kangaroo_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, d->stream, k->st, k->flags, k->key, k->N, k->staging, idx ? k->idx : nullptr, first, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(d->stream));
    return BSGS_OK;
}
extern "C" int bsgs_kangaroo_upload(bsgs_dev *d, uint32_t first, uint32_t n, const bsgs_kangaroo_state *states)
{
    return kangaroo_put(d, nullptr, first, n, states);
}
extern "C" int bsgs_kangaroo_upload_list(bsgs_dev *d, const uint32_t *idx, uint32_t n, const bsgs_kangaroo_state *states)
{
    if (!idx) return fail(BSGS_ERR_ARG, "null");
    return kangaroo_put(d, idx, 0, n, states);
}

extern "C" int bsgs_kangaroo_download(bsgs_dev *d, uint32_t first, uint32_t n, bsgs_kangaroo_state *states)
{
    if (!d || !states) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = d->kangaroo;
    if (!k) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_setup first");
    if ((uint64_t)first + n > k->N) return fail(BSGS_ERR_ARG, "kangaroos [%u, %u) of %u", first, first + n, k->N);
    if (!n) return BSGS_OK;
    HIPCHK(hipSetDevice(d->id));
    u32x4 *out = nullptr;
    HIPCHK(hipMalloc(&out, (size_t)n * 96));
    hipLaunchKernelGGL(kangaroo_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, d->stream, k->st, k->flags, k->key, k->N, out, first, n);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(states, out, (size_t)n * 96, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    (void)hipFree(out);
    HIPCHK(e);
    return BSGS_OK;
}

// one launch of the walk on the engine's stream, timed from ev0; bsgs_kangaroo_run and bsgs_kangaroo_run_tames (kangaroo_tames.hip) share the three steps
int bsgs_kangaroo_launch(bsgs_dev *d, uint32_t steps)
{
    bsgs_kangaroo *k = d->kangaroo;
    const u32 dp_mask = k->dp ? ~0u << (32u - k->dp) : 0u;
    HIPCHK(hipMemsetAsync(k->rec, 0, KANG_REC_HEADER, d->stream));
    HIPCHK(hipEventRecord(d->ev0, d->stream));
    if (k->R) {
        KangSymArgs S;
        S.st = k->st; S.flags = k->flags; S.chain = k->chain; S.table = k->table; S.rec = k->rec; S.mark = k->mark;
        S.N = k->N; S.T = k->T; S.G = k->G; S.steps = steps; S.dp_mask = dp_mask; S.cap = k->cap; S.rmask = k->R - 1u;
        S.mark_step = steps > BSGS_KANGAROO_CYCLE_WINDOW ? steps - 1u - BSGS_KANGAROO_CYCLE_WINDOW : ~0u;
        if (k->key) {
            if (k->block == 256u) hipLaunchKernelGGL(kangaroo_sym_keys_kernel<true>, dim3(k->T / 256u), dim3(256), KANG_TABLE_OFF, d->stream, S);
            else hipLaunchKernelGGL(kangaroo_sym_keys_kernel<false>, dim3(k->T / 64u), dim3(64), 0, d->stream, S);
        } else if (k->block == 256u) hipLaunchKernelGGL(kangaroo_sym_kernel<true>, dim3(k->T / 256u), dim3(256), KANG_TABLE_OFF, d->stream, S);
        else hipLaunchKernelGGL(kangaroo_sym_kernel<false>, dim3(k->T / 64u), dim3(64), 0, d->stream, S);
    } else {
        KangArgs A;
        A.st = k->st; A.flags = k->flags; A.chain = k->chain; A.table = k->table; A.rec = k->rec;
        A.N = k->N; A.T = k->T; A.G = k->G; A.steps = steps; A.dp_mask = dp_mask; A.cap = k->cap;
        if (k->block == 256u) hipLaunchKernelGGL(kangaroo_kernel<true>, dim3(k->T / 256u), dim3(256), KANG_LDS, d->stream, A);
        else hipLaunchKernelGGL(kangaroo_kernel<false>, dim3(k->T / 64u), dim3(64), KANG_LDS, d->stream, A);
    }
    HIPCHK(hipGetLastError());
    return BSGS_OK;
}
// ev1 behind what has been launched since bsgs_kangaroo_launch, then the count of records the walk produced (and the count at the head of `other`, a
// second record buffer, when there is one) and the synchronisation
int bsgs_kangaroo_finish(bsgs_dev *d, uint64_t *count, const u32 *other, uint64_t *other_count, float *kernel_ms)
{
    bsgs_kangaroo *k = d->kangaroo;
    HIPCHK(hipEventRecord(d->ev1, d->stream));
    HIPCHK(hipMemcpyAsync(count, k->rec, 8, hipMemcpyDeviceToHost, d->stream));
    if (other) HIPCHK(hipMemcpyAsync(other_count, other, 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    if (kernel_ms) HIPCHK(hipEventElapsedTime(kernel_ms, d->ev0, d->ev1));
    return BSGS_OK;
}
// the first min(held, max_recs) records of a record buffer -> recs (nullptr: none)
int bsgs_kangaroo_copy_out(bsgs_dev *d, const u32 *buf, uint64_t held, bsgs_kangaroo_record *recs, uint32_t max_recs, uint32_t *given)
{
    bsgs_kangaroo *k = d->kangaroo;
    const uint64_t give = recs ? std::min<uint64_t>(held, max_recs) : 0;
    if (give) {
        HIPCHK(hipMemcpyAsync(k->rec_host, (const char *)buf + KANG_REC_HEADER, give * 64, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
        memcpy(recs, k->rec_host, give * 64);
    }
    *given = (uint32_t)give;
    return BSGS_OK;
}

extern "C" int bsgs_kangaroo_run(bsgs_dev *d, uint32_t steps, bsgs_kangaroo_record *recs, uint32_t max_recs, uint32_t *nrecs, uint64_t *dropped, float *kernel_ms)
{
    if (!d || !nrecs) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = d->kangaroo;
    if (!k) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_setup first");
    HIPCHK(hipSetDevice(d->id));
    if (int rc = bsgs_kangaroo_launch(d, steps)) return rc;
    uint64_t count = 0;
    if (int rc = bsgs_kangaroo_finish(d, &count, nullptr, nullptr, kernel_ms)) return rc;
    if (int rc = bsgs_kangaroo_copy_out(d, k->rec, std::min<uint64_t>(count, k->cap), recs, max_recs, nrecs)) return rc;
    if (dropped) *dropped = count - *nrecs;
    return BSGS_OK;
}

extern "C" int bsgs_kangaroo_geometry(bsgs_dev *d, uint32_t *threads, uint32_t *per_thread, uint32_t *block)
{
    if (!d) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = d->kangaroo;
    if (!k) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_setup first");
    if (threads) *threads = k->T;
    if (per_thread) *per_thread = k->G;
    if (block) *block = k->block;
    return BSGS_OK;
}
