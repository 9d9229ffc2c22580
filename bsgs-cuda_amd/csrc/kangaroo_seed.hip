// kangaroo_seed.hip -- the start points of kangaroos on gfx950: offsets d in, states (d*G or Q + d*G, d, flags) out (include/bsgs_hip.h, "Kangaroo":
// bsgs_kangaroo_seed; "Kangaroo, many keys": bsgs_kangaroo_set_keys, bsgs_kangaroo_seed_keys).  What the host's comb did on CPU threads before every run and
// between launches at every re-seed.
//
// Fixed-base comb, 16 windows of 8 bits: table T[k][v] = v * 2^(8k) * G for v = 1..255 (4080 affine points, 255 KiB, built once per herd on the host and
// kept in device memory; it stays in L2).  A thread takes B positions of the call, k = b * TT + thread (a wave's staging and state accesses are contiguous).
// Pass 1, per position: |d| * G by at most sixteen Jacobian mixed additions, y negated for d < 0, then + Q for a wild one; X, Y go to the kangaroo's own
// state slots, Z to a scratch, the running product of the thread's Z's to the walk's batch scratch.  One inversion per block of four waves (fe_inv_block,
// as the walk).  Pass 2, backwards: 1 / Z from the running products, x = X / Z^2, y = Y / Z^3 canonical, d and flags stored.
// Inside the comb no addition is degenerate: before window k the partial sum is a multiple of G below 2^(8k), the addend a multiple of 2^(8k) below 2^128,
// and 2^128 is far below the group order; a zero digit is skipped and the first nonzero digit is a copy.  Only + Q can double (d*G == Q) or cancel
// (d*G == -Q): the last addition tests for both.  A start at infinity (that, or tame d = 0) puts 1 into the batch, never 0, and leaves the kangaroo dead.
//
// A herd that serves a LIST of public keys (bsgs_kangaroo_seed_keys): a wild position adds Q of ITS key, gathered from the key list in device memory (64
// bytes per wild start; a list of 1000 keys is 64 KB and stays in L2) as a seventeenth addend of the comb loop, and its stored flags keep the key's list
// position in bits 8..23.  The plain walk never looks at those bits and copies the word into every record, so a record names the key its kangaroo was
// seeded for.
//
// Two kernels, one host path (seed_run).  The list kernel run with a list of one entry and key 0 computes what the single-Q kernel computes, but Q then
// comes from L2 where the single-Q kernel holds it in SGPRs, and a full herd pays for it: 2^22 starts, half of them wild, four launches summed from a kernel
// trace, 3.96 ms (3.93 .. 3.98 over 30 calls) with the single-Q kernel against 4.01 ms (3.98 .. 4.03) with the list kernel
// (profiles/r22a_kangaroo_seed_one_kernel.log).
#include "kangaroo_seed.hip.h"

// the two kernels' arguments: the same fields under the same names (seed_run fills them for either), then the call's Q itself or the key list
struct SeedArgs {
    u32x4 *st;             // [5][N]: x.lo, x.hi, y.lo, y.hi, d
    u32 *flags;            // [N]
    u32x4 *prefix;         // the walk's batch scratch (2 N vectors), here [2][N] by position: running products of Z
    u32x4 *z;              // [2][cap] by position
    const u32x4 *comb;     // [16][255] points, x || y
    const u32x4 *d;        // [n] offsets, two's complement
    const u32 *fl;         // [n] BSGS_KANGAROO_WILD or 0
    const u32 *idx;        // [n] kangaroo of each position, or NULL: first + position
    u32 *out;              // {count of starts at infinity, lowest position of one}
    fe qx, qy;
    u32 N, cap, first, n, B, TT, pos0;
};
struct KeySeedArgs {
    u32x4 *st;             // [5][N]: x.lo, x.hi, y.lo, y.hi, d
    u32 *flags;            // [N]
    u32x4 *prefix;         // the walk's batch scratch (2 N vectors), here [2][N] by position: running products of Z
    u32x4 *z;              // [2][cap] by position
    const u32x4 *comb;     // [16][255] points, x || y
    const u32x4 *keys;     // [n_keys] points Q_k, x || y
    const u32x4 *d;        // [n] offsets, two's complement
    const u32 *fl;         // [n] 0, or BSGS_KANGAROO_WILD | key << BSGS_KANGAROO_KEY_SHIFT
    const u32 *idx;        // [n] kangaroo of each position, or NULL: first + position
    u32 *out;              // {count of starts at infinity, lowest position of one}
    u32 N, cap, first, n, B, TT, pos0;
};

// one Q for the call, in SGPRs: sixteen addends in the loop, none of which can double or cancel, then + Q
__global__ void __launch_bounds__(256) kangaroo_seed_kernel(const SeedArgs A)
{
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;            // the launch has exactly TT threads, B * TT >= n
    const u32 lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 N = A.N, n = A.n, TT = A.TT;
    u32x4 *const sx0 = A.st, *const sx1 = A.st + N, *const sy0 = A.st + 2 * (u64)N, *const sy1 = A.st + 3 * (u64)N, *const sd = A.st + 4 * (u64)N;
    fe acc;
    fe_set_one(acc);
    u32 infinite = 0;                                                // bit b: position b * TT + t starts at infinity
#pragma nounroll
    for (u32 b = 0; b < A.B; b++) {
        const u32 k = b * TT + t;
        if (k >= n) break;                                           // (positions only grow with b)
        const u32 i = A.idx ? A.idx[k] : A.first + k;
        const u32x4 dv = A.d[k];
        const bool wild = (A.fl[k] & BSGS_KANGAROO_WILD) != 0u, neg = (dv.w >> 31) != 0u;
        u32 m0 = dv.x, m1 = dv.y, m2 = dv.z, m3 = dv.w;              // |d|
        if (neg) {
            u32 c = 0, co;
            m0 = __builtin_subc(0u, m0, c, &co); c = co;
            m1 = __builtin_subc(0u, m1, c, &co); c = co;
            m2 = __builtin_subc(0u, m2, c, &co); c = co;
            m3 = __builtin_subc(0u, m3, c, &co);
        }
        fe X, Y, Z;
        bool empty = true;
#pragma nounroll
        for (u32 w = 0; w < SEED_WINDOWS; w++) {
            const u32 v = m0 & 255u;
            m0 = (m0 >> 8) | (m1 << 24); m1 = (m1 >> 8) | (m2 << 24); m2 = (m2 >> 8) | (m3 << 24); m3 >>= 8;
            if (!v) continue;
            const u32x4 *p = A.comb + (u64)(w * 255u + v - 1u) * 4u;
            fe ax, ay;
            fe_load2(ax, p, p + 1);
            fe_load2(ay, p + 2, p + 3);
            if (empty) { X = ax; Y = ay; fe_set_one(Z); empty = false; }
            else jac_madd<false>(X, Y, Z, ax, ay);
        }
        if (neg && !empty) fe_neg(Y, Y);                             // (no point of the curve has y = 0)
        if (wild) {
            if (empty) { X = A.qx; Y = A.qy; fe_set_one(Z); empty = false; }
            else {
                const u32 kind = jac_madd<true>(X, Y, Z, A.qx, A.qy);
                if (__builtin_expect(kind == 1u, 0)) jac_double_affine(X, Y, Z, A.qx, A.qy);
                else if (__builtin_expect(kind == 2u, 0)) empty = true;
            }
        }
        if (empty) { fe_set_one(Z); infinite |= 1u << b; }
        else if (i < N) { fe_store2(sx0 + i, sx1 + i, X); fe_store2(sy0 + i, sy1 + i, Y); }
        fe_mul(acc, acc, Z);
        fe_store2(A.z + k, A.z + A.cap + k, Z);
        fe_store2(A.prefix + k, A.prefix + N + k, acc);
    }
    fe inv;
    fe_inv_block<SEED_REGION, 4>(inv, acc, lane, wave, blockIdx.x & 3u);
#pragma nounroll
    for (u32 bb = 0; bb < A.B; bb++) {
        const u32 b = A.B - 1u - bb;
        const u32 k = b * TT + t;
        if (k >= n) continue;
        fe zi;
        if (b > 0) {
            fe c, z;
            fe_load2(c, A.prefix + (k - TT), A.prefix + N + (k - TT));
            fe_load2(z, A.z + k, A.z + A.cap + k);
            fe_mul(zi, inv, c);
            fe_mul(inv, inv, z);
        } else zi = inv;
        const u32 i = A.idx ? A.idx[k] : A.first + k;
        if (i >= N) continue;                                        // (the host has checked: never taken)
        const u32 fl = A.fl[k] & BSGS_KANGAROO_WILD;
        sd[i] = A.d[k];
        if (__builtin_expect((infinite >> b) & 1u, 0)) {
            const u32x4 zero = {0u, 0u, 0u, 0u};
            sx0[i] = zero; sx1[i] = zero; sy0[i] = zero; sy1[i] = zero;
            A.flags[i] = fl | BSGS_KANGAROO_DEAD;
            atomicAdd(A.out, 1u);
            atomicMin(A.out + 1, A.pos0 + k);
            continue;
        }
        fe X, Y, z2, z3;
        fe_load2(X, sx0 + i, sx1 + i);
        fe_load2(Y, sy0 + i, sy1 + i);
        fe_sqr(z2, zi);
        fe_mul(z3, z2, zi);
        fe_mul(X, X, z2);
        fe_canon(X);
        fe_mul(Y, Y, z3);
        fe_canon(Y);
        fe_store2(sx0 + i, sx1 + i, X);
        fe_store2(sy0 + i, sy1 + i, Y);
        A.flags[i] = fl;
    }
}

// one Q per key of a list: the same shape (B positions per thread, one fe_inv_block per block of four waves, states in the walk's SoA layout); Q of the
// position's key is gathered from the list as a seventeenth addend of the comb loop, and the stored flags keep the key
__global__ void __launch_bounds__(256) kangaroo_seed_keys_kernel(const KeySeedArgs A)
{
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;            // the launch has exactly TT threads, B * TT >= n
    const u32 lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 N = A.N, n = A.n, TT = A.TT;
    u32x4 *const sx0 = A.st, *const sx1 = A.st + N, *const sy0 = A.st + 2 * (u64)N, *const sy1 = A.st + 3 * (u64)N, *const sd = A.st + 4 * (u64)N;
    fe acc;
    fe_set_one(acc);
    u32 infinite = 0;                                                // bit b: position b * TT + t starts at infinity
#pragma nounroll
    for (u32 b = 0; b < A.B; b++) {
        const u32 k = b * TT + t;
        if (k >= n) break;                                           // (positions only grow with b)
        const u32 i = A.idx ? A.idx[k] : A.first + k;
        const u32x4 dv = A.d[k];
        const u32 flw = A.fl[k];                                     // WILD | key << BSGS_KANGAROO_KEY_SHIFT (the host has checked key < n_keys)
        const bool wild = (flw & BSGS_KANGAROO_WILD) != 0u, neg = (dv.w >> 31) != 0u;
        u32 m0 = dv.x, m1 = dv.y, m2 = dv.z, m3 = dv.w;              // |d|
        if (neg) {
            u32 c = 0, co;
            m0 = __builtin_subc(0u, m0, c, &co); c = co;
            m1 = __builtin_subc(0u, m1, c, &co); c = co;
            m2 = __builtin_subc(0u, m2, c, &co); c = co;
            m3 = __builtin_subc(0u, m3, c, &co);
        }
        fe X, Y, Z;
        bool empty = true, twice = false;
        // seventeen addends: the comb's sixteen windows, then Q of the kangaroo's key as one more (64 bytes, from L2 after the first touch).  One load and
        // one addition site serve both, so Q costs no registers beyond the comb's own addend; only the last addition can double or cancel.
#pragma nounroll
        for (u32 w = 0; w <= SEED_WINDOWS; w++) {
            const u32x4 *p;
            if (w < SEED_WINDOWS) {
                const u32 v = m0 & 255u;
                m0 = (m0 >> 8) | (m1 << 24); m1 = (m1 >> 8) | (m2 << 24); m2 = (m2 >> 8) | (m3 << 24); m3 >>= 8;
                if (!v) continue;                                    // (also for the top digit: the loop bound w <= SEED_WINDOWS still brings the Q step)
                p = A.comb + (u64)(w * 255u + v - 1u) * 4u;
            } else {
                if (neg && !empty) fe_neg(Y, Y);                     // (no point of the curve has y = 0)
                if (!wild) break;
                p = A.keys + (u64)(flw >> BSGS_KANGAROO_KEY_SHIFT) * 4u;
            }
            fe ax, ay;
            fe_load2(ax, p, p + 1);
            fe_load2(ay, p + 2, p + 3);
            if (empty) { X = ax; Y = ay; fe_set_one(Z); empty = false; }
            else {
                const u32 kind = jac_madd_if(X, Y, Z, ax, ay, w == SEED_WINDOWS);
                if (__builtin_expect(kind == 1u, 0)) twice = true;
                else if (__builtin_expect(kind == 2u, 0)) empty = true;
            }
        }
        if (__builtin_expect(twice, 0)) {                             // d*G == Q: the start is 2 Q, from Q read again (held across the additions it would cost
            const u32x4 *q = A.keys + (u64)(flw >> BSGS_KANGAROO_KEY_SHIFT) * 4u;      // sixteen registers and the fourth wave)
            fe qx, qy;
            fe_load2(qx, q, q + 1);
            fe_load2(qy, q + 2, q + 3);
            jac_double_affine(X, Y, Z, qx, qy);
        }
        if (empty) { fe_set_one(Z); infinite |= 1u << b; }
        else if (i < N) { fe_store2(sx0 + i, sx1 + i, X); fe_store2(sy0 + i, sy1 + i, Y); }
        fe_mul(acc, acc, Z);
        fe_store2(A.z + k, A.z + A.cap + k, Z);
        fe_store2(A.prefix + k, A.prefix + N + k, acc);
    }
    fe inv;
    fe_inv_block<SEED_REGION, 4>(inv, acc, lane, wave, blockIdx.x & 3u);
#pragma nounroll
    for (u32 bb = 0; bb < A.B; bb++) {
        const u32 b = A.B - 1u - bb;
        const u32 k = b * TT + t;
        if (k >= n) continue;
        fe zi;
        if (b > 0) {
            fe c, z;
            fe_load2(c, A.prefix + (k - TT), A.prefix + N + (k - TT));
            fe_load2(z, A.z + k, A.z + A.cap + k);
            fe_mul(zi, inv, c);
            fe_mul(inv, inv, z);
        } else zi = inv;
        const u32 i = A.idx ? A.idx[k] : A.first + k;
        if (i >= N) continue;                                        // (the host has checked: never taken)
        // the key index stays in the kangaroo's flags: the plain walk copies the word into every record.  A herd of bsgs_kangaroo_setup_sym_keys holds the
        // word only until kangaroo_split_keys_kernel, queued behind this launch on the same stream, has moved the key to the key array: no walk runs between
        // the two, so the symmetric step never takes key bits for its last jump index
        const u32 fl = A.fl[k];
        sd[i] = A.d[k];
        if (__builtin_expect((infinite >> b) & 1u, 0)) {
            const u32x4 zero = {0u, 0u, 0u, 0u};
            sx0[i] = zero; sx1[i] = zero; sy0[i] = zero; sy1[i] = zero;
            A.flags[i] = fl | BSGS_KANGAROO_DEAD;
            atomicAdd(A.out, 1u);
            atomicMin(A.out + 1, A.pos0 + k);
            continue;
        }
        fe X, Y, z2, z3;
        fe_load2(X, sx0 + i, sx1 + i);
        fe_load2(Y, sy0 + i, sy1 + i);
        fe_sqr(z2, zi);
        fe_mul(z3, z2, zi);
        fe_mul(X, X, z2);
        fe_canon(X);
        fe_mul(Y, Y, z3);
        fe_canon(Y);
        fe_store2(sx0 + i, sx1 + i, X);
        fe_store2(sy0 + i, sy1 + i, Y);
        A.flags[i] = fl;
    }
}

// ---- one seed call: the staging, a launch per chunk, the two result words -------------------------------------------------------------------------------
// kernel and A: either kernel with its arguments, the call's Q or the key list filled in, everything else zero.  fl[0..n): the words the kernel reads and
// stores.  split: a herd of bsgs_kangaroo_setup_sym_keys seeded from its list: the key then moves from the stored word to the key array (the kernel sits at
// its register budget: a pass of its own)
template <class ARGS>
static int seed_run(bsgs_dev *d, bsgs_kangaroo *k, void (*kernel)(const ARGS), ARGS &A, bool split, const uint32_t *idx, uint32_t first, uint32_t n,
                    const uint8_t *d_le, const uint32_t *fl, uint32_t *n_infinite, uint32_t *first_infinite)
{
    HIPCHK(hipSetDevice(d->id));
    if (int rc = seed_staging(d, k, n)) return rc;
    A.st = k->st; A.flags = k->flags; A.prefix = k->chain; A.z = k->seed_z; A.comb = k->comb; A.out = k->seed_out;
    A.d = k->seed_in;
    A.fl = (const u32 *)(k->seed_in + k->seed_cap);
    A.idx = idx ? A.fl + k->seed_cap : nullptr;
    A.N = k->N; A.cap = k->seed_cap;
    for (uint32_t pos = 0; pos < n; pos += SEED_CHUNK) {
        const uint32_t m = std::min(n - pos, SEED_CHUNK);
        HIPCHK(hipMemcpyAsync((void *)A.d, d_le + (size_t)pos * 16, (size_t)m * 16, hipMemcpyHostToDevice, d->stream));
        HIPCHK(hipMemcpyAsync((void *)A.fl, fl + pos, (size_t)m * 4, hipMemcpyHostToDevice, d->stream));
        if (idx) HIPCHK(hipMemcpyAsync((void *)A.idx, idx + pos, (size_t)m * 4, hipMemcpyHostToDevice, d->stream));
        A.first = first + pos; A.n = m; A.pos0 = pos;
        A.B = m >= (1u << 18) ? 4u : 1u;                             // four starts share a thread's inversion once the launch fills the GPU without
        A.TT = ((m + A.B - 1) / A.B + 255u) / 256u * 256u;
        hipLaunchKernelGGL(kernel, dim3(A.TT / 256u), dim3(256), SEED_LDS, d->stream, A);
        HIPCHK(hipGetLastError());
        if (split) if (int rc = bsgs_kangaroo_split_keys(d, A.idx, A.first, m)) return rc;
    }
    uint32_t out[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(out, k->seed_out, 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));                                 // (the callers' buffers are free again)
    if (n_infinite) *n_infinite = out[0];
    if (first_infinite) *first_infinite = out[0] ? out[1] : 0u;
    return BSGS_OK;
}

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int bsgs_kangaroo_seed(bsgs_dev *d, const uint8_t *q_xy_le, const uint32_t *idx, uint32_t first, uint32_t n, const uint8_t *d_le,
                                  const uint32_t *flags, uint32_t *n_infinite, uint32_t *first_infinite)
{
    if (!d || !d_le || !flags) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = d->kangaroo;
    if (!k) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_setup first");
    if (n_infinite) *n_infinite = 0;
    if (first_infinite) *first_infinite = 0;
    if (!n) return BSGS_OK;
    if (int rc = seed_check_positions(k, idx, first, n)) return rc;
    bool any_wild = false;
    for (uint32_t q = 0; q < n; q++) {
        if (flags[q] & ~BSGS_KANGAROO_WILD) return fail(BSGS_ERR_ARG, "flags of position %u: BSGS_KANGAROO_WILD or 0", q);
        any_wild |= flags[q] != 0;
    }
    if (any_wild && !q_xy_le) return fail(BSGS_ERR_ARG, "wild kangaroos need Q");
    SeedArgs A;
    memset(&A, 0, sizeof A);
    if (q_xy_le) { memcpy(A.qx.v, q_xy_le, 32); memcpy(A.qy.v, q_xy_le + 32, 32); }
    // (the stored flags hold no key bits, so a herd of bsgs_kangaroo_setup_sym_keys needs no split pass; its key array and the key list stay as they are)
    return seed_run(d, k, kangaroo_seed_kernel, A, false, idx, first, n, d_le, flags, n_infinite, first_infinite);
}

extern "C" int bsgs_kangaroo_set_keys(bsgs_dev *d, const uint8_t *q_xy_le, uint32_t n_keys)
{
    if (!d || !q_xy_le) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = d->kangaroo;
    if (!k) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_setup first");
    if (k->R && !k->key) return fail(BSGS_ERR_STATE, "a herd of the symmetric walk takes one key (its flags hold the last jump index where the key index would go; bsgs_kangaroo_setup_sym_keys makes one that takes a list)");
    if (!n_keys || n_keys > BSGS_KANGAROO_MAX_KEYS) return fail(BSGS_ERR_ARG, "%u keys: 1..%u", n_keys, BSGS_KANGAROO_MAX_KEYS);
    HIPCHK(hipSetDevice(d->id));
    HIPCHK(hipStreamSynchronize(d->stream));
    if (k->keys) (void)hipFree(k->keys);
    k->keys = nullptr; k->n_keys = 0;
    HIPCHK(hipMalloc(&k->keys, (size_t)n_keys * 64));
    HIPCHK(hipMemcpyAsync(k->keys, q_xy_le, (size_t)n_keys * 64, hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));                                 // (the caller's buffer is free again)
    k->n_keys = n_keys;
    return BSGS_OK;
}

extern "C" int bsgs_kangaroo_seed_keys(bsgs_dev *d, const uint32_t *idx, uint32_t first, uint32_t n, const uint8_t *d_le, const uint32_t *flags,
                                       const uint32_t *key, uint32_t *n_infinite, uint32_t *first_infinite)
{
    if (!d || !d_le || !flags || !key) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = d->kangaroo;
    if (!k) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_setup first");
    if (k->R && !k->key) return fail(BSGS_ERR_STATE, "a herd of the symmetric walk takes one key");
    if (n_infinite) *n_infinite = 0;
    if (first_infinite) *first_infinite = 0;
    if (!n) return BSGS_OK;
    if (int rc = seed_check_positions(k, idx, first, n)) return rc;
    std::vector<uint32_t> fl(n);                                             // what the kernel reads and stores: the type and the key in one word
    for (uint32_t q = 0; q < n; q++) {
        if (flags[q] & ~BSGS_KANGAROO_WILD) return fail(BSGS_ERR_ARG, "flags of position %u: BSGS_KANGAROO_WILD or 0", q);
        if (!flags[q]) {
            if (key[q]) return fail(BSGS_ERR_ARG, "position %u: a tame kangaroo has key 0", q);
        } else {
            if (!k->keys) return fail(BSGS_ERR_STATE, "wild kangaroos need bsgs_kangaroo_set_keys first");
            if (key[q] >= k->n_keys) return fail(BSGS_ERR_ARG, "position %u: key %u of %u", q, key[q], k->n_keys);
        }
        fl[q] = flags[q] | key[q] << BSGS_KANGAROO_KEY_SHIFT;
    }
    KeySeedArgs A;
    memset(&A, 0, sizeof A);
    A.keys = k->keys;
    return seed_run(d, k, kangaroo_seed_keys_kernel, A, k->key != nullptr, idx, first, n, d_le, fl.data(), n_infinite, first_infinite);
}
