// kangaroo_verify.hip -- the kangaroo counterpart of the table verification (include/bsgs_hip.h, "Kangaroo, verification": bsgs_kangaroo_verify,
// bsgs_kangaroo_verify_points).  A kangaroo with state (x, y, d, flags) stands at sigma*Q + d*G, sigma = 0 tame, +1 wild, -1 wild with NEG: the
// fixed-base comb of the seeding unit (kangaroo_seed.hip.h: sixteen windows on |d|, y negated for d < 0, then Q of the kangaroo as a seventeenth addend, the
// only one that can double or cancel) computes that point again and compares.
//   herd in place    d and flags come from the herd's own arrays, nothing crosses the bus; the comparison stays in Jacobian form, X == x Z^2 and Y == y Z^3
//                    (four multiplications, no inversion, no LDS, no scratch per position); the herd is only read
//   points of a list (d, flags) staged, compared with the low 64 bits of the affine x: those do not determine x Z^2, so Z is inverted, one Fermat inversion
//                    per block of four waves (fe_inv_block, as the seeding kernels' second pass; one position per thread, so no running products)
// Both count the positions that fail with one atomic per wave and write the first `cap` of them with vector stores (the pattern of kang_record).
#include "kangaroo_seed.hip.h"

struct VerifyArgs {
    const u32x4 *st;       // [5][N]: x.lo, x.hi, y.lo, y.hi, d (herd in place)
    const u32 *flags;      // [N]
    const u32 *key;        // [N]: the keys of a bsgs_kangaroo_setup_sym_keys herd checked against its list (its flags hold no key), else nullptr
    const u32x4 *comb;     // [16][255] points, x || y
    const u32x4 *q;        // [nq] points Q_k, x || y: the call's one Q (nq = 1, key_mask = 0) or the herd's key list
    const u32x4 *d;        // [n] staged offsets, two's complement (points of a list)
    const u32 *fl;         // [n] staged flags
    const u64 *x64;        // [n] staged low 64 bits of the affine x
    u32 *out;              // {positions that failed, then the first `cap` of them}
    u32 N, first, n, nq, key_mask, cap, pos0;
};

// (X, Y, Z) = sigma*Q + d*G with Q = q[0 .. 3] (nullptr: sigma = 0), sigma = -1 with NEG; X and Y canonical.  false: the sum is the point at infinity
__device__ __forceinline__ bool verify_point(fe &X, fe &Y, fe &Z, const u32x4 *comb, const u32x4 *q, const u32x4 dv, const bool qneg)
{
    const bool neg = (dv.w >> 31) != 0u;
    u32 m0 = dv.x, m1 = dv.y, m2 = dv.z, m3 = dv.w;                  // |d|
    if (neg) {
        u32 c = 0, co;
        m0 = __builtin_subc(0u, m0, c, &co); c = co;
        m1 = __builtin_subc(0u, m1, c, &co); c = co;
        m2 = __builtin_subc(0u, m2, c, &co); c = co;
        m3 = __builtin_subc(0u, m3, c, &co);
    }
    bool empty = true, twice = false;
    // seventeen addends through one load and one addition site, as kangaroo_seed_keys_kernel's own loop (two loops, not one function: shared, it costs
    // that kernel 130 VGPRs and its fourth wave, kangaroo_seed.hip.h): only the last one can double or cancel
#pragma nounroll
    for (u32 w = 0; w <= SEED_WINDOWS; w++) {
        const u32x4 *p;
        if (w < SEED_WINDOWS) {
            const u32 v = m0 & 255u;
            m0 = (m0 >> 8) | (m1 << 24); m1 = (m1 >> 8) | (m2 << 24); m2 = (m2 >> 8) | (m3 << 24); m3 >>= 8;
            if (!v) continue;
            p = comb + (u64)(w * 255u + v - 1u) * 4u;
        } else {
            if (neg && !empty) fe_neg(Y, Y);                         // (no point of the curve has y = 0)
            if (!q) break;
            p = q;
        }
        fe ax, ay;
        fe_load2(ax, p, p + 1);
        fe_load2(ay, p + 2, p + 3);
        if (w == SEED_WINDOWS && qneg) fe_neg(ay, ay);
        if (empty) { X = ax; Y = ay; fe_set_one(Z); empty = false; }
        else {
            const u32 kind = jac_madd_if(X, Y, Z, ax, ay, w == SEED_WINDOWS);
            if (__builtin_expect(kind == 1u, 0)) twice = true;
            else if (__builtin_expect(kind == 2u, 0)) empty = true;
        }
    }
    if (__builtin_expect(twice, 0)) {                                 // d*G == sigma*Q: the point is 2 sigma Q, from Q read again
        fe qx, qy;
        fe_load2(qx, q, q + 1);
        fe_load2(qy, q + 2, q + 3);
        if (qneg) fe_neg(qy, qy);
        jac_double_affine(X, Y, Z, qx, qy);
    }
    return !empty;
}

// one entry per lane with `bad`: the count by one atomic per wave, the index by a vector store while the list has room (kang_record's pattern)
__device__ __forceinline__ void verify_report(u32 *out, u32 cap, bool bad, u32 idx, u32 lane)
{
    const u64 m = __ballot(bad);
    if (m) {
        u32 base = 0;
        const int leader = __builtin_ctzll(m);
        if ((int)lane == leader) base = atomicAdd(out, (u32)__builtin_popcountll(m));
        base = __shfl(base, leader);
        const u32 slot = base + (u32)__builtin_popcountll(m & ((1ull << lane) - 1));
        if (bad && slot < cap) out[1u + slot] = idx;
    }
}

__device__ __forceinline__ bool verify_canonical(const fe &a) { fe c = a; fe_canon(c); return fe_eq(c, a); }

__global__ void __launch_bounds__(256) kangaroo_verify_kernel(const VerifyArgs A)
{
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u;
    const u32 N = A.N, i = A.first + k;
    bool bad = false;
    if (k < A.n && i < N) {                                          // (the host has checked first + n <= N)
        const u32 fl = A.flags[i];
        const u32x4 dv = A.st[4 * (u64)N + i];
        const bool wild = (fl & BSGS_KANGAROO_WILD) != 0u;
        const u32 key = A.key ? A.key[i] : (fl >> BSGS_KANGAROO_KEY_SHIFT) & A.key_mask;      // 0 with the call's one Q: a symmetric herd keeps its last jump index in these bits
        if (wild ? key >= A.nq : (key != 0u || (fl & BSGS_KANGAROO_NEG) != 0u)) bad = true;       // a key beyond the list (nothing is read for it), a tame
                                                                                                  // kangaroo with a key or with NEG: the state is wrong
        else {
            fe X, Y, Z, x, y;
            const bool finite = verify_point(X, Y, Z, A.comb, wild ? A.q + (u64)key * 4u : nullptr, dv, (fl & BSGS_KANGAROO_NEG) != 0u);
            fe_load2(x, A.st + i, A.st + N + i);
            fe_load2(y, A.st + 2 * (u64)N + i, A.st + 3 * (u64)N + i);
            if (!finite) bad = !((fl & BSGS_KANGAROO_DEAD) && seed_is_zero(x) && seed_is_zero(y));        // what the seeding leaves for a start at infinity
            else {
                fe zz, t;
                bad = !verify_canonical(x) || !verify_canonical(y);
                fe_sqr(zz, Z);
                fe_mul(t, x, zz);
                fe_canon(t);
                bad |= !fe_eq(t, X);
                fe_mul(zz, zz, Z);
                fe_mul(t, y, zz);
                fe_canon(t);
                bad |= !fe_eq(t, Y);
            }
        }
    }
    verify_report(A.out, A.cap, bad, i, lane);
}

__global__ void __launch_bounds__(256) kangaroo_verify_points_kernel(const VerifyArgs A)
{
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool active = k < A.n;
    fe X, Y, Z;
    bool finite = false;
    if (active) {
        const u32 fl = A.fl[k];
        const bool wild = (fl & BSGS_KANGAROO_WILD) != 0u;
        const u32 key = (fl >> BSGS_KANGAROO_KEY_SHIFT) & A.key_mask;
        if (wild ? key < A.nq : (key == 0u && !(fl & BSGS_KANGAROO_NEG)))       // (a key beyond the list: refused by the host); a tame entry has no key, no NEG
            finite = verify_point(X, Y, Z, A.comb, wild ? A.q + (u64)key * 4u : nullptr, A.d[k], (fl & BSGS_KANGAROO_NEG) != 0u);
    }
    if (!finite) { fe_set_one(X); fe_set_one(Z); }                   // every thread of the block takes part in the inversion; 1, never 0
    fe zi;
    fe_inv_block<SEED_REGION, 4>(zi, Z, lane, wave, blockIdx.x & 3u);
    fe_sqr(zi, zi);
    fe_mul(X, X, zi);
    fe_canon(X);
    const bool bad = active && (!finite || (((u64)X.v[1] << 32) | X.v[0]) != A.x64[k]);      // a table never holds the point at infinity
    verify_report(A.out, A.cap, bad, A.pos0 + k, lane);
}

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------------------------------
#define VERIFY_LIST_MAX (1u << 20)                          // entries of the device's list of failures

// the comb, the call's Q or the key list, the cleared result words
static int verify_begin(bsgs_dev *d, bsgs_kangaroo *k, const uint8_t *q_xy_le, uint32_t max_bad, VerifyArgs &A)
{
    if (!q_xy_le && !k->keys) return fail(BSGS_ERR_STATE, "no Q: bsgs_kangaroo_set_keys first, or name one");
    HIPCHK(hipSetDevice(d->id));
    if (int rc = seed_comb(d, k)) return rc;
    const uint32_t cap = std::min(max_bad, VERIFY_LIST_MAX);
    if (!k->verify_out || k->verify_cap < cap) {
        if (k->verify_out) (void)hipFree(k->verify_out);
        k->verify_out = nullptr; k->verify_cap = 0;
        HIPCHK(hipMalloc(&k->verify_out, 4 * ((size_t)cap + 1)));
        k->verify_cap = cap;
    }
    if (!k->verify_q) HIPCHK(hipMalloc(&k->verify_q, 64));
    HIPCHK(hipMemsetAsync(k->verify_out, 0, 4, d->stream));
    if (q_xy_le) HIPCHK(hipMemcpyAsync(k->verify_q, q_xy_le, 64, hipMemcpyHostToDevice, d->stream));
    memset(&A, 0, sizeof A);
    A.st = k->st; A.flags = k->flags; A.comb = k->comb; A.out = k->verify_out; A.N = k->N; A.cap = cap;
    A.q = q_xy_le ? k->verify_q : k->keys;
    A.nq = q_xy_le ? 1u : k->n_keys;
    A.key_mask = q_xy_le ? 0u : 0xFFFFu;
    A.key = q_xy_le ? nullptr : k->key;
    return BSGS_OK;
}
// the count and what the list holds of it, ascending (launches of one stream fill the list in their order: the lowest-numbered chunk's failures come first)
static int verify_end(bsgs_dev *d, bsgs_kangaroo *k, uint32_t cap, uint32_t *n_bad, uint32_t *bad_idx)
{
    uint32_t count = 0;
    HIPCHK(hipMemcpyAsync(&count, k->verify_out, 4, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    const uint32_t give = std::min(count, cap);
    if (give) {
        HIPCHK(hipMemcpyAsync(bad_idx, k->verify_out + 1, 4 * (size_t)give, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
        std::sort(bad_idx, bad_idx + give);
    }
    *n_bad = count;
    return BSGS_OK;
}

extern "C" int bsgs_kangaroo_verify(bsgs_dev *d, const uint8_t *q_xy_le, uint32_t first, uint32_t n, uint32_t *n_bad, uint32_t *bad_idx, uint32_t max_bad)
{
    if (!d || !n_bad || (max_bad && !bad_idx)) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = d->kangaroo;
    if (!k) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_setup first");
    *n_bad = 0;
    if ((uint64_t)first + n > k->N) return fail(BSGS_ERR_ARG, "kangaroos [%u, %llu) of %u", first, (unsigned long long)first + n, k->N);
    VerifyArgs A;
    if (int rc = verify_begin(d, k, q_xy_le, max_bad, A)) return rc;
    for (uint32_t pos = 0; pos < n; pos += SEED_CHUNK) {
        const uint32_t m = std::min(n - pos, SEED_CHUNK);
        A.first = first + pos; A.n = m; A.pos0 = pos;
        hipLaunchKernelGGL(kangaroo_verify_kernel, dim3((m + 255u) / 256u), dim3(256), 0, d->stream, A);
        HIPCHK(hipGetLastError());
    }
    return verify_end(d, k, A.cap, n_bad, bad_idx);
}

extern "C" int bsgs_kangaroo_verify_points(bsgs_dev *d, const uint8_t *q_xy_le, uint32_t n, const uint8_t *d_le, const uint32_t *flags, const uint64_t *x_lo64,
                                           uint32_t *n_bad, uint32_t *bad_idx, uint32_t max_bad)
{
    if (!d || !n_bad || (max_bad && !bad_idx) || (n && (!d_le || !flags || !x_lo64))) return fail(BSGS_ERR_ARG, "null");
    bsgs_kangaroo *k = d->kangaroo;
    if (!k) return fail(BSGS_ERR_STATE, "bsgs_kangaroo_setup first");
    *n_bad = 0;
    if (!q_xy_le && !k->keys) return fail(BSGS_ERR_STATE, "no Q: bsgs_kangaroo_set_keys first, or name one");
    if (!q_xy_le) for (uint32_t p = 0; p < n; p++)
        if ((flags[p] & BSGS_KANGAROO_WILD) && ((flags[p] >> BSGS_KANGAROO_KEY_SHIFT) & 0xFFFFu) >= k->n_keys)
            return fail(BSGS_ERR_ARG, "entry %u: key %u of %u", p, (flags[p] >> BSGS_KANGAROO_KEY_SHIFT) & 0xFFFFu, k->n_keys);
    VerifyArgs A;
    if (int rc = verify_begin(d, k, q_xy_le, max_bad, A)) return rc;
    if (!n) return verify_end(d, k, A.cap, n_bad, bad_idx);
    // the staging of a seed call serves: offsets and flags where they go there, the 64-bit words in the room of the Z's (32 bytes per position)
    if (int rc = seed_staging(d, k, n)) return rc;
    A.d = k->seed_in;
    A.fl = (const u32 *)(k->seed_in + k->seed_cap);
    A.x64 = (const u64 *)k->seed_z;
    for (uint32_t pos = 0; pos < n; pos += SEED_CHUNK) {
        const uint32_t m = std::min(n - pos, SEED_CHUNK);
        HIPCHK(hipMemcpyAsync((void *)A.d, d_le + (size_t)pos * 16, (size_t)m * 16, hipMemcpyHostToDevice, d->stream));
        HIPCHK(hipMemcpyAsync((void *)A.fl, flags + pos, (size_t)m * 4, hipMemcpyHostToDevice, d->stream));
        HIPCHK(hipMemcpyAsync((void *)A.x64, x_lo64 + pos, (size_t)m * 8, hipMemcpyHostToDevice, d->stream));
        A.n = m; A.pos0 = pos;
        hipLaunchKernelGGL(kangaroo_verify_points_kernel, dim3((m + 255u) / 256u), dim3(256), SEED_LDS, d->stream, A);
        HIPCHK(hipGetLastError());
    }
    return verify_end(d, k, A.cap, n_bad, bad_idx);
}
