// kangaroo_seed.hip.h -- what the herd seeding unit (kangaroo_seed.hip) and the verification unit (kangaroo_verify.hip) share: the launch constants,
// Jacobian + affine addition and the doubling of an affine point on gfx950, and on the host the comb table, the checks of a call's positions and its staging.
//
// The comb loop itself (seventeen addends through one load and one addition site) is NOT here: it stands twice, in kangaroo_seed_keys_kernel and in
// verify_point of kangaroo_verify.hip.  As one __forceinline__ function called from both, the seeding kernel compiles to 130 VGPRs and three waves per SIMD
// (measured, --offload-arch=gfx950; forced to four waves: 128 VGPRs, 4 of them spilled, 16 bytes of scratch) against 128 VGPRs and four waves with its own
// inlined loop, which is its budget (tests/test_kangaroo_seed_build.py).  The second copy is also what makes the verification an independent check of what
// the seeding writes.
#pragma once
#include "bsgs_internal.h"
#include "host_secp.h"

#include <algorithm>

#define SEED_LDS (4u * SEED_REGION)
#define SEED_WINDOWS 16u
#define SEED_CHUNK (1u << 20)                               // positions per launch: bounds the staging (52 bytes per position)


__device__ __forceinline__ bool seed_is_zero(const fe &a)
{
    return (a.v[0] | a.v[1] | a.v[2] | a.v[3] | a.v[4] | a.v[5] | a.v[6] | a.v[7]) == 0u;
}
__device__ __forceinline__ void seed_twice(fe &r, const fe &a) { fe_add(r, a, a); fe_canon(r); }      // a canonical

// (X, Y, Z) += (ax, ay): Jacobian + affine, X and Y canonical on entry and on return.  CHECK: returns 1 when the two points are equal and 2 when they are
// opposite, (X, Y, Z) untouched; without CHECK the caller knows they are neither.  8 multiplications, 3 squarings.
// (jac_madd_if: CHECK as an argument, for a caller whose one addition site serves both kinds.  jac_madd<CHECK> forwards a constant, which the inliner
// folds: tests/test_kangaroo_seed_build.py pins the single-Q kernel's budget and would show it if that ever stopped.)
__device__ __forceinline__ u32 jac_madd_if(fe &X, fe &Y, fe &Z, const fe &ax, const fe &ay, const bool CHECK)
{
    fe zz, h, r, hh, hhh, v, t;
    fe_sqr(zz, Z);
    fe_mul(h, ax, zz);
    fe_sub(h, h, X);                                       // H = ax Z^2 - X
    fe_mul(t, Z, zz);
    fe_mul(r, ay, t);
    fe_sub(r, r, Y);                                       // R = ay Z^3 - Y
    if (CHECK) {
        fe_canon(h);
        if (__builtin_expect(seed_is_zero(h), 0)) { fe_canon(r); return seed_is_zero(r) ? 1u : 2u; }
    }
    fe_sqr(hh, h);
    fe_mul(hhh, h, hh);
    fe_canon(hhh);
    fe_mul(v, X, hh);
    fe_canon(v);
    fe_mul(Z, Z, h);
    fe_sqr(t, r);
    fe_sub(t, t, hhh);
    fe_sub(t, t, v);
    fe_sub(X, t, v);                                       // X3 = R^2 - H^3 - 2 V
    fe_canon(X);
    fe_sub(t, v, X);
    fe_mul(t, r, t);
    fe_mul(hhh, Y, hhh);
    fe_canon(hhh);
    fe_sub(Y, t, hhh);                                     // Y3 = R (V - X3) - Y H^3
    fe_canon(Y);
    return 0u;
}
template <bool CHECK>
__device__ __forceinline__ u32 jac_madd(fe &X, fe &Y, fe &Z, const fe &ax, const fe &ay) { return jac_madd_if(X, Y, Z, ax, ay, CHECK); }
// (X, Y, Z) = 2 (ax, ay): S = 4 x y^2, M = 3 x^2, X3 = M^2 - 2 S, Y3 = M (S - X3) - 8 y^4, Z3 = 2 y
__device__ __forceinline__ void jac_double_affine(fe &X, fe &Y, fe &Z, const fe &ax, const fe &ay)
{
    fe yy, s, m, t, y4;
    fe_sqr(yy, ay);
    fe_canon(yy);
    fe_mul(s, ax, yy);
    fe_canon(s);
    seed_twice(s, s);
    seed_twice(s, s);
    fe_sqr(t, ax);
    fe_canon(t);
    seed_twice(m, t);
    fe_add(m, m, t);
    fe_canon(m);
    fe_sqr(y4, yy);
    fe_canon(y4);
    seed_twice(y4, y4);
    seed_twice(y4, y4);
    seed_twice(y4, y4);
    fe_sqr(X, m);
    fe_sub(X, X, s);
    fe_sub(X, X, s);
    fe_canon(X);
    fe_sub(t, s, X);
    fe_mul(t, m, t);
    fe_sub(Y, t, y4);
    fe_canon(Y);
    seed_twice(Z, ay);
}


// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------
static inline int seed_comb(bsgs_dev *d, bsgs_kangaroo *k)
{
    if (k->comb) return BSGS_OK;
    std::vector<uint8_t> tab((size_t)SEED_WINDOWS * 255 * 64);
    hs::Affine base = hs::G;
    for (uint32_t w = 0; w < SEED_WINDOWS; w++) {
        const std::vector<hs::Affine> m = hs::multiples(base, 256);          // base, 2 base, ..., 256 base
        for (uint32_t v = 0; v < 255; v++) hs::affine_to_le(m[v], &tab[((size_t)w * 255 + v) * 64], &tab[((size_t)w * 255 + v) * 64 + 32]);
        base = m.back();
    }
    HIPCHK(hipMalloc(&k->comb, tab.size()));
    HIPCHK(hipMemcpyAsync(k->comb, tab.data(), tab.size(), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));                                 // (tab leaves scope)
    return BSGS_OK;
}


// the positions of a seed call: idx[0..n) distinct kangaroos of the herd, or [first, first + n) inside it
static inline int seed_check_positions(const bsgs_kangaroo *k, const uint32_t *idx, uint32_t first, uint32_t n)
{
    if (n > k->N) return fail(BSGS_ERR_ARG, "%u kangaroos of %u", n, k->N);
    if (idx) {
        std::vector<uint32_t> s(idx, idx + n);
        std::sort(s.begin(), s.end());
        if (s.back() >= k->N) return fail(BSGS_ERR_ARG, "kangaroo %u of %u", s.back(), k->N);
        if (std::adjacent_find(s.begin(), s.end()) != s.end()) return fail(BSGS_ERR_ARG, "a kangaroo is listed twice");
    } else if ((uint64_t)first + n > k->N) return fail(BSGS_ERR_ARG, "kangaroos [%u, %u) of %u", first, first + n, k->N);
    return BSGS_OK;
}
// the comb, the staging of one chunk (offsets [cap] | flags [cap] | index list [cap]; Z [2][cap]) and the cleared result words
static inline int seed_staging(bsgs_dev *d, bsgs_kangaroo *k, uint32_t n)
{
    if (int rc = seed_comb(d, k)) return rc;
    const uint32_t cap = std::min(n, SEED_CHUNK);
    if (k->seed_cap < cap) {
        if (k->seed_in) (void)hipFree(k->seed_in);
        if (k->seed_z) (void)hipFree(k->seed_z);
        k->seed_in = k->seed_z = nullptr; k->seed_cap = 0;
        HIPCHK(hipMalloc(&k->seed_in, (size_t)cap * 24));
        HIPCHK(hipMalloc(&k->seed_z, (size_t)cap * 32));
        k->seed_cap = cap;
    }
    if (!k->seed_out) HIPCHK(hipMalloc(&k->seed_out, 8));
    static const uint32_t init[2] = {0u, 0xFFFFFFFFu};
    HIPCHK(hipMemcpyAsync(k->seed_out, init, 8, hipMemcpyHostToDevice, d->stream));
    return BSGS_OK;
}
