// curve.hip — scalar multiplications on short Weierstrass curves y^2 = x^3 + a*x + b over the library's field (include/gstark_curve.h):
// the products, public keys and nonce points the reference's examples/elliptic/pointmul.aa and VerifySchnorrSignature (assembly/lib224.aa)
// assert.  One thread runs one multiplication, left to right (most significant bit first), the accumulator in Jacobian coordinates
// (X / Z^2, Y / Z^3; Z = 0 is infinity) in registers; nothing but the flavour-neutral fe_* API, no LDS of its own, nothing crosses lanes.
//   bit loop    `bits` is the same in every lane: the loop is wave-uniform.  Every bit doubles the accumulator and adds the base point;
//               the scalar's bit picks the sum or the doubled accumulator by selects, so a wave never diverges on scalar bits.
//   base point  affine, so every addition is a mixed addition (11 products; a doubling is 10 for a general `a`).  With one base point for
//               all (FIXED) it is read at lane-independent indexes: scalar loads, like the Hades constants.  It is re-read from memory
//               (through the cache) in every iteration rather than held in registers.
//   a           a kernel argument (SGPRs); no formula is special to a = -3.
//   complete    Z = 0 stands for infinity and the formulas keep it: doubling infinity or a point with Y = 0 gives Z3 = 2 * Y * Z = 0, and
//               adding the opposite point (H = 0, R != 0) gives Z3 = Z1 * H = 0.  Infinity + P is P by a select.  P + P (H = 0 and R = 0)
//               is the one case the addition formula does not cover: a rare branch doubles the accumulator instead.
//   output      the addend is one more mixed addition, then ONE inversion (fe_inv: a chain of products like the rest, a tenth of the
//               multiplication's) gives affine, canonical coordinates; infinity is (0, 0) with its flag set.
#include "common.h"
#include "curve_jac.h"                         // jac, fe_select, jac_double, jac_add_affine: shared with msm.hip
#include "../../include/gstark_curve.h"

#define GS_CURVE_BLOCK 64                      // one wave: a batch of 2^12 multiplications spreads over 64 compute units
#define GS_CURVE_MAX_COUNT (1ull << 20)

// out[k] = addends[k] + scalars[k] * points[FIXED ? 0 : k]; 1 <= bits <= 256 (the entry has checked it)
template <bool FIXED>
__global__ __launch_bounds__(GS_CURVE_BLOCK) void k_curve_mul(const fe a, const fe *__restrict__ points, const uint32_t *__restrict__ scalars, uint32_t bits,
                                                              const fe *__restrict__ addends, const uint8_t *__restrict__ addend_inf, uint64_t count,
                                                              fe *__restrict__ out, uint8_t *__restrict__ inf_out) {
    const uint64_t k = (uint64_t)blockIdx.x * GS_CURVE_BLOCK + threadIdx.x;
    if (k >= count) return;                                                  // (nothing below crosses lanes)
    const fe *__restrict__ base = FIXED ? points : points + 2 * k;
    const uint32_t *__restrict__ scalar = scalars + 8 * k;
    jac acc;
    acc.X = fe_zero(); acc.Y = fe_one(); acc.Z = fe_zero();
    uint32_t word = scalar[(bits - 1) >> 5];
#pragma unroll 1
    for (int i = (int)bits - 1; i >= 0; i--) {
        if ((i & 31) == 31) word = scalar[i >> 5];                           // (uniform: i is the same in every lane)
        acc = jac_double(acc, a);
        const jac sum = jac_add_affine(acc, base[0], base[1], a);
        const bool bit = (word >> (i & 31)) & 1u;
        acc.X = fe_select(bit, sum.X, acc.X);
        acc.Y = fe_select(bit, sum.Y, acc.Y);
        acc.Z = fe_select(bit, sum.Z, acc.Z);
    }
    if (addends && !(addend_inf && addend_inf[k])) acc = jac_add_affine(acc, addends[2 * k], addends[2 * k + 1], a);
    const bool inf = fe_is_zero(acc.Z);
    const fe zi = fe_inv(acc.Z), zi2 = fe_sqr(zi);                           // (0 -> 0)
    out[2 * k] = fe_select(inf, fe_zero(), fe_mul(acc.X, zi2));
    out[2 * k + 1] = fe_select(inf, fe_zero(), fe_mul(acc.Y, fe_mul(zi2, zi)));
    inf_out[k] = inf ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_curve_contains(const fe a, const fe b, const fe *__restrict__ points, uint64_t count, uint8_t *__restrict__ flags) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= count) return;
    const fe x = points[2 * k], y = points[2 * k + 1];
    const fe rhs = fe_add(fe_mul(fe_add(fe_sqr(x), a), x), b);               // (x^2 + a) x + b
    flags[k] = fe_eq(fe_sqr(y), rhs) ? 1 : 0;
}

namespace {

// products of one multiplication's group law (the traffic tally's work units): the final inversion, a chain the field header owns, is not counted
uint64_t curve_products(uint32_t bits, bool addend) {
    return (uint64_t)bits * (GS_CURVE_DOUBLE_PRODUCTS + GS_CURVE_ADD_PRODUCTS) + (addend ? GS_CURVE_ADD_PRODUCTS : 0) + 4;
}

int check_element(gs_ctx *c, const char *who, const char *name, const gs_elt *v, fe *out) {
    if (!v) return gs_fail(c, GS_ERR_ARG, "%s: %s is required", who, name);
    *out = fe_from_bytes(v);
    return fe_ge_p(*out) ? gs_fail(c, GS_ERR_ARG, "%s: %s is not a canonical element", who, name) : GS_OK;
}

}  // namespace

extern "C" {

int gs_curve_mul(gs_ctx *c, const gs_elt *a_host, const void *points, uint64_t npoints, const void *scalars, uint32_t bits, const void *addends,
                 const void *addend_inf, uint64_t count, void *out, void *inf_out) {
    if (!c) return GS_ERR_ARG;
    fe a;
    int rc = check_element(c, "curve_mul", "a", a_host, &a);
    if (rc) return rc;
    if (count > GS_CURVE_MAX_COUNT) return gs_fail(c, GS_ERR_ARG, "curve_mul: at most 2^20 multiplications per call, not %llu", (unsigned long long)count);
    if (bits < 1 || bits > 256) return gs_fail(c, GS_ERR_ARG, "curve_mul: %u bits of a scalar are outside 1 .. 256", bits);
    if (!count) return GS_OK;
    if (npoints != 1 && npoints != count)
        return gs_fail(c, GS_ERR_ARG, "curve_mul: %llu points for %llu multiplications: one for all, or one each", (unsigned long long)npoints, (unsigned long long)count);
    if (!points || !scalars || !out || !inf_out) return gs_fail(c, GS_ERR_ARG, "curve_mul: points, scalars, out and inf_out are required");
    const bool fixed = npoints == 1;
    const unsigned blocks = (unsigned)((count + GS_CURVE_BLOCK - 1) / GS_CURVE_BLOCK);
    gs_traffic(c, count * ((fixed ? 2 : 4) * GS_ELT + 33 + (addends ? 2 * GS_ELT : 0) + (addend_inf ? 1 : 0)), count * curve_products(bits, addends != nullptr),
               "k_curve_mul<%s>", fixed ? "fixed" : "variable");
    if (fixed)
        hipLaunchKernelGGL(k_curve_mul<true>, dim3(blocks), dim3(GS_CURVE_BLOCK), 0, c->stream, a, (const fe *)points, (const uint32_t *)scalars, bits,
                           (const fe *)addends, (const uint8_t *)addend_inf, count, (fe *)out, (uint8_t *)inf_out);
    else
        hipLaunchKernelGGL(k_curve_mul<false>, dim3(blocks), dim3(GS_CURVE_BLOCK), 0, c->stream, a, (const fe *)points, (const uint32_t *)scalars, bits,
                           (const fe *)addends, (const uint8_t *)addend_inf, count, (fe *)out, (uint8_t *)inf_out);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

int gs_curve_contains(gs_ctx *c, const gs_elt *a_host, const gs_elt *b_host, const void *points, uint64_t count, void *flags_out) {
    if (!c) return GS_ERR_ARG;
    fe a, b;
    int rc;
    if ((rc = check_element(c, "curve_contains", "a", a_host, &a)) || (rc = check_element(c, "curve_contains", "b", b_host, &b))) return rc;
    if (count > GS_CURVE_MAX_COUNT) return gs_fail(c, GS_ERR_ARG, "curve_contains: at most 2^20 points per call, not %llu", (unsigned long long)count);
    if (!count) return GS_OK;
    if (!points || !flags_out) return gs_fail(c, GS_ERR_ARG, "curve_contains: points and flags_out are required");
    gs_traffic(c, count * (2 * GS_ELT + 1), count * 4, "k_curve_contains");
    hipLaunchKernelGGL(k_curve_contains, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream, a, b, (const fe *)points, count, (uint8_t *)flags_out);
    GS_LAUNCH_CHECK(c);
    return GS_OK;
}

}  // extern "C"
