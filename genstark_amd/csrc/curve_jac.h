// curve_jac.h — the group law of y^2 = x^3 + a*x + b in Jacobian coordinates (X / Z^2, Y / Z^3; Z = 0 is infinity, whatever X and Y hold),
// once for curve.hip (scalar multiplications) and msm.hip (sums of scalar multiples).  Device code over the flavour-neutral fe_* API.
//   complete    every formula keeps Z = 0 for infinity: doubling infinity or a point with Y = 0 gives Z3 = 2 * Y * Z = 0, and adding the
//               opposite point (H = 0, R != 0) gives Z3 = Z1 * [Z2 *] H = 0.  An infinite operand is replaced by the other one with selects.
//               Equal points (H = 0 and R = 0, both finite) are the one case the addition formulas do not cover: a branch doubles instead.
#pragma once
#include "common.h"

#define GS_CURVE_DOUBLE_PRODUCTS 10
#define GS_CURVE_ADD_PRODUCTS 11               // Jacobian + affine
#define GS_CURVE_FULL_ADD_PRODUCTS 16          // Jacobian + Jacobian

struct jac { fe X, Y, Z; };

__device__ __forceinline__ fe fe_select(bool take, const fe &a, const fe &b) {     // take ? a : b, limb by limb: v_cndmask, no branch
    fe r;
#pragma unroll
    for (int i = 0; i < GF_LIMBS; i++) fe_set_limb(r, i, take ? fe_limb(a, i) : fe_limb(b, i));
    return r;
}
__device__ __forceinline__ fe fe_dbl(const fe &a) { return fe_add(a, a); }

__device__ __forceinline__ jac jac_infinity() {
    jac r;
    r.X = fe_zero(); r.Y = fe_one(); r.Z = fe_zero();
    return r;
}

// 2 * p for any a (10 products).  Z3 = 2 * Y * Z: infinity stays infinity, a point with Y = 0 becomes infinity.
__device__ __forceinline__ jac jac_double(const jac &p, const fe &a) {
    const fe yy = fe_sqr(p.Y), zz = fe_sqr(p.Z);
    jac r;
    r.Z = fe_dbl(fe_mul(p.Y, p.Z));
    const fe s = fe_dbl(fe_dbl(fe_mul(p.X, yy)));                               // 4 X Y^2
    const fe xx = fe_sqr(p.X);
    const fe m = fe_add(fe_add(fe_dbl(xx), xx), fe_mul(a, fe_sqr(zz)));         // 3 X^2 + a Z^4
    r.X = fe_sub(fe_sqr(m), fe_dbl(s));
    const fe y4 = fe_dbl(fe_dbl(fe_dbl(fe_sqr(yy))));                           // 8 Y^4
    r.Y = fe_sub(fe_mul(m, fe_sub(s, r.X)), y4);
    return r;
}

// p + (x2, y2), the second point affine and finite (11 products).  p infinity: (x2, y2, 1).  Opposite points: H = 0 makes Z3 = 0.
// Equal points (H = 0 and R = 0, p finite): the doubling of p, by a branch that a scalar multiplication on a curve of cryptographic size
// never takes.
__device__ __forceinline__ jac jac_add_affine(const jac &p, const fe &x2, const fe &y2, const fe &a) {
    const fe zz = fe_sqr(p.Z);
    const fe h = fe_sub(fe_mul(x2, zz), p.X);
    const fe r = fe_sub(fe_mul(y2, fe_mul(p.Z, zz)), p.Y);
    const bool at_infinity = fe_is_zero(p.Z);
    jac o;
    if (fe_is_zero(h) && fe_is_zero(r) && !at_infinity) {
        o = jac_double(p, a);
    } else {
        const fe hh = fe_sqr(h);
        const fe hhh = fe_mul(h, hh), v = fe_mul(p.X, hh);
        o.Z = fe_mul(p.Z, h);
        o.X = fe_sub(fe_sub(fe_sqr(r), hhh), fe_dbl(v));
        o.Y = fe_sub(fe_mul(r, fe_sub(v, o.X)), fe_mul(p.Y, hhh));
    }
    o.X = fe_select(at_infinity, x2, o.X);
    o.Y = fe_select(at_infinity, y2, o.Y);
    o.Z = fe_select(at_infinity, fe_one(), o.Z);
    return o;
}

// p + q, both Jacobian (16 products), complete: either operand infinity (the other one, by selects), opposite points (H = 0 makes
// Z3 = 0), equal points (H = 0 and R = 0, both finite: the doubling of p, by a branch).  Inlined like the
// rest (operands stay in registers): a kernel calls it from ONE place, inside a loop that is not unrolled.
__device__ __forceinline__ jac jac_add(const jac &p, const jac &q, const fe &a) {
    const fe z1z1 = fe_sqr(p.Z), z2z2 = fe_sqr(q.Z);
    const fe u1 = fe_mul(p.X, z2z2), u2 = fe_mul(q.X, z1z1);
    const fe s1 = fe_mul(p.Y, fe_mul(q.Z, z2z2)), s2 = fe_mul(q.Y, fe_mul(p.Z, z1z1));
    const fe h = fe_sub(u2, u1), r = fe_sub(s2, s1);
    const bool p_inf = fe_is_zero(p.Z), q_inf = fe_is_zero(q.Z);
    jac o;
    if (fe_is_zero(h) && fe_is_zero(r) && !p_inf && !q_inf) {
        o = jac_double(p, a);
    } else {
        const fe hh = fe_sqr(h);
        const fe hhh = fe_mul(h, hh), v = fe_mul(u1, hh);
        o.Z = fe_mul(fe_mul(p.Z, q.Z), h);
        o.X = fe_sub(fe_sub(fe_sqr(r), hhh), fe_dbl(v));
        o.Y = fe_sub(fe_mul(r, fe_sub(v, o.X)), fe_mul(s1, hhh));
    }
    o.X = fe_select(q_inf, p.X, fe_select(p_inf, q.X, o.X));
    o.Y = fe_select(q_inf, p.Y, fe_select(p_inf, q.Y, o.Y));
    o.Z = fe_select(q_inf, p.Z, fe_select(p_inf, q.Z, o.Z));
    return o;
}
