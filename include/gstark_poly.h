/* gstark_poly.h — long polynomials at ARBITRARY points, on the device (csrc/poly.hip, planned by csrc/poly_plan.h): the vanishing
 * polynomial of a set, quotient and remainder, the values of a polynomial at many points, the interpolant through many points — each in
 * a number of field products that grows as n log^2 n, where gs_small_interpolate and gs_eval_polys_at_points (both unchanged) take n^2.
 *
 * Coefficients are low-order first; polynomials, points and values are canonical elements in DEVICE memory.  `omega` is ONE element in
 * host memory of exact order 2^omega_log2: every entry derives the roots of its shorter transforms from it by squaring on the host, as
 * gs_boundary_polys does from its omega.  A call whose plan needs a transform of more than 2^omega_log2 points is refused.
 *
 * The entry points are OPTIONAL on an implementation of the ABI, exactly as those of gstark_msm.h are: the HIP library exports them; a
 * binding that does not find them computes on host integers by the quadratic definitions (genstark_amd/field.py) or says so
 * (js/galois.js).  Everything is enqueued on the context's stream; workspace comes from the context's block cache, at most 4 GiB per call
 * (4 294 967 296 bytes; the largest plan, an interpolation through 2^20 points of 32-byte elements, takes 2.4 GiB).  Nothing is read back,
 * with ONE exception: gs_poly_div downloads the leading coefficient of its divisor — one element — before it enqueues anything.
 *
 * At most 2^20 coefficients or points per operand.  Every refusal is GS_ERR_ARG before anything is enqueued, the message naming the
 * argument: a count above 2^20, a missing pointer, a non-canonical omega or one that is not of order 2^omega_log2, an omega_log2 too
 * small for the plan (the message names both exponents), a zero leading coefficient. */
#ifndef GSTARK_POLY_H
#define GSTARK_POLY_H

#include "gstark.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out = the n + 1 coefficients of prod over i < n of (x - xs[i]).  n == 0 writes the polynomial 1. */
int gs_poly_from_roots(gs_ctx *ctx, const gs_elt *omega, uint32_t omega_log2, const void *xs, uint64_t n, void *out);

/* a = q * b + r for a of la and b of lb coefficients (both at least 1), b[lb - 1] != 0.
 *   q   la - lb + 1 coefficients; r   lb - 1 coefficients, high zeros included.  Either may be NULL: it is not written.
 *   la < lb: q = 0 (ONE coefficient), r = a, zero-extended.  lb == 1: the division by a constant.
 * b[lb - 1] is downloaded (the family's only read-back) and a zero is refused with GS_ERR_ARG. */
int gs_poly_div(gs_ctx *ctx, const gs_elt *omega, uint32_t omega_log2, const void *a, uint64_t la, const void *b, uint64_t lb, void *q, void *r);

/* out[k] = poly(xs[k]), k < npoints.  Repeated points are allowed; len may be smaller than, equal to or larger than npoints (len == 0 is
 * the zero polynomial). */
int gs_poly_eval_points(gs_ctx *ctx, const gs_elt *omega, uint32_t omega_log2, const void *poly, uint64_t len, const void *xs, uint64_t npoints,
                        void *out);

/* out = the n coefficients of the polynomial of degree below n through (xs[i], ys[i]), n >= 1.  flag (device, ONE byte) is set to 1 when
 * two xs are equal — some M'(x_i) is 0 — and to 0 otherwise; out is then unspecified.  The entry does not read flag. */
int gs_poly_interpolate_points(gs_ctx *ctx, const gs_elt *omega, uint32_t omega_log2, const void *xs, const void *ys, uint64_t n, void *out,
                               void *flag);

/* Tree steps whose child nodes lie in slots of at most 2^log2_len elements are per-thread schoolbook sums, longer ones go through the
 * batched transforms (clamped to 1 .. 12; the default is 8).  Returns the previous value.  No result depends on it. */
uint32_t gs_poly_schoolbook_log2(uint32_t log2_len);

#ifdef __cplusplus
}
#endif
#endif
