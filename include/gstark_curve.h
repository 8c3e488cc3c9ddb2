/* gstark_curve.h — scalar multiplications on short Weierstrass curves y^2 = x^3 + a*x + b over the library's field, on the device
 * (csrc/curve.hip): the numbers the reference's elliptic-curve statements assert (examples/elliptic/pointmul.aa: the product k*P;
 * assembly/lib224.aa VerifySchnorrSignature: a public key x*G, a nonce point k*G, and the check s*G = R + h*P) in batches.
 *
 * A point is two canonical elements (x, y).  The point at infinity is carried by a flag byte beside the coordinates, which are then
 * (0, 0).  There is no handle: `a` and `b` travel with every call as ONE element each in host memory, like `omega` elsewhere.  Every
 * result is what the affine group law gives on host integers — complete: every mix of infinity, equal points, opposite points and
 * points with y = 0.
 *
 * These entry points are OPTIONAL on an implementation of the ABI (include/gstark.h lists the mandatory ones), like those of
 * gstark_hades.h: the HIP library exports them; a binding that does not find them computes on host integers (genstark_amd/curve.py) or
 * says so (js/curve.js).  Everything is enqueued on the context's stream; nothing is read back. */
#ifndef GSTARK_CURVE_H
#define GSTARK_CURVE_H

#include "gstark.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[k] = addends[k] + scalars[k] * points[k] for k < count, one thread each.
 *   points      (device) npoints x 2 elements, finite points of the curve; npoints == count, or npoints == 1: every multiplication
 *               uses row 0 (the fixed-base case x*G)
 *   scalars     (device) count x 32 bytes: little-endian 256-bit integers, of which the low `bits` (1 .. 256) are used
 *   addends     (device, or NULL: every addend is infinity) count x 2 elements
 *   addend_inf  (device, or NULL: no addend is infinity) count bytes, non-zero = addend k is infinity whatever addends[k] holds
 *   out         (device) count x 2 elements, affine and canonical; inf_out (device) count bytes, 1 = result k is infinity
 * count == 0 does nothing; at most 2^20 multiplications per call.  `b` is not needed: the group law does not read it. */
int gs_curve_mul(gs_ctx *ctx, const gs_elt *a, const void *points, uint64_t npoints, const void *scalars, uint32_t bits, const void *addends,
                 const void *addend_inf, uint64_t count, void *out, void *inf_out);

/* flags_out[k] (device, count bytes) = 1 when y^2 = x^3 + a*x + b for row k of points (device, count x 2 elements), else 0.
 * count == 0 does nothing; at most 2^20 rows per call. */
int gs_curve_contains(gs_ctx *ctx, const gs_elt *a, const gs_elt *b, const void *points, uint64_t count, void *flags_out);

#ifdef __cplusplus
}
#endif
#endif
