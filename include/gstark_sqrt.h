/* gstark_sqrt.h — square roots in the library's field and the lift of an x coordinate to a point of y^2 = x^3 + a*x + b, on the device
 * (csrc/sqrt.hip): what a caller needs before the entries of gstark_curve.h and gstark_msm.h when keys, nonce points and commitments
 * arrive compressed or x-only (assembly/lib224.aa and examples/elliptic/pointmul.aa state their points in full).
 *
 * A root is the EVEN one of r and p - r as canonical integers (the parity convention of SEC1's compressed points); 0 is a square with
 * root 0; a non-residue has flag 0 and root 0.  A compressed point is its x and one parity byte (y & 1); a point that does not exist
 * comes back as (0, 0) with flag 0, the convention of infinity in gstark_curve.h.  Every result is what the definition gives on host
 * integers.  The schedule (csrc/sqrt_plan.h) depends on the modulus alone: no trip count depends on a value.
 *
 * These entry points are OPTIONAL on an implementation of the ABI (include/gstark.h lists the mandatory ones), like those of
 * gstark_curve.h: the HIP library exports them; a binding that does not find them computes on host integers (genstark_amd/field.py,
 * genstark_amd/curve.py) or says so (js/galois.js, js/curve.js).  Everything is enqueued on the context's stream; nothing is read
 * back.  The context builds its tables with the first call and frees them when it is destroyed.  A modulus that is not prime (the
 * runtime-modulus build takes any odd one) is refused by that first call: GS_ERR_UNSUPPORTED, "modulus is not prime". */
#ifndef GSTARK_SQRT_H
#define GSTARK_SQRT_H

#include "gstark.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags_out[k] (device, count bytes) = 1 when values[k] is a square (0 included), else 0; roots_out[k] (device, count elements, or
 * NULL: flags only, by Euler's criterion) = its even root, 0 where the flag is 0.  values: (device) count canonical elements.
 * count == 0 does nothing; at most 2^20 elements per call. */
int gs_field_sqrt(gs_ctx *ctx, const void *values, uint64_t count, void *roots_out, void *flags_out);

/* points_out[k] (device, count x 2 elements) = (xs[k], y) with y^2 = xs[k]^3 + a*xs[k] + b and (y & 1) == parities[k], flags_out[k]
 * (device, count bytes) = 1; where the right-hand side is not a square: (0, 0) and flag 0.  y = 0 answers both parities.
 *   a, b        ONE canonical element each in host memory
 *   xs          (device) count canonical elements
 *   parities    (device, or NULL: every y even) count bytes, of which the low bit is used
 * count == 0 does nothing; at most 2^20 points per call. */
int gs_curve_lift_x(gs_ctx *ctx, const gs_elt *a, const gs_elt *b, const void *xs, const void *parities, uint64_t count, void *points_out,
                    void *flags_out);

/* xs_out[k] (device, count elements) = x and parities_out[k] (device, count bytes) = y & 1 of row k of points (device, count x 2
 * elements).  count == 0 does nothing; at most 2^20 points per call. */
int gs_curve_compress(gs_ctx *ctx, const void *points, uint64_t count, void *xs_out, void *parities_out);

/* The plan the context's field uses: p - 1 = 2^two_adicity * t, the width of a window of the discrete logarithm, the number of
 * windows, and the field products one root takes (the work unit of the traffic tally).  Any pointer may be NULL. */
int gs_field_sqrt_plan(gs_ctx *ctx, uint32_t *two_adicity, uint32_t *window_bits, uint32_t *windows, uint32_t *products_per_root);

#ifdef __cplusplus
}
#endif
#endif
