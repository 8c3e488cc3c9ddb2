/* gstark_msm.h — sums of scalar multiples on short Weierstrass curves y^2 = x^3 + a*x + b over the library's field, on the device
 * (csrc/msm.hip, planned by csrc/msm_plan.h): what include/gstark_curve.h multiplies, added up in the same call — a Pedersen-style
 * commitment to a device column, the one equation that checks a block of Schnorr signatures, any linear combination of public keys.
 *
 * Points, `a` and the infinity flag are those of gstark_curve.h: two canonical elements (x, y) per point, `a` as ONE element in host
 * memory, infinity as a flag byte beside coordinates (0, 0).  The result is what the affine group law gives on host integers, whatever
 * order the device adds in.
 *
 * The entry point is OPTIONAL on an implementation of the ABI, exactly as those of gstark_curve.h are: the HIP library exports it; a
 * binding that does not find it computes on host integers (genstark_amd/curve.py) or says so (js/curve.js).  Everything is enqueued on
 * the context's stream; nothing is read back; workspace comes from the context's block cache. */
#ifndef GSTARK_MSM_H
#define GSTARK_MSM_H

#include "gstark.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out = sum over k < count of (scalars[k] mod 2^bits) * points[k], affine and canonical.
 *   points         (device) count x 2 elements, finite points of the curve
 *   scalars        (device) count little-endian integers of scalar_stride bytes each
 *   scalar_stride  32: the layout of gs_curve_mul.  16: a column of 16-byte field elements is a scalar column as it stands; bits <= 128
 *   bits           1 .. 256: the low bits of every scalar that count
 *   window         0: the plan chooses the route and the window width.  1 .. 16: the bucket method with windows of that many bits
 *   out            (device) 2 elements; inf_out (device) 1 byte, 1 = the sum is infinity, and then out is (0, 0)
 * count == 0 is the empty sum: infinity.  At most 2^20 terms per call.  Refused with GS_ERR_ARG before anything is enqueued, the
 * message naming the argument: count above 2^20, a scalar_stride other than 16 or 32, bits outside 1 .. 256 or above 128 with a stride
 * of 16, window above 16 or a forced window whose workspace would exceed the plan's cap (512 MiB), a missing pointer, a non-canonical
 * `a`.  `b` is not needed: the group law does not read it. */
int gs_curve_msm(gs_ctx *ctx, const gs_elt *a, const void *points, const void *scalars, uint32_t scalar_stride, uint32_t bits, uint64_t count,
                 uint32_t window, void *out, void *inf_out);

#ifdef __cplusplus
}
#endif
#endif
