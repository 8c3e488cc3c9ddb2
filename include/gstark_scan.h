/* gstark_scan.h — running sums, running products and the linear recurrence x[i] = a[i]*x[i-1] + b[i] over device vectors, on the device
 * (csrc/scan.hip): what an accumulator register of a trace holds (a running balance over the runs of an input register, the grand
 * product of a permutation check, a Horner chain, a geometric sum), computed where the vector already lies.
 *
 * Every result is what the definition gives on integers modulo p; inputs are canonical elements and outputs are canonical.  For a
 * segment v[0 .. m):
 *   sum        inclusive out[i] = v[0] + ... + v[i];  exclusive out[i] = v[0] + ... + v[i-1], out[0] = 0
 *   product    inclusive out[i] = v[0] * ... * v[i];  exclusive out[i] = v[0] * ... * v[i-1], out[0] = 1
 *   affine     inclusive out[i] = x[i] with x[i] = a[i]*x[i-1] + b[i], x[-1] = x0;  exclusive out[i] = x[i-1], out[0] = x0
 * A call scans rows * cols elements, lying contiguously, in one of three segment forms:
 *   one vector          rows = 1, heads = NULL: a single segment of cols elements
 *   uniform segments    heads = NULL: rows segments of cols elements each (a row-major matrix, every row on its own)
 *   flagged segments    rows = 1, heads = cols bytes on the device: heads[i] & 1 starts a new segment at i (element 0 starts one
 *                       whatever its byte says)
 * Segments never influence each other.  At most 2^24 elements per call, all segments together; 0 elements does nothing; cols == 0
 * with rows > 0 is refused.  `out` may be exactly the input (`values`; for the affine op `b`, never `a`); any other overlap between
 * an output and an input, or between two outputs, is refused.  A refused call enqueues nothing and leaves the context usable.
 *
 * These entry points are OPTIONAL on an implementation of the ABI (include/gstark.h lists the mandatory ones), like those of
 * gstark_sqrt.h: the HIP library exports them; a binding that does not find them computes on host integers (genstark_amd/field.py) or
 * says so (js/galois.js).  Everything is enqueued on the context's stream; nothing is read back; temporaries come from the context's
 * pooled allocator and go back to it.  The schedule (csrc/scan_plan.h) is at most three launches and depends on the element count
 * alone; no workgroup waits for another inside a kernel. */
#ifndef GSTARK_SCAN_H
#define GSTARK_SCAN_H

#include "gstark.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_SCAN_SUM 0
#define GS_SCAN_PRODUCT 1

/* out (device, rows * cols elements) = the running sums (op = GS_SCAN_SUM) or products (GS_SCAN_PRODUCT) of values (device, rows * cols
 * canonical elements), inclusive (exclusive = 0) or exclusive (1).  heads: NULL, or (device) cols bytes with rows == 1.
 * totals_out: NULL, or (device, rows elements, heads == NULL) the sum or product of each whole row, whichever form `out` has. */
int gs_scan(gs_ctx *ctx, int op, int exclusive, const void *values, const void *heads, uint64_t rows, uint64_t cols, void *out, void *totals_out);

/* out (device, rows * cols elements) = x[i] (exclusive = 0) or x[i-1] (1) of x[i] = a[i]*x[i-1] + b[i], every segment starting from x0.
 *   a           (device) rows * cols canonical elements, or NULL: a_scalar_host is the factor of every step
 *   a_scalar_host   ONE canonical element in host memory (Horner chains, geometric sums); read only where a is NULL
 *   b           (device) rows * cols canonical elements
 *   x0_host     ONE canonical element in host memory, or NULL for 0.  A start that differs from segment to segment is folded into
 *               that segment's first b: b'[first] = a[first]*x0[segment] + b[first], x0 = 0.
 *   heads       as in the sum and product entry */
int gs_scan_affine(gs_ctx *ctx, int exclusive, const void *a, const gs_elt *a_scalar_host, const void *b, const gs_elt *x0_host, const void *heads,
                   uint64_t rows, uint64_t cols, void *out);

/* totals_out (device, rows elements) = the sum or product of each row of values (device, rows * cols canonical elements); no running
 * values are written. */
int gs_reduce(gs_ctx *ctx, int op, const void *values, uint64_t rows, uint64_t cols, void *totals_out);

/* The plan of the context's field: the elements one workgroup scans (a tile), the consecutive elements one thread owns, the most
 * elements one call takes, and the launches a call of n elements enqueues (0 for n == 0 or n above the maximum).  Any pointer may
 * be NULL. */
int gs_scan_plan(gs_ctx *ctx, uint64_t n, uint32_t *tile_elements, uint32_t *elements_per_thread, uint64_t *max_elements, uint32_t *launches);

#ifdef __cplusplus
}
#endif
#endif
