/* gstark_absorb.h — variable-length algebraic hashes on the device: records of any length into one or two field elements, with the
 * Hades permutation (csrc/hades.hip) or the Rescue permutation (csrc/rescue.hip), the shared checks in csrc/sponge_common.h.
 *
 * The function is the same for both families.  pi is a permutation of `width` elements, 1 <= rate <= width - 1, digest is 1 or 2 and at
 * most rate, and m[0 .. length) are the inputs of one row, 1 <= length <= 2^16 (the length is below the modulus):
 *
 *     state = width zeros;  state[rate] = length            (the first capacity element carries the length)
 *     for b in 0 .. ceil(length / rate) - 1:
 *         state[j] += m[b * rate + j]   for j < rate while b * rate + j < length      (added, not overwritten; a short last block adds nothing more)
 *         state = pi(state)
 *     the digest is state[0 .. digest)
 *
 * For gs_hades_absorb pi is the permutation of gstark_hades.h.  For gs_rescue_absorb pi is what gs_rescue_hash applies to a row of
 * `width` inputs: modifiedSponge (modified = 1) or sponge (modified = 0) of gstark_rescue.h, the whole last state.
 *
 * This is NOT gs_hades_hash / gs_rescue_hash of the same inputs, for rows short enough to fit one permutation either: the length in the
 * capacity keeps the rows [a] and [a, 0] apart, which the zero padding of the one-permutation entries does not.
 *
 * Element i of row k is read at in[k * row_stride + i * elem_stride] (strides in elements).  Two layouts are served, every other pair
 * of strides is refused:
 *     rows      elem_stride = 1, row_stride >= length: a count x length matrix, or the leading columns of a wider one
 *     columns   row_stride = 1, elem_stride >= count: the register-major length x count matrix of a trace, or the leading rows' worth of
 *               columns of a wider one
 *
 * out (device) receives count x digest elements and must not overlap what is read of `in`.  count = 0 is GS_OK and touches nothing;
 * count * ceil(length / rate) is at most 2^36.  A refused call leaves `out` untouched.
 *
 * These entry points are OPTIONAL on an implementation of the ABI, like those of gstark_hades.h: the HIP library exports them; a
 * binding that does not find them computes on host integers (genstark_amd/hades.py, genstark_amd/rescue_hash.py) or says so
 * (js/hades.js, js/rescue.js).  Everything is enqueued on the context's stream; nothing is read back. */
#ifndef GSTARK_ABSORB_H
#define GSTARK_ABSORB_H

#include "gstark_hades.h"
#include "gstark_rescue.h"

#ifdef __cplusplus
extern "C" {
#endif

int gs_hades_absorb(gs_ctx *ctx, const gs_hades *h, const void *in, uint64_t count, uint32_t length, uint64_t row_stride, uint64_t elem_stride, uint32_t rate,
                    uint32_t digest, void *out);

int gs_rescue_absorb(gs_ctx *ctx, const gs_rescue *h, const void *in, uint64_t count, uint32_t length, uint64_t row_stride, uint64_t elem_stride, uint32_t rate,
                     uint32_t digest, uint32_t modified, void *out);

#ifdef __cplusplus
}
#endif
#endif
