/* gstark_rescue.h — Rescue permutations (the hashes of examples/rescue) and Rescue Merkle trees on the device (csrc/rescue.hip).
 *
 * The permutation is the one of the reference's examples/rescue/utils.ts (class Rescue): a state of `width` elements, the inputs
 * followed by zeros; a half round raises every element to a power, replaces the state by mds * state (new[i] = sum_j mds[i][j] *
 * state[j]) and adds one row of keys.  `keys` are the 2 * rounds + 3 rows that unrollConstants() returns.
 *   sponge (modified = 0, utils.ts:49-88):           add keys[0]; then for r < rounds: (x^inv, matrix, keys[2r + 1]), (x^alpha, matrix,
 *                                                    keys[2r + 2])
 *   modifiedSponge (modified = 1, utils.ts:90-124):  no initial key; for r < rounds - 1: (x^alpha, matrix, keys[2r + 2]), (x^inv,
 *                                                    matrix, keys[2r + 3])
 * x^inv is x to the POSITIVE exponent `inv_exponent` (what the reference's field.exp(x, invAlpha) amounts to for its negative invAlpha:
 * p - 1 - |invAlpha|; 0 maps to 0).  The digest is the first `digest` elements of the last state.  Every result is an exact field
 * element: what host integers give.
 *
 * The tree is the reference's MerkleTree (utils.ts:232-273) over makeHashFunction (:11-15) in its heap layout: 2n elements, the leaves
 * at nodes n .. 2n - 1, node i = element 0 of modifiedSponge([node 2i, node 2i + 1, 0, ...]), the root at 1, node 0 zero.
 * Authentication paths come from gs_hades_merkle_paths (gstark_hades.h) with digest = 1.  That gather belongs to no hash family: it
 * reads nothing but a node array in the heap layout, and keeps the name it was first exported with.
 *
 * These entry points are OPTIONAL on an implementation of the ABI (include/gstark.h lists the mandatory ones), like those of
 * gstark_hades.h: the HIP library exports them; a binding that does not find them computes on host integers
 * (genstark_amd/rescue_hash.py) or says so (js/rescue.js).  Everything is enqueued on the context's stream; nothing is read back. */
#ifndef GSTARK_RESCUE_H
#define GSTARK_RESCUE_H

#include "gstark.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gs_rescue gs_rescue;

/* One parameter set, its constants uploaded once: 2 <= width <= 8, rounds >= 1, alpha >= 2; inv_exponent: one canonical element
 * (gs_element_size() bytes) in [1, p - 1); mds_host: width x width elements, row-major; keys_host: (2 * rounds + 3) x width elements,
 * row-major.  The exponent is turned into a sliding-window schedule here, once.  The handle belongs to the context that made it. */
int gs_rescue_create(gs_ctx *ctx, uint32_t width, uint32_t rounds, uint64_t alpha, const uint8_t *inv_exponent, const uint8_t *mds_host,
                     const uint8_t *keys_host, gs_rescue **out);
int gs_rescue_destroy(gs_ctx *ctx, gs_rescue *h);

/* `count` permutations: in (device) holds count x arity elements, row k the inputs of permutation k (1 <= arity <= width); out (device)
 * receives count x digest elements (digest 1 or 2).  modified: 0 sponge, 1 modifiedSponge.  form: 1 = one thread per permutation,
 * 2 = one lane per state element (a permutation on 2, 4 or 8 adjacent lanes), 0 = form 2 for count <= gs_rescue_spread_limit(), form 1
 * above. */
int gs_rescue_hash(gs_ctx *ctx, const gs_rescue *h, const void *in, uint64_t count, uint32_t arity, uint32_t digest, uint32_t modified,
                   uint32_t form, void *out);
uint64_t gs_rescue_spread_limit(void);

/* The tree over n single-element leaves (n a power of two >= 2, width >= 3): nodes_out (device) receives 2n elements in the heap layout
 * above.  leaves may be nodes_out + n elements (the leaves already in place).  Every level is one gs_rescue_hash launch. */
int gs_rescue_merkle(gs_ctx *ctx, const gs_rescue *h, const void *leaves, uint64_t n, void *nodes_out);

#ifdef __cplusplus
}
#endif
#endif
