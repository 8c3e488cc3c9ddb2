/* gstark_tree_verify.h — the roots that batches of authentication paths imply, for the Merkle trees of gs_hades_merkle (gstark_hades.h)
 * and gs_rescue_merkle (gstark_rescue.h): the consuming side of gs_hades_merkle_paths and of gstark_tree_update.h
 * (csrc/tree_verify.h; the path walks are kernels of csrc/hades.hip and csrc/rescue.hip, the gather that feeds them one of csrc/field_tree.hip).
 *
 * `paths` is a device array of count x (depth + 1) x digest elements in exactly the layout gs_hades_merkle_paths and the before_out of
 * gs_*_merkle_update write: per path the leaf, then its `depth` siblings bottom-up (digest = 1 for Rescue).  indexes_host[k] < 2^depth is
 * the leaf index of path k: bit l says on which side the running node enters level l — on the right when the bit is 1.  `leaves`, when
 * not NULL, is a device array of count x digest elements, and path k starts from leaves[k] instead of paths[k][0]: the second half of
 * checking an update record (same siblings, new leaf).  The call delivers
 *   roots_out   count x digest elements: the root path k implies.  A node is what the family's tree build computes: for Hades the
 *               first `digest` elements of the permutation of left || right || zeros (2 * digest < width), for Rescue element 0 of the
 *               modified sponge of (left, right, zeros) (width 3 .. 8); every output is a canonical field element.
 * A path is valid for a root when its entry of roots_out equals that root: the comparison is the caller's, on the device or after one
 * read-back.  The cost is count x depth permutations in ONE launch: a path's running node never leaves its registers.
 *
 * depth is 1 .. 36 and count is at most 2^20 paths per call (a larger batch is several calls).  count = 0 is GS_OK and touches
 * nothing.  paths, leaves and roots_out do not overlap.  Everything is enqueued on the context's stream; nothing is read back.
 *
 * These entry points are OPTIONAL on an implementation of the ABI, like those of gstark_tree_update.h: the HIP library exports them; a
 * binding that does not find them walks the paths on host integers (genstark_amd/field_tree.py) or says so (js/field_tree.js). */
#ifndef GSTARK_TREE_VERIFY_H
#define GSTARK_TREE_VERIFY_H

#include "gstark_hades.h"
#include "gstark_rescue.h"

#ifdef __cplusplus
extern "C" {
#endif

/* paths of a tree of gs_hades_merkle(ctx, h, .., 2^depth, digest, ..): 2 * digest < width, as there */
int gs_hades_merkle_path_roots(gs_ctx *ctx, const gs_hades *h, const void *paths, uint32_t depth, uint32_t digest, const uint64_t *indexes_host,
                               const void *leaves /* may be NULL */, uint64_t count, void *roots_out);

/* paths of a tree of gs_rescue_merkle(ctx, h, .., 2^depth, ..): nodes of one element, width 3 .. 8, as there */
int gs_rescue_merkle_path_roots(gs_ctx *ctx, const gs_rescue *h, const void *paths, uint32_t depth, const uint64_t *indexes_host,
                                const void *leaves /* may be NULL */, uint64_t count, void *roots_out);

#ifdef __cplusplus
}
#endif
#endif
