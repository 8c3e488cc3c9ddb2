/* gstark_sparse_tree.h — sparse Merkle trees of fixed depth kept on the device, over the node functions of gs_hades_merkle
 * (gstark_hades.h) and gs_rescue_merkle (gstark_rescue.h): csrc/field_tree.hip, csrc/sparse_tree_plan.h.
 *
 * A tree of depth d, 1 .. 36, IS the dense heap tree of 2^d leaves of gs_*_merkle whose leaves all hold one `empty` value until they are
 * set: every node, path and update record is bit for bit that tree's.  empties[0] = empty, empties[l + 1] = node(empties[l], empties[l]);
 * the root of a tree with nothing stored is empties[d].  A node whose whole subtree is empty is not stored and is read as
 * empties[level], so a path of an index that was never set starts with `empty`: the non-membership path.
 *
 * Memory: the nodes live in a device store of slots x digest elements that is append-only (a node keeps its slot for life) and grows by
 * doubling with one device copy; the host keeps, per level, an index from node number to slot.  Each stored leaf costs up to d stored
 * nodes and d index entries.  Setting a leaf back to `empty` keeps its nodes stored: nothing is pruned.  The store does not grow past
 * 2^31 slots; the call that would need more is refused.
 *
 * gs_sparse_update sets leaf indexes_host[j] to leaves[j] in order j = 0 .. count - 1, repeated indexes allowed, and delivers what
 * gs_*_merkle_update (gstark_tree_update.h) delivers, in its layouts: before_out, count x (d + 1) x digest elements, per update the leaf
 * and its d siblings bottom-up as they stood just before it; roots_out, count x digest elements, the root just after update j.
 * gs_sparse_paths delivers count x (d + 1) x digest elements in the layout of gs_hades_merkle_paths: per path the leaf, then its
 * siblings bottom-up.  Both take at most 2^20 indexes per call (a larger batch is several calls: the tree carries over); count = 0 is
 * GS_OK and touches nothing.  leaves, before_out, roots_out, out and root_out are device arrays that do not overlap each other.  A
 * refused call leaves the tree as it was.  Everything is enqueued on the context's stream; nothing is read back by the library.
 *
 * The create entries keep the hash handle: it must outlive the tree.  The library knows which hash handles are live: after
 * gs_hades_destroy / gs_rescue_destroy of its hash, every entry but gs_sparse_destroy and gs_sparse_stored refuses the tree with
 * GS_ERR_ARG and "the tree's hash has been destroyed", and the create entries refuse a destroyed handle, with nothing launched.  A tree
 * is destroyed before its context: gs_ctx_destroy does not free the trees made on it, and the host index of a tree is up to d entries
 * per stored leaf.  slots_hint, at least 1, is the initial capacity of the store.
 * empty_leaf_host: `digest` canonical elements on the host, or NULL for zeros.
 *
 * These entry points are OPTIONAL on an implementation of the ABI, like those of gstark_tree_update.h: the HIP library exports them; a
 * binding that does not find the family computes on host integers (genstark_amd/sparse_tree.py) or says so (js/field_tree.js). */
#ifndef GSTARK_SPARSE_TREE_H
#define GSTARK_SPARSE_TREE_H

#include "gstark_hades.h"
#include "gstark_rescue.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gs_sparse gs_sparse;

/* nodes of `digest` elements (1 or 2), 2 * digest < width, as gs_hades_merkle */
int gs_hades_sparse_create(gs_ctx *ctx, const gs_hades *h, uint32_t depth, uint32_t digest, const void *empty_leaf_host, uint64_t slots_hint, gs_sparse **tree);

/* nodes of one element, width 3 .. 8, as gs_rescue_merkle */
int gs_rescue_sparse_create(gs_ctx *ctx, const gs_rescue *h, uint32_t depth, const void *empty_leaf_host, uint64_t slots_hint, gs_sparse **tree);

int gs_sparse_update(gs_ctx *ctx, gs_sparse *tree, const uint64_t *indexes_host, const void *leaves, uint64_t count, void *before_out, void *roots_out);

int gs_sparse_paths(gs_ctx *ctx, const gs_sparse *tree, const uint64_t *indexes_host, uint64_t count, void *out);

/* root_out: `digest` elements on the device */
int gs_sparse_root(gs_ctx *ctx, const gs_sparse *tree, void *root_out);

/* out: (depth + 1) x digest elements on the device, empties[0 .. depth] */
int gs_sparse_empties(gs_ctx *ctx, const gs_sparse *tree, void *out);

/* the nodes stored on `level` (0: leaves .. depth: the root); 0 for a null tree or a level above the root */
uint64_t gs_sparse_stored(const gs_sparse *tree, uint32_t level);

int gs_sparse_destroy(gs_ctx *ctx, gs_sparse *tree);

#ifdef __cplusplus
}
#endif
#endif
