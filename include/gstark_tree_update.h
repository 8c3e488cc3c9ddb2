/* gstark_tree_update.h — batches of leaf updates applied to a device-resident Merkle tree of gs_hades_merkle (gstark_hades.h) or
 * gs_rescue_merkle (gstark_rescue.h), with the witness of every update (csrc/field_tree.hip, csrc/tree_update_plan.h).
 *
 * `nodes` is a tree in the heap layout those entries write: 2n x digest elements, leaves at n .. 2n - 1, root at 1.  Update j sets leaf
 * indexes_host[j] to leaves[j]; the updates are applied in order j = 0, 1, .. count - 1, repeated indexes allowed, a leaf equal to the
 * old one included.  For every update the call delivers what the statement ComputeMerkleUpdate (assembly/lib128.aa, lib224.aa of the
 * reference) takes:
 *   before_out  count x (log2 n + 1) x digest elements: per update the leaf as it stood just before that update and its log2 n
 *               siblings bottom-up as they stood just before it — the path gs_hades_merkle_paths would have delivered between
 *               update j - 1 and update j;
 *   roots_out   count x digest elements: the root just after update j.  The root before it is roots_out[j - 1], or node 1 as it
 *               stood at the call for j = 0.
 * Afterwards `nodes` holds the tree of the last update.  The cost is count x log2 n permutations, not count trees: a level is one
 * hash launch over the whole batch, and a node an update computes is bit for bit the node gs_*_merkle computes.
 *
 * count is at most 2^20 updates per call (a larger ledger is several calls: the tree carries over).  count = 0 is GS_OK and touches
 * nothing.  leaves, before_out and roots_out are device arrays that overlap neither each other nor `nodes`.  Everything is enqueued
 * on the context's stream; nothing is read back.
 *
 * These entry points are OPTIONAL on an implementation of the ABI, like those of gstark_hades.h: the HIP library exports them; a
 * binding that does not find them updates on host integers (genstark_amd/field_tree.py) or says so (js/field_tree.js). */
#ifndef GSTARK_TREE_UPDATE_H
#define GSTARK_TREE_UPDATE_H

#include "gstark_hades.h"
#include "gstark_rescue.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a tree of gs_hades_merkle(ctx, h, .., n, digest, nodes): 2 * digest < width, as there */
int gs_hades_merkle_update(gs_ctx *ctx, const gs_hades *h, void *nodes, uint64_t n, uint32_t digest, const uint64_t *indexes_host, const void *leaves,
                           uint64_t count, void *before_out, void *roots_out);

/* a tree of gs_rescue_merkle(ctx, h, .., n, nodes): nodes of one element, width 3 .. 8, as there */
int gs_rescue_merkle_update(gs_ctx *ctx, const gs_rescue *h, void *nodes, uint64_t n, const uint64_t *indexes_host, const void *leaves, uint64_t count,
                            void *before_out, void *roots_out);

#ifdef __cplusplus
}
#endif
#endif
